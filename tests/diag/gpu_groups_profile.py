import sys, os
sys.path.insert(0, 'tests'); sys.path.insert(0, '.')
import numpy as np
from egdst_amd import build, runtime, workloads
wl, nd = sys.argv[1], int(sys.argv[2])
m, gen = workloads.WORKLOADS[wl]()
flags = workloads.BATCH_BUILD_FLAGS.get(wl, [])
lib = build.build_model(m, extra_flags=flags)
P = gen(nd)
s = runtime.Solver(lib, m.descriptor(), ndraw=nd, keep_history=False)
s.set_params(P); s.solve(raise_on_error=False)
print('solved', s.schedule())
s.close()
if len(sys.argv) > 3 and sys.argv[3]:
    os.environ['EGDST_DEBUG_SYNC'] = sys.argv[3]   # (read when a handle is created: a new handle below)
s = runtime.Solver(lib, m.descriptor(), ndraw=nd, keep_history=False)
s.set_params(P); s.solve(raise_on_error=False)
s.set_profile(True); s.solve(raise_on_error=False); print('profiled', np.round(s.profile()[0], 1))
s.set_groups(1); print('groups 1', s.schedule())
s.solve(raise_on_error=False); print('serial', np.round(s.profile()[0], 1))
