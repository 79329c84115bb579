"""CPU harness, no sanitizer: the default schedule of a handle (egdst_get_schedule) for the GPU_MAX_HW_QUEUES of this process's
environment ('unset' as first argument: removed before the first handle) at the draw counts given -- a small C2 form, one cell per draw.
python run_emu_schedule.py HWQ|unset NDRAW [NDRAW ...]
One line per draw count: cells, groups and lanes at create, then groups, lanes and stragglers after a solve."""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, os.path.join(ROOT, 'tests', 'cpu_emu'))
import build_emu
from egdst_amd import runtime, workloads
from estimation_emu import write_modelspec

if sys.argv[1] == 'unset':
    os.environ.pop('GPU_MAX_HW_QUEUES', None)   # (import egdst_amd sets a default; the library reads it when a handle is created)
else:
    os.environ['GPU_MAX_HW_QUEUES'] = sys.argv[1]
os.environ.pop('EGDST_GROUPS', None)
m, gen = workloads.c2(a0=0, ngridm=12, T=3, ny=3)
d = write_modelspec(m)
lib = runtime.ModelLibrary(build_emu.build(d, False, 1, False, 1))
for nd in [int(a) for a in sys.argv[2:]]:
    s = runtime.Solver(lib, m.descriptor(), ndraw=nd, keep_history=False)
    g0, l0, _ = s.schedule()
    s.set_params(gen(nd))
    s.solve(raise_on_error=False)
    g1, l1, ns = s.schedule()
    print('cells %d create %d %d solved %d %d %d' % (nd * lib.info.nst, g0, l0, g1, l1, ns), flush=True)
    s.close()
