"""Diagnostic: the clock stamps of one set (egdst_device.h: env, walk, seg, sort, wg, tpsort, tpwalk).

    python tests/diag/gpu_stamps.py SET [WORKLOAD] [NDRAW] [extra -D flags]

builds WORKLOAD (C1 .. C5, default C2) with -DEGDST_STAMPS=SET and the extra flags, solves NDRAW draws (default 1: the
workload's own parameters) twice and prints every slot of the second solve that is not zero, by name, summed over the draws:
ticks of 10 ns with their milliseconds (counters: the number alone), and for a batch the median and the largest draw.
Environment: EGDST_DIAG_A0 (C2's a0, default 0), and whatever the library reads at create -- EGDST_ENV_TP=1 puts the envelope
step on the throughput path (tpsort, tpwalk; only a large batch takes it by itself), EGDST_NOSEG=1 keeps walks in one piece;
EGDST_DIAG_PER_DRAW=1 prints every draw."""
import os
import sys
import time
sys.path.insert(0, 'tests'); sys.path.insert(0, '.')
import numpy as np
from egdst_amd import build, runtime, workloads

COUNTERS = ('walk.steps', 'walk.batches', 'seg.onewave_walks', 'seg.onewave_why', 'tpsort.sorts',
            'tpsort.sorts_out_of_order', 'tpwalk.stage0_walks', 'tpwalk.stage1_walks')
WHY = ('kink log', 'no scratch', 'too few waves', 'short list', 'scratch too small', 'other')

args = sys.argv[1:]
if not args:
    sys.exit(__doc__)
stamp_set = args.pop(0)
extra = [a for a in args if a.startswith('-')]
rest = [a for a in args if not a.startswith('-')]
wl = rest[0] if rest else 'C2'
nd = int(rest[1]) if len(rest) > 1 else 1
m, gen = workloads.c2(a0=float(os.environ.get('EGDST_DIAG_A0', '0'))) if wl == 'C2' else workloads.WORKLOADS[wl]()
lib = build.build_model(m, extra_flags=['-DEGDST_STAMPS=' + stamp_set] + extra)
s = runtime.Solver(lib, m.descriptor(), ndraw=nd, keep_history=False)
s.set_params(gen(nd) if nd > 1 else m.param_vector()[None])
s.solve(raise_on_error=False)
t = time.perf_counter(); s.solve(raise_on_error=False); dt = time.perf_counter() - t
per = [s.stamps(d) for d in range(nd)]   # (the slots are zeroed when a solve starts: these are the second solve's)
print('%s x %d, stamps %s %s: solve %.2f ms | walks cut and merged / fallen back %s | guard records %d' % (
    wl, nd, stamp_set, ' '.join(extra), dt * 1e3, s.walk_stats().sum(axis=0).tolist(), sum(int(s.debug(d)[0] != 0) for d in range(nd))))
if not any(v for p in per for v in p.values()):
    print('  no stamp of this set was taken (tpsort, tpwalk: is the envelope step on the throughput path?)')
for name in per[0]:
    v = np.array([p[name] for p in per], dtype=np.float64)
    if not v.any():
        continue
    if name == 'seg.onewave_why':
        # (10 bits per reason, per draw)
        print('  %-28s %s' % (name, ', '.join('%s %d' % (w, sum((p[name] >> (10 * k)) & 1023 for p in per)) for k, w in enumerate(WHY))))
    elif name in COUNTERS:
        print('  %-28s %14d' % (name, v.sum()))
    else:
        print('  %-28s %14d ticks %12.3f ms' % (name, v.sum(), v.sum() * 1e-5) +
              ('   per draw: median %.3f ms, max %.3f ms' % (np.median(v) * 1e-5, v.max() * 1e-5) if nd > 1 else ''))
    if os.environ.get('EGDST_DIAG_PER_DRAW'):
        print('      ' + ' '.join('%d' % x for x in v))
