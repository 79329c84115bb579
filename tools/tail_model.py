"""What would shorten the tail launch of a C2 batch's envelope step, modelled from the device census (-DEGDST_CENSUS build).

A (group, period) tail launch lasts as long as its slowest leftover cell.  From the census records of one solve -- kind 2, a
leftover cell; kind 1, a sort + walk job of such a cell -- this prints, per chain (draw group), the sum over the periods of
  * the slowest cell as it is;
  * the same with every counted sort (a stream out of order that took the quadratic counting ranks) costing the median network sort;
  * the same with every split-eligible cell (deferral reasons 5 and 7 by default) shortened by min(job 0, job 1), the shorter of
    its two secondary envelopes, as if they ran on workgroups of their own;
  * both together.
The records carry (draw, period) but not the state, so a cell's jobs are those of its (draw, period); where two leftover cells share
one, the jobs go to the longer cell (the count of such pairs is printed).

   python tools/tail_model.py [a0=-5] [ndraw=4096] [split reasons=5,7]
"""
import ctypes as C
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np
from egdst_amd import build, runtime, workloads

a0 = float(sys.argv[1]) if len(sys.argv) > 1 else -5.0
nd = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
reasons = [int(x) for x in (sys.argv[3] if len(sys.argv) > 3 else '5,7').split(',')]
m = workloads.c2(a0=a0)[0]
P = workloads.c2(a0=0)[1](nd)
lib = build.build_model(m, extra_flags=workloads.BATCH_BUILD_FLAGS['C2'] + ['-DEGDST_CENSUS'])
L = lib.lib
L.egdst_census_read.argtypes = [C.c_void_p, C.c_int, C.c_int]
s = runtime.Solver(lib, m.descriptor(), ndraw=nd, keep_history=False)
s.set_params(P)
s.solve(raise_on_error=False)
L.egdst_census_read(None, 0, 1)
s.solve(raise_on_error=False)
cap = 1 << 20
buf = np.zeros((cap, 8), dtype=np.int32)
n = L.egdst_census_read(buf.ctypes.data, cap, 1)
rec = buf[:min(n, cap)]
ng = s.schedule()[0]
s.close()

us = 0.01  # ticks of 10 ns
cells, jobs = rec[rec[:, 0] == 2], rec[rec[:, 0] == 1]
bad, sort_us = (jobs[:, 6] >> 20) & 15, (jobs[:, 6] & 0xfffff).astype(float)
lds = (jobs[:, 5] >> 16) == 0
net = np.median(sort_us[(bad == 1) & lds]) if ((bad == 1) & lds).any() else 0.0
print('C2 a0=%g ndraw=%d, %d groups: %d leftover cells, %d jobs; LDS sorts in order %d, network %d (median %.0f us), counted %d (median %.0f us)' % (
    a0, nd, ng, len(cells), len(jobs), int(((bad == 0) & lds).sum()), int(((bad == 1) & lds).sum()), net, int(((bad >= 2) & lds).sum()),
    np.median(sort_us[(bad >= 2) & lds]) if ((bad >= 2) & lds).any() else 0.0))
# per (draw, period): what the counted sorts cost beyond a network sort, and the two secondary envelopes
save_sort, sec = {}, {}
for j, b_, su in zip(jobs, bad, sort_us):
    key = (int(j[1]), int(j[2]))
    if b_ >= 2 and (j[5] >> 16) == 0:
        save_sort[key] = save_sort.get(key, 0.0) + max(0.0, su - net)
    if j[3] < 2:
        sec.setdefault(key, {})[int(j[3])] = j[7] * us
grp = np.searchsorted(np.arange(ng + 1) * nd // ng, cells[:, 1], side='right') - 1
order = np.argsort(-cells[:, 7], kind='stable')   # the longer cell of a (draw, period) first: it gets the jobs
seen, shared = set(), 0
now = np.zeros((ng, int(cells[:, 2].max()) + 1 if len(cells) else 1))
m_sort, m_split, m_both = now.copy(), now.copy(), now.copy()
nsplit = 0
for i in order:
    c = cells[i]
    key, g, it, t = (int(c[1]), int(c[2])), grp[i], int(c[2]), c[7] * us
    first = key not in seen
    shared += not first
    seen.add(key)
    ds = save_sort.get(key, 0.0) if first else 0.0
    dp = 0.0
    if first and int(c[6]) in reasons and len(sec.get(key, {})) == 2:
        dp = min(sec[key].values())
        nsplit += 1
    now[g, it] = max(now[g, it], t)
    m_sort[g, it] = max(m_sort[g, it], t - ds)
    m_split[g, it] = max(m_split[g, it], t - dp)
    m_both[g, it] = max(m_both[g, it], t - ds - dp)
print('cells that share a (draw, period) with a longer one: %d; split-eligible cells (reasons %s, both secondary jobs ran): %d' % (shared, reasons, nsplit))
print('per chain, sum over the periods of the slowest leftover cell (ms):')
print('  group      now   sorts by network   (saves)   split   (saves)    both   (saves)')
for g in range(ng):
    a, b_, c_, d = now[g].sum() / 1e3, m_sort[g].sum() / 1e3, m_split[g].sum() / 1e3, m_both[g].sum() / 1e3
    print('  %5d  %7.2f  %17.2f  %8.2f  %6.2f  %8.2f  %6.2f  %8.2f' % (g, a, b_, a - b_, c_, a - c_, d, a - d))
launches = now > 0
print('launches with a leftover cell: %d; slowest cell median %.0f us, p90 %.0f us' % (int(launches.sum()), np.median(now[launches]), np.percentile(now[launches], 90)))
