"""Cost of the fit to a resident data panel inside the solve (egdst_attach_panel, egdst_fit_dev) against the kept-history door: C2
(T=60) x 1024 draws, the observations the present pairs of one simulated panel of 2000 agents (120 000), the case of
gpu_policy_fit_time.py.  Warm-up first, then the median of `reps` (argv[1], default 5) per leg; one process is one run.  Legs:
  (a) the parent's way: a kept-history solve, then policy_batch fit-only (reported apart: solve, fit)
  (b) a handle without history: set_params_dev, solve_async, sync -- no panel
  (c) the same handle with the panel attached, fit_dev behind the solve, sync
(c) - (b) is what the fit costs inside the solve; (a)'s fit is what it costs through the door.  Also the device memory of the
tables with and without history (24 B per row of M, C, V: periods x draws x states x row stride), the attach itself, and whether
(c)'s ssr and hits are (a)'s bits.  For k_policy_period's time per launch and the launch counts of a solve with and without a
panel run it under a kernel trace with statistics, a run of its own (reps 1 keeps the trace short; argv[2] = 'nokept' leaves
leg (a) out of it)."""
import json, sys, time
sys.path.insert(0, 'tests'); sys.path.insert(0, '.')  # run from the repo root
import numpy as np
import torch
from egdst_amd import build, datafit, runtime, workloads
from estimation_case import uniforms

ndraw, nsim = 1024, 2000
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
with_kept = 'nokept' not in sys.argv[2:]
m, gen = workloads.c2()
lib = build.build_model(m)
P = gen(ndraw)
out = {'config': 'C2 T=60, %d draws' % ndraw, 'ms': {}}


def timed(name, run, warm=2):
    for _ in range(warm):
        run()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        run()
        ts.append((time.perf_counter() - t) * 1e3)
    out['ms'][name] = {'median': float(np.median(ts)), 'min': float(np.min(ts)), 'max': float(np.max(ts))}
    print(name, out['ms'][name], flush=True)


# the observations: one kept-history solve of the first draw that solves
one = runtime.Solver(lib, m.descriptor(), ndraw=8, keep_history=True)
one.set_params(P[:8])
one.solve(raise_on_error=False)
d0 = int(np.nonzero(one.status()[0] == 0)[0][0])
nt = one.nt
init = np.column_stack([np.ones(nsim), np.random.default_rng(5).uniform(m.a0, m.mmax, nsim)])
obs = datafit.Observations.from_panel(one.simulate(init, uniforms(11, 4 * nt * nsim), 0, draw=d0), lib.info).pack()
one.close()
nobs = len(obs)
out['config'] += ', %d observations (panel of draw %d, %d agents), resid 0' % (nobs, d0, nsim)

ssr = torch.empty(2, ndraw, dtype=torch.float64, device='cuda')
hits = torch.empty(2, ndraw, dtype=torch.int32, device='cuda')
par = torch.from_numpy(np.ascontiguousarray(P)).cuda()
torch.cuda.synchronize()

if with_kept:
    kept = runtime.Solver(lib, m.descriptor(), ndraw=ndraw, keep_history=True)
    kept.set_params(P)
    timed('a_kept_solve', lambda: kept.solve(raise_on_error=False))
    timed('a_policy_fit_only', lambda: kept.policy_batch(obs, ssr_dev=ssr[0].data_ptr(), hits_dev=hits[0].data_ptr()))
    rows_cap, stride = kept.geometry()
    out['table_bytes_kept'] = 24 * nt * ndraw * lib.info.nst * stride
    kept.close()

stream = torch.cuda.Stream()
s = runtime.Solver(lib, m.descriptor(), ndraw=ndraw, keep_history=False, stream=stream.cuda_stream)
rows_cap, stride = s.geometry()
out['table_bytes_no_history'] = 24 * 2 * ndraw * lib.info.nst * stride
out['term_bytes'] = 12 * nobs * ndraw


def solve_only():
    s.set_params_dev(par.data_ptr())
    s.solve_async()
    s.sync(raise_on_error=False)


def solve_and_fit():
    s.set_params_dev(par.data_ptr())
    s.solve_async()
    s.fit_dev(ssr[1].data_ptr(), hits[1].data_ptr())
    s.sync(raise_on_error=False)


timed('b_solve_no_panel', solve_only)
t = time.perf_counter()
s.attach_panel(obs)
out['ms']['attach'] = (time.perf_counter() - t) * 1e3
timed('c_solve_with_panel_and_fit', solve_and_fit)
s.detach_panel()
timed('b_again_after_detach', solve_only)
solved = s.status()[0] == 0
s.close()
out['solved_draws'] = int(solved.sum())
out['fit_inside_the_solve_ms'] = out['ms']['c_solve_with_panel_and_fit']['median'] - out['ms']['b_solve_no_panel']['median']
h_ssr, h_hits = ssr.cpu().numpy(), hits.cpu().numpy()
if with_kept:
    nan = np.isnan(h_ssr[0])
    out['same_bits_as_the_kept_door'] = bool(np.array_equal(nan, np.isnan(h_ssr[1])) and h_ssr[0][~nan].tobytes() == h_ssr[1][~nan].tobytes()
                                             and np.array_equal(h_hits[0], h_hits[1]))
out['own_draw'] = {'ssr': float(h_ssr[1][d0]), 'hits': int(h_hits[1][d0])}
print(json.dumps(out))
