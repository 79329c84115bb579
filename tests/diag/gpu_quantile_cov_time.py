"""Cost of quantile records in the covariance of the moments (egdst_simulate_batch_spec_cov with banded kind-3 records:
k_quantiles, k_quantile_band and the kind-3 branch of k_moment_scores): C2 (T=60) x 1024 draws x 2000 agents, output buffers
allocated once, warm-up first, median of `reps` (argv[1], default 5).  Legs: (a) the 3T = 180 moments of gpu_moment_cov_time.py
with Omega; (b) the same with its 60 per-period means of M as banded medians (2000 candidates each: LDS); (c) (a) plus three
banded quantiles pooled over all periods (120 000 candidates each: two selections of eight strided passes).  For the kernels'
own times run it under a kernel trace with statistics (reps 1 keeps the trace short)."""
import json, sys, time
sys.path.insert(0, 'tests'); sys.path.insert(0, '.')  # run from the repo root
import numpy as np
import torch
from egdst_amd import build, runtime, workloads
from egdst_amd import moments as mo

ndraw, nsim = 1024, 2000
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
m, gen = workloads.c2()
s = runtime.Solver(build.build_model(m), m.descriptor(), ndraw=ndraw, keep_history=True)
s.set_params(gen(ndraw))
s.solve(raise_on_error=False)
nt = s.nt
init = np.column_stack([np.ones(nsim), np.random.default_rng(5).uniform(m.a0, m.mmax, nsim)])
h = mo.quantile_bandwidth(0.5, nsim)
shares = [mo.share('id', 1, periods=it) for it in range(nt)] + [mo.mean('C', periods=it) for it in range(nt)]
specs = {
    'a_cov_3T': mo.MomentSpec(shares + [mo.mean('M', periods=it) for it in range(nt)], layout=s),
    'b_cov_60_banded_medians': mo.MomentSpec(shares + [mo.median('M', periods=it, bandwidth=h) for it in range(nt)], layout=s),
    'c_cov_3T_plus_3_pooled': mo.MomentSpec(shares + [mo.mean('M', periods=it) for it in range(nt)]
                                            + [mo.quantile('M', p, bandwidth=mo.quantile_bandwidth(p, nsim * nt)) for p in (0.25, 0.5, 0.75)],
                                            layout=s),
}
nmax = max(len(v) for v in specs.values())
tm = torch.empty(ndraw, nmax, dtype=torch.float64, device='cuda')
tc = torch.empty(ndraw, nmax, dtype=torch.int32, device='cuda')
tv = torch.empty(ndraw, nmax, nmax, dtype=torch.float64, device='cuda')
torch.cuda.synchronize()
out = {'config': 'C2 T=%d, %d draws, %d agents, rndtype 0, generated uniforms, bandwidth %.4f' % (nt, ndraw, nsim, h), 'ms': {},
       'finite_quantile_diagonals': {}}
solved = s.status()[0] == 0
for name, spec in specs.items():
    run = lambda: s.simulate_batch_cov(init, spec, seed=7, means_dev=tm.data_ptr(), counts_dev=tc.data_ptr(), cov_dev=tv.data_ptr())  # noqa: E731
    for _ in range(2):
        run()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        run()   # (returns after the handle's stream is synchronised)
        ts.append((time.perf_counter() - t) * 1e3)
    out['ms'][name] = {'median': float(np.median(ts)), 'min': float(np.min(ts)), 'max': float(np.max(ts)), 'moments': len(spec)}
    n = len(spec)
    quant = np.array([q.kind == 3 for q in spec])
    if quant.any():   # (the buffers are written [ndraw][n][n] from their start)
        cov = tv.flatten()[:ndraw * n * n].reshape(ndraw, n, n).cpu().numpy()
        dg = np.diagonal(cov, axis1=1, axis2=2)[solved][:, quant]
        out['finite_quantile_diagonals'][name] = '%d of %d, %d positive' % (int(np.isfinite(dg).sum()), dg.size, int((dg > 0).sum()))
    print(name, out['ms'][name], flush=True)
out['solved_draws'] = int(solved.sum())
out['ms']['b_minus_a'] = out['ms']['b_cov_60_banded_medians']['median'] - out['ms']['a_cov_3T']['median']
out['ms']['c_minus_a'] = out['ms']['c_cov_3T_plus_3_pooled']['median'] - out['ms']['a_cov_3T']['median']
print(json.dumps(out))
