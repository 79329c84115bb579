"""Cost of the covariance of the moments (egdst_simulate_batch_spec_cov) over the step without it (egdst_simulate_batch_spec,
moments and counts only) on the same spec: C2 (T=60) x 1024 draws x 2000 agents, the 3T = 180 moments of gpu_moment_spec_time.py,
output buffers allocated once, warm-up first, median of `reps` (argv[1], default 5).  For the split between k_moment_scores and
k_moment_cov run it under a kernel trace with statistics (reps 1 keeps the trace short)."""
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
spec = mo.MomentSpec([mo.share('id', 1, periods=it) for it in range(nt)] + [mo.mean('C', periods=it) for it in range(nt)]
                     + [mo.mean('M', periods=it) for it in range(nt)], layout=s)
nmom = len(spec)
tm = torch.empty(ndraw, nmom, dtype=torch.float64, device='cuda')
tc = torch.empty(ndraw, nmom, dtype=torch.int32, device='cuda')
tv = torch.empty(ndraw, nmom, nmom, dtype=torch.float64, device='cuda')
torch.cuda.synchronize()
legs = {
    'batch_spec_3T': lambda: s.simulate_batch_spec(init, spec, seed=7, means_dev=tm.data_ptr(), counts_dev=tc.data_ptr()),
    'batch_cov_3T': lambda: s.simulate_batch_cov(init, spec, seed=7, means_dev=tm.data_ptr(), counts_dev=tc.data_ptr(),
                                                 cov_dev=tv.data_ptr()),
}
out = {'config': 'C2 T=%d, %d draws, %d agents, %d moments, rndtype 0, generated uniforms' % (nt, ndraw, nsim, nmom), 'ms': {}}
for name, run in legs.items():
    for _ in range(2):
        run()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        run()   # (returns after the handle's stream is synchronised)
        ts.append((time.perf_counter() - t) * 1e3)
    out['ms'][name] = {'median': float(np.median(ts)), 'min': float(np.min(ts)), 'max': float(np.max(ts))}
    print(name, out['ms'][name], flush=True)
solved = s.status()[0] == 0
cov = tv.cpu().numpy()
out['solved_draws'] = int(solved.sum())
out['finite_cov_draws'] = int(np.isfinite(cov).all(axis=(1, 2)).sum())
out['ms']['cov_over_spec'] = out['ms']['batch_cov_3T']['median'] - out['ms']['batch_spec_3T']['median']
print(json.dumps(out))
