"""Timing of the estimation step with quantile moments (kind 3, k_quantiles): C2 (T=60) x 1024 draws x 2000 agents, output
buffers allocated once, warm-up first, median of 5.  Three specs with a full W:
  a  the 180 moments (3 T) that gpu_moment_spec_time.py times: no quantile, so nothing new is launched
  b  the same with its 60 per-period means of M replaced by per-period medians (2000 candidates each: selection in LDS)
  c  a plus three quantiles pooled over all periods (120 000 candidates each: every pass reads the column again)
Run it under a time limit (timeout 600 python tests/diag/gpu_quantile_time.py [a b c])."""
import json, sys, time
sys.path.insert(0, 'tests'); sys.path.insert(0, '.')  # run from the repo root
import numpy as np
import torch
from egdst_amd import build, runtime, workloads
from egdst_amd import moments as mo

ndraw, nsim, reps = 1024, 2000, 5
which = [a for a in sys.argv[1:] if a in ('a', 'b', 'c')] or ['a', 'b', 'c']
m, gen = workloads.c2()
s = runtime.Solver(build.build_model(m), m.descriptor(), ndraw=ndraw, keep_history=True)
s.set_params(gen(ndraw))
s.solve(raise_on_error=False)
nt = s.nt
head = [mo.share('id', 1, periods=it) for it in range(nt)] + [mo.mean('C', periods=it) for it in range(nt)]
specs = {
    'a': head + [mo.mean('M', periods=it) for it in range(nt)],
    'b': head + [mo.median('M', periods=it) for it in range(nt)],
    'c': head + [mo.mean('M', periods=it) for it in range(nt)] + [mo.median('M'), mo.quantile('C', 0.25), mo.quantile('A', 0.9)],
}
init = np.column_stack([np.ones(nsim), np.random.default_rng(5).uniform(m.a0, m.mmax, nsim)])
out = {'config': 'C2 T=%d, %d draws, %d agents, rndtype 0, generated uniforms, QNT_LDS_KEYS %d'
       % (nt, ndraw, nsim, s.lib.quantile_lds_keys), 'ms': {}}
for name in which:
    spec = mo.MomentSpec(specs[name], layout=s)
    nmom = len(spec)
    a = np.random.default_rng(1).normal(size=(nmom, nmom))
    W = a @ a.T / nmom
    tm = torch.empty(ndraw, nmom, dtype=torch.float64, device='cuda')
    tc = torch.empty(ndraw, nmom, dtype=torch.int32, device='cuda')
    to = torch.empty(ndraw, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    ptrs = dict(means_dev=tm.data_ptr(), counts_dev=tc.data_ptr(), obj_dev=to.data_ptr())
    target = np.zeros(nmom)
    for _ in range(2):
        s.simulate_batch_spec(init, spec, seed=7, target=target, W=W, **ptrs)
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        s.simulate_batch_spec(init, spec, seed=7, target=target, W=W, **ptrs)   # (returns after the handle's stream is synchronised)
        ts.append((time.perf_counter() - t) * 1e3)
    nq = int((spec.pack(nt, s.lib.info)['kind'] == 3).sum())
    out['ms'][name] = {'nmom': nmom, 'quantiles': nq, 'median': float(np.median(ts)), 'min': float(np.min(ts)), 'max': float(np.max(ts)),
                       'empty_quantiles': int((tc.cpu().numpy()[:, -nq:] == 0).sum()) if nq else 0}
    print(name, out['ms'][name], flush=True)
print(json.dumps(out))
