"""Timing of the estimation step with user-defined moments (egdst_simulate_batch_spec) against the per-period path
(egdst_simulate_batch_moments): C2 (T=60) x 1024 draws x 2000 agents, output buffers allocated once, warm-up first."""
import json, sys, time
sys.path.insert(0, 'tests'); sys.path.insert(0, '.')  # run from the repo root
import numpy as np
import torch
from egdst_amd import build, runtime, workloads
from egdst_amd import moments as mo

ndraw, nsim, reps = 1024, 2000, 5
m, gen = workloads.c2()
s = runtime.Solver(build.build_model(m), m.descriptor(), ndraw=ndraw, keep_history=True)
s.set_params(gen(ndraw))
s.solve(raise_on_error=False)
nt, info = s.nt, s.lib.info
nout = 11 + info.nnst + info.nnd + info.neq
init = np.column_stack([np.ones(nsim), np.random.default_rng(5).uniform(m.a0, m.mmax, nsim)])
per = mo.MomentSpec([mo.mean(c, periods=it) for it in range(nt) for c in range(nout)], layout=s)
occ = mo.MomentSpec([mo.share('id', 1, periods=it) for it in range(nt)] + [mo.mean('C', periods=it) for it in range(nt)]
                    + [mo.mean('M', periods=it) for it in range(nt)], layout=s)
a = np.random.default_rng(1).normal(size=(len(occ), len(occ)))
legs = {
    'batch_moments_per_period': (None, np.ones(nout * nt)),
    'batch_spec_per_period_diagW': (per, np.ones(len(per))),
    'batch_spec_3T_fullW': (occ, a @ a.T / len(occ)),
}
out = {'config': 'C2 T=%d, %d draws, %d agents, rndtype 0, generated uniforms' % (nt, ndraw, nsim), 'ms': {}}
for name, (spec, W) in legs.items():
    nmom = nout * nt if spec is None else len(spec)
    tm = torch.empty(ndraw, nmom, dtype=torch.float64, device='cuda')
    tc = torch.empty(ndraw, nmom, dtype=torch.int32, device='cuda')
    to = torch.empty(ndraw, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    ptrs = dict(means_dev=tm.data_ptr(), counts_dev=tc.data_ptr(), obj_dev=to.data_ptr())
    target = np.zeros(nmom)

    def run():
        if spec is None:
            s.simulate_batch_moments(init, seed=7, target=target, weight=W, **ptrs)
        else:
            s.simulate_batch_spec(init, spec, seed=7, target=target, W=W, **ptrs)
    for _ in range(2):
        run()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        run()   # (returns after the handle's stream is synchronised)
        ts.append((time.perf_counter() - t) * 1e3)
    out['ms'][name] = {'nmom': nmom, 'median': float(np.median(ts)), 'min': float(np.min(ts)), 'max': float(np.max(ts))}
    print(name, out['ms'][name], flush=True)
print(json.dumps(out))
