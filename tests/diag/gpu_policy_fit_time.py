"""Cost of the policy at a data panel's observations (egdst_policy_batch): C2 (T=60) x 1024 draws, the observations the present
pairs of one simulated panel of 2000 agents (120 000), output buffers allocated once, warm-up first, median of `reps` (argv[1],
default 5).  Legs: the predictions alone (cons, id, vf), the predictions with the fit (ssr, hits), the fit alone; and, in the same
process as the scale to read them against, the 3T = 180-record moment step of gpu_moment_spec_time.py.  For the split between
k_policy_obs and k_policy_fit run it under a kernel trace with statistics (reps 1 keeps the trace short)."""
import json, sys, time
sys.path.insert(0, 'tests'); sys.path.insert(0, '.')  # run from the repo root
import numpy as np
import torch
from egdst_amd import build, datafit, runtime, workloads
from egdst_amd import moments as mo
from estimation_case import uniforms

ndraw, nsim = 1024, 2000
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
m, gen = workloads.c2()
s = runtime.Solver(build.build_model(m, extra_flags=sys.argv[2:]), m.descriptor(), ndraw=ndraw, keep_history=True)   # (argv[2:]: build flags of a variant to time)
s.set_params(gen(ndraw))
s.solve(raise_on_error=False)
nt = s.nt
solved = s.status()[0] == 0
d0 = int(np.nonzero(solved)[0][0])
init = np.column_stack([np.ones(nsim), np.random.default_rng(5).uniform(m.a0, m.mmax, nsim)])
panel = s.simulate(init, uniforms(11, 4 * nt * nsim), 0, draw=d0)
obs = datafit.Observations.from_panel(panel, s.lib.info).pack()
nobs = len(obs)
spec = mo.MomentSpec([mo.share('id', 1, periods=it) for it in range(nt)] + [mo.mean('C', periods=it) for it in range(nt)]
                     + [mo.mean('M', periods=it) for it in range(nt)], layout=s)
nmom = len(spec)
tm = torch.empty(ndraw, nmom, dtype=torch.float64, device='cuda')
tc = torch.empty(ndraw, nmom, dtype=torch.int32, device='cuda')
pc = torch.empty(ndraw, nobs, dtype=torch.float64, device='cuda')
pv = torch.empty(ndraw, nobs, dtype=torch.float64, device='cuda')
pi = torch.empty(ndraw, nobs, dtype=torch.int32, device='cuda')
ssr = torch.empty(ndraw, dtype=torch.float64, device='cuda')
hits = torch.empty(ndraw, dtype=torch.int32, device='cuda')
torch.cuda.synchronize()
pred = dict(cons_dev=pc.data_ptr(), id_dev=pi.data_ptr(), vf_dev=pv.data_ptr())
fit = dict(ssr_dev=ssr.data_ptr(), hits_dev=hits.data_ptr())
legs = {
    'batch_spec_3T': lambda: s.simulate_batch_spec(init, spec, seed=7, means_dev=tm.data_ptr(), counts_dev=tc.data_ptr()),
    'policy_predictions': lambda: s.policy_batch(obs, **pred),
    'policy_predictions_fit': lambda: s.policy_batch(obs, **pred, **fit),
    'policy_fit_only': lambda: s.policy_batch(obs, **fit),
}
out = {'config': 'C2 T=%d, %d draws, %d observations (panel of draw %d, %d agents), resid 0' % (nt, ndraw, nobs, d0, nsim), 'ms': {}}
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
out['solved_draws'] = int(solved.sum())
out['evaluations_per_s'] = {k: ndraw * nobs / (out['ms'][k]['median'] * 1e-3) for k in out['ms'] if k.startswith('policy')}
# what the run computed: the panel's own draw reproduces its consumption (ssr 0, every choice hit), failed draws read NaN / -1
h_ssr, h_hits = ssr.cpu().numpy(), hits.cpu().numpy()
out['own_draw'] = {'ssr': float(h_ssr[d0]), 'hits': int(h_hits[d0])}
out['failed_pattern_ok'] = bool(np.isnan(h_ssr[~solved]).all() and (h_hits[~solved] == -1).all() and not np.isnan(h_ssr[solved]).any())
out['solved_draws_with_infinite_ssr'] = int(np.isinf(h_ssr[solved]).sum())   # (an interpolation over two equal M rows: the simulator's inf)
print(json.dumps(out))
