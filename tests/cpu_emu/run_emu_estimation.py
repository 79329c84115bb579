"""Harness build: the on-device estimation step (batch simulation with generated uniforms, moments, objective) of a few
C2-like draws against the oracle fed with the host replay of the same uniforms: within the tolerances of
estimation_case.check, and bit for bit against MomentSpec.evaluate(block=1) and moments.objective on the oracle's paths."""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, os.path.join(ROOT, 'tests', 'cpu_emu'))
import numpy as np
import build_emu
from egdst_amd import runtime, workloads
from estimation_emu import write_modelspec
from egdst_amd import moments as mo
from oracle_harness import Oracle
import estimation_case
from estimation_case import bits_equal


def check_bits(s, orc, P, init, seed, rndtype):
    """simulate_batch_moments against the per-period spec evaluated on the oracle's paths in the device's order (one
    partial: MOM_BS is 1 in this build) and the objective against moments.objective with the weights as a diagonal"""
    nt, nout, nsim = s.nt, s.lib.nout, len(init)
    spec = mo.MomentSpec([mo.mean(c, periods=it) for it in range(nt) for c in range(nout)], layout=s)
    target = np.random.default_rng(3).uniform(0, 2, nt * nout)
    weight = np.zeros((nt, nout))
    weight[1:, 1] = 1.0
    weight[1:, 4] = 4.0
    weight = weight.reshape(-1)
    means = np.zeros((s.ndraw, nt * nout))
    counts = np.zeros((s.ndraw, nt * nout), dtype=np.int32)
    obj = np.zeros(s.ndraw)
    s.simulate_batch_moments(init, seed=seed, rndtype=rndtype, target=target, weight=weight, means_dev=means.ctypes.data,
                             counts_dev=counts.ctypes.data, obj_dev=obj.ctypes.data)
    rs = estimation_case.uniforms(seed, 4 * nt * (1 if rndtype == 1 else nsim))
    bad, solved = [], 0
    for d in range(s.ndraw):
        sol = orc.solve(P[d])
        if sol.rc != 0:
            continue   # (estimation_case.check holds the device to NaN there)
        solved += 1
        rm, rc = spec.evaluate(orc.sim(sol, init, rs, rndtype=rndtype, params=P[d]), block=1)
        if not np.array_equal(counts[d], rc):
            bad.append('rndtype %d draw %d: counts differ from the spec\'s' % (rndtype, d))
        if not bits_equal(means[d], rm):
            bad.append('rndtype %d draw %d: means differ in bits' % (rndtype, d))
        ro = mo.objective(rm, rc, target, weight)
        if not bits_equal(obj[d], ro):
            bad.append('rndtype %d draw %d: objective %r vs %r in bits' % (rndtype, d, obj[d], ro))
    if not solved:
        bad.append('rndtype %d: the oracle solved no draw' % rndtype)
    return bad


if __name__ == '__main__':
    san = os.environ.get('EMU_SANITIZE', 'address')
    m, gen = workloads.c2(a0=0, ngridm=60, T=10, ny=5)
    P = gen(5)
    d = write_modelspec(m)
    lib = runtime.ModelLibrary(build_emu.build(d, {'0': False}.get(san, san), 1, False, 1))
    s = runtime.Solver(lib, m.descriptor(), ndraw=len(P), keep_history=True)
    s.set_params(P)
    s.solve(raise_on_error=False)
    rng = np.random.default_rng(5)
    nsim = 40
    init = np.column_stack([np.ones(nsim), rng.uniform(m.a0 - 0.5, m.mmax + 0.5, nsim)])
    bad = []
    for rndtype in (0, 1):
        bad += estimation_case.check(s, Oracle(m), P, init, seed=12345 + rndtype, rndtype=rndtype, lib=lib)
        bad += check_bits(s, Oracle(m), P, init, seed=12345 + rndtype, rndtype=rndtype)
    print('estimation problems: %d %s' % (len(bad), bad[:3]))
