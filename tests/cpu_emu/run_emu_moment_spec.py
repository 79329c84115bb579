"""Harness build: the estimation step with user-defined moments and a full weighting matrix (egdst_simulate_batch_spec) on
occ3 draws -- device-generated uniforms, every moment kind, bins, conditions -- against MomentSpec.evaluate(block=1) on the
oracle's paths for the host replay of the same uniforms, and the objective against moments.objective."""
import ctypes as C
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, os.path.join(ROOT, 'tests', 'cpu_emu'))
import numpy as np
import build_emu
from egdst_amd import examples, runtime
from estimation_emu import full_w, write_modelspec
from egdst_amd import moments as mo
from oracle_harness import Oracle
import estimation_case
from estimation_case import bits_equal


def occ3_spec(nt, layout):
    """every kind: sector shares by period, consumption by sector, M*C, a 3-period bin, conditions on a state column"""
    items = [mo.share('id', k, periods=it) for it in range(nt) for k in range(3)]
    items += [mo.mean('C', where=('id', k, k)) for k in range(3)]
    items += [mo.cross('M', 'C'), mo.cross('C', 'C', periods=2), mo.mean('M', periods=(1, 3)),
              mo.mean('C', where=('st1', 0, 0)), mo.mean('A', periods=(2, 4), where=('M', 1.0, 3.0)),
              mo.share('M', 0.5, 2.0), mo.mean('eq1', periods=(1, nt - 1)), mo.cross('eq3', 'id', periods=(0, 3), where=('dc1', 2, 2))]
    return mo.MomentSpec(items, layout=layout)


if __name__ == '__main__':
    san = os.environ.get('EMU_SANITIZE', 'address')
    m = examples.occ3(T=6, ngridm=30, ngridmax=100)
    d = write_modelspec(m)
    lib = runtime.ModelLibrary(build_emu.build(d, {'0': False}.get(san, san), 1, False, 1))
    rng = np.random.default_rng(4)
    P = m.param_vector()[None] * (1 + 0.15 * rng.uniform(-1, 1, (4, len(m.param_vector()))))
    s = runtime.Solver(lib, m.descriptor(), ndraw=len(P), keep_history=True)
    s.set_params(P)
    s.solve(raise_on_error=False)
    st = s.status()[0]
    orc = Oracle(m)
    nsim = 48
    init = np.column_stack([np.ones(nsim), rng.uniform(m.a0, m.mmax, nsim)])
    spec = occ3_spec(s.nt, lib.info)
    nmom = len(spec)
    target = rng.uniform(0, 1, nmom)
    W = full_w(nmom)
    bad = []
    finite = 0
    for rndtype in (0, 1):
        seed = 777 + rndtype
        means = np.zeros((s.ndraw, nmom))
        counts = np.zeros((s.ndraw, nmom), dtype=np.int32)
        obj = np.zeros(s.ndraw)
        s.simulate_batch_spec(init, spec, seed=seed, rndtype=rndtype, target=target, W=W, means_dev=means.ctypes.data,
                              counts_dev=counts.ctypes.data, obj_dev=obj.ctypes.data)
        rs = estimation_case.uniforms(seed, 4 * s.nt * (1 if rndtype == 1 else nsim))
        for dr in range(s.ndraw):
            sol = orc.solve(P[dr])
            if sol.rc != 0:
                if st[dr] == 0 or not np.isnan(obj[dr]) or counts[dr].any() or not np.isnan(means[dr]).all():
                    bad.append('rndtype %d draw %d: oracle fails, device status %d' % (rndtype, dr, st[dr]))
                continue
            ref_m, ref_c = spec.evaluate(orc.sim(sol, init, rs, rndtype=rndtype, params=P[dr]), block=1)
            if not np.array_equal(counts[dr], ref_c):
                bad.append('rndtype %d draw %d: counts differ' % (rndtype, dr))
            if not bits_equal(means[dr], ref_m):
                bad.append('rndtype %d draw %d: means differ' % (rndtype, dr))
            if not bits_equal(obj[dr], mo.objective(ref_m, ref_c, target, W)):
                bad.append('rndtype %d draw %d: objective %r vs %r' % (rndtype, dr, obj[dr], mo.objective(ref_m, ref_c, target, W)))
            finite += int(np.isfinite(obj[dr]))   # (a draw with an empty moment -- nobody in a sector -- has a NaN objective)
    if finite < 4:
        bad.append('only %d finite objectives: the case does not check the quadratic form' % finite)
    # a malformed record is refused before anything runs, and the handle stays usable
    rec = spec.pack(s.nt, lib.info)
    nout = 11 + lib.info.nnst + lib.info.nnd + lib.info.neq
    for field, value in (('kind', 3), ('col', nout), ('col2', -1), ('cond_col', -2), ('it_first', 4), ('it_last', s.nt)):
        r = rec.copy()
        r[field][5] = value
        if field == 'it_first':
            r['it_last'][5] = 3
        out = np.zeros(s.ndraw)
        rc = lib.lib.egdst_simulate_batch_spec(s.h, init.ctypes.data_as(C.POINTER(C.c_double)), nsim, None, 0, 1, 0,
                                               r.ctypes.data_as(C.c_void_p), nmom, target.ctypes.data_as(C.POINTER(C.c_double)),
                                               W.ctypes.data_as(C.POINTER(C.c_double)), None, None, C.c_void_p(out.ctypes.data))
        if rc != 1:
            bad.append('malformed %s = %d: code %d' % (field, value, rc))
    means2 = np.zeros((s.ndraw, nmom))
    counts2 = np.zeros((s.ndraw, nmom), dtype=np.int32)
    s.simulate_batch_spec(init, spec, seed=778, rndtype=1, means_dev=means2.ctypes.data, counts_dev=counts2.ctypes.data)
    if not (bits_equal(means2, means) and np.array_equal(counts2, counts)):
        bad.append('the handle changed after the refused calls')
    print('moment spec: %d moments, draw status %s' % (nmom, list(st)))
    print('moment spec problems: %d %s' % (len(bad), bad[:3]))
