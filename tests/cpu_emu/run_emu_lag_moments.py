"""Harness build, no sanitizer: moments across two periods (egdst_simulate_batch_spec_lag) on occ3 draws -- transitions, lagged
and leading conditions and crosses, quantiles with a lagged condition per period and pooled, next to records without lags --
against MomentSpec.evaluate(block=1) on the oracle's paths for the host replay of the uniforms, and the objective with a full W
against moments.objective.  EMU_EXTRA_FLAGS chooses what the build exercises: -DQNT_LDS_KEYS=64 puts the 48 agents of a period
into LDS and the pooled quantiles into the global regime; -DEG_SIM_SLICE_BYTES=... makes the draws take several slices of
paths.  Nothing is preloaded."""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, os.path.join(ROOT, 'tests', 'cpu_emu'))
import numpy as np
import build_emu
from egdst_amd import build, codegen, runtime
from egdst_amd import moments as mo
from oracle_harness import Oracle
import estimation_case
from run_emu_moment_spec import bits_equal, full_w
from run_emu_quantiles import occ3_case, flag

NSIM, NDRAW = 48, 4
INF = float('inf')


def lag_spec(nt, layout):
    """every kind with and without lags: the 9 pooled transitions of the sector, hazards by period, crosses a period back, a
    period ahead and nt - 1 back, means of those about to move and of the survivors, quantiles with a lagged condition per
    period (the LDS regime under QNT_LDS_KEYS=64) and pooled (the global one), and a record nothing satisfies"""
    items = [mo.transition('id', a, b) for a in range(3) for b in range(3)]
    items += [mo.transition('id', 0, 1, periods=it) for it in range(1, nt)]
    items += [mo.cross('C', 'C', lag=1), mo.cross('M', 'A', lag=1), mo.cross('C', 'M', periods=(2, 4), lag=-1),
              mo.cross('M', 'M', periods=nt - 1, lag=nt - 1), mo.cross('C', 'eq1', lag=2, where=('st1', 0, 0, -1)),
              mo.mean('C', periods=(1, nt - 2), where=('id', 2, 2, -1)), mo.mean('C', periods=(0, nt - 2), where=('C', -INF, INF, -1)),
              mo.share('M', 0.5, 2.0, where=('id', 1, 2, 2))]
    items += [mo.median('M', periods=it, where=('id', 0, 1, 1)) for it in (1, 3, nt - 1)]
    items += [mo.quantile('C', 0.9, periods=(2, 4), where=('id', 0, 2, 2)), mo.quantile('A', 0.25, where=('st1', 0, 0, -1)),
              mo.mean('C', where=('id', 9, 9, 1)), mo.median('C', where=('id', 9, 9, -1)),
              mo.mean('C'), mo.share('id', 1, periods=2), mo.cross('M', 'C'), mo.median('M', periods=2)]
    return mo.MomentSpec(items, layout=layout)


if __name__ == '__main__':
    san = os.environ.get('EMU_SANITIZE', '0')
    m = occ3_case()
    text = codegen.generate_modelspec(m)
    d = os.path.join(build.MODELS_DIR, build.model_tag(m, text))
    os.makedirs(d, exist_ok=True)
    open(os.path.join(d, 'modelspec.h'), 'w').write(text)
    lib = runtime.ModelLibrary(build_emu.build(d, {'0': False}.get(san, san), 1, False, 1))
    rng = np.random.default_rng(4)
    P = m.param_vector()[None] * (1 + 0.15 * rng.uniform(-1, 1, (NDRAW, len(m.param_vector()))))
    s = runtime.Solver(lib, m.descriptor(), ndraw=NDRAW, keep_history=True)
    s.set_params(P)
    s.solve(raise_on_error=False)
    st = s.status()[0]
    init = np.column_stack([np.ones(NSIM), rng.uniform(m.a0, m.mmax, NSIM)])
    spec = lag_spec(s.nt, lib.info)
    rec = spec.pack_lag(s.nt, lib.info)
    nmom = len(spec)
    bad = []
    if not spec.lagged:
        bad.append('the spec has no lag')
    # what the build exercises, from the arithmetic of the library (QNT_LDS_KEYS; estimation_step's slices)
    q = lib.quantile_lds_keys
    if q != flag('QNT_LDS_KEYS', 2048):
        bad.append('the library reports QNT_LDS_KEYS = %d' % q)
    lagged_q = (rec['kind'] == 3) & (rec['cond_lag'] != 0)
    cand = NSIM * (rec['it_last'] - rec['it_first'] + 1)[lagged_q]
    regimes = (int((cand <= q).sum()), int((cand > q).sum()))
    slice_ = max(1, min(NDRAW, flag('EG_SIM_SLICE_BYTES', 2 << 30) // (8 * lib.nout * s.nt * NSIM)))
    nslices = -(-NDRAW // slice_)
    if 'EG_SIM_SLICE_BYTES' in os.environ.get('EMU_EXTRA_FLAGS', '') and nslices < 2:
        bad.append('EG_SIM_SLICE_BYTES is set but the %d draws take %d slice' % (NDRAW, nslices))
    empty = [j for j, r in enumerate(rec) if r['cond_lo'] == 9]
    target = rng.uniform(0, 1, nmom)
    W = full_w(nmom)
    W[empty, :] = 0.0   # (the records nothing satisfies stay out of the objective, which is then finite)
    W[:, empty] = 0.0
    orc = Oracle(m)
    solved = finite = 0
    for rndtype in (0, 1):
        seed = 654 + rndtype
        means = np.zeros((NDRAW, nmom))
        counts = np.zeros((NDRAW, nmom), dtype=np.int32)
        obj = np.zeros(NDRAW)
        s.simulate_batch_spec(init, spec, seed=seed, rndtype=rndtype, target=target, W=W, means_dev=means.ctypes.data,
                              counts_dev=counts.ctypes.data, obj_dev=obj.ctypes.data)
        rs = estimation_case.uniforms(seed, 4 * s.nt * (1 if rndtype == 1 else NSIM))
        for dr in range(NDRAW):
            sol = orc.solve(P[dr])
            if sol.rc != 0:
                if st[dr] == 0 or not np.isnan(obj[dr]) or counts[dr].any() or not np.isnan(means[dr]).all():
                    bad.append('rndtype %d draw %d: oracle fails, device status %d' % (rndtype, dr, st[dr]))
                continue
            solved += 1
            ref_m, ref_c = spec.evaluate(orc.sim(sol, init, rs, rndtype=rndtype, params=P[dr]), block=1)
            if not np.array_equal(counts[dr], ref_c):
                bad.append('rndtype %d draw %d: counts differ at %s' % (rndtype, dr, np.nonzero(counts[dr] != ref_c)[0][:5]))
            if not bits_equal(means[dr], ref_m):
                bad.append('rndtype %d draw %d: means differ' % (rndtype, dr))
            ref_o = mo.objective(ref_m, ref_c, target, W)
            if not bits_equal(obj[dr], ref_o):
                bad.append('rndtype %d draw %d: objective %r vs %r' % (rndtype, dr, obj[dr], ref_o))
            finite += int(np.isfinite(ref_o))
            if ref_c[empty].any() or not (ref_c[lagged_q & (rec['cond_lo'] != 9)] > 0).all():
                bad.append('rndtype %d draw %d: the empty records count, or a lagged quantile is empty' % (rndtype, dr))
    if solved < 4:
        bad.append('only %d solved (draw, rndtype) pairs' % solved)
    if finite < 2:
        bad.append('only %d finite objectives: the case does not check the quadratic form' % finite)
    print('lag moments: %d moments, draw status %s' % (nmom, list(st)))
    print('lagged quantile regimes (lds, global): %s  slices: %d' % (regimes, nslices))
    print('lag moment problems: %d %s' % (len(bad), bad[:3]))
