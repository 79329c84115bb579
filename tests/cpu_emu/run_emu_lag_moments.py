"""Harness build, no sanitizer: moments across two periods (egdst_simulate_batch_spec_lag) on occ3 draws -- transitions, lagged
and leading conditions and crosses, quantiles with a lagged condition per period and pooled, next to records without lags --
against MomentSpec.evaluate(block=1) on the oracle's paths for the host replay of the uniforms, and the objective with a full W
against moments.objective.  EMU_EXTRA_FLAGS chooses what the build exercises: -DQNT_LDS_KEYS=64 puts the 48 agents of a period
into LDS and the pooled quantiles into the global regime; -DEG_SIM_SLICE_BYTES=... makes the draws take several slices of
paths.  Nothing is preloaded."""
import numpy as np
import estimation_emu as emu
from estimation_emu import NSIM, NDRAW, flag, full_w
from egdst_amd import moments as mo
from estimation_case import bits_equal

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
    b = emu.solved_batch()
    lib, s, init, st = b.lib, b.s, b.init, b.st
    spec = lag_spec(s.nt, lib.info)
    rec = spec.pack_lag(s.nt, lib.info)
    nmom = len(spec)
    bad = []
    if not spec.lagged:
        bad.append('the spec has no lag')
    # what the build exercises, from the arithmetic of the library (QNT_LDS_KEYS)
    q = lib.quantile_lds_keys
    if q != flag('QNT_LDS_KEYS', 2048):
        bad.append('the library reports QNT_LDS_KEYS = %d' % q)
    lagged_q = (rec['kind'] == 3) & (rec['cond_lag'] != 0)
    cand = NSIM * (rec['it_last'] - rec['it_first'] + 1)[lagged_q]
    regimes = (int((cand <= q).sum()), int((cand > q).sum()))
    nslices = emu.slices(b, bad)
    empty = [j for j, r in enumerate(rec) if r['cond_lo'] == 9]
    target = b.rng.uniform(0, 1, nmom)
    W = full_w(nmom)
    W[empty, :] = 0.0   # (the records nothing satisfies stay out of the objective, which is then finite)
    W[:, empty] = 0.0
    solved = finite = 0
    for rndtype in (0, 1):
        seed = 654 + rndtype
        means = np.zeros((NDRAW, nmom))
        counts = np.zeros((NDRAW, nmom), dtype=np.int32)
        obj = np.zeros(NDRAW)
        s.simulate_batch_spec(init, spec, seed=seed, rndtype=rndtype, target=target, W=W, means_dev=means.ctypes.data,
                              counts_dev=counts.ctypes.data, obj_dev=obj.ctypes.data)
        for dr, sims in emu.oracle_panels(b, seed, rndtype):
            if sims is None:
                if st[dr] == 0 or not np.isnan(obj[dr]) or counts[dr].any() or not np.isnan(means[dr]).all():
                    bad.append('rndtype %d draw %d: oracle fails, device status %d' % (rndtype, dr, st[dr]))
                continue
            solved += 1
            ref_m, ref_c = spec.evaluate(sims, block=1)
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
