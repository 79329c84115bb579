"""Harness build, no sanitizer: the covariance of the moments (egdst_simulate_batch_spec_cov: k_moment_scores, k_moment_cov) on
occ3 draws -- records of kinds 0, 1 and 2 with and without lags and conditions and one nothing satisfies -- against
MomentSpec.covariance(block=1, parts=egdst_cov_parts()) on the oracle's paths for the host replay of the uniforms, and the means
and counts against the step without the covariance.  EMU_EXTRA_FLAGS: -DEG_SIM_SLICE_BYTES=... makes the draws take several
slices once the scores count beside the paths.  Nothing is preloaded."""
import numpy as np
import estimation_emu as emu
from estimation_emu import NDRAW, cov_tile
from egdst_amd import moments as mo
from estimation_case import bits_equal

INF = float('inf')


def cov_spec(nt, layout):
    """the records of run_emu_lag_moments.lag_spec without its quantiles: 9 pooled transitions, hazards by period, crosses a
    period back, a period ahead and nt - 1 back, conditions that lead, a record nothing satisfies, and records without lags"""
    items = [mo.transition('id', a, b) for a in range(3) for b in range(3)]
    items += [mo.transition('id', 0, 1, periods=it) for it in range(1, nt)]
    items += [mo.cross('C', 'C', lag=1), mo.cross('M', 'A', lag=1), mo.cross('C', 'M', periods=(2, 4), lag=-1),
              mo.cross('M', 'M', periods=nt - 1, lag=nt - 1), mo.cross('C', 'eq1', lag=2, where=('st1', 0, 0, -1)),
              mo.mean('C', periods=(1, nt - 2), where=('id', 2, 2, -1)), mo.mean('C', periods=(0, nt - 2), where=('C', -INF, INF, -1)),
              mo.share('M', 0.5, 2.0, where=('id', 1, 2, 2)),
              mo.mean('C', where=('id', 9, 9, 1)),
              mo.mean('C'), mo.share('id', 1, periods=2), mo.cross('M', 'C')]
    return mo.MomentSpec(items, layout=layout)


if __name__ == '__main__':
    b = emu.solved_batch()
    lib, s, init, st = b.lib, b.s, b.init, b.st
    spec = cov_spec(s.nt, lib.info)
    rec = spec.pack_lag(s.nt, lib.info)
    nmom = len(spec)
    parts = lib.cov_parts
    bad = []
    if not spec.lagged or (rec['kind'] == 3).any() or sorted(set(rec['kind'])) != [0, 1, 2]:
        bad.append('the spec is not one of kinds 0, 1 and 2 with lags')
    if parts < 1 or parts > 256 or parts & (parts - 1):
        bad.append('egdst_cov_parts() = %d is no power of two in [1, 256]' % parts)
    nslices = emu.slices(b, bad, scores=nmom)   # (paths and padded scores of a draw)
    empty = [j for j, r in enumerate(rec) if r['cond_lo'] == 9]
    solved = 0
    for rndtype in (0, 1):
        seed = 654 + rndtype
        means = np.zeros((NDRAW, nmom))
        counts = np.zeros((NDRAW, nmom), dtype=np.int32)
        cov = np.zeros((NDRAW, nmom, nmom))
        s.simulate_batch_cov(init, spec, seed=seed, rndtype=rndtype, means_dev=means.ctypes.data, counts_dev=counts.ctypes.data,
                             cov_dev=cov.ctypes.data)
        m2 = np.zeros((NDRAW, nmom))
        c2 = np.zeros((NDRAW, nmom), dtype=np.int32)
        s.simulate_batch_spec(init, spec, seed=seed, rndtype=rndtype, means_dev=m2.ctypes.data, counts_dev=c2.ctypes.data)
        if not (bits_equal(means, m2) and np.array_equal(counts, c2)):
            bad.append('rndtype %d: means or counts differ from the step without the covariance' % rndtype)
        for dr, sims in emu.oracle_panels(b, seed, rndtype):
            if sims is None:
                if st[dr] == 0 or counts[dr].any() or not np.isnan(means[dr]).all() or not np.isnan(cov[dr]).all():
                    bad.append('rndtype %d draw %d: oracle fails, device status %d' % (rndtype, dr, st[dr]))
                continue
            solved += 1
            ref_m, ref_c, ref_v = spec.covariance(sims, block=1, parts=parts)
            if not np.array_equal(counts[dr], ref_c) or not bits_equal(means[dr], ref_m):
                bad.append('rndtype %d draw %d: means or counts differ' % (rndtype, dr))
            if not bits_equal(cov[dr], ref_v):
                where = np.argwhere(~((cov[dr] == ref_v) | (np.isnan(cov[dr]) & np.isnan(ref_v))))
                bad.append('rndtype %d draw %d: covariance differs at %s' % (rndtype, dr, where[:3].tolist()))
            nan = ref_c == 0
            if not np.array_equal(np.isnan(cov[dr]), nan[:, None] | nan[None, :]) or not nan[empty].all():
                bad.append('rndtype %d draw %d: NaN is not exactly the rows and columns of the empty moments' % (rndtype, dr))
            if not np.array_equal(cov[dr].view(np.int64), cov[dr].T.view(np.int64)):
                bad.append('rndtype %d draw %d: the mirror entries differ in bits' % (rndtype, dr))
    if solved < 4:
        bad.append('only %d solved (draw, rndtype) pairs' % solved)
    print('moment covariance: %d moments, %d partials, tile %d, draw status %s' % (nmom, parts, cov_tile(), list(st)))
    print('slices: %d' % nslices)
    print('moment covariance problems: %d %s' % (len(bad), bad[:3]))
