"""Harness build, no sanitizer: quantile records in the covariance of the moments (egdst_simulate_batch_spec_cov with kind-3
records that carry a bandwidth: k_quantiles, k_quantile_band, k_moment_scores, k_moment_cov) on occ3 draws -- banded quantiles per
period, pooled, with a lagged condition, on the tied choice column and one nothing satisfies, next to the records of
run_emu_moment_cov -- against MomentSpec.covariance(block=1, parts=egdst_cov_parts()) on the oracle's paths for the host replay of
the uniforms; the means and counts against the step without the covariance, on the same records and on the records without
their bandwidth; and k_quantile_band alone (egdst_quantile_band_eval) against moments.quantile_band on arrays on both sides of
the library's QNT_LDS_KEYS.  EMU_EXTRA_FLAGS chooses what the build exercises: -DQNT_LDS_KEYS=64 puts the 48 agents of a period into LDS and
the pooled records into the global regime; -DEG_SIM_SLICE_BYTES=... makes the draws take several slices.  Nothing is preloaded."""
import numpy as np
import estimation_emu as emu
from estimation_emu import NSIM, NDRAW, cov_tile, flag
from egdst_amd import moments as mo
from estimation_case import bits_equal
from run_emu_moment_cov import cov_spec


def quantile_cov_spec(nt, layout):
    """the records of run_emu_moment_cov.cov_spec with banded quantiles between and behind them"""
    items = list(cov_spec(nt, layout))
    items[3:3] = [mo.median('M', periods=it, bandwidth=0.2) for it in range(nt)]
    items += [mo.quantile('C', 0.25, bandwidth=0.1), mo.quantile('A', 0.9, periods=(1, 3), bandwidth=0.05),
              mo.quantile('M', 0.75, periods=(1, nt - 1), where=('id', 0, 1, 1), bandwidth=0.2),
              mo.median('id', bandwidth=0.05), mo.median('V', where=('id', 9, 9), bandwidth=0.25),
              mo.mean('M', periods=1)]
    return mo.MomentSpec(items, layout=layout)


if __name__ == '__main__':
    b = emu.solved_batch()
    lib, s, init, st = b.lib, b.s, b.init, b.st
    spec = quantile_cov_spec(s.nt, lib.info)
    rec = spec.pack_lag(s.nt, lib.info)
    nmom = len(spec)
    parts = lib.cov_parts
    bad = []
    quant = rec['kind'] == 3
    if not quant.any() or (rec['hi'][quant] <= 0).any() or sorted(set(rec['kind'])) != [0, 1, 2, 3]:
        bad.append('the spec is not one of kinds 0-3 with a bandwidth on every quantile')
    q = lib.quantile_lds_keys
    if q != flag('QNT_LDS_KEYS', 2048):
        bad.append('the library reports QNT_LDS_KEYS = %d' % q)
    cand = NSIM * (rec['it_last'] - rec['it_first'] + 1)[quant]
    regimes = (int((cand <= q).sum()), int((cand > q).sum()))
    nslices = emu.slices(b, bad, scores=nmom)
    plain = rec.copy()
    plain['hi'][quant] = 0.0
    solved = 0
    for rndtype in (0, 1):
        seed = 777 + rndtype
        means = np.zeros((NDRAW, nmom))
        counts = np.zeros((NDRAW, nmom), dtype=np.int32)
        cov = np.zeros((NDRAW, nmom, nmom))
        s.simulate_batch_cov(init, spec, seed=seed, rndtype=rndtype, means_dev=means.ctypes.data, counts_dev=counts.ctypes.data,
                             cov_dev=cov.ctypes.data)
        for records in (rec, plain):   # the other door does not read the bandwidth
            m2 = np.zeros((NDRAW, nmom))
            c2 = np.zeros((NDRAW, nmom), dtype=np.int32)
            s.simulate_batch_spec(init, records, seed=seed, rndtype=rndtype, means_dev=m2.ctypes.data, counts_dev=c2.ctypes.data)
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
            nan = np.isnan(spec.scores(sims, block=1)[2]).any(axis=0)   # the records the mirror makes NaN
            if not np.array_equal(np.isnan(cov[dr]), nan[:, None] | nan[None, :]) or not nan[ref_c == 0].all():
                bad.append('rndtype %d draw %d: NaN is not exactly the rows and columns of the mirror\'s NaN records' % (rndtype, dr))
            if not np.array_equal(np.nan_to_num(cov[dr]).view(np.int64), np.nan_to_num(cov[dr].T).view(np.int64)):
                bad.append('rndtype %d draw %d: the mirror entries differ in bits' % (rndtype, dr))
            live = quant & ~nan
            if not (live.any() and (np.diag(ref_v)[live] > 0).any() and np.isfinite(ref_v[np.ix_(live, ~nan)]).all()):
                bad.append('rndtype %d draw %d: no quantile row is finite with a positive diagonal' % (rndtype, dr))
    if solved < 4:
        bad.append('only %d solved (draw, rndtype) pairs' % solved)
    # the kernel alone (egdst_quantile_band_eval) on both sides of the library's threshold: ties, NaNs, signed zeros, infinities
    x = b.rng.normal(size=q + 37)
    x[::7], x[3], x[4], x[5], x[6], x[8:11] = np.nan, -0.0, 0.0, -np.inf, np.inf, 1.25
    bands = [(0.5, 0.25), (0.1, 0.05), (0.9, 0.09), (0.5, float(np.nextafter(1, 0)) - 0.5), (0.25, 2.0 ** -60)]
    for xs in (x[:1], x[:40], x[:q], x, np.full(9, np.nan)):
        got, count = lib.quantile_band_eval(xs, [p for p, _ in bands], [h for _, h in bands])
        want = np.array([mo.quantile_band(xs, p, h) for p, h in bands])
        if count != int((~np.isnan(xs)).sum()) or not bits_equal(got, want):
            bad.append('quantile_band_eval on %d values differs from moments.quantile_band' % len(xs))
    print('quantile covariance: %d moments, %d quantiles, %d partials, tile %d, draw status %s'
          % (nmom, int(quant.sum()), parts, cov_tile(), list(st)))
    print('quantile regimes (lds, global): %s  slices: %d' % (regimes, nslices))
    print('quantile covariance problems: %d %s' % (len(bad), bad[:3]))
