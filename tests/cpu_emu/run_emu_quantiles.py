"""Harness build, no sanitizer: quantile moments (kind 3, k_quantiles) in the estimation step on occ3 draws -- per period and
pooled, next to the other kinds -- against MomentSpec.evaluate(block=1) on the oracle's paths for the host replay of the
uniforms.  EMU_EXTRA_FLAGS chooses what the build exercises: -DQNT_LDS_KEYS=64 puts the 48 agents of a period into LDS and the
pooled records into the global regime; -DEG_SIM_SLICE_BYTES=... makes the draws take several slices of paths."""
import numpy as np
import estimation_emu as emu
from estimation_emu import NSIM, NDRAW, flag, full_w
from egdst_amd import moments as mo
from estimation_case import bits_equal


def quantile_spec(nt, layout):
    """medians and quartiles by period, pooled and conditional quantiles, a column with ties, and the other kinds between"""
    items = [mo.median('C', periods=it) for it in range(nt)] + [mo.mean('C'), mo.share('id', 1, periods=2)]
    items += [mo.quantile('M', p, periods=it) for it in (0, nt - 1) for p in (0.25, 0.75)]
    items += [mo.quantile('A', 0.1), mo.median('id'), mo.cross('M', 'C'), mo.quantile('V', 0.9, periods=(1, 3)),
              mo.median('C', where=('id', 2, 2)), mo.quantile('eq1', 1 / 3, periods=(1, nt - 1), where=('st1', 0, 0))]
    return mo.MomentSpec(items, layout=layout)


if __name__ == '__main__':
    b = emu.solved_batch()
    lib, s, init, st = b.lib, b.s, b.init, b.st
    spec = quantile_spec(s.nt, lib.info)
    rec = spec.pack(s.nt, lib.info)
    nmom = len(spec)
    bad = []
    # what the build exercises, from the arithmetic of the library (QNT_LDS_KEYS)
    q = lib.quantile_lds_keys
    if q != flag('QNT_LDS_KEYS', 2048):
        bad.append('the library reports QNT_LDS_KEYS = %d' % q)
    cand = NSIM * (rec['it_last'] - rec['it_first'] + 1)[rec['kind'] == 3]
    regimes = (int((cand <= q).sum()), int((cand > q).sum()))
    nslices = emu.slices(b, bad)
    target = b.rng.uniform(0, 1, nmom)
    W = full_w(nmom)
    solved = 0
    for rndtype in (0, 1):
        seed = 321 + rndtype
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
                bad.append('rndtype %d draw %d: counts differ' % (rndtype, dr))
            if not bits_equal(means[dr], ref_m):
                bad.append('rndtype %d draw %d: means differ' % (rndtype, dr))
            if not bits_equal(obj[dr], mo.objective(ref_m, ref_c, target, W)):
                bad.append('rndtype %d draw %d: objective %r vs %r' % (rndtype, dr, obj[dr], mo.objective(ref_m, ref_c, target, W)))
            if not (ref_c[rec['kind'] == 3] > 0).any():
                bad.append('rndtype %d draw %d: every quantile is empty' % (rndtype, dr))
    if solved < 4:
        bad.append('only %d solved (draw, rndtype) pairs' % solved)
    print('quantiles: %d moments, draw status %s' % (nmom, list(st)))
    print('quantile regimes (lds, global): %s  slices: %d' % (regimes, nslices))
    print('quantile problems: %d %s' % (len(bad), bad[:3]))
