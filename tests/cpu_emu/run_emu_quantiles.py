"""Harness build, no sanitizer: quantile moments (kind 3, k_quantiles) in the estimation step on occ3 draws -- per period and
pooled, next to the other kinds -- against MomentSpec.evaluate(block=1) on the oracle's paths for the host replay of the
uniforms.  EMU_EXTRA_FLAGS chooses what the build exercises: -DQNT_LDS_KEYS=64 puts the 48 agents of a period into LDS and the
pooled records into the global regime; -DEG_SIM_SLICE_BYTES=... makes the draws take several slices of paths."""
import os
import re
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, os.path.join(ROOT, 'tests', 'cpu_emu'))
import numpy as np
import build_emu
from egdst_amd import build, codegen, examples, runtime
from egdst_amd import moments as mo
from oracle_harness import Oracle
import estimation_case
from run_emu_moment_spec import bits_equal, full_w

NSIM, NDRAW = 48, 4


def occ3_case():
    return examples.occ3(T=6, ngridm=30, ngridmax=100)


def quantile_spec(nt, layout):
    """medians and quartiles by period, pooled and conditional quantiles, a column with ties, and the other kinds between"""
    items = [mo.median('C', periods=it) for it in range(nt)] + [mo.mean('C'), mo.share('id', 1, periods=2)]
    items += [mo.quantile('M', p, periods=it) for it in (0, nt - 1) for p in (0.25, 0.75)]
    items += [mo.quantile('A', 0.1), mo.median('id'), mo.cross('M', 'C'), mo.quantile('V', 0.9, periods=(1, 3)),
              mo.median('C', where=('id', 2, 2)), mo.quantile('eq1', 1 / 3, periods=(1, nt - 1), where=('st1', 0, 0))]
    return mo.MomentSpec(items, layout=layout)


def flag(name, default):
    m = re.search(r'-D%s=(\d+)' % name, os.environ.get('EMU_EXTRA_FLAGS', ''))
    return int(m.group(1)) if m else default


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
    spec = quantile_spec(s.nt, lib.info)
    rec = spec.pack(s.nt, lib.info)
    nmom = len(spec)
    bad = []
    # what the build exercises, from the arithmetic of the library (QNT_LDS_KEYS; estimation_step's slices)
    q = lib.quantile_lds_keys
    if q != flag('QNT_LDS_KEYS', 2048):
        bad.append('the library reports QNT_LDS_KEYS = %d' % q)
    cand = NSIM * (rec['it_last'] - rec['it_first'] + 1)[rec['kind'] == 3]
    regimes = (int((cand <= q).sum()), int((cand > q).sum()))
    slice_ = max(1, min(NDRAW, flag('EG_SIM_SLICE_BYTES', 2 << 30) // (8 * lib.nout * s.nt * NSIM)))
    nslices = -(-NDRAW // slice_)
    if 'EG_SIM_SLICE_BYTES' in os.environ.get('EMU_EXTRA_FLAGS', '') and nslices < 2:
        bad.append('EG_SIM_SLICE_BYTES is set but the %d draws take %d slice' % (NDRAW, nslices))
    target = rng.uniform(0, 1, nmom)
    W = full_w(nmom)
    orc = Oracle(m)
    solved = 0
    for rndtype in (0, 1):
        seed = 321 + rndtype
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
