"""Harness build, no sanitizer: the covariance of the moments (egdst_simulate_batch_spec_cov: k_moment_scores, k_moment_cov) on
occ3 draws -- records of kinds 0, 1 and 2 with and without lags and conditions and one nothing satisfies -- against
MomentSpec.covariance(block=1, parts=egdst_cov_parts()) on the oracle's paths for the host replay of the uniforms, and the means
and counts against the step without the covariance.  EMU_EXTRA_FLAGS: -DEG_SIM_SLICE_BYTES=... makes the draws take several
slices once the scores count beside the paths.  Nothing is preloaded."""
import os
import re
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, os.path.join(ROOT, 'tests', 'cpu_emu'))
import numpy as np
import build_emu
from egdst_amd import build, codegen, runtime
from egdst_amd import moments as mo
from oracle_harness import Oracle
import estimation_case
from run_emu_moment_spec import bits_equal
from run_emu_quantiles import occ3_case, flag

NSIM, NDRAW = 48, 4
INF = float('inf')


def cov_tile():
    """COV_T, the records per side of k_moment_cov's tile: the scores of a draw are padded to a multiple of it"""
    text = open(os.path.join(ROOT, 'egdst_amd', 'csrc', 'egdst_kernels.hip')).read()
    return int(re.search(r'^#define COV_T (\d+)', text, flags=re.M).group(1))


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


def write_modelspec(m):
    """the model's directory under egdst_amd/_models with its modelspec.h (left alone when it is already that text)"""
    text = codegen.generate_modelspec(m)
    d = os.path.join(build.MODELS_DIR, build.model_tag(m, text))
    os.makedirs(d, exist_ok=True)
    spec_h = os.path.join(d, 'modelspec.h')
    if not os.path.exists(spec_h) or open(spec_h).read() != text:
        open(spec_h, 'w').write(text)
    return d


if __name__ == '__main__':
    san = os.environ.get('EMU_SANITIZE', '0')
    m = occ3_case()
    lib = runtime.ModelLibrary(build_emu.build(write_modelspec(m), {'0': False}.get(san, san), 1, False, 1))
    rng = np.random.default_rng(4)
    P = m.param_vector()[None] * (1 + 0.15 * rng.uniform(-1, 1, (NDRAW, len(m.param_vector()))))
    s = runtime.Solver(lib, m.descriptor(), ndraw=NDRAW, keep_history=True)
    s.set_params(P)
    s.solve(raise_on_error=False)
    st = s.status()[0]
    init = np.column_stack([np.ones(NSIM), rng.uniform(m.a0, m.mmax, NSIM)])
    spec = cov_spec(s.nt, lib.info)
    rec = spec.pack_lag(s.nt, lib.info)
    nmom = len(spec)
    parts = lib.cov_parts
    bad = []
    if not spec.lagged or (rec['kind'] == 3).any() or sorted(set(rec['kind'])) != [0, 1, 2]:
        bad.append('the spec is not one of kinds 0, 1 and 2 with lags')
    if parts < 1 or parts > 256 or parts & (parts - 1):
        bad.append('egdst_cov_parts() = %d is no power of two in [1, 256]' % parts)
    # the slices of estimation_step, from the arithmetic of the library: paths and padded scores of a draw
    tile = cov_tile()
    per_draw = 8 * lib.nout * s.nt * NSIM + 8 * NSIM * (-(-nmom // tile) * tile)
    slice_ = max(1, min(NDRAW, flag('EG_SIM_SLICE_BYTES', 2 << 30) // per_draw))
    nslices = -(-NDRAW // slice_)
    if 'EG_SIM_SLICE_BYTES' in os.environ.get('EMU_EXTRA_FLAGS', '') and nslices < 2:
        bad.append('EG_SIM_SLICE_BYTES is set but the %d draws take %d slice' % (NDRAW, nslices))
    empty = [j for j, r in enumerate(rec) if r['cond_lo'] == 9]
    orc = Oracle(m)
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
        rs = estimation_case.uniforms(seed, 4 * s.nt * (1 if rndtype == 1 else NSIM))
        for dr in range(NDRAW):
            sol = orc.solve(P[dr])
            if sol.rc != 0:
                if st[dr] == 0 or counts[dr].any() or not np.isnan(means[dr]).all() or not np.isnan(cov[dr]).all():
                    bad.append('rndtype %d draw %d: oracle fails, device status %d' % (rndtype, dr, st[dr]))
                continue
            solved += 1
            ref_m, ref_c, ref_v = spec.covariance(orc.sim(sol, init, rs, rndtype=rndtype, params=P[dr]), block=1, parts=parts)
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
    print('moment covariance: %d moments, %d partials, tile %d, draw status %s' % (nmom, parts, tile, list(st)))
    print('slices: %d' % nslices)
    print('moment covariance problems: %d %s' % (len(bad), bad[:3]))
