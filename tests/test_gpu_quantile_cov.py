"""Quantile records in the covariance of the simulated moments on the device (egdst_simulate_batch_spec_cov with kind-3 records
that carry a bandwidth: k_quantile_band, the kind-3 branch of k_moment_scores) against MomentSpec.covariance on the oracle's
paths for the host replay of the uniforms, bit for bit; and k_quantile_band alone through egdst_quantile_band_eval against
moments.quantile_band.  The models, the 8 perturbed draws, the 700 agents and the oracle's panels are those of
tests/test_gpu_lag_moments.py (its cached case is shared): the 700 candidates of a per-period quantile are selected in LDS, the
28 700 (occ3) or 17 500 (retirement_mortal) of one pooled over every period from global memory."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (first: the model libraries then bind torch's HIP runtime, which the result tensors need)

from egdst_amd import build, examples, runtime
from egdst_amd import moments as mo
from oracle_harness import Oracle
import estimation_case
from estimation_case import bits_equal
from test_gpu_lag_moments import NDRAW, NSIM, SEED, MODELS, _case
from test_gpu_moment_cov import COV_T, _c2_case, _spec_a
from test_quantile_cov import BANDS, SETS, special_values

pytestmark = pytest.mark.gpu

H = mo.quantile_bandwidth(0.5, NSIM)      # Bofinger's bandwidth for the median of 700 values
PERIODS = (0, 3, 5, 9, 12)                # the per-period medians of spec A


def _banded(name):
    """spec A of the covariance test and, behind it: per-period medians of M, a quantile of C pooled over every period, one with
    a condition two periods back, the median of the choice column, and one nothing satisfies.  (spec, positions by name)"""
    m, s = _case(name)[:2]
    nch = s.lib.info.nd
    spec_a, empty_a, _ = _spec_a(name)
    base = len(spec_a)
    items = list(spec_a) + [mo.median('M', periods=it, bandwidth=H) for it in PERIODS]
    ix = dict(empty_a=empty_a, per_period=range(base, base + len(PERIODS)), pooled=len(items), lagged=len(items) + 1,
              tied=len(items) + 2, empty=len(items) + 3)
    items += [mo.quantile('C', 0.25, bandwidth=0.05),
              mo.quantile('C', 0.9, periods=(4, 6), where=('id', 1, nch - 1, 2), bandwidth=0.05),
              mo.median('id', bandwidth=0.01),
              mo.median('C', where=('id', 9, 9, 1), bandwidth=0.1)]
    return mo.MomentSpec(items, layout=m), ix


def _mirror(spec, panel, parts):
    """(means, counts, cov, nan): the mirror's covariance and the records whose scores it makes NaN"""
    rm, rc, rv = spec.covariance(panel, block=256, parts=parts)
    nan = np.isnan(spec.scores(panel, block=256)[2]).any(axis=0)
    return rm, rc, rv, nan


def _check_draw(cov, means, counts, ref):
    """one draw against the mirror: equal bits; the mirror entries equal in bits; NaN exactly on the rows and columns of the
    records the mirror makes NaN"""
    rm, rc, rv, nan = ref
    assert np.array_equal(counts, rc), np.nonzero(counts != rc)[0]
    assert bits_equal(means, rm)
    assert bits_equal(cov, rv), np.argwhere(~((cov == rv) | (np.isnan(cov) & np.isnan(rv))))[:5]
    assert np.array_equal(np.isnan(cov), np.isnan(cov.T))
    assert np.array_equal(np.nan_to_num(cov).view(np.int64), np.nan_to_num(cov.T).view(np.int64))
    assert np.array_equal(np.isnan(cov), nan[:, None] | nan[None, :])
    assert nan[rc == 0].all()


@pytest.mark.parametrize('rndtype', [0, 1])
@pytest.mark.parametrize('name', list(MODELS))
def test_banded_quantiles_against_the_mirror(name, rndtype):
    """spec A plus nine banded quantiles: Omega of every draw bit-equal to spec.covariance(panel, block=256, parts=lib.cov_parts),
    symmetric in bits, NaN exactly on the rows and columns of the records the mirror makes NaN (the two empty ones among
    them); means and counts bit-equal to simulate_batch_spec on the same spec.  From the mirror, so that all-NaN rows cannot
    pass: in every draw the per-period medians and the pooled quantile are finite with a positive diagonal"""
    m, s, init, _, panels, _ = _case(name)
    spec, ix = _banded(name)
    rec = spec.pack_lag(s.nt, s.lib.info)
    q = s.lib.quantile_lds_keys
    cand = NSIM * (rec['it_last'] - rec['it_first'] + 1)
    assert all(rec['kind'][j] == 3 and cand[j] == NSIM <= q for j in ix['per_period'])
    assert rec['kind'][ix['pooled']] == 3 and cand[ix['pooled']] == NSIM * s.nt > q
    assert rec['cond_lag'][ix['lagged']] == 2 and rec['col'][ix['tied']] == 4 and rec['cond_lo'][ix['empty']] == 9
    assert s.lib.cov_parts == 4 and (s.status()[0] == 0).all()
    means, counts, cov = s.simulate_batch_cov(init, spec, seed=SEED + rndtype, rndtype=rndtype)
    m2, c2, _ = s.simulate_batch_spec(init, spec, seed=SEED + rndtype, rndtype=rndtype)
    assert cov.shape == (NDRAW, len(spec), len(spec))
    assert bits_equal(means, m2) and np.array_equal(counts, c2)
    zero_rows = 0
    for d in range(NDRAW):
        ref = _mirror(spec, panels[rndtype, d], s.lib.cov_parts)
        _check_draw(cov[d], means[d], counts[d], ref)
        rv, nan = ref[2], ref[3]
        assert nan[ix['empty']] and nan[ix['empty_a']]
        live = list(ix['per_period']) + [ix['pooled']]
        assert not nan[live].any() and np.isfinite(rv[np.ix_(live, ~nan)]).all() and (np.diag(rv)[live] > 0).all(), d
        assert (np.diag(cov[d])[live] > 0).all()
        if not nan[ix['tied']]:
            zero_rows += int(not (rv[ix['tied']][~nan] != 0).any())
    assert zero_rows > 0   # (the median of the choice column lies inside a mass point: s = 0 and a zero row)


def test_quantile_records_in_every_tile():
    """occ3, rndtype 0: the 146-record spec of the covariance test with the 41 per-period shares of choice 1 replaced by banded
    medians of M, so that every one of the five tiles of k_moment_cov holds quantile records"""
    m, s, init, _, panels, _ = _case('occ3_n400')
    spec_a, _, _ = _spec_a('occ3_n400')
    base = len(spec_a)
    items = list(spec_a)
    for it in range(s.nt):
        items += [mo.share('id', 0, periods=it), mo.median('M', periods=it, bandwidth=H), mo.share('id', 2, periods=it)]
    spec = mo.MomentSpec(items, layout=m)
    n = len(spec)
    kinds = spec.pack_lag(s.nt, s.lib.info)['kind']
    assert s.nt == 41 and n == 146 and (kinds == 3).sum() == 41
    assert all((kinds[t * COV_T:(t + 1) * COV_T] == 3).any() for t in range(-(-n // COV_T)))
    means, counts, cov = s.simulate_batch_cov(init, spec, seed=SEED, rndtype=0)
    for d in range(NDRAW):
        ref = _mirror(spec, panels[0, d], s.lib.cov_parts)
        _check_draw(cov[d], means[d], counts[d], ref)
        quant = (kinds == 3) & ~ref[3]
        assert quant.sum() >= 30 and (np.diag(cov[d])[quant] > 0).all(), d
        assert base + 1 in np.nonzero(quant)[0]


@functools.lru_cache(maxsize=None)
def _lib():
    return build.build_model(examples.deaton1())


@pytest.mark.parametrize('kind', SETS)
def test_the_kernel_alone_against_quantile_band(kind):
    """k_quantile_band through quantile_band_eval: sizes around the wave, the workgroup and the LDS threshold, bands among which
    p - h and p + h lie at the edge of acceptance, arrays with ties, NaNs, signed zeros, infinities and denormals; a, b and s
    carry the bits of moments.quantile_band (mask, sort the keys, index)"""
    lib = _lib()
    assert lib.quantile_lds_keys == 2048
    rng = np.random.default_rng(10 + SETS.index(kind))
    p = np.array([b[0] for b in BANDS])
    h = np.array([b[1] for b in BANDS])
    seen = 0
    for n in (1, 2, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 5000):
        x = special_values(kind, n, rng)
        out, count = lib.quantile_band_eval(x, p, h)
        assert count == int((~np.isnan(x)).sum()), (kind, n)
        want = np.array([mo.quantile_band(x, pi, hi) for pi, hi in BANDS])
        assert out.shape == want.shape == (len(BANDS), 3)
        assert bits_equal(out, want), (kind, n, out, want)
        seen += int(np.isfinite(out[:, 2]).sum())
    assert seen > 0
    out, count = lib.quantile_band_eval(np.full(300, np.nan), p, h)
    assert count == 0 and np.isnan(out).all()


def test_the_eval_entry_refuses_what_the_step_refuses():
    lib = _lib()
    x = np.arange(10.0)
    for pp, hh in (([0.5], [0.0]), ([0.5], [np.nan]), ([0.5], [-0.1]), ([0.3], [0.3]), ([0.7], [0.3]), ([0.5, 0.5], [0.1, 0.5]),
                   ([1.0], [0.1])):
        with pytest.raises(runtime.EgdstRuntimeError) as e:
            lib.quantile_band_eval(x, np.array(pp), np.array(hh))
        assert e.value.code == 1
    for xx in (np.zeros(0),):
        with pytest.raises(runtime.EgdstRuntimeError) as e:
            lib.quantile_band_eval(xx, np.array([0.5]), np.array([0.1]))
        assert e.value.code == 1


def test_a_failed_draw_is_all_nan():
    """the failed C2 draw of the covariance test (draw 2 of gen(4096)[:4]) with banded quantiles in the spec: counts 0, means and
    Omega NaN; draws 0, 1 and 3 bit-equal to the mirror"""
    m, P, s, init = _c2_case()
    nt = s.nt
    spec = mo.MomentSpec([mo.mean('C'), mo.median('M', periods=10, bandwidth=H), mo.cross('C', 'C', lag=1),
                          mo.quantile('C', 0.25, bandwidth=0.05), mo.share('id', 1, periods=30),
                          mo.median('A', periods=(5, 6), where=('id', 0, 0, 1), bandwidth=0.1), mo.transition('id', 0, 1)], layout=m)
    st = s.status()[0]
    assert st[2] != 0 and (st[[0, 1, 3]] == 0).all(), st
    means, counts, cov = s.simulate_batch_cov(init, spec, seed=SEED, rndtype=0)
    assert (counts[2] == 0).all() and np.isnan(means[2]).all() and np.isnan(cov[2]).all()
    orc = Oracle(m)
    rs = estimation_case.uniforms(SEED, 4 * nt * NSIM)
    for d in (0, 1, 3):
        sol = orc.solve(P[d])
        assert sol.rc == 0, d
        panel = orc.sim(sol, init, rs, rndtype=0, params=P[d])
        ref = _mirror(spec, panel, s.lib.cov_parts)
        _check_draw(cov[d], means[d], counts[d], ref)
        assert not ref[3][[1, 3]].any() and (np.diag(cov[d])[[1, 3]] > 0).all()


def test_refusals_and_the_handle_stays_usable():
    """every new refusal answers code 1 with the record's index, "quantile" and "bandwidth"; hi = 0 is refused as before;
    afterwards the handle returns the bits it returned before; and simulate_batch_spec does not read the bandwidth"""
    m, s, init, _, _, _ = _case('retirement_mortal')
    spec, ix = _banded('retirement_mortal')
    good = s.simulate_batch_cov(init, spec, seed=1)
    rec = spec.pack_lag(s.nt, s.lib.info)
    j = ix['pooled']
    assert rec['kind'][j] == 3 and rec['lo'][j] == 0.25
    for hi in (np.nan, -0.05, -np.inf, np.inf, 0.25, 0.3, 0.75, 0.8):   # NaN, hi <= 0, lo - hi <= 0, lo + hi >= 1
        r = rec.copy()
        r['hi'][j] = hi
        with pytest.raises(runtime.EgdstRuntimeError) as e:
            s.simulate_batch_cov(init, r, seed=1)
        assert e.value.code == 1 and 'moment %d:' % j in str(e.value), (hi, str(e.value))
        assert 'quantile' in str(e.value) and 'bandwidth' in str(e.value), (hi, str(e.value))
    r = rec.copy()
    r['lo'][ix['tied']], r['hi'][ix['tied']] = 0.5, float(np.nextafter(0.5, 0))   # the sum rounds to 1.0
    with pytest.raises(runtime.EgdstRuntimeError) as e:
        s.simulate_batch_cov(init, r, seed=1)
    assert e.value.code == 1 and 'moment %d:' % ix['tied'] in str(e.value) and 'bandwidth' in str(e.value)
    plain = rec.copy()
    plain['hi'][j] = 0.0
    with pytest.raises(runtime.EgdstRuntimeError) as e:
        s.simulate_batch_cov(init, plain, seed=1)
    assert e.value.code == 1 and 'moment %d:' % j in str(e.value) and 'quantile' in str(e.value)
    again = s.simulate_batch_cov(init, spec, seed=1)
    assert bits_equal(again[0], good[0]) and np.array_equal(again[1], good[1]) and bits_equal(again[2], good[2])
    assert np.isfinite(good[2]).any() and (np.diagonal(good[2], axis1=1, axis2=2)[:, j] > 0).all()
    plain['hi'][rec['kind'] == 3] = 0.0
    a = s.simulate_batch_spec(init, rec, seed=1)
    b = s.simulate_batch_spec(init, plain, seed=1)
    assert bits_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and bits_equal(a[0], good[0]) and (a[1] > 0).any()
