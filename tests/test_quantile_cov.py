"""Quantile records in the covariance of the moments, the host side without a GPU: MomentSpec.scores / covariance with banded
quantiles (a kind-3 record with its bandwidth h in hi; include/egdst.h, egdst_simulate_batch_spec_cov) against plain Python loops
written in the contract's order, bit for bit; a known answer that does not come from the code; the refusals; and the helpers
quantile_bandwidth and quantile_band against what is written out here."""
import functools
import math
import struct
from statistics import NormalDist

import numpy as np
import pytest

from egdst_amd import moments as mo
from estimation_case import bits_equal
from test_moment_cov import LAYOUT, NT, _cov_by_loops, _panel, _term

INF = float('inf')
NAN = float('nan')
# positions in _spec of the quantile records the tests name
PER_PERIOD, POOLED, LAGGED, TIED, EMPTY, ONE_VALUE = 2, 4, 6, 8, 10, 11


def _spec():
    """banded quantiles -- per period, pooled, with a lagged condition, on the tied choice column (the band inside a mass point:
    s = 0), one nothing satisfies, and one whose two ranks coincide when a single value qualifies -- next to kinds 0, 1 and 2"""
    return mo.MomentSpec([
        mo.mean('C'), mo.cross('M', 'C', lag=1),
        mo.median('M', periods=2, bandwidth=0.2),                                                # PER_PERIOD
        mo.share('id', 1, periods=3),
        mo.quantile('C', 0.3, bandwidth=0.1),                                                    # POOLED
        mo.mean('C', periods=(1, 4), where=('id', 1, 2)),
        mo.quantile('M', 0.75, periods=(1, 4), where=('id', 0, 1, 1), bandwidth=0.15),           # LAGGED
        mo.transition('id', 0, 1),
        mo.median('id', bandwidth=0.05),                                                         # TIED
        mo.share('id', 0),
        mo.median('C', where=('id', 9, 9), bandwidth=0.1),                                       # EMPTY: nobody chooses 9
        mo.median('M', periods=0, bandwidth=0.25),                                               # ONE_VALUE at nsim = 1
        mo.cross('M', 'M', periods=NT - 1, lag=NT - 1)], layout=LAYOUT)


def _key(x):
    """the key of include/egdst.h on a Python float, as a Python int"""
    u = struct.unpack('<Q', struct.pack('<d', x))[0]
    return (~u) & (2 ** 64 - 1) if u >> 63 else u | 1 << 63


def _value(key):
    return struct.unpack('<d', struct.pack('<Q', key & (2 ** 63 - 1) if key >> 63 else (~key) & (2 ** 64 - 1)))[0]


def _rank(p, n):
    return min(max(math.ceil(p * float(n)), 1), n)


def _band_by_loops(vals, p, h):
    """(q, a, b, s) of the contract from the list of qualifying values: sorted keys, three ranks, one difference, two quotients"""
    n = len(vals)
    if n == 0:
        return NAN, NAN, NAN, NAN
    keys = sorted(_key(v) for v in vals)
    k_lo, k_hi = _rank(p - h, n), _rank(p + h, n)
    a, b = _value(keys[k_lo - 1]), _value(keys[k_hi - 1])
    mass = float(k_hi - k_lo) / float(n)
    diff = b - a                       # (inf - inf is NaN without an exception)
    s = NAN if mass == 0.0 else diff / mass   # (equal ranks are one value: 0 / 0 or NaN / 0, NaN either way; Python raises instead)
    return _value(keys[_rank(p, n) - 1]), a, b, s


def _scores_by_loops(rec, sims, means, counts):
    """d [nsim][nmom] in Python floats: kinds 0-2 as tests/test_moment_cov.py writes them, kind 3 as
    (s_j * (p * c_ij - t_ij)) / N_j; also the sparsities, and the quantiles found here are held to `means`"""
    nmom = len(rec)
    band = [None] * nmom
    for j, q in enumerate(rec):
        if q['kind'] == 3:
            vals = [x for row in sims for it in range(int(q['it_first']), int(q['it_last']) + 1)
                    for x in [_term(q, row, it)] if x is not None]
            assert len(vals) == counts[j]
            band[j] = _band_by_loops(vals, float(q['lo']), float(q['hi']))
            assert bits_equal(np.array([band[j][0]]), np.array([means[j]]))
    d = []
    for row in sims:
        dr = []
        for j, q in enumerate(rec):
            m, n = float(means[j]), int(counts[j])
            c, t, s = 0, 0, 0.0
            for it in range(int(q['it_first']), int(q['it_last']) + 1):
                x = _term(q, row, it)
                if x is None:
                    continue
                c += 1
                if q['kind'] == 3:
                    t += 1 if _key(x) <= _key(m) else 0
                else:
                    s = s + x
            if not n:
                dr.append(NAN)
            elif q['kind'] == 3:
                dr.append((band[j][3] * (float(q['lo']) * float(c) - float(t))) / float(n))
            else:
                dr.append((s - m * float(c)) / float(n))
        d.append(dr)
    return d, [b[3] if b else None for b in band]


@functools.lru_cache(maxsize=None)
def _loops(nsim):
    spec, sims = _spec(), _panel(nsim)
    means, counts = spec.evaluate(sims)
    return _scores_by_loops(spec.pack_lag(NT), sims, means, counts)


@pytest.mark.parametrize('nsim', [1, 3, 255, 700])
@pytest.mark.parametrize('parts', [1, 4, 16, 256])
def test_mirror_against_loops_in_the_contracts_order(parts, nsim):
    """scores and Omega bit-equal to the loops; NaN exactly on the rows and columns of the records whose sparsity the loops make
    NaN (the empty one always, the one-value one at nsim = 1); the record on the tied column has s = 0 and a zero row; the mirror
    entries of Omega carry equal bits; means and counts are evaluate's"""
    spec, sims = _spec(), _panel(nsim)
    rec = spec.pack_lag(NT)
    assert [j for j in range(len(rec)) if rec['kind'][j] == 3] == [PER_PERIOD, POOLED, LAGGED, TIED, EMPTY, ONE_VALUE]
    assert rec['cond_lag'][LAGGED] == 1 and (rec['hi'][rec['kind'] == 3] > 0).all()
    d_loops, s_loops = _loops(nsim)
    means, counts, d = spec.scores(sims)
    em, ec = spec.evaluate(sims)
    assert bits_equal(means, em) and np.array_equal(counts, ec)
    assert bits_equal(d, np.array(d_loops)), np.argwhere(~((d == np.array(d_loops)) | (np.isnan(d) & np.isnan(np.array(d_loops)))))[:5]
    m2, c2, cov = spec.covariance(sims, parts=parts)
    assert bits_equal(m2, em) and np.array_equal(c2, ec)
    want = _cov_by_loops(d_loops, parts)
    assert bits_equal(cov, want), np.argwhere(~((cov == want) | (np.isnan(cov) & np.isnan(want))))[:5]
    assert np.array_equal(np.isnan(cov), np.isnan(cov.T))
    assert np.array_equal(np.nan_to_num(cov).view(np.int64), np.nan_to_num(cov.T).view(np.int64))
    nan = np.array([(counts[j] == 0) or (s_loops[j] is not None and math.isnan(s_loops[j])) for j in range(len(rec))])
    assert np.array_equal(np.isnan(cov), nan[:, None] | nan[None, :])
    assert nan[EMPTY] and counts[EMPTY] == 0
    if nsim == 1:
        assert counts[ONE_VALUE] == 1 and nan[ONE_VALUE]          # k_hi == k_lo: 0 / 0
    if nsim >= 255:
        assert nan.sum() == 1                                        # (only the empty record)
        assert s_loops[TIED] == 0.0 and not (d[:, TIED] != 0).any() and not (cov[TIED][~nan] != 0).any()
        for j in (PER_PERIOD, POOLED, LAGGED, ONE_VALUE):
            assert math.isfinite(s_loops[j]) and s_loops[j] > 0 and cov[j, j] > 0


def test_known_answer_of_a_uniform_grid():
    """one period, x_i = i for i < 100, p = 0.5, h = 0.25: q = 49 (the lower middle value), a = 24, b = 74, s = 50 / (50 / 100) = 100,
    d_i = 100 (0.5 - [i <= 49]) / 100 = +-0.5 and Omega = 100 * 0.25 = 25 exactly: p (1 - p) / (n f^2) with f = 1 / 100"""
    sims = np.zeros((100, 1, 11))
    sims[:, 0, 0] = np.arange(100.0)
    spec = mo.MomentSpec([mo.median('M', periods=0, bandwidth=0.25)], layout=(0, 0, 0))
    assert mo.quantile_band(sims[:, 0, 0], 0.5, 0.25) == (24.0, 74.0, 100.0)
    means, counts, d = spec.scores(sims)
    assert means[0] == 49.0 and counts[0] == 100
    assert np.array_equal(d[:, 0], np.where(np.arange(100) <= 49, -0.5, 0.5))
    for parts in (1, 4, 256):
        assert spec.covariance(sims, parts=parts)[2][0, 0] == 25.0
    assert 25.0 == 0.5 * 0.5 / (100 * (1 / 100) ** 2)


def test_evaluate_does_not_look_at_the_bandwidth():
    sims = _panel(255)
    banded = _spec()
    plain = mo.MomentSpec([mo.Moment(q.kind, q.col, q.col2, q.periods, q.where, q.lo, 0.0 if q.kind == 3 else q.hi, q.lag)
                           for q in banded], layout=LAYOUT)
    assert (plain.pack_lag(NT)['hi'][[PER_PERIOD, POOLED, LAGGED, TIED, EMPTY, ONE_VALUE]] == 0).all()
    a, b = banded.evaluate(sims), plain.evaluate(sims)
    assert bits_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and (a[1] > 0).any()
    # a record packed without a bandwidth keeps the bits it had: hi = 0.0
    assert mo.median('M').hi == 0.0 and mo.quantile('M', 0.3).hi == 0.0
    assert np.array_equal(mo.MomentSpec([mo.median('M', periods=2)], layout=LAYOUT).pack_lag(NT).view(np.uint8),
                          mo.MomentSpec([mo.Moment(3, 'M', periods=2, lo=0.5)], layout=LAYOUT).pack_lag(NT).view(np.uint8))


def test_every_new_value_error():
    sims = _panel(255)
    for p, h in ((0.5, NAN), (0.5, -0.1), (0.5, -INF), (0.5, INF), (0.3, 0.3), (0.3, 0.31), (0.7, 0.3), (0.7, 0.5),
                 (np.nextafter(1, 0), 2.0 ** -53), (1e-300, 1e-300)):
        with pytest.raises(ValueError, match='bandwidth'):
            mo.MomentSpec([mo.quantile('M', p, bandwidth=h)], layout=LAYOUT).pack_lag(NT)
        with pytest.raises(ValueError, match='bandwidth'):
            mo.quantile_band(np.arange(10.0), p, h)
    # the edge of acceptance is the rounded sum and difference
    edge = np.nextafter(0.3, 0)
    assert 0.3 - edge > 0 and 0.7 + edge < 1
    mo.MomentSpec([mo.quantile('M', 0.3, bandwidth=edge), mo.quantile('M', 0.7, bandwidth=edge)], layout=LAYOUT).pack_lag(NT)
    for how in ('scores', 'covariance'):   # without a bandwidth: refused as before, banded records beside it or not
        with pytest.raises(ValueError, match='quantile'):
            getattr(mo.MomentSpec([mo.median('M', periods=2, bandwidth=0.1), mo.median('C')], layout=LAYOUT), how)(sims)
    with pytest.raises(ValueError, match='bandwidth'):
        mo.quantile_band(np.arange(10.0), 0.5, 0.0)
    with pytest.raises(ValueError):
        mo.quantile_band(np.arange(10.0), 1.0, 0.1)
    with pytest.raises(ValueError):
        mo.quantile_bandwidth(0.5, 100, rule='silverman')
    with pytest.raises(ValueError):
        mo.quantile_bandwidth(1.0, 100)
    with pytest.raises(ValueError):
        mo.quantile_bandwidth(0.5, 0)


@pytest.mark.parametrize('rule', ['bofinger', 'hall-sheather'])
def test_quantile_bandwidth_against_the_formula(rule):
    nd = NormalDist()

    def formula(p, n):
        z = nd.inv_cdf(p)
        f = nd.pdf(z)
        if rule == 'bofinger':
            return n ** (-1 / 5) * (4.5 * f ** 4 / (2 * z * z + 1) ** 2) ** (1 / 5)
        return n ** (-1 / 3) * nd.inv_cdf(0.975) ** (2 / 3) * (1.5 * f * f / (2 * z * z + 1)) ** (1 / 3)

    unclipped = 0
    for p in (0.001, 0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99):
        for n in (1, 10, 700, 2000, 120000):
            h = mo.quantile_bandwidth(p, n, rule=rule)
            want = formula(p, n)
            assert 0 < h <= want * (1 + 1e-12)
            assert p - h > 0 and p + h < 1
            mo.MomentSpec([mo.quantile('M', p, bandwidth=h)], layout=LAYOUT).pack_lag(NT)   # the record is accepted
            if p - want > 0 and p + want < 1 and want <= 0.5 * min(p, 1 - p):
                assert h == pytest.approx(want, rel=1e-12)
                unclipped += 1
    assert unclipped >= 15
    assert mo.quantile_bandwidth(0.5, 2000) == mo.quantile_bandwidth(0.5, 2000, rule='bofinger')
    # the median of 2000 values: Bofinger's band is wider than Hall and Sheather's
    assert mo.quantile_bandwidth(0.5, 2000, 'bofinger') > mo.quantile_bandwidth(0.5, 2000, 'hall-sheather') > 0.01


def _np_keys(x):
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))


def band_by_sort(x, p, h):
    """mask, sort the keys, index: (a, b, s) as numpy doubles (also what tests/test_gpu_quantile_cov.py holds the kernel to)"""
    x = np.asarray(x, dtype=np.float64)
    v = x[~np.isnan(x)]
    n = len(v)
    if n == 0:
        return np.nan, np.nan, np.nan
    v = v[np.argsort(_np_keys(v), kind='stable')]
    p, h = np.float64(p), np.float64(h)
    k_lo = min(max(math.ceil(float((p - h) * np.float64(n))), 1), n)
    k_hi = min(max(math.ceil(float((p + h) * np.float64(n))), 1), n)
    with np.errstate(all='ignore'):
        return v[k_lo - 1], v[k_hi - 1], (v[k_hi - 1] - v[k_lo - 1]) / (np.float64(k_hi - k_lo) / np.float64(n))


def special_values(kind, n, rng):
    tiny = np.nextafter(0, 1)
    if kind == 'normal':
        return rng.normal(size=n)
    if kind == 'equal':
        return np.full(n, -1.75)
    if kind == 'two_values':
        return rng.choice([3.5, -2.0], n)
    if kind == 'normal_with_nan':
        x = rng.normal(size=n)
        x[rng.random(n) < 0.2] = np.nan
        return x
    if kind == 'zeros':
        return rng.choice([0.0, -0.0], n)
    if kind == 'denormals':
        return rng.integers(-40, 40, n) * tiny
    assert kind == 'specials'
    return rng.choice([0.0, -0.0, np.inf, -np.inf, tiny, -tiny, np.finfo(np.float64).max, 1.0, np.nan], n)


SETS = ['normal', 'equal', 'two_values', 'normal_with_nan', 'zeros', 'denormals', 'specials']
BANDS = [(0.5, 0.25), (0.5, 0.01), (0.1, 0.05), (0.9, 0.09), (1 / 3, 0.2), (0.3, float(np.nextafter(0.3, 0))),
         (0.7, float(np.nextafter(0.3, 0))), (0.5, float(np.nextafter(1, 0)) - 0.5), (0.25, 2.0 ** -60)]   # (among them p - h and p + h at the edge of acceptance)


@pytest.mark.parametrize('kind', SETS)
def test_quantile_band_against_mask_sort_index(kind):
    """ties (s = 0 or NaN), NaNs (masked), -0.0 before +0.0, infinite ends (s = inf or NaN), denormals: a and b carry the bits of
    the order statistics, s those of the three operations"""
    rng = np.random.default_rng(SETS.index(kind))
    seen = set()
    for n in (1, 2, 3, 10, 257, 2049):
        x = special_values(kind, n, rng)
        for p, h in BANDS:
            got = np.array(mo.quantile_band(x, p, h))
            want = np.array(band_by_sort(x, p, h))
            assert bits_equal(got[:2], want[:2]) and bits_equal(got[2:], want[2:]), (kind, n, p, h, got, want)
            seen.add('nan' if math.isnan(got[2]) else 'zero' if got[2] == 0 else 'inf' if math.isinf(got[2]) else 'finite')
    assert {'equal': {'nan', 'zero'}, 'normal': {'nan', 'finite'}, 'zeros': {'nan', 'zero'}}.get(kind, seen) <= seen
    if kind == 'specials':
        assert {'nan', 'inf'} <= seen
    assert np.isnan(mo.quantile_band(np.full(5, np.nan), 0.5, 0.25)).all()
    # -0.0 comes before +0.0: the band of [+0.0, -0.0] ends at -0.0 and +0.0
    a, b, s = mo.quantile_band(np.array([0.0, -0.0]), 0.5, 0.4)
    assert math.copysign(1, a) == -1 and math.copysign(1, b) == 1 and s == 0.0
