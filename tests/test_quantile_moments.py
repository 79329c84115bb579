"""Quantile moments (kind 3 of egdst_moment, egdst_amd/moments.py) without a GPU: the packed records, the refusal of a p
outside (0, 1), MomentSpec.evaluate against a mask-sort-index written out here, and the objective of a spec that mixes all
four kinds."""
import math

import numpy as np
import pytest

from egdst_amd import moments as mo

NT, NOUT = 7, 14
PS = [0.01, 0.25, 0.5, 0.75, 0.99, 1 / 3]


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def keys(x):
    """the order of the contract, written out: u = bits(x), key = (u >> 63) ? ~u : u | 1 << 63"""
    return np.array([(~int(u)) & (2**64 - 1) if int(u) >> 63 else int(u) | 1 << 63 for u in bits(x).ravel()], dtype=np.uint64)


def test_packed_records():
    spec = mo.MomentSpec([mo.quantile('M', 0.25, periods=3, where=('id', 1, 1)), mo.median('C')], layout=(1, 1, 1))
    rec = spec.pack(NT)
    assert rec.dtype.itemsize == mo.MOMENT_DTYPE.itemsize == 56
    assert mo.QUANTILE == 3
    assert tuple(rec[0]) == (3, 0, 0, 3, 3, 4, 0.25, 0.0, 1.0, 1.0)
    assert tuple(rec[1]) == (3, 1, 1, 0, NT - 1, -1, 0.5, 0.0, 0.0, 0.0)


@pytest.mark.parametrize('p', [0, 1, -0.1, 1.5, float('nan')])
def test_p_outside_the_open_unit_interval_raises(p):
    with pytest.raises(ValueError):
        mo.MomentSpec([mo.quantile('C', p)]).pack(NT)
    with pytest.raises(ValueError):
        mo.MomentSpec([mo.Moment(mo.QUANTILE, 'C', lo=p)]).pack(NT)


def _panel(seed, nsim):
    """holes, agents that leave, an integer column with three values (4), negative values, and a column (5) of -0.0 and
    +0.0 only"""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(nsim, NT, NOUT)) * rng.uniform(0.1, 100, NOUT)
    x[..., 4] = rng.integers(0, 3, (nsim, NT))
    x[..., 5] = np.where(rng.random((nsim, NT)) < 0.5, -0.0, 0.0)
    x[rng.random((nsim, NT, NOUT)) < 0.2] = np.nan
    dead = rng.integers(0, NT + 1, nsim)
    x[np.arange(NT)[None, :] >= dead[:, None]] = np.nan
    return x


def _qualifying(sims, q):
    f, l_ = int(q['it_first']), int(q['it_last']) + 1
    v = sims[:, f:l_, q['col']]
    ok = ~np.isnan(v)
    if q['cond_col'] >= 0:
        c = sims[:, f:l_, q['cond_col']]
        with np.errstate(invalid='ignore'):
            ok &= (c >= q['cond_lo']) & (c <= q['cond_hi'])
    return v[ok]


def _items():
    items = []
    for p in PS:
        items += [mo.quantile(0, p, periods=2), mo.quantile('C', p), mo.quantile('id', p, periods=(1, 4)),
                  mo.quantile(5, p), mo.quantile(5, p, periods=0), mo.quantile('A', p, where=('id', 1, 1)),
                  mo.quantile(12, p, periods=(3, 6), where=('M', -50, 10)), mo.quantile('V', p, where=('id', 7, 9))]
    return items


@pytest.mark.parametrize('nsim', [1, 2, 255, 256, 257, 1000])
def test_evaluate_agrees_with_mask_sort_index(nsim):
    sims = _panel(100 + nsim, nsim)
    spec = mo.MomentSpec(_items(), layout=(1, 1, 1))
    rec = spec.pack(NT)
    results = [spec.evaluate(sims, block=b) for b in (1, 256)]
    assert np.array_equal(bits(results[0][0]), bits(results[1][0])) and np.array_equal(results[0][1], results[1][1])
    means, counts = results[1]
    seen_empty = seen_zero = False
    for j, q in enumerate(rec):
        v = _qualifying(sims, q)
        n = len(v)
        assert counts[j] == n, j
        if n == 0:
            assert np.isnan(means[j]), j
            seen_empty = True
            continue
        k = math.ceil(q['lo'] * float(n))
        k = min(max(k, 1), n)
        if q['col'] == 5:   # -0.0 and +0.0: np.sort of the doubles does not order them; sort the keys
            want = np.sort(keys(v))[k - 1]
            assert keys(means[j])[0] == want, (j, means[j])
            seen_zero = True
        else:
            assert bits(means[j]) == bits(np.sort(v)[k - 1]), (j, means[j])
    assert seen_empty and seen_zero   # (the where on id in [7, 9] never holds)


def test_zero_column_holds_both_signs_and_orders_them():
    sims = _panel(5, 400)
    z = sims[:, :, 5]
    z = z[~np.isnan(z)]
    assert np.signbit(z).any() and not np.signbit(z).all()
    nneg = int(np.signbit(z).sum())
    spec = mo.MomentSpec([mo.quantile(5, (nneg - 0.5) / len(z)), mo.quantile(5, (nneg + 0.5) / len(z))])
    means, counts = spec.evaluate(sims)
    assert counts.tolist() == [len(z)] * 2
    assert means[0] == 0 and np.signbit(means[0]) and means[1] == 0 and not np.signbit(means[1])


def test_median_of_an_even_count_is_the_lower_middle_value():
    sims = np.full((4, 1, 11), np.nan)
    sims[:, 0, 1] = [4.0, 1.0, 3.0, 2.0]
    means, counts = mo.MomentSpec([mo.median('C'), mo.quantile('C', 0.51)]).evaluate(sims)
    assert means.tolist() == [2.0, 3.0] and counts.tolist() == [4, 4]


def test_objective_of_a_spec_mixing_all_kinds():
    sims = _panel(11, 300)
    spec = mo.MomentSpec([mo.mean('C'), mo.median('C'), mo.cross('M', 'C', periods=(0, 3)), mo.quantile('A', 0.9, periods=2),
                          mo.share('id', 1), mo.quantile('id', 0.25), mo.median(5)], layout=(1, 1, 1))
    means, counts = spec.evaluate(sims)
    assert (counts > 0).all() and [int(k) for k in spec.pack(NT)['kind']] == [0, 3, 1, 3, 2, 3, 3]
    n = len(spec)
    rng = np.random.default_rng(2)
    a = rng.normal(size=(n, n))
    W = a @ a.T / n
    W[4, :] = W[:, 4] = 0
    target = rng.normal(size=n)
    e = means - target
    ref = 0.0
    for j in range(n):   # the documented order: r_j over k ascending, then e_j * r_j over j ascending
        if W[j].any():
            r = 0.0
            for k in range(n):
                if W[j, k] != 0:
                    r += W[j, k] * e[k]
            ref += e[j] * r
    assert mo.objective(means, counts, target, W) == ref
    c = counts.copy()
    c[1] = 0   # an empty quantile that W touches
    assert np.isnan(mo.objective(means, c, target, W))
