"""MomentSpec.covariance, the host mirror of egdst_simulate_batch_spec_cov (include/egdst.h), without a GPU: against plain
Python loops written out in the contract's order, bit for bit; against known answers that do not come from the code under
test; and against a long-double sum of the same products within the bound the summation order allows."""
import functools
import math

import numpy as np
import pytest

from egdst_amd import moments as mo
from estimation_case import bits_equal

LAYOUT = (1, 1, 1)            # nout = 14
NT, NOUT = 6, 14
INF = float('inf')
EMPTY = 12                    # the record of _spec nothing satisfies


def _spec():
    """kinds 0, 1 and 2, each with and without a condition and a lag, pooled and per period, and one empty record"""
    return mo.MomentSpec([
        mo.mean('C'), mo.mean('M', periods=2), mo.mean('C', periods=(1, 4), where=('id', 1, 2)),
        mo.mean('C', periods=(0, NT - 2), where=('C', -INF, INF, -1)),                         # a lead: the survivors
        mo.cross('M', 'C'), mo.cross('C', 'C', lag=1), mo.cross('M', 'A', periods=(2, 4), lag=-1, where=('id', 0, 1, 1)),
        mo.cross('M', 'M', periods=NT - 1, lag=NT - 1),
        mo.share('id', 1, periods=3), mo.share('id', 0), mo.share('M', -0.5, 0.5, where=('id', 0, 1)),
        mo.transition('id', 0, 1),
        mo.mean('C', where=('id', 9, 9, 1)),                                                   # EMPTY: nobody chooses 9
        mo.share('id', 2, periods=3)], layout=LAYOUT)


@functools.lru_cache(maxsize=None)
def _panel(nsim):
    """[nsim, NT, NOUT]: normal values, choices 0..2 in column 4; every seventh agent never has a value, every third of the
    others dies mid-path (NaN rows from then on), and a few single rows are NaN"""
    rng = np.random.default_rng(100 + nsim)
    sims = rng.normal(size=(nsim, NT, NOUT))
    sims[:, :, 4] = rng.integers(0, 3, size=(nsim, NT))
    for i in range(nsim):
        if i % 7 == 6:
            sims[i] = np.nan
        elif i % 3 == 1:
            sims[i, 1 + i % (NT - 1):] = np.nan
        elif i % 5 == 2:
            sims[i, i % NT] = np.nan
    sims.setflags(write=False)
    return sims


def _term(rec, row, it):
    """eg_moment_term and the share's 1.0 / 0.0 on agent panel `row` [NT, NOUT]: None, or the value the pair adds"""
    v = float(row[it, rec['col']])
    if v != v:
        return None
    if rec['cond_col'] >= 0:
        c = float(row[it - int(rec['cond_lag']), rec['cond_col']])
        if not (c >= rec['cond_lo'] and c <= rec['cond_hi']):
            return None
    x = v
    if rec['kind'] == 1:
        w = float(row[it - int(rec['lag2']), rec['col2']])
        if w != w:
            return None
        x = v * w
    if rec['kind'] == 2:
        x = 1.0 if rec['lo'] <= x <= rec['hi'] else 0.0
    return x


def _scores_by_loops(rec, sims, means, counts):
    """d [nsim][nmom] as the contract writes it, in Python floats (IEEE doubles, every operation rounded once)"""
    nan = float('nan')
    d = []
    for row in sims:
        dr = []
        for j, q in enumerate(rec):
            c, s = 0, 0.0
            for it in range(int(q['it_first']), int(q['it_last']) + 1):
                x = _term(q, row, it)
                if x is not None:
                    s = s + x
                    c += 1
            m, n = float(means[j]), int(counts[j])
            dr.append((s - m * float(c)) / float(n) if n else nan)   # (0 / 0 and NaN / 0 are NaN; Python raises instead)
        d.append(dr)
    return d


def _cov_by_loops(d, parts):
    nsim, nmom = len(d), len(d[0])
    cov = [[0.0] * nmom for _ in range(nmom)]
    for j in range(nmom):
        for k in range(j, nmom):
            p = [0.0] * parts
            for i in range(nsim):
                p[i % parts] = p[i % parts] + (d[i][j] * d[i][k])
            o = parts // 2
            while o >= 1:
                for t in range(o):
                    p[t] = p[t] + p[t + o]
                o //= 2
            cov[j][k] = cov[k][j] = p[0]
    return np.array(cov)


@functools.lru_cache(maxsize=None)
def _loop_scores(nsim):
    spec, sims = _spec(), _panel(nsim)
    means, counts = spec.evaluate(sims)
    return _scores_by_loops(spec.pack_lag(NT), sims, means, counts)


@pytest.mark.parametrize('nsim', [1, 3, 255, 700])
@pytest.mark.parametrize('parts', [1, 4, 16, 256])
def test_mirror_against_loops_in_the_contracts_order(parts, nsim):
    """fewer agents than partials, no multiple of them, and 700 = 2 * 256 + 188: Omega bit-equal to the loops; its mirror
    entries carry equal bits; NaN exactly on the empty record's row and column; means and counts are evaluate's"""
    spec, sims = _spec(), _panel(nsim)
    means, counts, cov = spec.covariance(sims, parts=parts)
    em, ec = spec.evaluate(sims)
    assert bits_equal(means, em) and np.array_equal(counts, ec)
    assert counts[EMPTY] == 0 and (nsim < 255 or (np.delete(counts, EMPTY) > 0).all())
    want = _cov_by_loops(_loop_scores(nsim), parts)
    assert bits_equal(cov, want), np.argwhere(~((cov == want) | (np.isnan(cov) & np.isnan(want))))[:5]
    assert np.array_equal(cov.view(np.int64), cov.T.view(np.int64))
    empty = counts == 0
    assert np.array_equal(np.isnan(cov), empty[:, None] | empty[None, :])
    if nsim >= 255:
        assert empty.sum() == 1 and np.isfinite(np.delete(np.delete(cov, EMPTY, 0), EMPTY, 1)).all()


def test_a_quantile_is_refused():
    sims = _panel(255)
    with pytest.raises(ValueError, match='quantile'):
        mo.MomentSpec([mo.mean('C'), mo.median('M', periods=2)], layout=LAYOUT).covariance(sims)
    with pytest.raises(ValueError):
        _spec().covariance(sims, parts=3)
    with pytest.raises(ValueError):
        _spec().covariance(sims, parts=512)


def _full_panel(nsim, seed=5):
    rng = np.random.default_rng(seed)
    sims = rng.normal(size=(nsim, NT, NOUT))
    sims[:, :, 4] = rng.integers(0, 3, size=(nsim, NT))
    return sims


@pytest.mark.parametrize('nsim', [255, 700])
def test_known_answers_on_panels_without_nan(nsim):
    """what Omega must be where a textbook gives it: a one-period mean has var(x) / n, a share p (1 - p) / n, two shares of one
    column and period -p1 p2 / n, and a mean pooled over every period of a panel in which each agent carries ONE value in all
    periods has var(a) / n -- not divided by the number of periods, because an agent's periods are one cluster"""
    sims = _full_panel(nsim)
    spec = mo.MomentSpec([mo.mean('C', periods=2), mo.share('id', 0, periods=3), mo.share('id', 1, periods=3)], layout=LAYOUT)
    means, counts, cov = spec.covariance(sims)
    x = sims[:, 2, 1]
    p0, p1 = (sims[:, 3, 4] == 0).mean(), (sims[:, 3, 4] == 1).mean()
    assert (counts == nsim).all()
    assert cov[0, 0] == pytest.approx(np.var(x) / nsim, rel=1e-12)
    assert cov[1, 1] == pytest.approx(p0 * (1 - p0) / nsim, rel=1e-12)
    assert cov[2, 2] == pytest.approx(p1 * (1 - p1) / nsim, rel=1e-12)
    assert cov[1, 2] == pytest.approx(-p0 * p1 / nsim, rel=1e-12)
    a = np.random.default_rng(9).normal(size=nsim)
    flat = np.repeat(a[:, None, None], NT, axis=1).repeat(NOUT, axis=2)
    m, c, v = mo.MomentSpec([mo.mean('C')], layout=LAYOUT).covariance(flat)
    assert c[0] == nsim * NT
    assert v[0, 0] == pytest.approx(np.var(a) / nsim, rel=1e-12)


def order_free_bound(d):
    """(long-double D'D of the scores d [nsim, nmom], the bound on what any summation order of the rounded products may differ
    from it): n products and n sums round once each, at most n + 1 roundings of relative size 2^-53 on every term's path, and
    by Cauchy-Schwarz sum |d_ij d_ik| <= sqrt(Omega_jj Omega_kk)"""
    ld = d.astype(np.longdouble)
    exact = ld.T @ ld
    diag = np.sqrt(np.diag(exact))
    return exact, 2 * d.shape[0] * 2.0 ** -53 * diag[:, None] * diag[None, :]


@pytest.mark.parametrize('parts', [1, 4, 256])
def test_summation_order_stays_inside_the_bound(parts):
    """scores computed elementwise by the contract (IEEE operations: no order to choose); Omega within
    2 nsim 2^-53 sqrt(Omega_jj Omega_kk) of the long-double sum of the same products"""
    nsim = 700
    spec, sims = _spec(), _panel(nsim)
    means, counts, cov = spec.covariance(sims, parts=parts)
    d = np.array(_loop_scores(nsim))
    keep = np.arange(len(spec)) != EMPTY
    exact, bound = order_free_bound(d[:, keep])
    got = cov[np.ix_(keep, keep)]
    assert np.isfinite(got).all() and (np.abs(got.astype(np.longdouble) - exact) <= bound).all()
    assert math.isfinite(float(bound.max())) and (np.diag(got) > 0).all()
