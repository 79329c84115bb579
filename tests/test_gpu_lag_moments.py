"""Moments across two periods on the device (egdst_simulate_batch_spec_lag: transitions, lagged and leading conditions and
crosses, quantiles with a lagged condition): against MomentSpec.evaluate on the oracle's paths, the objective with a full W,
zero lags through the new entry against the old one, and the refusals the lags add.  700 agents throughout: more than two
rounds of the 256-thread block and no multiple of it (threads 0-187 add three agents, the rest two); the 700 candidates of a
per-period quantile are selected in LDS, the 2100 of one pooled over three periods from global memory."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (first: the model libraries then bind torch's HIP runtime, which the result tensors need)

from egdst_amd import examples, runtime
from egdst_amd import moments as mo
from oracle_harness import Oracle
from test_gpu_parity import gpu_solve
import estimation_case
from estimation_case import bits_equal

pytestmark = pytest.mark.gpu

NSIM, NDRAW, SEED = 700, 8, 500
INF = float('inf')
MODELS = {
    # (model, how far the agents' cash is drawn outside [a0, mmax])
    'occ3_n400': (lambda: examples.occ3(ngridm=400, ngridmax=4000, nthrhmax=400, ny=15), 0.0),   # nt = 41
    'retirement_mortal': (lambda: examples.retirement_mortal(), 0.5),                             # nt = 25
}


def _lag_items(nt, nch):
    items = [mo.transition('id', a, b) for a in range(nch) for b in range(nch)]           # [0, nch^2): pooled, lag 1
    items += [mo.transition('id', nch - 1, 0, periods=it) for it in range(1, 6)]           # [nch^2, nch^2 + 5)
    items += [mo.cross('C', 'C', lag=1), mo.cross('M', 'A', lag=1), mo.cross('C', 'M', periods=(3, 10), lag=-1),
              mo.mean('C', periods=(2, nt - 2), where=('id', nch - 1, nch - 1, -1)),
              mo.mean('C', periods=(0, nt - 2), where=('C', -INF, INF, -1)),               # LEAD: the survivors into it + 1
              mo.cross('M', 'M', periods=nt - 1, lag=nt - 1),
              mo.median('M', periods=5, where=('id', nch - 1, nch - 1, 1)),
              mo.quantile('C', 0.9, periods=(4, 6), where=('id', 1, nch - 1, 2)),
              mo.mean('C', where=('id', 9, 9, 1)),                                         # EMPTY: nobody chooses 9
              mo.mean('C'), mo.share('id', 1, periods=2)]                                  # the two records without lags
    return items


def _index(nch):
    """positions of the records the tests name"""
    base = nch * nch + 5
    return dict(per_period=range(nch * nch, base), lead=base + 4, median=base + 6, pooled_q=base + 7, empty=base + 8, plain=(base + 9, base + 10))


@functools.lru_cache(maxsize=None)
def _case(name):
    """8 perturbed draws solved once on the device; the oracle's panels and their evaluation per (rndtype, draw).  The oracle
    solves all eight draws of both models: one that fails here fails the test."""
    make, off = MODELS[name]
    m = make()
    rng = np.random.default_rng(21)
    p0 = m.param_vector()
    P = p0[None] * (1 + 0.15 * rng.uniform(-1, 1, (NDRAW, len(p0))))
    init = np.column_stack([np.ones(NSIM), rng.uniform(m.a0 - off, m.mmax + off, NSIM)])
    s = gpu_solve(m, P)
    nch = s.lib.info.nd
    spec = mo.MomentSpec(_lag_items(s.nt, nch), layout=m)
    orc = Oracle(m)
    sols = [orc.solve(p) for p in P]
    assert [sol.rc for sol in sols] == [0] * NDRAW
    panels, refs = {}, {}
    for rndtype in (0, 1):
        rs = estimation_case.uniforms(SEED + rndtype, 4 * s.nt * (1 if rndtype == 1 else NSIM))
        for d, sol in enumerate(sols):
            panels[rndtype, d] = orc.sim(sol, init, rs, rndtype=rndtype, params=P[d])
            refs[rndtype, d] = spec.evaluate(panels[rndtype, d], block=256)
    return m, s, init, spec, panels, refs


def _weights(n, empty):
    """target and a full symmetric W whose row and column of the empty record are zero"""
    rng = np.random.default_rng(77)
    a = rng.normal(size=(n, n))
    W = a @ a.T / n
    W[empty, :] = 0.0
    W[:, empty] = 0.0
    return rng.uniform(0, 1, n), W


def test_the_population_the_lags_meet_on_the_oracle_paths():
    """What the cases are chosen for, on the oracle's evaluation (rndtype 0): the block and LDS arithmetic of 700 agents; in
    retirement_mortal agents that never have a value and agents that die mid-path, so that the lead condition reads NaNs; in
    occ3 every origin of a pooled transition populated, per-period transitions out of entrepreneurship empty in periods 3-5 of
    draw 2, and the record on choice 9 empty everywhere.  (With these 8 draws and agents, 49 agents of retirement_mortal never
    have a value and 442 die mid-path; the lead condition keeps 11 187 of the 11 629 present pairs.  Drawing the parameters of
    4 draws instead of 8 before the agents gives other agents: 51 and 437.)"""
    assert NSIM > 2 * 256 and NSIM % 256 == 188
    for name in MODELS:
        m, s, init, spec, panels, refs = _case(name)
        nch, ix = s.lib.info.nd, _index(s.lib.info.nd)
        rec = spec.pack_lag(s.nt, s.lib.info)
        assert s.nt == (41 if name == 'occ3_n400' else 25) and spec.lagged
        q = s.lib.quantile_lds_keys
        cand = NSIM * (rec['it_last'] - rec['it_first'] + 1)
        assert rec['kind'][ix['median']] == 3 and cand[ix['median']] == NSIM <= q
        assert rec['kind'][ix['pooled_q']] == 3 and cand[ix['pooled_q']] == 3 * NSIM > q
        for d in range(NDRAW):
            rm, rc = refs[0, d]
            assert rc[ix['empty']] == 0 and np.isnan(rm[ix['empty']]), (name, d)
        if name == 'retirement_mortal':
            for d in range(NDRAW):
                c = panels[0, d][:, :, 1]
                present = ~np.isnan(c)
                assert int((~present).all(axis=1).sum()) == 49, d
                assert int((present[:, :-1] & ~present[:, 1:]).sum()) == 442, d   # (nobody comes back: one death per agent)
                assert int(present[:, :-1].sum()) == 11629 and refs[0, d][1][ix['lead']] == 11187, d
        else:
            for d in range(NDRAW):
                rc = refs[0, d][1]
                origins = [int(rc[a * nch]) for a in range(nch)]   # (the count of a transition is its origin's)
                assert all(rc[a * nch + b] == origins[a] for a in range(nch) for b in range(nch))
                assert all(682 <= n <= 25813 for n in origins), (d, origins)
            assert [int(refs[0, 2][1][j]) for j in ix['per_period']][2:] == [0, 0, 0]


@pytest.mark.parametrize('rndtype', [0, 1])
@pytest.mark.parametrize('name', list(MODELS))
def test_lagged_moments_against_the_oracle_paths(name, rndtype):
    """means and counts of every draw bit-identical to MomentSpec.evaluate(block=256) on the oracle's paths for the host replay
    of the uniforms; the objective with a full symmetric W that leaves the empty record out bit-identical to
    moments.objective and finite; with a weight on the empty record NaN"""
    m, s, init, spec, panels, refs = _case(name)
    ix = _index(s.lib.info.nd)
    n = len(spec)
    target, W = _weights(n, ix['empty'])
    assert (s.status()[0] == 0).all()
    means, counts, obj = s.simulate_batch_spec(init, spec, seed=SEED + rndtype, rndtype=rndtype, target=target, W=W)
    W2 = W.copy()
    W2[ix['empty'], ix['empty']] = 1.0
    obj2 = s.simulate_batch_spec(init, spec, seed=SEED + rndtype, rndtype=rndtype, target=target, W=W2)[2]
    for d in range(NDRAW):
        rm, rc = refs[rndtype, d]
        assert np.array_equal(counts[d], rc), (d, np.nonzero(counts[d] != rc)[0])
        assert bits_equal(means[d], rm), (d, np.nonzero(~(means[d] == rm) & ~(np.isnan(means[d]) & np.isnan(rm)))[0])
        ro = mo.objective(rm, rc, target, W)
        if (rc[np.arange(n) != ix['empty']] > 0).all():   # (a per-period hazard nobody is at risk of empties the objective too)
            assert np.isfinite(ro), d
        assert bits_equal(obj[d], ro), (d, obj[d], ro)
        assert np.isnan(obj2[d]) and np.isnan(mo.objective(rm, rc, target, W2)), d
    assert np.isfinite(obj).any()


@pytest.mark.parametrize('name', list(MODELS))
def test_zero_lags_through_the_new_entry_are_the_old_entry(name):
    """the same records with every lag set to zero: the new entry on the 64-byte records and the old entry on their first 56
    bytes give the same bits"""
    m, s, init, spec, panels, refs = _case(name)
    rec = spec.pack_lag(s.nt, s.lib.info)
    rec['lag2'] = 0
    rec['cond_lag'] = 0
    old = np.zeros(len(rec), dtype=mo.MOMENT_DTYPE)
    for f in mo.MOMENT_DTYPE.names:
        old[f] = rec[f]
    n = len(rec)
    target, W = _weights(n, _index(s.lib.info.nd)['empty'])
    a = s.simulate_batch_spec(init, rec, seed=SEED, rndtype=0, target=target, W=W)
    b = s.simulate_batch_spec(init, old, seed=SEED, rndtype=0, target=target, W=W)
    assert np.array_equal(a[1], b[1]) and bits_equal(a[0], b[0]) and bits_equal(a[2], b[2])
    assert (a[1] > 0).any()
    lagged = s.simulate_batch_spec(init, spec, seed=SEED, rndtype=0)
    assert not np.array_equal(lagged[1], a[1])   # (and the lags do count other pairs)


def test_the_new_refusals_and_the_handle_stays_usable():
    m, s, init, spec, panels, refs = _case('retirement_mortal')
    nt = s.nt
    good = s.simulate_batch_spec(init, spec, seed=1)
    rec = spec.pack_lag(nt, s.lib.info)
    ix = _index(s.lib.info.nd)
    plain, lead = ix['plain'][0], ix['lead']
    assert rec['kind'][plain] == 0 and rec['cond_col'][plain] == -1 and rec['cond_lag'][lead] == -1
    bad = []
    r = rec.copy()
    r['lag2'][plain] = 1                       # lag2 on a kind other than 1
    bad.append(r)
    r = rec.copy()
    r['it_first'][plain], r['cond_lag'][plain] = 1, 1   # cond_lag without a condition
    bad.append(r)
    for field, j, first, last, lag in (('cond_lag', lead, 0, nt - 1, -1), ('cond_lag', lead, 0, nt - 2, 1),
                                        ('lag2', ix['per_period'][0] + 5, 1, nt - 1, -2 ** 31), ('lag2', ix['per_period'][0] + 5, 1, nt - 1, 2 ** 31 - 1)):
        r = rec.copy()                         # a lag in use that leaves [0, nt), at either end and at the ends of int
        r['it_first'][j], r['it_last'][j], r[field][j] = first, last, lag
        bad.append(r)
    assert rec['kind'][ix['per_period'][0] + 5] == 1
    for r in bad:
        with pytest.raises(runtime.EgdstRuntimeError) as e:
            s.simulate_batch_spec(init, r, seed=1, target=np.zeros(len(r)), W=np.eye(len(r)))
        assert e.value.code == 1
    with pytest.raises(ValueError):
        s.simulate_batch_spec(init, mo.MomentSpec([mo.cross('C', 'C', periods=0, lag=1)], layout=m), seed=1)
    again = s.simulate_batch_spec(init, spec, seed=1)
    assert bits_equal(again[0], good[0]) and np.array_equal(again[1], good[1])
