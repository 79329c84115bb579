"""The estimation step with user-defined moments and a full weighting matrix on the device (egdst_simulate_batch_spec):
the same bits as egdst_simulate_batch_moments where the two overlap, the oracle's paths reduced by MomentSpec.evaluate with
the device's summation order, several slices of draws, and malformed records."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (first: the model libraries then bind torch's HIP runtime, which the result tensors need)

from egdst_amd import examples, runtime, workloads
from egdst_amd import moments as mo
from oracle_harness import Oracle
from test_gpu_parity import gpu_solve
import estimation_case
from estimation_case import bits_equal

pytestmark = pytest.mark.gpu


def _nout(s):
    return s.lib.nout


def _per_period(s, cols=None):
    """kind 0 of every (col, it), ordered col + nout * it: the cells of simulate_batch_moments"""
    nout = _nout(s)
    cols = range(nout) if cols is None else cols
    return mo.MomentSpec([mo.mean(c, periods=it) for it in range(s.nt) for c in cols], layout=s)


@functools.lru_cache(maxsize=None)
def _c2_case():
    """C2 setup of test_estimation_step_on_device, solved once on the device and once by the oracle"""
    m, gen = workloads.c2(a0=0, ngridm=300, T=30)
    P = gen(1024)[[0, 1, 2, 3, 5, 8, 13, 771]]
    orc = Oracle(m)
    return m, P, gpu_solve(m, P), orc, [orc.solve(p) for p in P]


@pytest.mark.parametrize('rndtype', [0, 1])
def test_per_period_spec_is_the_batch_moments_path(rndtype):
    """C2 setup of test_estimation_step_on_device: means, counts and the objective with a diagonal W bit-identical to
    simulate_batch_moments; a failing draw would give NaN / 0 / NaN, but at ngridm=300 none of these fails (draws that do:
    tests/test_gpu_estimation_loop.py::test_estimation_step_with_draws_that_fail).  The two are doors of one kernel, so simulate_batch_moments is
    pinned by itself as well: for every draw (the oracle solves all eight) bit-identical to the per-period spec evaluated in
    the device's order on the oracle's paths for the host replay of the uniforms, and to moments.objective with the weights as
    a diagonal; 420 cells, so the objective kernel crosses a boundary of its 256-row chunks."""
    m, P, s, orc, sols = _c2_case()
    st = s.status()[0]
    rng = np.random.default_rng(5)
    nsim = 2000
    init = np.column_stack([np.ones(nsim), rng.uniform(m.a0 - 0.5, m.mmax + 0.5, nsim)])
    nout = _nout(s)
    target = np.random.default_rng(3).uniform(0, 2, (s.nt, nout))
    weight = np.zeros((s.nt, nout))
    weight[1:, 1] = 1.0
    weight[1:, 4] = 4.0
    seed = 99 + rndtype
    bm, bc, bo = s.simulate_batch_moments(init, seed=seed, rndtype=rndtype, target=target, weight=weight)
    spec = _per_period(s)
    for W in (weight.reshape(-1), np.diag(weight.reshape(-1))):
        sm, sc, so = s.simulate_batch_spec(init, spec, seed=seed, rndtype=rndtype, target=target.reshape(-1), W=W)
        assert np.array_equal(sc, bc.reshape(s.ndraw, -1))
        assert bits_equal(sm, bm.reshape(s.ndraw, -1))
        assert bits_equal(so, bo)
    for d in np.nonzero(st)[0]:
        assert np.isnan(sm[d]).all() and not sc[d].any() and np.isnan(so[d])
    assert np.isfinite(so[st == 0]).all()
    assert s.nt * nout > 256
    rs = estimation_case.uniforms(seed, 4 * s.nt * (1 if rndtype == 1 else nsim))
    for d in range(s.ndraw):
        assert sols[d].rc == 0 and st[d] == 0, (d, sols[d].rc, st[d])
        rm, rc = spec.evaluate(orc.sim(sols[d], init, rs, rndtype=rndtype, params=P[d]), block=256)
        assert np.array_equal(bc[d].reshape(-1), rc), (rndtype, d)
        assert bits_equal(bm[d].reshape(-1), rm), (rndtype, d)
        ro = mo.objective(rm, rc, target.reshape(-1), weight.reshape(-1))
        assert bits_equal(bo[d], ro), (rndtype, d, bo[d], ro)


def _full_spec(m, nt, nch):
    """sector / choice shares by period, consumption by choice, M*C, a 3-period bin, conditions on a state column"""
    items = [mo.share('id', k, periods=it) for it in range(nt) for k in range(nch)]
    items += [mo.mean('C', where=('id', k, k)) for k in range(nch)]
    items += [mo.cross('M', 'C'), mo.cross('C', 'C', periods=2), mo.mean('M', periods=(1, 3)), mo.mean('C', where=('st1', 0, 0)),
              mo.mean('A', periods=(2, 4), where=('M', 1.0, 3.0)), mo.share('M', 0.5, 2.0), mo.mean('eq1', periods=(1, nt - 1))]
    return mo.MomentSpec(items, layout=m)


@pytest.mark.parametrize('name', ['occ3_n400', 'retirement2'])
def test_full_spec_against_the_oracle(name):
    """8 perturbed draws: means and counts bit-identical to MomentSpec.evaluate(block=256) on the oracle's paths for the host
    replay of the uniforms; the objective with a full symmetric W bit-identical to moments.objective."""
    m = examples.occ3(ngridm=400, ngridmax=4000, nthrhmax=400, ny=15) if name == 'occ3_n400' else examples.retirement2()
    rng = np.random.default_rng(21)
    p0 = m.param_vector()
    P = p0[None] * (1 + 0.15 * rng.uniform(-1, 1, (8, len(p0))))
    s = gpu_solve(m, P)
    st = s.status()[0]
    nsim = 2000
    init = np.column_stack([np.ones(nsim), rng.uniform(m.a0, m.mmax, nsim)])
    spec = _full_spec(m, s.nt, s.lib.info.nd)
    n = len(spec)
    a = rng.normal(size=(n, n))
    W = a @ a.T / n
    target = rng.uniform(0, 1, n)
    orc = Oracle(m)
    finite = 0
    for rndtype in (0, 1):
        seed = 500 + rndtype
        means, counts, obj = s.simulate_batch_spec(init, spec, seed=seed, rndtype=rndtype, target=target, W=W)
        rs = estimation_case.uniforms(seed, 4 * s.nt * (1 if rndtype == 1 else nsim))
        for d in range(s.ndraw):
            sol = orc.solve(P[d])
            if sol.rc != 0:
                assert st[d] != 0 and np.isnan(means[d]).all() and not counts[d].any() and np.isnan(obj[d]), d
                continue
            rm, rc = spec.evaluate(orc.sim(sol, init, rs, rndtype=rndtype, params=P[d]), block=256)
            assert np.array_equal(counts[d], rc), (rndtype, d)
            assert bits_equal(means[d], rm), (rndtype, d)
            assert bits_equal(obj[d], mo.objective(rm, rc, target, W)), (rndtype, d, obj[d], mo.objective(rm, rc, target, W))
            finite += int(np.isfinite(obj[d]))
    assert finite >= 4


def test_bins_over_several_slices():
    """C2 at T=60 with enough agents that the draws take three slices of paths: 10-period bins add up to their periods, the
    per-period moments are bit-equal to simulate_batch_moments."""
    m, gen = workloads.c2(a0=0)
    P = gen(1024)[[0, 1, 2, 3, 5, 8]]
    s = gpu_solve(m, P)
    nout = _nout(s)
    nsim = 120000
    slice_ = (2 << 30) // (8 * nout * s.nt * nsim)
    assert s.nt == 60 and 1 <= slice_ and -(-s.ndraw // slice_) >= 3
    init = np.column_stack([np.ones(nsim), np.random.default_rng(8).uniform(m.a0, m.mmax, nsim)])
    cols = (0, 1, 4)
    per = _per_period(s, cols)
    bins = [mo.mean(c, periods=(b, b + 9)) for b in range(0, 60, 10) for c in cols]
    spec = mo.MomentSpec(list(per) + bins, layout=s)
    assert len(spec) == 198
    means, counts, obj = s.simulate_batch_spec(init, spec, seed=4, rndtype=0)
    assert obj is None
    bm, bc, _ = s.simulate_batch_moments(init, seed=4, rndtype=0)
    np_ = len(per)
    assert np.array_equal(counts[:, :np_], bc[:, :, list(cols)].reshape(s.ndraw, -1))
    assert bits_equal(means[:, :np_], bm[:, :, list(cols)].reshape(s.ndraw, -1))
    pm, pc = means[:, :np_].reshape(s.ndraw, s.nt, len(cols)), counts[:, :np_].reshape(s.ndraw, s.nt, len(cols))
    for j, q in enumerate(bins):
        b, c = q.periods[0], cols.index(q.col)
        for d in range(s.ndraw):
            n = pc[d, b:b + 10, c]
            assert counts[d, np_ + j] == n.sum()
            if n.sum():
                ref = float(np.sum(np.where(n > 0, pm[d, b:b + 10, c], 0.0) * n))
                got = means[d, np_ + j] * counts[d, np_ + j]
                assert abs(got - ref) <= 1e-12 * max(abs(ref), 1e-300), (d, j, got, ref)
    assert (counts[:, np_:] > 0).any()


def test_malformed_spec_is_refused_and_the_handle_stays_usable():
    m = examples.retirement2()
    s = gpu_solve(m, m.param_vector()[None])
    init = np.column_stack([np.ones(300), np.linspace(m.a0, m.mmax, 300)])
    spec = _full_spec(m, s.nt, s.lib.info.nd)
    good = s.simulate_batch_spec(init, spec, seed=1)
    rec = spec.pack(s.nt, s.lib.info)
    for field, value in (('kind', 7), ('col', _nout(s)), ('cond_col', -3), ('it_last', s.nt)):
        r = rec.copy()
        r[field][3] = value
        with pytest.raises(runtime.EgdstRuntimeError) as e:
            s.simulate_batch_spec(init, r, seed=1, target=np.zeros(len(r)), W=np.eye(len(r)))
        assert e.value.code == 1
    with pytest.raises(ValueError):
        s.simulate_batch_spec(init, mo.MomentSpec([mo.mean('C', periods=s.nt)]), seed=1)
    again = s.simulate_batch_spec(init, spec, seed=1)
    assert bits_equal(again[0], good[0]) and np.array_equal(again[1], good[1])


def test_diagonal_weights_of_the_batch_moments_path():
    """The weight vector of simulate_batch_moments is the diagonal of W: retirement2, one draw, 300 agents of whom some
    start outside [a0, mmax] and have no value anywhere (on the oracle's paths 260 of the 300 count in every cell that has
    a value; columns 6, 7, 8 and 13 have none in the first period), and the same agents all started above mmax, which
    empties every cell, those of the last period included.  All weights zero: exactly 0.0 whatever is empty; a weight on an
    empty cell: NaN; a weight on a populated cell: w * e * e in the order of the contract, e = mean - target, from the
    returned mean; and np.diag of each vector through simulate_batch_spec with the per-period spec: the same bits."""
    m = examples.retirement2()
    s = gpu_solve(m, m.param_vector()[None])
    nsim, nout = 300, _nout(s)
    ncell = s.nt * nout
    spec = _per_period(s)
    target = np.random.default_rng(17).uniform(0, 2, ncell)
    x = np.random.default_rng(2).uniform(m.a0 - 1, m.mmax + 1, nsim)
    mixed = np.column_stack([np.ones(nsim), x])
    outside = np.column_stack([np.ones(nsim), m.mmax + 1 + np.abs(x)])

    def both_doors(init, w):
        means, counts, obj = s.simulate_batch_moments(init, seed=31, target=target, weight=w)
        sm, sc, so = s.simulate_batch_spec(init, spec, seed=31, target=target, W=np.diag(w))
        assert np.array_equal(sc, counts.reshape(1, -1)) and bits_equal(sm, means.reshape(1, -1)) and bits_equal(so, obj)
        return means.reshape(-1), counts.reshape(-1), obj[0]

    zero = np.zeros(ncell)
    means, counts, obj = both_doors(mixed, zero)
    assert (counts == 0).any() and (counts[-nout:] > 0).all() and 0 < counts.max() < nsim
    assert obj == 0.0 and not np.signbit(obj)
    empty, full = int(np.nonzero(counts == 0)[0][-1]), ncell - nout + 1   # (consumption in the last period)
    w = zero.copy()
    w[empty] = 3.0
    assert np.isnan(both_doors(mixed, w)[2])
    w = zero.copy()
    w[full] = 3.0
    e = means[full] - target[full]
    assert bits_equal(both_doors(mixed, w)[2], w[full] * e * e) and e != 0.0

    means, counts, obj = both_doors(outside, zero)
    assert not counts.any() and np.isnan(means).all()
    assert obj == 0.0 and not np.signbit(obj)
    assert np.isnan(both_doors(outside, w)[2])
