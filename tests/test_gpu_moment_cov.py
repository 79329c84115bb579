"""The covariance of the simulated moments on the device (egdst_simulate_batch_spec_cov: k_moment_scores, k_moment_cov) against
MomentSpec.covariance on the oracle's paths for the host replay of the uniforms, bit for bit.  The models, the 8 perturbed
draws, the 700 agents and the oracle's panels are those of tests/test_gpu_lag_moments.py (its cached case is shared): 700
agents are 175 rounds of the 4 partials, 10 passes of 64 staged agents and a last one of 60.  The tile of k_moment_cov is
COV_T = 32 records wide (egdst_amd/csrc/egdst_kernels.hip): spec A (23 / 18 records) is one ragged tile, spec B (146) five tiles
in each direction with a last one of 18, and two more specs have 1 record and exactly 32."""
import functools
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  (first: the model libraries then bind torch's HIP runtime, which the result tensors need)

from egdst_amd import build, runtime, workloads
from egdst_amd import moments as mo
from oracle_harness import Oracle
import estimation_case
from estimation_case import bits_equal
from test_gpu_lag_moments import MODELS, NDRAW, NSIM, SEED, _case, _index, _lag_items

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COV_T = int(re.search(r'^#define COV_T (\d+)', open(os.path.join(ROOT, 'egdst_amd', 'csrc', 'egdst_kernels.hip')).read(),
                      flags=re.M).group(1))


def _spec_a(name):
    """the lag test's records without its two quantiles; the position of the empty record"""
    m, s = _case(name)[:2]
    nch, ix = s.lib.info.nd, _index(s.lib.info.nd)
    items = _lag_items(s.nt, nch)
    assert items[ix['median']].kind == 3 and items[ix['pooled_q']].kind == 3 and ix['pooled_q'] == ix['median'] + 1
    del items[ix['median']:ix['pooled_q'] + 1]
    spec = mo.MomentSpec(items, layout=m)
    assert len(spec) == {'occ3_n400': 23, 'retirement_mortal': 18}[name] and not any(q.kind == 3 for q in spec)
    return spec, ix['empty'] - 2, ix['lead']


def _check_draw(cov, means, counts, ref, empty=None):
    """one draw against the mirror's (means, counts, cov): equal bits; the mirror entries equal in bits; NaN exactly on the rows
    and columns of the records nothing satisfies (the named empty record among them)"""
    rm, rc, rv = ref
    assert np.array_equal(counts, rc), np.nonzero(counts != rc)[0]
    assert bits_equal(means, rm)
    assert bits_equal(cov, rv), np.argwhere(~((cov == rv) | (np.isnan(cov) & np.isnan(rv))))[:5]
    assert np.array_equal(np.isnan(cov), np.isnan(cov.T)) and np.array_equal(np.nan_to_num(cov).view(np.int64),
                                                                             np.nan_to_num(cov.T).view(np.int64))
    nan = rc == 0
    assert np.array_equal(np.isnan(cov), nan[:, None] | nan[None, :])
    if empty is not None:
        assert nan[empty]


@pytest.mark.parametrize('rndtype', [0, 1])
@pytest.mark.parametrize('name', list(MODELS))
def test_spec_a_against_the_mirror(name, rndtype):
    """23 (occ3) / 18 (retirement_mortal) records with the empty one, the lead and lag nt - 1: Omega of every draw bit-equal to
    spec.covariance(panel, block=256, parts=lib.cov_parts), symmetric in bits, NaN exactly on the rows and columns of the
    records nothing satisfies; means and counts bit-equal to simulate_batch_spec on the same spec"""
    m, s, init, _, panels, _ = _case(name)
    spec, empty, lead = _spec_a(name)
    rec = spec.pack_lag(s.nt, s.lib.info)
    assert rec['cond_lag'][lead] == -1 and (rec['lag2'] == s.nt - 1).any() and rec['cond_lo'][empty] == 9
    assert s.lib.cov_parts == 4 and (s.status()[0] == 0).all()
    means, counts, cov = s.simulate_batch_cov(init, spec, seed=SEED + rndtype, rndtype=rndtype)
    m2, c2, _ = s.simulate_batch_spec(init, spec, seed=SEED + rndtype, rndtype=rndtype)
    assert cov.shape == (NDRAW, len(spec), len(spec))
    assert bits_equal(means, m2) and np.array_equal(counts, c2)
    finite = 0
    for d in range(NDRAW):
        ref = spec.covariance(panels[rndtype, d], block=256, parts=s.lib.cov_parts)
        _check_draw(cov[d], means[d], counts[d], ref, empty)
        finite += int(np.isfinite(cov[d]).sum())
    assert finite >= NDRAW * (len(spec) // 2) ** 2


def _bound(d):
    """long-double D'D of the scores and what a summation order may differ from it: n products and n sums of relative error
    2^-53 each, at most n + 1 on a term's path, and sum |d_ij d_ik| <= sqrt(Omega_jj Omega_kk) by Cauchy-Schwarz"""
    ld = d.astype(np.longdouble)
    exact = ld.T @ ld
    diag = np.sqrt(np.diag(exact))
    return exact, 2 * d.shape[0] * 2.0 ** -53 * diag[:, None] * diag[None, :]


def test_spec_b_more_than_one_tile_in_each_direction():
    """occ3, rndtype 0: spec A and the three choice shares of each of the 41 periods, 146 records = 4 tiles of 32 and one of 18.
    Bit-equal to the mirror; within 2 nsim 2^-53 sqrt(Omega_jj Omega_kk) of the long-double D'D of the mirror's scores; and
    in every period the 3 x 3 block of the three shares has rows that sum to zero within the sum of its entries' bounds: shares
    that sum to one have a singular covariance (the scores of an agent sum to (1 - sum of the means) / N, a few roundings)"""
    m, s, init, _, panels, _ = _case('occ3_n400')
    spec_a, empty, _ = _spec_a('occ3_n400')
    base = len(spec_a)
    spec = mo.MomentSpec(list(spec_a) + [mo.share('id', k, periods=it) for it in range(s.nt) for k in range(3)], layout=m)
    n = len(spec)
    assert s.nt == 41 and n == 146 and n > COV_T and n % 16 and n % COV_T
    means, counts, cov = s.simulate_batch_cov(init, spec, seed=SEED, rndtype=0)
    for d in range(NDRAW):
        rm, rc, sc = spec.scores(panels[0, d], block=256)
        ref = spec.covariance(panels[0, d], block=256, parts=s.lib.cov_parts)
        _check_draw(cov[d], means[d], counts[d], ref, empty)
        keep = rc > 0
        exact, bound = _bound(sc[:, keep])
        got = cov[d][np.ix_(keep, keep)].astype(np.longdouble)
        assert (np.abs(got - exact) <= bound).all(), d
        full = np.zeros((n, n), dtype=np.longdouble)
        full[np.ix_(keep, keep)] = bound
        for it in range(s.nt):
            j = base + 3 * it
            assert (rc[j:j + 3] > 0).all(), (d, it)
            blk = cov[d][j:j + 3, j:j + 3].astype(np.longdouble)
            assert (np.abs(blk.sum(axis=1)) <= full[j:j + 3, j:j + 3].sum(axis=1)).all(), (d, it)
            assert (np.diag(cov[d])[j:j + 3] >= 0).all()


@pytest.mark.parametrize('nmom', [1, COV_T])
def test_one_record_and_exactly_one_tile(nmom):
    """nmom = 1 (a tile with one live entry) and nmom = COV_T = 32, the documented width of k_moment_cov's tile (no padding
    column at all): choice 1's share in the first nmom periods of occ3, against the mirror"""
    m, s, init, _, panels, _ = _case('occ3_n400')
    assert COV_T == 32 and nmom <= s.nt
    spec = mo.MomentSpec([mo.share('id', 1, periods=it) for it in range(nmom)], layout=m)
    means, counts, cov = s.simulate_batch_cov(init, spec, seed=SEED, rndtype=0)
    assert cov.shape == (NDRAW, nmom, nmom)
    for d in range(NDRAW):
        _check_draw(cov[d], means[d], counts[d], spec.covariance(panels[0, d], block=256, parts=s.lib.cov_parts))
    assert np.isfinite(cov).all() and (np.diagonal(cov, axis1=1, axis2=2) > 0).any()


@functools.lru_cache(maxsize=None)
def _c2_case():
    m, gen = workloads.c2()
    P = gen(4096)[[0, 1, 2, 3]]
    lib = build.build_model(m)
    s = runtime.Solver(lib, m.descriptor(), ndraw=len(P), keep_history=True)
    s.set_params(P)
    s.solve(raise_on_error=False)
    init = np.column_stack([np.ones(NSIM), np.random.default_rng(8).uniform(m.a0, m.mmax, NSIM)])
    return m, P, s, init


def test_a_failed_draw_is_all_nan():
    """C2 at its defaults (T = 60, 1000 points, a0 = -5), draws 0-3 of gen(4096): draw 2 fails to solve (on the oracle too), so its
    status is not 0, its counts are 0 and its means and Omega NaN; draws 0, 1 and 3 are bit-equal to the mirror"""
    m, P, s, init = _c2_case()
    nt = s.nt
    spec = mo.MomentSpec([mo.mean('C'), mo.mean('M', periods=10), mo.cross('C', 'C', lag=1), mo.cross('M', 'C'),
                          mo.share('id', 1, periods=30), mo.share('id', 0), mo.transition('id', 0, 1), mo.transition('id', 1, 1),
                          mo.mean('C', periods=(0, nt - 2), where=('id', 1, 1, -1)), mo.mean('A', where=('id', 0, 0)),
                          mo.cross('M', 'M', periods=nt - 1, lag=nt - 1), mo.share('M', 0.0, 10.0, periods=(5, 40))], layout=m)
    st = s.status()[0]
    assert st[2] != 0 and (st[[0, 1, 3]] == 0).all(), st
    means, counts, cov = s.simulate_batch_cov(init, spec, seed=SEED, rndtype=0)
    assert (counts[2] == 0).all() and np.isnan(means[2]).all() and np.isnan(cov[2]).all()
    orc = Oracle(m)
    rs = estimation_case.uniforms(SEED, 4 * nt * NSIM)
    for d in range(4):
        sol = orc.solve(P[d])
        assert (sol.rc == 0) == (d != 2), d
        if sol.rc == 0:
            panel = orc.sim(sol, init, rs, rndtype=0, params=P[d])
            _check_draw(cov[d], means[d], counts[d], spec.covariance(panel, block=256, parts=s.lib.cov_parts))
            assert np.isfinite(cov[d]).any()


def test_refusals_and_the_handle_stays_usable():
    """a kind-3 record and one of the lag refusals answer code 1 with the record's index in the message, a null cov_dev code 1;
    afterwards the handle gives the bits it gave before"""
    m, s, init, _, _, _ = _case('retirement_mortal')
    spec, _, _ = _spec_a('retirement_mortal')
    good = s.simulate_batch_cov(init, spec, seed=1)
    rec = spec.pack_lag(s.nt, s.lib.info)
    j = len(rec) - 2
    assert rec['kind'][j] == 0 and rec['cond_col'][j] == -1
    quant = rec.copy()
    quant['kind'][j], quant['lo'][j] = 3, 0.5
    with pytest.raises(runtime.EgdstRuntimeError) as e:
        s.simulate_batch_cov(init, quant, seed=1)
    assert e.value.code == 1 and 'moment %d:' % j in str(e.value) and 'quantile' in str(e.value)
    with pytest.raises(runtime.EgdstRuntimeError) as e:
        s.simulate_batch_cov(init, mo.MomentSpec(list(spec) + [mo.median('M')], layout=m), seed=1)
    assert e.value.code == 1 and 'moment %d:' % len(spec) in str(e.value)
    lagged = rec.copy()
    lagged['lag2'][j] = 1                      # lag2 on a kind other than 1
    with pytest.raises(runtime.EgdstRuntimeError) as e:
        s.simulate_batch_cov(init, lagged, seed=1)
    assert e.value.code == 1 and 'moment %d:' % j in str(e.value)
    tm = torch.zeros(NDRAW, len(rec), dtype=torch.float64, device='cuda')
    torch.cuda.current_stream().synchronize()
    with pytest.raises(runtime.EgdstRuntimeError) as e:    # means_dev given, cov_dev not
        s.simulate_batch_cov(init, spec, seed=1, means_dev=tm.data_ptr())
    assert e.value.code == 1 and 'cov_dev' in str(e.value)
    again = s.simulate_batch_cov(init, spec, seed=1)
    assert bits_equal(again[0], good[0]) and np.array_equal(again[1], good[1]) and bits_equal(again[2], good[2])
    assert np.isfinite(good[2]).any()


def test_the_existing_doors_are_unchanged_after_a_covariance_call():
    """simulate_batch_spec (with quantiles and an objective) and simulate_batch_moments return after a simulate_batch_cov call
    the bits they returned before it: the scores and the slice size of the covariance do not reach them"""
    m, s, init, lag_spec, _, _ = _case('occ3_n400')
    spec, _, _ = _spec_a('occ3_n400')
    n = len(lag_spec)
    rng = np.random.default_rng(3)
    target, W = rng.uniform(0, 1, n), np.diag(rng.uniform(0.5, 1.5, n))
    before = s.simulate_batch_spec(init, lag_spec, seed=SEED, rndtype=0, target=target, W=W)
    cells = s.simulate_batch_moments(init, seed=SEED, rndtype=0)
    s.simulate_batch_cov(init, spec, seed=SEED + 1, rndtype=1)
    after = s.simulate_batch_spec(init, lag_spec, seed=SEED, rndtype=0, target=target, W=W)
    cells2 = s.simulate_batch_moments(init, seed=SEED, rndtype=0)
    assert bits_equal(after[0], before[0]) and np.array_equal(after[1], before[1]) and bits_equal(after[2], before[2])
    assert bits_equal(cells2[0], cells[0]) and np.array_equal(cells2[1], cells[1])
    assert (before[1] > 0).any()
