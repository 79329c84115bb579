"""Quantile moments (kind 3) in the estimation step on the device (egdst_simulate_batch_spec, k_quantiles): against
MomentSpec.evaluate on the oracle's paths and against a mask-sort-index written out here, both regimes of the kernel, agents
without values, refused records, and the moments of kinds 0-2 untouched beside them."""
import functools
import math

import numpy as np
import pytest
import torch  # noqa: F401  (first: the model libraries then bind torch's HIP runtime, which the result tensors need)

from egdst_amd import examples, runtime
from egdst_amd import moments as mo
from oracle_harness import Oracle
from test_gpu_parity import gpu_solve
from test_gpu_moment_spec import _full_spec
import estimation_case
from estimation_case import bits_equal

pytestmark = pytest.mark.gpu

SIGNED = 'V'   # a column that takes both signs on the oracle's panel (asserted below)


def _keys(x):
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))


def mask_sort_index(sims, q):
    """(value, count) of the kind-3 record q on a host panel, without moments.py's mirror: the qualifying values, a sort of
    their keys, the key of rank ceil(p n) clamped to [1, n]"""
    f, l_ = int(q['it_first']), int(q['it_last']) + 1
    v = sims[:, f:l_, q['col']]
    ok = ~np.isnan(v)
    if q['cond_col'] >= 0:
        c = sims[:, f:l_, q['cond_col']]
        with np.errstate(invalid='ignore'):
            ok &= (c >= q['cond_lo']) & (c <= q['cond_hi'])
    v = v[ok]
    n = len(v)
    if n == 0:
        return np.nan, 0
    order = np.argsort(_keys(v), kind='stable')
    return v[order[min(max(math.ceil(q['lo'] * float(n)), 1), n) - 1]], n


def _quantile_items(nt, nch):
    items = [mo.median('M', periods=it) for it in range(nt)]
    items += [mo.quantile('A', 0.25, periods=(2, 4)), mo.quantile('A', 0.75, periods=(2, 4)), mo.median('id')]
    items += [mo.median('C', where=('id', k, k)) for k in range(nch)]
    items += [mo.quantile(SIGNED, 0.1), mo.quantile('C', 0.9)]   # pooled over all periods: the global regime
    return items


@functools.lru_cache(maxsize=None)
def _retirement2_case():
    """the 8 perturbed draws of test_full_spec_against_the_oracle, solved once on the device; the oracle's panels per
    (rndtype, draw), None where the oracle fails"""
    m = examples.retirement2()
    rng = np.random.default_rng(21)
    p0 = m.param_vector()
    P = p0[None] * (1 + 0.15 * rng.uniform(-1, 1, (8, len(p0))))
    s = gpu_solve(m, P)
    nsim = 2000
    init = np.column_stack([np.ones(nsim), rng.uniform(m.a0, m.mmax, nsim)])
    base = _full_spec(m, s.nt, s.lib.info.nd)
    spec = mo.MomentSpec(list(base) + _quantile_items(s.nt, s.lib.info.nd), layout=m)
    orc = Oracle(m)
    sols = [orc.solve(p) for p in P]
    panels = {}
    for rndtype in (0, 1):
        rs = estimation_case.uniforms(500 + rndtype, 4 * s.nt * (1 if rndtype == 1 else nsim))
        for d, sol in enumerate(sols):
            panels[rndtype, d] = None if sol.rc != 0 else orc.sim(sol, init, rs, rndtype=rndtype, params=P[d])
    return m, s, init, base, spec, panels


def test_quantiles_against_the_oracle_paths():
    """retirement2, 8 draws, 2000 agents, both rndtype: per-period medians (LDS regime), pooled quantiles (3 periods and all 25:
    the global regime), the median of a column with massive ties, conditional medians and a quantile of a column with both
    signs, next to the moments of kinds 0-2.  Counts equal and means bit-equal to MomentSpec.evaluate(block=256) on the
    oracle's paths and, for the quantiles, to the mask-sort-index above; the objective with a full symmetric W bit-equal to
    moments.objective."""
    m, s, init, base, spec, panels = _retirement2_case()
    nsim, n, nb = len(init), len(spec), len(base)
    rec = spec.pack(s.nt, s.lib.info)
    assert (rec['kind'][nb:] == 3).all() and (rec['kind'][:nb] != 3).all()
    q = s.lib.quantile_lds_keys
    cand = nsim * (rec['it_last'] - rec['it_first'] + 1)
    assert nsim <= q < 3 * nsim and cand[-1] == nsim * s.nt > q and (cand[nb:nb + s.nt] == nsim).all()
    st = s.status()[0]
    rng = np.random.default_rng(77)
    a = rng.normal(size=(n, n))
    W = a @ a.T / n
    target = rng.uniform(0, 1, n)
    finite = 0
    both_signs = False
    for rndtype in (0, 1):
        means, counts, obj = s.simulate_batch_spec(init, spec, seed=500 + rndtype, rndtype=rndtype, target=target, W=W)
        for d in range(s.ndraw):
            sims = panels[rndtype, d]
            if sims is None:
                assert st[d] != 0 and np.isnan(means[d]).all() and not counts[d].any() and np.isnan(obj[d]), d
                continue
            rm, rc = spec.evaluate(sims, block=256)
            assert np.array_equal(counts[d], rc), (rndtype, d)
            assert bits_equal(means[d], rm), (rndtype, d)
            for j in range(nb, n):
                v, c = mask_sort_index(sims, rec[j])
                assert counts[d, j] == c and bits_equal(means[d, j], v), (rndtype, d, j, means[d, j], v)
            assert bits_equal(obj[d], mo.objective(rm, rc, target, W)), (rndtype, d, obj[d])
            finite += int(np.isfinite(obj[d]))
            col = sims[:, :, rec[n - 2]['col']]
            both_signs |= bool((col < 0).any() and (col > 0).any())
    assert finite >= 4 and both_signs


def test_kinds_0_to_2_are_untouched_by_quantile_records():
    """the kinds 0-2 part of the spec alone and inside the mixed spec: the same bits and counts"""
    m, s, init, base, spec, panels = _retirement2_case()
    alone = s.simulate_batch_spec(init, base, seed=500, rndtype=0)
    mixed = s.simulate_batch_spec(init, spec, seed=500, rndtype=0)
    nb = len(base)
    assert bits_equal(mixed[0][:, :nb], alone[0]) and np.array_equal(mixed[1][:, :nb], alone[1])
    assert (alone[1] > 0).any()


def test_agents_without_values():
    """retirement_mortal, one draw, 300 agents, per-period medians of C: deaths leave NaNs, so the counts fall; the same
    agents started above mmax have no value anywhere: every median NaN with count 0, the objective NaN where W touches one
    and exactly 0.0 with W = 0."""
    m = examples.retirement_mortal()
    s = gpu_solve(m)
    nsim = 300
    rng = np.random.default_rng(4)
    x = rng.uniform(m.a0, m.mmax, nsim)
    init = np.column_stack([np.ones(nsim), x])
    spec = mo.MomentSpec([mo.median('C', periods=it) for it in range(s.nt)], layout=m)
    rec = spec.pack(s.nt, s.lib.info)
    n = len(spec)
    target = np.random.default_rng(1).uniform(0, 2, n)
    means, counts, obj = s.simulate_batch_spec(init, spec, seed=12, target=target, W=np.eye(n))
    orc = Oracle(m)
    ref = orc.solve()
    assert ref.rc == 0 and s.status()[0][0] == 0
    sims = orc.sim(ref, init, estimation_case.uniforms(12, 4 * s.nt * nsim), rndtype=0)
    rm, rc = spec.evaluate(sims, block=256)
    assert np.array_equal(counts[0], rc) and bits_equal(means[0], rm)
    for j in range(n):
        v, c = mask_sort_index(sims, rec[j])
        assert counts[0, j] == c and bits_equal(means[0, j], v), j
    assert counts[0, 0] == nsim and 0 < counts[0, -1] < nsim
    assert bits_equal(obj[0], mo.objective(rm, rc, target, np.eye(n))) and np.isfinite(obj[0])

    outside = np.column_stack([np.ones(nsim), m.mmax + 1 + np.abs(x)])
    means, counts, obj = s.simulate_batch_spec(outside, spec, seed=12, target=target, W=np.eye(n))
    assert np.isnan(means).all() and not counts.any() and np.isnan(obj[0])
    w = np.zeros((n, n))
    w[3, 3] = 2.0
    assert np.isnan(s.simulate_batch_spec(outside, spec, seed=12, target=target, W=w)[2][0])
    obj = s.simulate_batch_spec(outside, spec, seed=12, target=target, W=np.zeros((n, n)))[2]
    assert obj[0] == 0.0 and not np.signbit(obj[0])


def test_a_p_outside_the_unit_interval_is_refused_and_the_handle_stays_usable():
    m = examples.retirement2()
    s = gpu_solve(m, m.param_vector()[None])
    init = np.column_stack([np.ones(300), np.linspace(m.a0, m.mmax, 300)])
    spec = mo.MomentSpec([mo.mean('C'), mo.median('M', periods=2), mo.quantile('A', 0.9)], layout=m)
    good = s.simulate_batch_spec(init, spec, seed=1)
    assert (good[1] > 0).all()
    rec = spec.pack(s.nt, s.lib.info)
    for value in (0.0, 1.0, float('nan')):
        r = rec.copy()
        r['lo'][1] = value
        with pytest.raises(runtime.EgdstRuntimeError) as e:
            s.simulate_batch_spec(init, r, seed=1, target=np.zeros(len(r)), W=np.eye(len(r)))
        assert e.value.code == 1
    again = s.simulate_batch_spec(init, spec, seed=1)
    assert bits_equal(again[0], good[0]) and np.array_equal(again[1], good[1])
