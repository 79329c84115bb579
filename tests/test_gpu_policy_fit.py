"""The policy at a data panel's observations on the device (egdst_policy_batch): the simulator identity on the oracle's panels,
every draw against datafit.policy_mirror on its oracle solution and the fit against datafit.fit_mirror, a long table, a failed
draw between solved ones, the refusals (a model with continuous states among them), and egdstmodel.policy.  All comparisons
bit for bit, NaNs matched.  The cases are those of test_gpu_lag_moments (8 perturbed draws, 700 agents: threads 0-187 of the
256 of k_policy_fit add one observation more than the rest in the last round)."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (first: the model libraries then bind torch's HIP runtime, which the result tensors need)

from egdst_amd import datafit, examples, runtime, workloads
from egdst_amd import moments as mo
from oracle_harness import Oracle
from test_gpu_parity import gpu_solve
from test_gpu_lag_moments import _case as lag_case, MODELS, NSIM, NDRAW
from test_gpu_moment_cov import _c2_case
import estimation_case
from estimation_case import bits_equal

pytestmark = pytest.mark.gpu


def _run(s, obs, resid=0, want=runtime.Solver.POLICY_OUTPUTS):
    return {k: v.cpu().numpy() for k, v in s.policy_batch(obs, resid=resid, want=want).items()}


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """the oracle's solutions of the 8 draws of test_gpu_lag_moments' case (the same generator, the same order)"""
    m = MODELS[name][0]()
    p0 = m.param_vector()
    P = p0[None] * (1 + 0.15 * np.random.default_rng(21).uniform(-1, 1, (NDRAW, len(p0))))
    orc = Oracle(m)
    sols = [orc.solve(p) for p in P]
    assert [sol.rc for sol in sols] == [0] * NDRAW
    return m, orc, P, sols


@functools.lru_cache(maxsize=None)
def _mirror(name):
    """observations: the oracle's panel of draw 0 with some consumptions, choices and weights taken out; per draw the mirror's
    predictions on that draw's oracle tables"""
    m, orc, P, sols = _oracle(name)
    panel = lag_case(name)[4][0, 0]
    obs = datafit.Observations.from_panel(panel, m)
    n = len(obs)
    rng = np.random.default_rng(5)
    obs.cons[rng.choice(n, n // 9, replace=False)] = np.nan
    obs.id[rng.choice(n, n // 7, replace=False)] = -1
    obs.w = rng.uniform(0.5, 2.0, n)
    obs.w[rng.choice(n, n // 8, replace=False)] = 0.0
    preds = [datafit.policy_mirror(sols[d], obs, call=lambda sw, a, d=d: orc.call(sols[d], sw, a, params=P[d]), t0=m.t0) for d in range(NDRAW)]
    return obs, preds


def _subset(obs, n):
    return datafit.Observations(obs.it[:n], obs.ist[:n], obs.cash[:n], id=obs.id[:n], cons=obs.cons[:n], w=obs.w[:n])


@pytest.mark.parametrize('name', list(MODELS))
def test_the_simulator_identity_on_every_draws_own_panel(name):
    """observations = all present pairs of the oracle's panel of draw d: the device's cons / id / vf of draw d are the panel's
    columns 1, 4 and 3 (the reference's simulator calls the same policy())"""
    m, s, init, spec, panels, refs = lag_case(name)
    assert NSIM % 256 == 188
    above = 0
    for d in range(NDRAW):
        panel = panels[0, d]
        obs = datafit.Observations.from_panel(panel, s.lib.info)
        present = ~np.isnan(panel[:, :, 0])
        assert len(obs) == present.sum() and len(obs) % 256 != 0
        got = _run(s, obs, want=('cons', 'id', 'vf'))
        rows = panel[present]
        assert bits_equal(got['cons'][d], rows[:, 1]), d
        assert np.array_equal(got['id'][d], rows[:, 4].astype(np.int32)), d
        assert bits_equal(got['vf'][d], rows[:, 3]), d
        above += int((obs.cash > m.mmax).sum())
    assert above > (10000 if name == 'occ3_n400' else 0)   # (agents grow past mmax, in occ3 most of them: the simulator extrapolates there, and so does the door)


@pytest.mark.parametrize('resid', [0, 1])
@pytest.mark.parametrize('name', list(MODELS))
def test_every_draw_against_the_mirror_and_the_fit(name, resid):
    """the panel of draw 0 against all 8 draws: predictions = policy_mirror on each draw's oracle tables, ssr and hits =
    fit_mirror with the library's parts, with some cons NaN, some id -1 and some w 0; and the first 1, 255, 256 and 257 of them"""
    m, s, init, spec, panels, refs = lag_case(name)
    obs, preds = _mirror(name)
    parts = s.lib.policy_parts
    assert parts == 256 and len(obs) % 256 != 0 and (s.status()[0] == 0).all()
    assert np.isnan(obs.cons).any() and (obs.id == -1).any() and (obs.w == 0).any()
    for n in (len(obs), 1, 255, 256, 257):
        sub = _subset(obs, n)
        got = _run(s, sub, resid=resid)
        for d in range(NDRAW):
            c, ids, vf = (a[:n] for a in preds[d])
            assert bits_equal(got['cons'][d], c) and np.array_equal(got['id'][d], ids) and bits_equal(got['vf'][d], vf), (n, d)
            ssr, hits = datafit.fit_mirror(sub, c, ids, resid=resid, block=parts)
            assert bits_equal(got['ssr'][d], ssr) and got['hits'][d] == hits, (n, d, got['ssr'][d], ssr, got['hits'][d], hits)
        if n == len(obs):
            fin = np.isfinite(got['ssr'])   # (resid 1: another draw's policy may extrapolate to a c <= 0 somewhere, whose log is -inf / NaN)
            assert (got['hits'] > 0).all() and (fin.all() if resid == 0 else fin.sum() >= NDRAW // 2)
            assert got['ssr'][0] == 0.0 and (got['ssr'][1:][fin[1:]] > 0).all()
            fit_only = _run(s, sub, resid=resid, want=('ssr', 'hits'))   # (no prediction buffer: the same fit)
            assert bits_equal(fit_only['ssr'], got['ssr']) and np.array_equal(fit_only['hits'], got['hits'])


def test_a_long_table():
    """C4 (deaton, one state) at ngridm = 6144 -- cells of 6145 rows or more, a bisection of 13 steps over a column of 48 KiB --
    2 draws, 300 observations uniform in [a0, mmax]; against the mirror on the device's exported tables (test_gpu_big.py
    holds this library's C4 tables to the oracle)"""
    rows = 6144
    m, gen = workloads.c4(ngridm=rows, T=12, ny=7)
    P = gen(2)
    s = gpu_solve(m, P)
    assert (s.status()[0] == 0).all()
    rng = np.random.default_rng(14)
    n = 300
    obs = datafit.Observations(rng.integers(0, s.nt, n), rng.integers(0, s.lib.info.nst, n), rng.uniform(m.a0, m.mmax, n),
                               id=rng.integers(-1, s.lib.info.nd, n), cons=rng.uniform(0.1, 5.0, n), w=rng.uniform(0.5, 2.0, n))
    got = _run(s, obs, resid=1)
    for d in range(2):
        assert s.dims(d)[0].min() > rows
        c, ids, vf = datafit.policy_mirror(s.solution(d), obs, call=lambda sw, a, d=d: s.call(sw, a, draw=d), t0=m.t0)
        assert bits_equal(got['cons'][d], c) and np.array_equal(got['id'][d], ids) and bits_equal(got['vf'][d], vf), d
        ssr, hits = datafit.fit_mirror(obs, c, ids, resid=1, block=s.lib.policy_parts)
        assert bits_equal(got['ssr'][d], ssr) and got['hits'][d] == hits and np.isfinite(ssr), d
    s.close()


def test_a_failed_draw_between_solved_ones():
    """C2 at its defaults, draws 0-3 of gen(4096): draw 2 fails to solve, so its rows are NaN / -1 / NaN, its ssr NaN and its hits
    -1; draw 0 reproduces the device's own simulated panel of draw 0, draws 1 and 3 the mirror on their exported tables"""
    m, P, s, init = _c2_case()
    st = s.status()[0]
    assert st[2] != 0 and (st[[0, 1, 3]] == 0).all(), st
    nsim = 40
    rs = estimation_case.uniforms(3, 4 * s.nt * nsim)
    panel = s.simulate(init[:nsim], rs, 0, draw=0)
    obs = datafit.Observations.from_panel(panel, s.lib.info)
    assert len(obs) > 1000 and len(obs) % 256 != 0
    got = _run(s, obs)
    assert np.isnan(got['cons'][2]).all() and (got['id'][2] == -1).all() and np.isnan(got['vf'][2]).all()
    assert np.isnan(got['ssr'][2]) and got['hits'][2] == -1
    rows = panel[~np.isnan(panel[:, :, 0])]
    assert bits_equal(got['cons'][0], rows[:, 1]) and np.array_equal(got['id'][0], rows[:, 4].astype(np.int32)) and bits_equal(got['vf'][0], rows[:, 3])
    assert got['ssr'][0] == 0.0 and got['hits'][0] == len(obs)
    for d in (1, 3):
        c, ids, vf = datafit.policy_mirror(s.solution(d), obs, call=lambda sw, a, d=d: s.call(sw, a, draw=d), t0=m.t0)
        assert bits_equal(got['cons'][d], c) and np.array_equal(got['id'][d], ids) and bits_equal(got['vf'][d], vf), d
        ssr, hits = datafit.fit_mirror(obs, c, ids, resid=0, block=s.lib.policy_parts)
        assert bits_equal(got['ssr'][d], ssr) and got['hits'][d] == hits and ssr > 0, d


def test_the_refusals_and_the_other_doors_stay_as_they_were():
    """every refusal answers EGDST_E_ARG and names the observation; simulate_batch_spec on the same handle gives the bits it gave
    before the policy calls"""
    m, s, init, spec, panels, refs = lag_case('retirement_mortal')
    before = s.simulate_batch_spec(init, spec, seed=1)
    obs, _ = _mirror('retirement_mortal')
    rec = obs.pack()[:300]
    k = 123
    good = _run(s, rec)
    cases = []
    for field, value in (('it', -1), ('it', s.nt), ('ist', -1), ('ist', s.lib.info.nst), ('id', -2), ('id', s.lib.info.nd), ('reserved', 7),
                         ('cash', np.nan), ('cash', np.nextafter(m.a0, -np.inf)), ('w', np.nan), ('w', -0.5)):
        r = rec.copy()
        r[field][k] = value
        cases.append((r, 0, ('cons',), 'observation %d:' % k))
    r = rec.copy()
    r['cons'][k] = 0.0
    cases += [(r, 1, ('ssr',), 'observation %d:' % k), (rec, 2, ('cons',), 'resid'), (rec, 0, (), 'no output'), (rec[:0], 0, ('cons',), '')]
    for r, resid, want, word in cases:
        with pytest.raises(runtime.EgdstRuntimeError) as e:
            s.policy_batch(r, resid=resid, want=want)
        assert e.value.code == 1 and word in str(e.value), (word, str(e.value))
    r = rec.copy()
    r['cons'][k] = 0.0   # (a consumption of zero is refused for the log residual only)
    _run(s, r, resid=0)
    again = _run(s, rec)
    assert all(bits_equal(again[key], good[key]) for key in good)
    after = s.simulate_batch_spec(init, spec, seed=1)
    assert bits_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    p = gpu_solve(m, keep_history=False)   # needs the history of every period
    with pytest.raises(runtime.EgdstRuntimeError) as e:
        p.policy_batch(rec, want=('cons',))
    assert e.value.code == 1 and 'keep_history' in str(e.value)
    p.close()


def test_a_model_with_continuous_states_is_refused():
    """retirement_hc (one continuous state, MS_NCONT = 1), solved: the door answers EGDST_E_ARG and says why -- there the
    simulator's policy is a blend over grid corners -- and the handle goes on serving its other doors"""
    m = examples.retirement_hc()
    s = gpu_solve(m)
    assert s.status()[0][0] == 0
    obs = datafit.Observations([0, 1], [0, 0], [m.a0 + 1.0, m.a0 + 2.0], cons=[0.5, 0.5])
    for want in (('cons',), ('ssr', 'hits'), runtime.Solver.POLICY_OUTPUTS):
        with pytest.raises(runtime.EgdstRuntimeError) as e:
            s.policy_batch(obs, want=want)
        assert e.value.code == 1 and 'continuous' in str(e.value), str(e.value)
    assert np.isfinite(s.call(3, [[m.t0, 1]])).all() and s.status()[0][0] == 0   # (the handle goes on serving its other doors)
    s.close()


def test_model_policy_agrees_with_the_batch_door():
    m = examples.retirement_mortal()
    m.compile()
    m.solve()
    s = gpu_solve(m)
    rng = np.random.default_rng(2)
    n = 257
    it, ist, cash = rng.integers(0, s.nt, n), rng.integers(0, s.lib.info.nst, n), rng.uniform(m.a0, m.mmax, n)
    got = _run(s, datafit.Observations(it, ist, cash), want=('cons', 'id', 'vf'))
    c, ids, vf = m.policy(it + m.t0, ist + 1, cash)   # (call's conventions: the model's period, state and decision 1-based)
    assert bits_equal(c, got['cons'][0]) and np.array_equal(ids, got['id'][0] + 1) and bits_equal(vf, got['vf'][0])
    assert (ids >= 1).all() and np.isfinite(c).all()
