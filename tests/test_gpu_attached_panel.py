"""A data panel attached to a handle and evaluated inside the solve (egdst_attach_panel, egdst_fit_dev, egdst_get_fit): ssr and hits
per draw from handles WITHOUT history (two ping-pong periods) on the caller's stream, enqueued behind egdst_solve_async with no
host synchronisation, held on bits (NaNs matched, no tolerance) to the kept-history door -- egdst_policy_batch fit-only on a
kept-history handle of the same library and draws -- and, where the cases of test_gpu_policy_fit have one, to datafit.fit_mirror on
the oracle's solutions.  Small models with both residuals and both histories, the estimation loop back to back, draws that
fail, one choice with a long table, a build whose schedule is permuted by straggler lanes, and the refusals and the lifetime of
the fit."""
import functools
import os

import numpy as np
import pytest
import torch  # (first: the model libraries then bind torch's HIP runtime, which the tensors here need)

from egdst_amd import build, datafit, examples, runtime, workloads
import estimation_case
from estimation_case import bits_equal
from test_gpu_parity import gpu_solve
from test_gpu_lag_moments import _case as lag_case, MODELS, NDRAW
from test_gpu_policy_fit import _mirror, _oracle, _subset
import test_gpu_estimation_loop as loop

pytestmark = pytest.mark.gpu

# The checking build of test_the_schedule_permuted_by_straggler_lanes: every third draw (i % 3 == 1) is taken for a straggler.
STRAGGLER_EVERY = 3
BUILD_VARIANTS = [(lambda: workloads.c2(a0=0, ngridm=300, T=30)[0], ['-DEG_STRAGGLER_EVERY=%d' % STRAGGLER_EVERY])]


def _yardstick(kept, obs, resid):
    """the kept-history door, fit only"""
    out = kept.policy_batch(obs, resid=resid, want=('ssr', 'hits'))
    return out['ssr'].cpu().numpy(), out['hits'].cpu().numpy()


def _handle(lib, m, ndraw, keep, groups):
    stream = torch.cuda.Stream()
    s = runtime.Solver(lib, m.descriptor(), ndraw=ndraw, keep_history=keep, stream=stream.cuda_stream)
    s.set_groups(groups)
    s._stream = stream   # (kept alive with the handle)
    return s


def _solve_and_fit(s, par, ssr, hits):
    """the loop's step: parameters on the device, the solve, the fit into device tensors; no synchronisation"""
    s.set_params_dev(par.data_ptr())
    s.solve_async()
    s.fit_dev(ssr.data_ptr(), hits.data_ptr())


@functools.lru_cache(maxsize=None)
def _mirror_fit(name, resid, n):
    obs, preds = _mirror(name)
    sub = _subset(obs, n)
    fits = [datafit.fit_mirror(sub, preds[d][0][:n], preds[d][1][:n], resid=resid, block=256) for d in range(NDRAW)]
    return np.array([f[0] for f in fits]), np.array([f[1] for f in fits], dtype=np.int32)


@pytest.mark.parametrize('keep', [False, True])
@pytest.mark.parametrize('resid', [0, 1])
@pytest.mark.parametrize('name', list(MODELS))
def test_small_models_both_residuals_both_histories(name, resid, keep):
    """occ3_n400 and retirement_mortal, the 8 draws, 700 agents and observations of test_gpu_policy_fit (some cons NaN, some id -1,
    some w 0): attach, set_params_dev, solve_async, fit_dev, one sync, with 1 and 3 groups, without and with history; then the
    first 1, 255, 256 and 257 observations, each a re-attach and a solve (n = 1 leaves every period but one without a launch).
    ssr and hits are the kept-history door's and fit_mirror's on policy_mirror's predictions from the oracle's solutions."""
    m, kept, init, spec, panels, refs = lag_case(name)
    P = _oracle(name)[2]
    obs, _ = _mirror(name)
    assert kept.lib.policy_parts == 256 and len(obs) % 256 != 0 and (kept.status()[0] == 0).all()
    assert np.isnan(obs.cons).any() and (obs.id == -1).any() and (obs.w == 0).any()
    par = torch.from_numpy(np.ascontiguousarray(P)).cuda()
    for groups in (1, 3):
        s = _handle(kept.lib, m, NDRAW, keep, groups)
        for n in (len(obs), 1, 255, 256, 257):
            sub = _subset(obs, n)
            ssr = torch.full((NDRAW,), -7.0, dtype=torch.float64, device='cuda')
            hits = torch.full((NDRAW,), -7, dtype=torch.int32, device='cuda')
            torch.cuda.synchronize()
            s.attach_panel(sub, resid=resid)
            _solve_and_fit(s, par, ssr, hits)
            assert s.sync(raise_on_error=False) == 0
            ssr, hits = ssr.cpu().numpy(), hits.cpu().numpy()
            ys, yh = _yardstick(kept, sub, resid)
            assert bits_equal(ssr, ys) and np.array_equal(hits, yh), (groups, n, ssr, ys, hits, yh)
            ms, mh = _mirror_fit(name, resid, n)
            assert bits_equal(ssr, ms) and np.array_equal(hits, mh), (groups, n, ssr, ms, hits, mh)
            if n == len(obs):   # what keeps the comparison from being vacuous
                fin = np.isfinite(ssr)
                assert (hits > 0).all() and ssr[0] == 0.0 and (fin.all() if resid == 0 else fin.sum() >= NDRAW // 2)
        hs, hh = s.fit()   # the host form: the last solve's
        assert bits_equal(hs, ssr) and np.array_equal(hh, hits)
        s.close()


def _panel_of(lib, m, p, nsim=40):
    """the device's own simulated panel of `nsim` agents from a kept-history solve of the draw p, as observations"""
    k = runtime.Solver(lib, m.descriptor(), ndraw=1, keep_history=True)
    k.set_params(p[None])
    assert k.solve(raise_on_error=False) == 0
    init = np.column_stack([np.ones(nsim), np.random.default_rng(8).uniform(m.a0, m.mmax, nsim)])
    panel = k.simulate(init, estimation_case.uniforms(3, 4 * k.nt * nsim), 0, draw=0)
    k.close()
    return datafit.Observations.from_panel(panel, lib.info)


def _run_loop(lib, m, chunks, groups, obs):
    """set_params_dev / solve_async / objective_dev (/ fit_dev with a panel) chunk after chunk, each into its own slice of device
    tensors, nothing else in the loop; one synchronisation afterwards"""
    chunk = len(chunks[0])
    s = _handle(lib, m, chunk, False, groups)
    par = torch.from_numpy(np.stack(chunks)).cuda()
    obj = torch.full((len(chunks), chunk, 2), float('nan'), dtype=torch.float64, device='cuda')
    ssr = torch.full((len(chunks), chunk), -7.0, dtype=torch.float64, device='cuda')
    hits = torch.full((len(chunks), chunk), -7, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    if obs is not None:
        s.attach_panel(obs)
    for c in range(len(chunks)):   # (no host synchronisation in here)
        s.set_params_dev(par[c].data_ptr())
        s.solve_async()
        s.objective_dev(obj[c].data_ptr())
        if obs is not None:
            s.fit_dev(ssr[c].data_ptr(), hits[c].data_ptr())
    s.sync(raise_on_error=False)
    out = obj.cpu().numpy(), ssr.cpu().numpy(), hits.cpu().numpy()
    s.close()
    return out


def _kept_fits(lib, m, chunks, obs):
    """the yardstick per chunk: a kept-history handle's policy_batch, fit only, on that chunk's draws"""
    kept = runtime.Solver(lib, m.descriptor(), ndraw=len(chunks[0]), keep_history=True)
    out = []
    for P in chunks:
        kept.set_params(P)
        kept.solve(raise_on_error=False)
        out.append(_yardstick(kept, obs, 0) + (kept.status()[0].copy(),))
    kept.close()
    return out


def _same_objective(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and loop.bits(a[~np.isnan(a)]) == loop.bits(b[~np.isnan(b)])


@functools.lru_cache(maxsize=None)
def _loop_case(name, draw):
    m, lib, chunks, failed, cache = loop.case(name)
    obs = _panel_of(lib, m, chunks[0][draw])
    return m, lib, chunks, failed, cache, obs, _kept_fits(lib, m, chunks, obs)


@pytest.mark.parametrize('groups', [1, 3])
def test_back_to_back(groups):
    """c2_small of test_gpu_estimation_loop (ngridm 300, T 30): three chunks of 96 draws and the first reversed; the observations
    are the device's own simulated panel of 40 agents of the first draw.  Inside the loop only set_params_dev, solve_async,
    objective_dev and fit_dev, no synchronisation; afterwards every chunk's ssr and hits are a kept-history handle's policy_batch
    on that chunk's draws, and objective_dev's bits are what the same loop gives without a panel."""
    m, lib, chunks, failed, cache, obs, want = _loop_case('c2_small', 0)
    assert len(obs) > 1000 and len(obs) % 256 != 0
    plain = _run_loop(lib, m, chunks, groups, None)[0]
    obj, ssr, hits = _run_loop(lib, m, chunks, groups, obs)
    assert _same_objective(obj, plain) and not np.isnan(obj).any()
    for c, (ys, yh, st) in enumerate(want):
        assert (st == 0).all()
        assert bits_equal(ssr[c], ys) and np.array_equal(hits[c], yh), c
        assert (hits[c] > 0).all() and np.isfinite(ssr[c]).all()
    assert ssr[0][0] == 0.0 and hits[0][0] == len(obs) and ssr[-1][-1] == 0.0   # (the panel's own draw, first and, reversed, last)


@pytest.mark.parametrize('groups', [1, 3])
def test_draws_that_fail(groups):
    """c2_full, the chunks FAIL_FIRST, FAIL_SECOND and the first reversed, in which the draws 67, 9 and 771 fail in the oracle (3, 2
    and 3 per chunk, asserted from the oracle's cache as the loop test does): a failed draw reads NaN and -1; a solved draw at the
    index where the previous chunk's failed, and the other way round, reads the yardstick's bits."""
    m, lib, chunks, failed, cache, obs, want = _loop_case('c2_full', 1)
    rcs = [[int(cache.solve(p).rc != 0) for p in ch] for ch in chunks]
    assert [sum(r) for r in rcs] == failed == [3, 2, 3]
    assert len(obs) % 256 != 0
    obj, ssr, hits = _run_loop(lib, m, chunks, groups, obs)
    swapped = 0
    for c, (ys, yh, st) in enumerate(want):
        bad = np.array(rcs[c], dtype=bool)
        assert np.array_equal(st != 0, bad), (c, st)
        assert np.isnan(ssr[c][bad]).all() and (hits[c][bad] == -1).all(), (c, ssr[c], hits[c])
        assert not np.isnan(ssr[c][~bad]).any() and (hits[c][~bad] > 0).all(), (c, ssr[c], hits[c])
        assert bits_equal(ssr[c], ys) and np.array_equal(hits[c], yh), c
        if c:
            swapped += int((bad != np.array(rcs[c - 1], dtype=bool)).sum())
    assert swapped > 0 and ssr[0][1] == 0.0 and hits[0][1] == len(obs)


def test_one_choice_long_table():
    """C4 at ngridm = 6144, T = 12, ny = 7, 2 draws, without history: the single-choice envelope step (k_env1), cells of more than
    6144 rows and a bisection of 13 steps; 300 uniform observations as in test_gpu_policy_fit's long table, log residuals."""
    rows = 6144
    m, gen = workloads.c4(ngridm=rows, T=12, ny=7)
    P = gen(2)
    kept = gpu_solve(m, P)
    assert (kept.status()[0] == 0).all() and min(kept.dims(d)[0].min() for d in range(2)) > rows
    rng = np.random.default_rng(14)
    n = 300
    obs = datafit.Observations(rng.integers(0, kept.nt, n), rng.integers(0, kept.lib.info.nst, n), rng.uniform(m.a0, m.mmax, n),
                               id=rng.integers(-1, kept.lib.info.nd, n), cons=rng.uniform(0.1, 5.0, n), w=rng.uniform(0.5, 2.0, n))
    ys, yh = _yardstick(kept, obs, 1)
    assert np.isfinite(ys).all()
    s = _handle(kept.lib, m, 2, False, 1)
    s.attach_panel(obs, resid=1)
    s.set_params(P)
    s.solve_async()
    assert s.sync(raise_on_error=False) == 0
    ssr, hits = s.fit()
    assert bits_equal(ssr, ys) and np.array_equal(hits, yh), (ssr, ys, hits, yh)
    s.close()
    kept.close()


def test_the_schedule_permuted_by_straggler_lanes():
    """The small C2 case, the first 96 draws, two groups, no history, on a checking build that forces stragglers.  The re-basing
    counter cannot single draws out of this case, whatever EG_STRAGGLER_CALLS is: Solver.work() on the default build is 0 for
    each of the 96 draws (and for the draws of C2 at full size, with a0 = 0 and a0 = -5: the fixed points that used to dominate
    are fast-forwarded), and with the kernel's floor of 64 calls lowered by hand it was one number for all 96 (205 up to a floor
    of 2, 5 at 4, 0 from 8 on; measured on the MI355X).  So the build is -DEG_STRAGGLER_EVERY=3: egdst_sync takes the draws
    i % 3 == 1 for stragglers, 32 of the 96.  The first solve runs the identity schedule; the second runs the 32 at the end of the
    order: on a lane of their own where the runtime's hardware queues allow one beside the two groups (GPU_MAX_HW_QUEUES unset
    or >= 4, the case on the MI355X machines: asserted), otherwise dealt out over the groups (build_schedule's other branch).
    Either way the order is a real permutation, and ssr and hits of the second solve are the first's and the yardstick's."""
    m, _, chunks, failed, cache, obs, want = _loop_case('c2_small', 0)
    lib = build.build_model(m, extra_flags=BUILD_VARIANTS[0][1])
    P = chunks[0]
    s = _handle(lib, m, len(P), False, 2)
    s.attach_panel(obs)
    par = torch.from_numpy(P).cuda()
    ssr = torch.full((2, len(P)), -7.0, dtype=torch.float64, device='cuda')
    hits = torch.full((2, len(P)), -7, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    assert s.schedule() == (2, 0, 0)
    _solve_and_fit(s, par, ssr[0], hits[0])
    assert s.sync(raise_on_error=False) == 0
    groups, lanes, strag = s.schedule()
    assert groups == 2 and strag == len(P) // STRAGGLER_EVERY and 0 < strag < len(P), (groups, lanes, strag)
    assert not s.work().any()   # (the counter names nobody: the stragglers are the build's)
    if max(int(os.environ.get('GPU_MAX_HW_QUEUES', 4)) - 1, 1) > groups:
        assert lanes > 0, (groups, lanes, strag)
    _solve_and_fit(s, par, ssr[1], hits[1])
    assert s.sync(raise_on_error=False) == 0
    assert s.schedule() == (groups, lanes, strag)
    ssr, hits = ssr.cpu().numpy(), hits.cpu().numpy()
    ys, yh, st = want[0]   # (the default build's kept-history handle: the constant changes the schedule alone)
    for k in (0, 1):
        assert bits_equal(ssr[k], ys) and np.array_equal(hits[k], yh), k
    s.close()


def test_refusals_and_lifetime():
    """every refusal of test_gpu_policy_fit's door through attach_panel, with EGDST_E_ARG and the observation's index named, and
    after each the handle solves and fits with the earlier bits; fit_dev without a panel (1), after the attach and before a
    solve (40), after set_solution on a kept-history handle (40); after the detach a solve's objective is what it was before the
    attach; retirement_hc (a continuous state) is refused with a message that says so."""
    name = 'retirement_mortal'
    m, kept, init, spec, panels, refs = lag_case(name)
    P = _oracle(name)[2]
    obs, _ = _mirror(name)
    rec = obs.pack()[:300]
    k = 123
    s = _handle(kept.lib, m, NDRAW, False, 3)
    s.set_params(P)
    out_s = torch.zeros(NDRAW, dtype=torch.float64, device='cuda')
    out_h = torch.zeros(NDRAW, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    s.solve()
    obj_before = s.objective()
    with pytest.raises(runtime.EgdstRuntimeError) as e:
        s.fit_dev(out_s.data_ptr(), out_h.data_ptr())
    assert e.value.code == 1 and 'panel' in str(e.value)
    s.attach_panel(rec)
    with pytest.raises(runtime.EgdstRuntimeError) as e:
        s.fit_dev(out_s.data_ptr(), out_h.data_ptr())
    assert e.value.code == 40
    s.solve()
    good = s.fit()
    ys, yh = _yardstick(kept, rec, 0)
    assert bits_equal(good[0], ys) and np.array_equal(good[1], yh)
    cases = []
    for field, value in (('it', -1), ('it', s.nt), ('ist', -1), ('ist', s.lib.info.nst), ('id', -2), ('id', s.lib.info.nd), ('reserved', 7),
                         ('cash', np.nan), ('cash', np.nextafter(m.a0, -np.inf)), ('w', np.nan), ('w', -0.5)):
        r = rec.copy()
        r[field][k] = value
        cases.append((r, 0, 'observation %d:' % k))
    r = rec.copy()
    r['cons'][k] = 0.0
    cases += [(r, 1, 'observation %d:' % k), (rec, 2, 'resid'), (rec[:0], 0, '')]
    for r, resid, word in cases:
        with pytest.raises(runtime.EgdstRuntimeError) as e:
            s.attach_panel(r, resid=resid)
        assert e.value.code == 1 and word in str(e.value), (word, str(e.value))
        s.solve()
        again = s.fit()   # (nothing was kept of the refused panel: the earlier one and its bits)
        assert bits_equal(again[0], good[0]) and np.array_equal(again[1], good[1]), word
    with pytest.raises(runtime.EgdstRuntimeError) as e:
        s.fit_dev(None, None)
    assert e.value.code == 1
    s.detach_panel()
    with pytest.raises(runtime.EgdstRuntimeError) as e:
        s.fit()
    assert e.value.code == 1
    s.solve()
    assert loop.bits(s.objective()) == loop.bits(obj_before)
    s.close()
    # an imported solution: the fit answers for solves alone
    h = runtime.Solver(kept.lib, m.descriptor(), ndraw=NDRAW, keep_history=True)
    h.set_params(P)
    h.attach_panel(rec)
    h.solve()
    first = h.fit()
    assert bits_equal(first[0], ys) and np.array_equal(first[1], yh)
    h.set_solution(kept.solution(0), 1)
    with pytest.raises(runtime.EgdstRuntimeError) as e:
        h.fit()
    assert e.value.code == 40
    h.solve()
    again = h.fit()
    assert bits_equal(again[0], ys) and np.array_equal(again[1], yh)
    h.close()
    # a model with continuous states
    mc = examples.retirement_hc()
    c = gpu_solve(mc, keep_history=False)
    with pytest.raises(runtime.EgdstRuntimeError) as e:
        c.attach_panel(datafit.Observations([0, 1], [0, 0], [mc.a0 + 1.0, mc.a0 + 2.0], cons=[0.5, 0.5]))
    assert e.value.code == 1 and 'continuous' in str(e.value), str(e.value)
    c.close()
