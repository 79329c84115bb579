"""The solve as an estimation loop runs it, held to the oracle: one handle without history (two ping-pong periods) on the
caller's stream, parameters by egdst_set_params_dev, egdst_solve_async and egdst_objective_dev chunk after chunk with no host
synchronisation in between.  Only status, counters and the objective leave the device in that mode, so after every chunk the
two live periods are copied where the handle keeps them (Solver.device_tables; tests/estimation_loop_case.py) and compared
with the oracle's: objective, lengths, rows and the zeros past a table's end, on bits.  Then the benchmark's protocol (a
synchronisation and the counters after every chunk), the objective of kept-history handles, the refusals of this surface, and
the estimation step on draws that really fail."""
import ctypes as C

import numpy as np
import pytest
import torch  # (first: the model libraries then bind torch's HIP runtime, which the tensors here need)

from egdst_amd import build, examples, runtime, workloads
from egdst_amd import moments as mo
import estimation_case
import estimation_loop_case as lc

pytestmark = pytest.mark.gpu

FAIL_FIRST, FAIL_SECOND = [67, 0, 1, 9, 2, 3, 771, 4], [5, 6, 67, 7, 8, 10, 11, 9]   # draws 67, 9 and 771 fail in the oracle


def _c2_small():
    m, gen = workloads.c2(a0=0, ngridm=300, T=30)
    return m, lc.chunks_then_first_reversed(gen(1024)[:288], 96, 3), [0, 0, 0, 0]


def _c2_full():
    m, gen = workloads.c2(a0=0)
    P = gen(1024)
    first = np.ascontiguousarray(P[FAIL_FIRST])
    return m, [first, np.ascontiguousarray(P[FAIL_SECOND]), np.ascontiguousarray(first[::-1])], [3, 2, 3]


def _c4():
    m, gen = workloads.c4(ngridm=5000, T=12, ny=7)
    return m, lc.chunks_then_first_reversed(gen(12), 6, 2), [0, 0, 0]


def _retirement8():
    m = examples.retirement8(T=12, ngridm=150, ny=5)
    p0 = m.param_vector()
    P = p0[None] * (1 + 0.15 * np.random.default_rng(21).uniform(-1, 1, (16, len(p0))))
    return m, lc.chunks_then_first_reversed(P, 8, 2), [0, 0, 0]


MODELS = {'c2_small': _c2_small, 'c2_full': _c2_full, 'c4': _c4, 'retirement8': _retirement8}
_CASES = {}


def case(name):
    """(model, its library, chunks of draws, draws per chunk that the oracle fails, the oracle's solutions solved once)"""
    if name not in _CASES:
        m, chunks, failed = MODELS[name]()
        _CASES[name] = (m, build.build_model(m), chunks, failed, lc.OracleCache(m))
    return _CASES[name]


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def run_loop(name, groups):
    """The protocol of every loop test; returns the handle (synchronised once, after the last chunk) and what the checker takes."""
    m, lib, chunks, failed, cache = case(name)
    chunk = len(chunks[0])
    stream = torch.cuda.Stream()
    s = runtime.Solver(lib, m.descriptor(), ndraw=chunk, keep_history=False, stream=stream.cuda_stream)
    s.set_groups(groups)
    par = torch.from_numpy(np.stack(chunks)).cuda()
    obj = torch.full((len(chunks), chunk, 2), float('nan'), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    snaps = []
    for c in range(len(chunks)):   # (no host synchronisation in here)
        s.set_params_dev(par[c].data_ptr())
        s.solve_async()
        s.objective_dev(obj[c].data_ptr())
        snaps.append({it: lc.snapshot_live_period_device(s, it, stream) for it in (0, 1)})
    s.sync(raise_on_error=False)
    st, wh = s.status()
    ev = s.evals()[1]
    obj = obj.cpu().numpy()
    res = [{'P': chunks[c], 'obj': obj[c], 'tabs': {it: lc.to_host(snaps[c][it]) for it in (0, 1)}} for c in range(len(chunks))]
    kept = runtime.Solver(lib, m.descriptor(), ndraw=chunk, keep_history=True)
    kept.set_params(chunks[-1])
    kept.solve(raise_on_error=False)
    last = {'status': st, 'where': wh, 'evals': ev, 'where_kept': kept.status()[1],
            'strerror': lambda code: lib.lib.egdst_strerror(code).decode()}
    kept.close()
    bad = lc.check(cache, res, failed, last)
    return s, bad


@pytest.mark.parametrize('groups', [1, 3])
@pytest.mark.parametrize('tp', ['1', '0'])
def test_loop_two_choices_through_the_throughput_path_and_k_envelope(tp, groups, monkeypatch):
    """C2 at ngridm=300, T=30: 288 draws in three chunks of 96 and the first chunk reversed, with the envelope step's throughput
    path forced on (which then really does cells) and off (k_envelope alone)."""
    monkeypatch.setenv('EGDST_ENV_TP', tp)   # (switches are read when the handle is created)
    s, bad = run_loop('c2_small', groups)
    assert not bad, bad[:6]
    if tp == '1':
        assert s.tp_stats()[:, 0].sum() > 0
    else:
        assert s.tp_stats().sum() == 0
    s.close()


@pytest.mark.parametrize('groups', [1, 3])
def test_loop_with_draws_that_fail(groups):
    """C2 at full size, chunks of 8 in which the draws 67, 9 and 771 fail as in the oracle: a failed draw is followed by a solved
    one at its index and the other way round; NaN objectives, the oracle's message, the kept-history solve's failing period."""
    s, bad = run_loop('c2_full', groups)
    assert not bad, bad[:6]
    s.close()


@pytest.mark.parametrize('groups', [1, 3])
@pytest.mark.parametrize('mode', ['fast', 'defer_late'])
def test_loop_single_choice_tiles(mode, groups, monkeypatch):
    """C4 at ngridm=5000, T=12, ny=7: k_env1 with five tiles per cell, and with every cell handed to k_envelope after its tiles
    wrote rows into the table (EGDST_E1_DEFER_ALL=2)."""
    if mode == 'defer_late':
        monkeypatch.setenv('EGDST_E1_DEFER_ALL', '2')
    s, bad = run_loop('c4', groups)
    assert not bad, bad[:6]
    s.close()


@pytest.mark.parametrize('groups', [1, 3])
def test_loop_eight_states(groups):
    """retirement8(T=12, ngridm=150, ny=5), 16 perturbed draws: the live tables of all eight states."""
    s, bad = run_loop('retirement8', groups)
    assert not bad, bad[:6]
    s.close()


def test_benchmark_protocol_against_the_oracle():
    """What bench.py's run_step does with a handle: after every chunk a synchronisation, status, evaluation counts and credited
    evaluations read back, then egdst_objective_dev on the handle's stream; default groups, history scheduling left on.  For
    every chunk status (zero or not, and the text), the evaluation counts of the solved draws and the objective are the
    oracle's, and the loop once more on the same handle gives the same bits."""
    m, lib, chunks, failed, cache = case('c2_full')
    chunk = len(chunks[0])
    stream = torch.cuda.Stream()
    s = runtime.Solver(lib, m.descriptor(), ndraw=chunk, keep_history=False, stream=stream.cuda_stream)
    par = torch.from_numpy(np.stack(chunks)).cuda()
    obj = torch.full((2, len(chunks), chunk, 2), float('nan'), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    read = []
    for rep in range(2):
        for c in range(len(chunks)):
            s.set_params_dev(par[c].data_ptr())
            s.solve_async()
            s.sync(raise_on_error=False)
            st, wh = s.status()
            read.append((st, wh, s.evals()[1], s.evals_credited()))
            with torch.cuda.stream(stream):
                s.objective_dev(obj[rep, c].data_ptr())
    torch.cuda.synchronize()
    obj = obj.cpu().numpy()
    nfail = []
    for c in range(len(chunks)):
        st, wh, ev, cred = read[c]
        refs = [cache.solve(p) for p in chunks[c]]
        nfail.append(sum(int(r.rc != 0) for r in refs))
        for d, ref in enumerate(refs):
            assert (st[d] == 0) == (ref.rc == 0), (c, d, st[d], ref.err)
            if ref.rc:
                assert lib.lib.egdst_strerror(int(st[d])).decode().strip() == ref.err.strip(), (c, d)
                assert np.isnan(obj[0, c, d]).all(), (c, d, obj[0, c, d])
            else:
                assert ev[d] == ref.nevals, (c, d, ev[d], ref.nevals)
                assert bits(obj[0, c, d]) == bits(np.array([ref.V[0, 0, 1], ref.C[0, 0, 1]])), (c, d, obj[0, c, d])
        again = read[len(chunks) + c]
        assert all(np.array_equal(a, b) for a, b in zip(read[c], again)), c
    assert nfail == failed
    nan = np.isnan(obj[0])
    assert np.array_equal(nan, np.isnan(obj[1])) and bits(obj[0][~nan]) == bits(obj[1][~nan])
    s.close()


@pytest.mark.parametrize('name', sorted(MODELS))
def test_objective_of_a_kept_history_handle(name):
    """8 draws solved synchronously with the history kept: objective() is the oracle's (V, C) of row 1 of the cell (it = 0,
    ist = 0), the same bits as the exported solution's, and NaN for a draw that fails."""
    m, lib, chunks, failed, cache = case(name)
    P = np.ascontiguousarray(np.concatenate(chunks[:-1])[:8])
    s = runtime.Solver(lib, m.descriptor(), ndraw=len(P), keep_history=True)
    s.set_params(P)
    s.solve(raise_on_error=False)
    obj = s.objective()
    refs = [cache.solve(p) for p in P]
    assert sum(int(r.rc != 0) for r in refs) == (failed[0] if name == 'c2_full' else 0)
    for d, ref in enumerate(refs):
        if ref.rc:
            assert np.isnan(obj[d]).all(), (d, obj[d])
            continue
        assert bits(obj[d]) == bits(np.array([ref.V[0, 0, 1], ref.C[0, 0, 1]])), (d, obj[d])
        sol = s.solution(d)
        assert bits(obj[d]) == bits(np.array([sol.V[0, 0, 1], sol.C[0, 0, 1]])), (d, obj[d])
    s.close()


def test_refusals_leave_the_handle_usable():
    """egdst_objective_dev before any solve, egdst_set_params_dev with another number of draws, egdst_device_tables past the last
    period, and the cell exports on a handle without history are refused with their codes; after each of them the handle
    solves and its objective is the oracle's."""
    m, lib, chunks, failed, cache = case('c2_small')
    P = np.ascontiguousarray(chunks[0][:4])
    want = np.array([[r.V[0, 0, 1], r.C[0, 0, 1]] for r in (cache.solve(p) for p in P)])
    assert all(cache.solve(p).rc == 0 for p in P)
    stream = torch.cuda.Stream()
    s = runtime.Solver(lib, m.descriptor(), ndraw=len(P), keep_history=False, stream=stream.cuda_stream)
    par = torch.from_numpy(P).cuda()
    obj = torch.full((len(P), 2), float('nan'), dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()

    def solves():
        obj.fill_(float('nan'))
        torch.cuda.synchronize()
        s.set_params_dev(par.data_ptr())
        s.solve_async()
        s.objective_dev(obj.data_ptr())
        assert s.sync(raise_on_error=False) == 0
        assert bits(obj.cpu().numpy()) == bits(want)

    refusals = [(40, lambda: s.objective_dev(obj.data_ptr())),
                (1, lambda: lib.check(lib.lib.egdst_set_params_dev(s.h, C.c_void_p(par.data_ptr()), s.ndraw + 1))),
                (1, lambda: s.device_tables(s.nt)),
                (1, lambda: s.checksums(0)),
                (1, lambda: s.cell_M(0, 0, 0))]
    for code, call in refusals:
        with pytest.raises(runtime.EgdstRuntimeError) as e:
            call()
        assert e.value.code == code, (code, e.value)
        solves()
    s.close()


def test_estimation_step_with_draws_that_fail():
    """C2 at full size with the history kept, eight draws of which 67, 9 and 771 fail, 500 agents: through simulate_batch_moments
    and through simulate_batch_spec with the per-period spec and a diagonal W the failed draws give all-NaN means, zero counts
    and a NaN objective (k_simulate skips them, k_fill_nan), and the solved ones the bits of MomentSpec.evaluate(block=256) and
    moments.objective on the oracle's paths for the host replay of the uniforms."""
    m, lib, chunks, failed, cache = case('c2_full')
    P = chunks[0]
    s = runtime.Solver(lib, m.descriptor(), ndraw=len(P), keep_history=True)
    s.set_params(P)
    s.solve(raise_on_error=False)
    st = s.status()[0]
    refs = [cache.solve(p) for p in P]
    assert [d for d, r in enumerate(refs) if r.rc] == [0, 3, 6] and [int(x != 0) for x in st] == [int(r.rc != 0) for r in refs]
    nsim, nout = 500, s.lib.nout
    init = np.column_stack([np.ones(nsim), np.random.default_rng(5).uniform(m.a0 - 0.5, m.mmax + 0.5, nsim)])
    target = np.random.default_rng(3).uniform(0, 2, (s.nt, nout))
    weight = np.zeros((s.nt, nout))
    weight[1:, 1] = 1.0
    weight[1:, 4] = 4.0
    spec = mo.MomentSpec([mo.mean(c, periods=it) for it in range(s.nt) for c in range(nout)], layout=s)
    for rndtype in (0, 1):
        seed = 77 + rndtype
        bm, bc, bo = s.simulate_batch_moments(init, seed=seed, rndtype=rndtype, target=target, weight=weight)
        sm, sc, so = s.simulate_batch_spec(init, spec, seed=seed, rndtype=rndtype, target=target.reshape(-1), W=np.diag(weight.reshape(-1)))
        rs = estimation_case.uniforms(seed, 4 * s.nt * (1 if rndtype == 1 else nsim))
        finite = 0
        for d, ref in enumerate(refs):
            for means, counts, obj in ((bm[d].reshape(-1), bc[d].reshape(-1), bo[d]), (sm[d], sc[d], so[d])):
                if ref.rc:
                    assert np.isnan(means).all() and not counts.any() and np.isnan(obj), (rndtype, d)
                    continue
                rm, rc = spec.evaluate(cache.orc.sim(ref, init, rs, rndtype=rndtype, params=P[d]), block=256)
                assert np.array_equal(counts, rc), (rndtype, d)
                nan = np.isnan(rm)
                assert np.array_equal(np.isnan(means), nan) and bits(means[~nan]) == bits(rm[~nan]), (rndtype, d)
                ro = mo.objective(rm, rc, target.reshape(-1), weight.reshape(-1))
                assert (np.isnan(ro) and np.isnan(obj)) or bits(np.float64(obj)) == bits(np.float64(ro)), (rndtype, d, obj, ro)
                finite += int(np.isfinite(obj))
        assert finite > 0
    s.close()
