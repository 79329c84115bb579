"""The tail launch of a period's envelope step (k_tp_tail, egdst_kernels.hip): the cells the throughput path left over and the
second tier of its stage 1 -- until now two launches, k_tp_big and then k_envelope's list pass -- behind one ticket in one
launch.  Both lists are final when it starts; a second-tier cell that gives up is done in place.  None of that may change a bit:
single solves against the oracle with and without the second tier, a 512-draw batch of full-size C2 at a0 = -5 against the
same batch without the second tier and without the throughput path, two solves on one handle, and periods whose lists are
both empty."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from egdst_amd import build, examples, runtime, workloads  # noqa: E402
from oracle_harness import Oracle  # noqa: E402
from parity import compare  # noqa: E402

pytestmark = pytest.mark.gpu
NDRAW = 512


@pytest.mark.parametrize('env', [
    {'EGDST_TP_LKCAP': '40'},                             # everything goes to the second tier
    {'EGDST_TP_LKCAP': '40', 'EGDST_TP_BIGCAP': '52'},    # second tier on, its list empty: this model's lists hold <= 40 or 53..60 points
    {'EGDST_TP_LKCAP': '40', 'EGDST_TP_BIG': '0'},        # leftover cells only
    {'EGDST_TP_LKCAP': '20', 'EGDST_TP_BIGCAP': '52'},    # both lists filled in the same launches
], ids=['second_tier', 'bigcap_52', 'leftover', 'both'])
def test_single_solve_roles_bit_exact(env, monkeypatch):
    monkeypatch.setenv('EGDST_ENV_TP', '1')
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = examples.retirement8(T=5, ngridm=30, ny=3)
    s = runtime.Solver(build.build_model(m), m.descriptor(), ndraw=1, keep_history=True)
    s.set_params(m.param_vector()[None])
    s.solve(raise_on_error=False)
    sol, ref = s.solution(0), Oracle(m).solve()
    assert (sol.status == 0) == (ref.rc == 0)
    ok, rep = compare(sol, ref, rtol=0.0, th_tol=0.0)
    assert ok and sol.nevals == ref.nevals, rep
    done, left = (int(x) for x in s.tp_stats()[0])
    rest, big = s.tp_tail_counts()
    print(env, 'done/left', done, left, 'listed: left over', int(rest.sum()), 'second tier', int(big.sum()), 'in place', int(s.tp_inplace()[0]))
    assert done + left == s.lib.info.nst * (s.nt - 1)   # every cell of every other period went through the path's last stage once
    assert int(rest.sum()) + int(s.tp_inplace()[0]) == left   # a cell is left over through the list or in place, never both
    if env.get('EGDST_TP_BIG') == '0':
        assert big.sum() == 0 and left > 0
    elif env.get('EGDST_TP_LKCAP') == '20':
        assert ((rest > 0) & (big > 0)).any() and left > 0 and done > 0
    elif env.get('EGDST_TP_BIGCAP'):
        assert big.sum() == 0 and left > 0 and done > 0
    else:
        assert big.sum() > 0 and done > 0
    s.close()


def _results(s):
    return (s.status()[0].copy(), s.evals()[1].copy(), s.evals_credited().copy(),
            np.stack([s.checksums(d) for d in range(s.ndraw)]), s.regenerations().copy())


def _same(a, b):
    for name, x, y in zip(('status', 'evaluations', 'credited evaluations', 'checksums', 'regenerations'), a, b):
        assert np.array_equal(x, y), name


def _c2_batch(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m, gen = workloads.c2(a0=-5.0)
    s = runtime.Solver(build.build_model(m, extra_flags=workloads.BATCH_BUILD_FLAGS['C2']), m.descriptor(), ndraw=NDRAW, keep_history=True)
    for k in env:
        monkeypatch.delenv(k)   # (switches are read when the handle is created)
    s.set_groups(3)
    s.set_adaptive(False)
    s.set_params(gen(NDRAW))
    return s


@pytest.fixture(scope='module')
def fused():
    """full-size C2 at a0 = -5, 512 draws on the batch build, three groups: solved twice on one handle"""
    mp = pytest.MonkeyPatch()
    s = _c2_batch(mp, {})
    s.solve(raise_on_error=False)
    first = _results(s) + (s.tp_stats().copy(), s.tp_inplace().copy()) + s.tp_tail_counts()
    s.solve(raise_on_error=False)
    second = _results(s) + (s.tp_stats().copy(), s.tp_inplace().copy()) + s.tp_tail_counts()
    s.close()
    mp.undo()
    return first, second


def test_both_roles_have_work_and_the_in_place_counter_is_exposed(fused):
    first, _ = fused
    tp, inplace, rest, big = first[5:]
    print('tp done/left', tp.sum(axis=0).tolist(), 'listed: left over', int(rest.sum()), 'second tier', int(big.sum()), 'in place', int(inplace.sum()))
    assert rest.sum() > 0 and big.sum() > 0 and ((rest > 0) & (big > 0)).any()
    assert inplace.shape == (NDRAW,) and int(rest.sum()) + int(inplace.sum()) == int(tp[:, 1].sum())


def test_second_solve_on_one_handle_equals_the_first(fused):
    """the ticket and both counters are cleared once per solve"""
    first, second = fused
    _same(second[:5], first[:5])
    for x, y in zip(first[5:], second[5:]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize('env', [{'EGDST_TP_BIG': '0'}, {'EGDST_ENV_TP': '0'}], ids=['no_second_tier', 'k_envelope_alone'])
def test_fused_launch_equals_the_batch_without_it(fused, env, monkeypatch):
    s = _c2_batch(monkeypatch, env)
    s.solve(raise_on_error=False)
    got, tp, big = _results(s), s.tp_stats(), s.tp_tail_counts()[1]
    s.close()
    _same(got, fused[0][:5])
    assert big.sum() == 0
    if 'EGDST_ENV_TP' in env:
        assert tp.sum() == 0                       # the path was off: k_envelope alone did the work
    else:
        # without the second tier its cells are left over instead; every cell still passes the last stage once
        assert np.array_equal(tp.sum(axis=1), fused[0][5].sum(axis=1)) and tp[:, 1].sum() > fused[0][5][:, 1].sum()


def test_periods_with_both_lists_empty_leave_every_table_alone(monkeypatch):
    """C2 at a0 = 0 on a small grid has periods in which the throughput path completes every cell within its regular budget: the
    tail launch reads two zero counts and returns.  Results equal k_envelope's alone."""
    m, gen = workloads.c2(a0=0, ngridm=300, T=30)
    P = gen(600)[:NDRAW]
    res = {}
    for tp in ('default', '0'):
        if tp == '0':
            monkeypatch.setenv('EGDST_ENV_TP', '0')
        s = runtime.Solver(build.build_model(m), m.descriptor(), ndraw=len(P), keep_history=True)
        if tp == '0':
            monkeypatch.delenv('EGDST_ENV_TP')
        s.set_groups(4)
        s.set_adaptive(False)
        s.set_params(P)
        s.solve(raise_on_error=False)
        res[tp] = _results(s) + (s.tp_stats(), s.schedule()[0]) + s.tp_tail_counts()
        s.close()
    _same(res['default'][:5], res['0'][:5])
    tp, groups, rest, big = res['default'][5:]
    nt = m.descriptor()['T'] - m.descriptor()['t0'] + 1
    empty = (rest[:groups, :nt - 1] == 0) & (big[:groups, :nt - 1] == 0)
    print('groups', groups, 'tp done/left', tp.sum(axis=0).tolist(), '(group, period) launches with both lists empty: %d of %d' % (empty.sum(), empty.size))
    assert tp[:, 0].sum() > 0 and empty.any()   # (on these draws: every launch of the solve)
    assert res['0'][5].sum() == 0
