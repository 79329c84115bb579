"""The envelope step's rare recoveries, forced in checking builds of the device code and held to the oracle bit for bit:

* -DEG_SEG_FAIL_EVERY=n  the check of a cut walk's predictions fails for every n-th walk (run_walk, egdst_kernels.hip): wave 0 walks
  the stream again from the job's own arrays after the segments have written the scratch rows -- in k_envelope's two-part form with
  the streams in LDS (run_walk<1>) and in global memory (<0>), with one workgroup per cell, and on the throughput path (<2>: the
  class words are row numbers by then and the stream is classified again), in its regular launches and in k_tp_tail's second tier;
* -DEG_TP_GIVEUP_EVERY=n -DEG_TP_GIVEUP_AT=13|14  a cell of the throughput path gives up AFTER its stage-0 walk has overwritten its
  lists (13) or after its stage-1 walk has written rows into the period's table and set the high-water marks to "unknown" (14):
  eg_envelope_cell redoes it from the untouched candidates, from the list or, in the second tier, in place;
* -DEG_TP_TAIL_GIVEUP_EVERY=2  a second-tier cell that gives up before it touches anything, on the device.

No tolerance anywhere: single solves equal Oracle(m).solve() (tables, thresholds, evaluations); batches equal the default build
on every draw (status, evaluations, credited evaluations, regenerations, the checksums of every cell) and the oracle on a sample.
Every shape is first shown to cut walks in the DEFAULT build in that configuration (walk_stats: merged + fallback > 0), and the
forced build must plan the same cuts: per draw merged + fallback is the default build's.

Shapes (a walk is cut from 2 * ENV_SEG_MINPTS = 384 sorted points up): C2 at ngridm = 300, T = 30 (two choices, ~600-point
primaries), occ3 at ngridm = 400 (three choices, 1200-point primaries, folded 400-point lists whose secondary walks are cut too),
occ3 at ngridm = 1400 for streams that do not fit the LDS."""
import functools
import os
import sys

import numpy as np
import pytest
import torch  # (first: the model libraries then bind torch's HIP runtime, which the copies of the live periods need)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from egdst_amd import build, examples, runtime, workloads  # noqa: E402
from oracle_harness import Oracle  # noqa: E402
from parity import compare  # noqa: E402

pytestmark = pytest.mark.gpu

MODELS = {
    'c2': lambda: workloads.c2(a0=0, ngridm=300, T=30)[0],
    'occ3': lambda: examples.occ3(ngridm=400, ngridmax=4000, nthrhmax=400, ny=15),                  # SCALED['occ3_n400']
    'occ3_n1400': lambda: examples.occ3(T=12, ngridm=1400, ngridmax=14000, nthrhmax=1400, ny=10),   # SCALED['occ3_n1400_global_path']
    'retire8': lambda: examples.retirement8(T=5, ngridm=30, ny=3),
}
NBATCH = 96   # draws of the C2 batches on the throughput path
NCELLS = 160  # draws of the batch for k_envelope with one workgroup per cell: C2 has one state, and up to EG_ENV_WIDE_MAX_CELLS = 128
              # (draw, state) cells per solve the host launches k_envelope in two parts (plan_launches, egdst_host.inc)


def _seg(n):
    return ['-DEG_SEG_FAIL_EVERY=%d' % n]


def _giveup(at, n):
    return ['-DEG_TP_GIVEUP_EVERY=%d' % n, '-DEG_TP_GIVEUP_AT=%d' % at]


COMBINED = _seg(2) + _giveup(14, 2)
TAIL_GIVEUP = ['-DEG_TP_TAIL_GIVEUP_EVERY=2']
FORCING = [_seg(1), _seg(2), _giveup(13, 1), _giveup(13, 2), _giveup(14, 1), _giveup(14, 2), COMBINED]
# (model factory, extra hipcc flags): compiled by __graft_entry__.build() beforehand.  Libraries are keyed by the model's plugin, not by its
# grid size: occ3 at 400 and at 1400 points share theirs.
BUILD_VARIANTS = [(MODELS[name], flags) for name in ('c2', 'occ3') for flags in FORCING] + [(MODELS['retire8'], TAIL_GIVEUP)]

# configurations of the issue: model, switches (read when the handle is created), draws, groups
TP0, TP1 = {'EGDST_ENV_TP': '0'}, {'EGDST_ENV_TP': '1'}
CONFIGS = {
    'a_c2_two_parts': ('c2', TP0, 1, 0),                                        # k_envelope parts 1 + 2, run_walk<1>
    'a_occ3_two_parts': ('occ3', TP0, 1, 0),
    'b_c2_global': ('c2', dict(TP0, EGDST_LCAP='200'), 1, 0),                   # streams in global memory: run_walk<0>
    'b_occ3_global': ('occ3', dict(TP0, EGDST_LCAP='200'), 1, 0),
    'b_occ3_n1400_global': ('occ3_n1400', TP0, 1, 0),                           # (3 x 1400 points do not fit the LDS as it is)
    'c_c2_batch_one_workgroup_per_cell': ('c2', TP0, NCELLS, 0),                 # part 0: the jobs of a cell one after another
    'd_occ3_tp': ('occ3', TP1, 1, 0),                                           # k_tp_walk stages 0 and 1, run_walk<2>
    'd_c2_tp_batch': ('c2', TP1, NBATCH, 3),
    # stream budgets below the ~600 / ~1200 points of the primaries: the cut walks of stage 1 are the second tier's, inside k_tp_tail
    'e_occ3_second_tier': ('occ3', dict(TP1, EGDST_TP_LKCAP='600'), 1, 0),
    'e_c2_second_tier_batch': ('c2', dict(TP1, EGDST_TP_LKCAP='400'), NBATCH, 3),
}
SECOND_TIER = ('e_occ3_second_tier', 'e_c2_second_tier_batch')
TP_CONFIGS = ('d_occ3_tp', 'd_c2_tp_batch') + SECOND_TIER


@functools.lru_cache(maxsize=None)
def _model(name):
    return MODELS[name]()


@functools.lru_cache(maxsize=None)
def _params(name, ndraw):
    if ndraw == 1:
        return _model(name).param_vector()[None].copy()
    assert name == 'c2'
    return workloads.c2(a0=0, ngridm=300, T=30)[1](600)[:ndraw]   # the first draws of the generator's 600


@functools.lru_cache(maxsize=None)
def _oracle(name, draw=None):
    """the oracle's solution of the model as shipped (draw None) or of a draw of the C2 batch: solved once, left unchanged"""
    return Oracle(_model(name)).solve(None if draw is None else _params(name, 600)[draw])


def _solver(name, flags, env, ndraw, groups, keep_history=True):
    m = _model(name)
    lib = build.build_model(m, extra_flags=flags)
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        s = runtime.Solver(lib, m.descriptor(), ndraw=ndraw, keep_history=keep_history)
    if groups:
        s.set_groups(groups)
        s.set_adaptive(False)
    s.set_params(_params(name, ndraw))
    return s


def _counts(s):
    rest, big = s.tp_tail_counts()
    return {'walks': s.walk_stats().astype(np.int64), 'tp': s.tp_stats().astype(np.int64), 'inplace': s.tp_inplace().astype(np.int64),
            'rest': rest.copy(), 'big': big.copy()}


def _results(s):
    """what the default build and a forced one must agree on for every draw (test_gpu_tp_tail.py), and the failing cell"""
    return (s.status()[0].copy(), s.evals()[1].copy(), s.evals_credited().copy(),
            np.stack([s.checksums(d) for d in range(s.ndraw)]), s.regenerations().copy(), s.status()[1].copy())


NAMES = ('status', 'evaluations', 'credited evaluations', 'checksums', 'regenerations', 'failing cell')


def _same(a, b, what):
    for name, x, y in zip(NAMES, a, b):
        assert np.array_equal(x, y), (what, name)


def _oracle_sample(ndraw, status):
    """draws held to the oracle: a single solve's one; of a batch eight spread over it and the first that fail"""
    if ndraw == 1:
        return [0]
    return sorted(set(range(0, ndraw, ndraw // 8)) | set(int(k) for k in np.nonzero(status)[0][:3]))


def _check_oracle(s, name, what):
    st = s.status()[0]
    for d in _oracle_sample(s.ndraw, st):
        ref = _oracle(name, None if s.ndraw == 1 else d)
        sol = s.solution(d)
        assert (sol.status == 0) == (ref.rc == 0), (what, d, sol.status, ref.err)
        if ref.rc:
            assert sol.err.strip() == ref.err.strip(), (what, d)
        ok, rep = compare(sol, ref, rtol=0.0, th_tol=0.0)   # (of a failing draw: the partial tables)
        # (the evaluations of a draw that fails are the default build's, not the oracle's: the device has evaluated the other cells of the
        #  failing period, as in every test of failing draws in test_gpu_parity.py)
        assert ok and (ref.rc != 0 or sol.nevals == ref.nevals), (what, d, rep, sol.nevals, ref.nevals)


@functools.lru_cache(maxsize=None)
def _default(cfg):
    """the default build in a configuration: (results, counts) of one solve, itself held to the oracle"""
    name, env, ndraw, groups = CONFIGS[cfg]
    s = _solver(name, [], env, ndraw, groups)
    s.solve(raise_on_error=False)
    _check_oracle(s, name, (cfg, 'default build'))
    out = _results(s), _counts(s)
    s.close()
    return out


def _cells(s):
    return s.lib.info.nst * (s.nt - 1)


@pytest.mark.parametrize('cfg', sorted(CONFIGS))
def test_the_shapes_cut_walks_in_the_default_build(cfg):
    """What every test below relies on.  On the throughput path of the three-choice model the cut walks outnumber the (period, state)
    cells: the secondary walks of stage 0 are cut as well as the primaries."""
    _, cnt = _default(cfg)
    merged, fallback = cnt['walks'].sum(axis=0)
    print(cfg, 'default build: merged/fallback', int(merged), int(fallback), 'tp done/left', cnt['tp'].sum(axis=0).tolist(),
          'listed: left over', int(cnt['rest'].sum()), 'second tier', int(cnt['big'].sum()), 'in place', int(cnt['inplace'].sum()))
    assert merged + fallback > 0
    nt, nst = _default(cfg)[0][3].shape[1:3]   # (the checksums: [draw, period, state, column])
    if cfg.startswith('c_'):
        assert CONFIGS[cfg][2] * nst > 128   # (more cells than k_envelope does in two parts)
    if cfg == 'd_occ3_tp':
        assert merged + fallback > nst * (nt - 1)
    if cfg in SECOND_TIER:
        assert cnt['big'].sum() > 0 and cnt['inplace'].sum() == 0
    if cfg in TP_CONFIGS:
        assert (cnt['tp'].sum(axis=1) == nst * (nt - 1)).all() and cnt['tp'][:, 0].sum() > 0
    else:
        assert cnt['tp'].sum() == 0


def _check_forced(cfg, flags, s, what):
    """one solve of a forced build against the oracle and the default build; returns its counts"""
    name = CONFIGS[cfg][0]
    ref_res, ref_cnt = _default(cfg)
    _check_oracle(s, name, what)
    _same(_results(s), ref_res, what)
    cnt = _counts(s)
    # the plan of the cuts does not depend on the outcome of the check -- unless the cell's path changed: a cell that gives up is walked
    # again by the envelope code, so only the builds that force nothing but the check are held to the default build's number of cut walks
    if not any(f.startswith('-DEG_TP_GIVEUP') for f in flags):
        assert np.array_equal(cnt['walks'].sum(axis=1), ref_cnt['walks'].sum(axis=1)), what
    return cnt


@pytest.mark.parametrize('n', [1, 2])
@pytest.mark.parametrize('cfg', sorted(CONFIGS))
def test_failed_predictions_are_walked_again_bit_exact(cfg, n):
    """-DEG_SEG_FAIL_EVERY=n.  n = 1: no cut walk is merged, every one is walked again by wave 0; n = 2: both outcomes, for the walks of
    one cell in the same workgroup's job loop (the primary's identity is period + state, a secondary's that plus its choice + 1)."""
    name, env, ndraw, groups = CONFIGS[cfg]
    s = _solver(name, _seg(n), env, ndraw, groups)
    s.solve(raise_on_error=False)
    cnt = _check_forced(cfg, _seg(n), s, (cfg, n))
    merged, fallback = cnt['walks'].sum(axis=0)
    print(cfg, 'EG_SEG_FAIL_EVERY=%d' % n, 'merged/fallback', int(merged), int(fallback), 'default build', _default(cfg)[1]['walks'].sum(axis=0).tolist())
    if n == 1:
        assert merged == 0 and fallback > 0
    else:
        assert merged > 0 and fallback > 0
    if cfg in TP_CONFIGS:   # falling back is no reason to give a cell up
        assert np.array_equal(cnt['tp'], _default(cfg)[1]['tp']) and np.array_equal(cnt['inplace'], _default(cfg)[1]['inplace'])
    s.solve(raise_on_error=False)
    assert np.array_equal(_counts(s)['walks'], cnt['walks'])   # the decision depends on the walk's identity alone
    s.close()


def _check_giveup_counts(cfg, at, n, s, cnt, what):
    ref_cnt = _default(cfg)[1]
    done, left = cnt['tp'][:, 0], cnt['tp'][:, 1]
    assert (done + left == _cells(s)).all(), what             # every cell passes the path's last stage once, whoever flagged it
    assert cnt['rest'].sum() + cnt['inplace'].sum() == left.sum(), what   # left over through the list or in place, never both
    if n == 1:
        if at == 14:
            assert done.sum() == 0, what
        else:   # every folded list's cell gives up after its secondary walk: more than gave up by themselves
            assert left.sum() > ref_cnt['tp'][:, 1].sum(), what
    else:
        assert done.sum() > 0 and left.sum() > 0, what
    if cfg in SECOND_TIER and at == 14:
        assert cnt['inplace'].sum() > 0, what
    else:
        assert cnt['inplace'].sum() == 0, what                # (a stage-0 give-up is seen by the stage-1 sort: the cell is never second tier)


@pytest.mark.parametrize('n', [1, 2])
@pytest.mark.parametrize('at', [13, 14])
@pytest.mark.parametrize('cfg', TP_CONFIGS)
def test_cells_that_give_up_after_their_walk_are_redone_bit_exact(cfg, at, n):
    """-DEG_TP_GIVEUP_EVERY=n -DEG_TP_GIVEUP_AT=13|14 on the throughput path and its second tier; a second solve on the handle counts
    the same and gives the same tables."""
    name, env, ndraw, groups = CONFIGS[cfg]
    s = _solver(name, _giveup(at, n), env, ndraw, groups)
    s.solve(raise_on_error=False)
    cnt = _check_forced(cfg, _giveup(at, n), s, (cfg, at, n))
    print(cfg, 'EG_TP_GIVEUP_AT=%d EVERY=%d' % (at, n), 'done/left', cnt['tp'].sum(axis=0).tolist(), 'listed', int(cnt['rest'].sum()),
          'second tier', int(cnt['big'].sum()), 'in place', int(cnt['inplace'].sum()), 'merged/fallback', cnt['walks'].sum(axis=0).tolist())
    _check_giveup_counts(cfg, at, n, s, cnt, (cfg, at, n))
    s.solve(raise_on_error=False)
    again = _counts(s)
    for k in cnt:
        assert np.array_equal(again[k], cnt[k]), (cfg, at, n, 'second solve', k)
    _same(_results(s), _default(cfg)[0], (cfg, at, n, 'second solve'))
    s.close()


def _live_periods(s):
    """{period: {'M', 'C', 'V', 'len'}} of the two periods a handle without history holds after a solve"""
    import estimation_loop_case as lc
    return {it: lc.to_host(lc.snapshot_live_period_device(s, it, torch.cuda.current_stream())) for it in (0, 1)}


def _check_live(s, kept, what):
    """status, evaluations, objective and the rows of periods 0 and 1 -- zeros past their ends -- against the kept-history solve"""
    assert np.array_equal(s.status()[0], kept.status()[0]) and np.array_equal(s.status()[1], kept.status()[1]), what
    assert np.array_equal(s.evals()[1], kept.evals()[1]), what
    assert s.objective().tobytes() == kept.objective().tobytes(), what
    tabs = _live_periods(s)
    for d in range(s.ndraw):
        if kept.status()[0][d]:
            continue
        sol = kept.solution(d)
        for it in (0, 1):
            for ist in range(s.lib.info.nst):
                n = int(sol.len[it, ist])
                assert int(tabs[it]['len'][d, ist]) == n, (what, d, it, ist)
                for col in 'MCV':
                    row = tabs[it][col][d, ist]
                    assert row[:n].tobytes() == getattr(sol, col)[it, ist, :n].tobytes(), (what, d, it, ist, col)
                    assert not row[n:].view(np.int64).any(), (what, d, it, ist, col, 'rows past the end')


@pytest.mark.parametrize('flags', [_seg(1), _seg(2), _giveup(13, 1), _giveup(13, 2), _giveup(14, 1), _giveup(14, 2)], ids=lambda f: '_'.join(x[4:] for x in f))
@pytest.mark.parametrize('cfg', ['d_occ3_tp', 'd_c2_tp_batch'])
def test_recoveries_without_history_solved_twice_on_one_handle(cfg, flags):
    """Two ping-pong periods: a walk that is done again, and a cell that is redone after its walk wrote rows into the slot's table, must
    leave nothing of the first attempt nor of the previous period or solve behind.  The kept-history solve of the same build (held to
    the oracle by the tests above) is the comparison, as in test_single_choice_envelope_tiles_and_hand_over."""
    name, env, ndraw, groups = CONFIGS[cfg]
    kept = _solver(name, flags, env, ndraw, groups)
    kept.solve(raise_on_error=False)
    _same(_results(kept), _default(cfg)[0], (cfg, flags, 'kept history'))
    s = _solver(name, flags, env, ndraw, groups, keep_history=False)
    counts = []
    for k in range(2):
        s.solve(raise_on_error=False)
        _check_live(s, kept, (cfg, flags, 'solve %d' % k))
        counts.append(_counts(s))
    want = _counts(kept)
    for k in want:
        assert np.array_equal(counts[0][k], want[k]) and np.array_equal(counts[1][k], want[k]), (cfg, flags, k)
    print(cfg, flags, 'no history: merged/fallback', want['walks'].sum(axis=0).tolist(), 'done/left', want['tp'].sum(axis=0).tolist(),
          'in place', int(want['inplace'].sum()))
    if flags[0].startswith('-DEG_SEG'):
        assert want['walks'][:, 1].sum() > 0
    else:
        _check_giveup_counts(cfg, int(flags[1][-2:]), int(flags[0][-1:]), s, want, (cfg, flags))
    s.close()
    kept.close()


@pytest.mark.parametrize('cfg', ['d_occ3_tp', 'd_c2_tp_batch'])
def test_fall_back_inside_a_walk_whose_cell_then_gives_up(cfg):
    """-DEG_SEG_FAIL_EVERY=2 -DEG_TP_GIVEUP_EVERY=2 -DEG_TP_GIVEUP_AT=14 in one build."""
    name, env, ndraw, groups = CONFIGS[cfg]
    s = _solver(name, COMBINED, env, ndraw, groups)
    s.solve(raise_on_error=False)
    cnt = _check_forced(cfg, COMBINED, s, (cfg, 'combined'))
    print(cfg, 'combined: merged/fallback', cnt['walks'].sum(axis=0).tolist(), 'done/left', cnt['tp'].sum(axis=0).tolist(), 'in place', int(cnt['inplace'].sum()))
    assert cnt['walks'][:, 0].sum() > 0 and cnt['walks'][:, 1].sum() > 0
    _check_giveup_counts(cfg, 14, 2, s, cnt, (cfg, 'combined'))
    s.close()


def _oracle_draws(s, orc, P, draws, what):
    for d in draws:
        ref = orc.solve(P[d])
        sol = s.solution(d)
        assert (sol.status == 0) == (ref.rc == 0), (what, d)
        if ref.rc:
            assert sol.err.strip() == ref.err.strip(), (what, d)
        ok, rep = compare(sol, ref, rtol=0.0, th_tol=0.0)   # (of a draw that fails: the tables it got to)
        assert ok and (ref.rc != 0 or sol.nevals == ref.nevals), (what, d, rep)   # (evaluations of a failing draw: the default build's)


def test_forced_recoveries_in_the_600_draw_batch():
    """The 600 draws of test_throughput_envelope_path_in_a_batch_with_failing_draws (the throughput path is their default) on the
    combined build: status, failing cell, evaluations and the checksums of every cell of every draw are the default build's, and eight
    draws and every draw that fails are the oracle's.  (At this grid size none of the 600 fails, in either build and in the oracle's
    sample: the draws on which the reference algorithm breaks down are in the test below.)"""
    m, gen = workloads.c2(a0=0, ngridm=300, T=30)
    P = gen(600)
    res = {}
    for flags in ([], COMBINED):
        s = runtime.Solver(build.build_model(m, extra_flags=flags), m.descriptor(), ndraw=len(P), keep_history=True)
        s.set_params(P)
        s.solve(raise_on_error=False)
        res[bool(flags)] = _results(s)
        if flags:
            failing = [int(k) for k in np.nonzero(s.status()[0])[0]]
            walks, tp = s.walk_stats().sum(axis=0), s.tp_stats().sum(axis=0)
            print('600 draws, combined build: failing draws', failing, 'merged/fallback', walks.tolist(), 'done/left', tp.tolist())
            assert walks[0] > 0 and walks[1] > 0 and tp[0] > 0 and tp[1] > 0
            _oracle_draws(s, Oracle(m), P, failing[:5] + list(range(0, 600, 75)), 'combined build')
        s.close()
    _same(res[True], res[False], 'combined build')


FAILING = [67, 0, 1, 9, 2, 3, 771, 4]   # of workloads.c2(a0=0)'s first 1024 draws; the reference algorithm breaks down on 67, 9 and 771


@pytest.mark.parametrize('flags', [_seg(1), _giveup(13, 1), COMBINED], ids=['seg_fail_1', 'giveup_13_1', 'combined'])
def test_forced_recoveries_on_draws_that_fail(flags):
    """C2 at full size (the plugin of the small C2, so its checking builds) on the throughput path, eight draws of which three fail: status,
    error text and the tables up to the failing cell stay the oracle's, and the failing cell the default build's, when every cut walk is
    walked again, when every cell with a folded list gives up after its secondary walk, and in the combined build."""
    m, gen = workloads.c2(a0=0)
    P = np.ascontiguousarray(gen(1024)[FAILING])
    res = {}
    for fl in ([], flags):
        lib = build.build_model(m, extra_flags=fl)
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv('EGDST_ENV_TP', '1')
            s = runtime.Solver(lib, m.descriptor(), ndraw=len(P), keep_history=True)
        s.set_params(P)
        s.solve(raise_on_error=False)
        res[bool(fl)] = _results(s)
        if fl:
            assert [int(k) for k in np.nonzero(s.status()[0])[0]] == [0, 3, 6]
            walks, tp = s.walk_stats().sum(axis=0), s.tp_stats().sum(axis=0)
            print('full-size C2, 3 of 8 draws fail', flags, 'merged/fallback', walks.tolist(), 'done/left', tp.tolist())
            if flags != _giveup(13, 1):
                assert walks[1] > 0
            if flags != _seg(1):
                assert tp[1] > 0
            _oracle_draws(s, _full_c2_oracle(), P, range(len(P)), flags)
        s.close()
    _same(res[True], res[False], flags)


@functools.lru_cache(maxsize=None)
def _full_c2_oracle():
    import estimation_loop_case as lc
    return lc.OracleCache(workloads.c2(a0=0)[0])   # (a draw's solution is computed once for the three builds)


@pytest.mark.parametrize('env', [
    {'EGDST_TP_LKCAP': '40'},
    {'EGDST_TP_LKCAP': '40', 'EGDST_TP_BIGCAP': '52'},
    {'EGDST_TP_LKCAP': '40', 'EGDST_TP_BIG': '0'},
    {'EGDST_TP_LKCAP': '20', 'EGDST_TP_BIGCAP': '52'},
], ids=['second_tier', 'bigcap_52', 'leftover', 'both'])
def test_second_tier_cell_that_gives_up_before_it_starts_on_the_device(env):
    """-DEG_TP_TAIL_GIVEUP_EVERY=2 on the four environments of test_gpu_tp_tail.py::test_single_solve_roles_bit_exact: every other
    second-tier entry is done in place by the workgroup that holds it."""
    m = _model('retire8')
    with pytest.MonkeyPatch.context() as mp:
        for k, v in dict(env, EGDST_ENV_TP='1').items():
            mp.setenv(k, v)
        s = runtime.Solver(build.build_model(m, extra_flags=TAIL_GIVEUP), m.descriptor(), ndraw=1, keep_history=True)
    s.set_params(m.param_vector()[None])
    seen = []
    for k in range(2):
        s.solve(raise_on_error=False)
        ref = _oracle('retire8')
        ok, rep = compare(s.solution(0), ref, rtol=0.0, th_tol=0.0)
        assert ok and s.solution(0).nevals == ref.nevals and ref.rc == 0, rep
        cnt = _counts(s)
        done, left = (int(x) for x in cnt['tp'][0])
        assert done + left == _cells(s) and cnt['rest'].sum() + cnt['inplace'].sum() == left
        # per launch the entries 0, 2, 4, ... of the second list give up
        assert cnt['inplace'].sum() == ((cnt['big'] + 1) // 2).sum()
        seen.append((done, left, int(cnt['inplace'].sum()), int(cnt['rest'].sum()), int(cnt['big'].sum())))
    print(env, 'done/left/in place/listed/second tier', seen[0])
    assert seen[0] == seen[1]
    if env == {'EGDST_TP_LKCAP': '40'} or env.get('EGDST_TP_LKCAP') == '20':
        assert seen[0][2] > 0 and seen[0][4] > 0
    else:
        assert seen[0][2] == 0 and seen[0][4] == 0   # no second tier, or its list is empty
    s.close()
