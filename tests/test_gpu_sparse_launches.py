"""The list-driven launches of a period (k_fixup, k_tp_big, k_envelope pass 3) take their entries by ticket and are sized to
their group, and group 0 runs on the handle's own stream (egdst_host.inc: enqueue_solve, eg_sparse_grid; egdst_kernels.hip:
eg_take_ticket): none of that may change a bit of a result.  Full-size C2 at a0 = -5, 512 draws on the batch build -- the
shape of tests/test_regeneration_reuse.py, which regenerates guess streams and leaves cells to pass 3 -- solved with one group
and compared with other groupings, with the build whose sparse launches are two workgroups wide, and with a second solve."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from egdst_amd import workloads  # noqa: E402

NDRAW = 512
# the checking build (__graft_entry__.build() compiles it): every list-driven launch at most two workgroups wide, so that the
# ticket loop of a workgroup turns many times per launch
CAPPED = ['-DEG_SPARSE_GRID_MAX=2']
BUILD_VARIANTS = [(lambda: workloads.c2()[0], workloads.BATCH_BUILD_FLAGS['C2'] + CAPPED)]


def _results(s):
    """what must not depend on the schedule: status, evaluations, credited evaluations, the checksums of every draw, regenerations"""
    return (s.status()[0].copy(), s.evals()[1].copy(), s.evals_credited().copy(),
            np.stack([s.checksums(d) for d in range(s.ndraw)]), s.regenerations().copy())


def _solver(flags, groups):
    from egdst_amd import build, runtime
    m, gen = workloads.c2(a0=-5.0)
    s = runtime.Solver(build.build_model(m, extra_flags=flags), m.descriptor(), ndraw=NDRAW, keep_history=True)
    s.set_groups(groups)
    s.set_adaptive(False)  # (the schedule under test is the one set here, also for a second solve)
    s.set_params(gen(NDRAW))
    return s


def _same(a, b):
    for name, x, y in zip(('status', 'evaluations', 'credited evaluations', 'checksums', 'regenerations'), a, b):
        assert np.array_equal(x, y), name


@pytest.fixture(scope='module')
def one_group():
    """the plain batch build with one group: the reference of every test here, computed once"""
    s = _solver(workloads.BATCH_BUILD_FLAGS['C2'], 1)
    s.solve(raise_on_error=False)
    ref = _results(s)
    tp = s.tp_stats()
    nt = s.desc['T'] - s.desc['t0'] + 1
    s.close()
    # a run that exercised nothing fails: streams were regenerated (k_fixup's list), cells were left to pass 3 (its list, which
    # k_tp_big appends to), and on average a period's k_fixup list is longer than the two workgroups of the capped build
    assert ref[4].sum() > 0 and tp[:, 1].sum() > 0, (ref[4].sum(), tp.sum(axis=0))
    assert ref[4].sum() > 2 * nt, (ref[4].sum(), nt)
    for r in ref:
        r.setflags(write=False)
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize('groups', [2, 3, 4])
def test_groups_on_the_handles_stream_and_beside_it_equal_one_group(one_group, groups):
    s = _solver(workloads.BATCH_BUILD_FLAGS['C2'], groups)
    assert s.schedule()[0] == groups
    s.solve(raise_on_error=False)
    got = _results(s)
    s.close()
    _same(got, one_group)


@pytest.mark.gpu
@pytest.mark.parametrize('groups', [1, 3])
def test_two_workgroups_per_sparse_launch_equal_the_plain_build(one_group, groups):
    s = _solver(workloads.BATCH_BUILD_FLAGS['C2'] + CAPPED, groups)
    s.solve(raise_on_error=False)
    got = _results(s)
    s.close()
    _same(got, one_group)


@pytest.mark.gpu
def test_second_solve_on_one_handle_equals_the_first(one_group):
    """the tickets are cleared with the lists' counters once per solve: a second solve that found them spent would do no entry"""
    s = _solver(workloads.BATCH_BUILD_FLAGS['C2'], 3)
    s.solve(raise_on_error=False)
    first = _results(s)
    s.solve(raise_on_error=False)
    second = _results(s)
    s.close()
    _same(first, one_group)
    _same(second, first)


_HISTORY_CHILD = r'''
import sys
sys.path.insert(0, sys.argv[1])
from egdst_amd import build, runtime, workloads
out = []
for a0 in (-5.0, 0.0):
    m, gen = workloads.c2(a0=a0)
    s = runtime.Solver(build.build_model(m, extra_flags=workloads.BATCH_BUILD_FLAGS['C2']), m.descriptor(), ndraw=1024, keep_history=False)
    s.set_params(gen(1024))
    g0 = s.schedule()[0]
    s.solve(raise_on_error=False)
    g1, share = s.schedule()[0], s.regenerations().sum() / (1024.0 * 2 * 59)
    s.solve(raise_on_error=False)
    out.append((a0, g0, g1, s.schedule()[0], float(share)))
    s.close()
print('RESULT', out)
'''


@pytest.mark.gpu
def test_group_count_follows_the_regenerated_share_on_four_queues():
    """With 4 hardware queues (read when the runtime starts: a child process) a 1024-draw C2 handle starts with 4 groups; the batch with
    a0 = -5 regenerates more than 0.5 % of its guess streams and goes on with 3 (queues - 1), the one with a0 = 0 stays at 4."""
    import subprocess
    env = dict(os.environ, GPU_MAX_HW_QUEUES='4')
    env.pop('EGDST_GROUPS', None)
    env.pop('EGDST_ADAPTIVE', None)
    r = subprocess.run([sys.executable, '-c', _HISTORY_CHILD, os.path.dirname(HERE)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = eval([ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')][0][7:])
    print(res)
    (_, a_create, a_first, a_second, a_share), (_, b_create, b_first, b_second, b_share) = res
    assert a_share >= 0.005 > b_share, res
    assert (a_create, a_first, a_second) == (4, 3, 3), res
    assert (b_create, b_first, b_second) == (4, 4, 4), res
