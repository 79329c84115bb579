"""blk_sort_lds (egdst_kernels.hip): a stream with a list out of comp1 order goes through the bitonic network whenever its padded
size fits the LDS, however many threads saw a pair out of order; the quadratic counting ranks are for streams whose padded size
does not fit.  Until now the number of threads that saw such a pair was read as 0 / 1 / 2, so a stream with two or more pairs out
of order (seen by different threads) took the counting ranks although the network fitted: the primaries of the slowest leftover
cells of the C2 batch (profiles/r05_census_*: draws 3136, 3577, 1878 and 959 of the 4096).  Both paths sort by pt_before, a strict
total order, so nothing may change a bit: single solves of those draws against the oracle at the handle's own LDS capacity and at
one that fits every padded stream, with the sort counters saying which way the sorts went (egdst_get_sort_stats); and one solve
with the capacity just below a padded size, which keeps the counting ranks in use."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from egdst_amd import build, runtime, workloads  # noqa: E402
from oracle_harness import Oracle  # noqa: E402
from parity import compare  # noqa: E402

pytestmark = pytest.mark.gpu
DRAWS = [3136, 3577, 1878, 959]


@pytest.fixture(scope='module')
def case():
    m = workloads.c2(a0=-5.0)[0]
    P = workloads.c2(a0=0)[1](4096)
    return m, P, Oracle(m), {}


def _reference(case, d):
    m, P, orc, cache = case
    if d not in cache:   # (one oracle solve per draw, shared by the tests)
        cache[d] = orc.solve(P[d])
    return cache[d]


def _solve(case, d, monkeypatch, env=None):
    m, P = case[:2]
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    s = runtime.Solver(build.build_model(m), m.descriptor(), ndraw=1, keep_history=True)
    for k in (env or {}):
        monkeypatch.delenv(k)   # (switches are read when the handle is created)
    s.set_params(P[d][None])
    s.solve(raise_on_error=False)
    return s


def _check(s, ref, what):
    sol = s.solution(0)
    st, where = s.status()
    assert (sol.status == 0) == (ref.rc == 0), what
    if ref.rc:
        assert sol.err.strip() == ref.err.strip(), what
    else:
        assert int(st[0]) == 0 and not np.any(where[0]), (what, st, where)
        assert sol.nevals == ref.nevals, what
    ok, rep = compare(sol, ref, rtol=0.0, th_tol=0.0)   # every table written, thresholds included
    assert ok, (what, rep)


CAPS = {'default': {}, 'lcap_4096': {'EGDST_LCAP': '4096'}}


@pytest.fixture(scope='module')
def sorts(case):
    """the four draws solved once per LDS capacity and held to the oracle: their sort counters (in order, network, counted, several
    pairs out of order).  The handle's own capacity is 3064 points (1.5 x 2 x 1000 + 64): a stream of 2049 to 3064 points pads to
    4096 and does not fit; with 4096 points of LDS every LDS-resident stream's padded size fits."""
    mp, out = pytest.MonkeyPatch(), {}
    for cap, env in CAPS.items():
        for d in DRAWS:
            s = _solve(case, d, mp, env)
            _check(s, _reference(case, d), (cap, d))
            out[cap, d] = [int(x) for x in s.sort_stats()[0]]
            s.close()
    mp.undo()
    return out


@pytest.mark.parametrize('d', DRAWS)
def test_where_the_padded_stream_fits_nothing_is_counted(sorts, d):
    for cap in CAPS:
        print('draw', d, cap, 'LDS sorts (in order, network, counted, with two or more pairs out of order):', sorts[cap, d])
    inorder, network, counted, several = sorts['lcap_4096', d]
    assert counted == 0 and network >= 1 and inorder >= 1 and several <= network
    # the handle's own capacity: the network for every stream out of order that pads to at most 2048 points (streams of more than
    # 3064 points sort in global memory there and are not counted here)
    inorder0, network0, counted0, several0 = sorts['default', d]
    assert network0 >= 1 and network0 + counted0 <= network and several0 <= several


def test_these_draws_have_streams_with_two_or_more_pairs_out_of_order(sorts):
    """what the order check used to misread as "no room for the network": without such a stream the tests above could not fail"""
    assert sum(v[3] for (cap, d), v in sorts.items() if cap == 'lcap_4096') >= 1, sorts


def test_counting_ranks_below_the_padded_size_stay_exact(case, monkeypatch):
    """LDS capacity just below the padded size of the draw's longer streams (2047 < 2048): a stream out of order with more than 1024
    points is counted, a shorter one still takes the network."""
    d = DRAWS[0]
    s = _solve(case, d, monkeypatch, {'EGDST_LCAP': '2047'})
    inorder, network, counted, several = (int(x) for x in s.sort_stats()[0])
    print('draw', d, 'capacity 2047, LDS sorts: in order', inorder, 'network', network, 'counted', counted, 'with two or more pairs out of order', several)
    _check(s, _reference(case, d), (d, 'lcap 2047'))
    s.close()
    assert counted >= 1
