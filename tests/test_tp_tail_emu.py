"""The tail launch of a period's envelope step (k_tp_tail: the cells the throughput path left over and the second tier of its
stage 1 behind one ticket) in the CPU harness build: the issue's three budgets, a budget pair that fills both lists of one
launch, and second-tier cells that give up and are done in place by the workgroup that holds them.  No sanitizer here
(tests/test_sanitizer.py runs the issue's shapes under one); bit-exact against the oracle."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ARGS = ['retirement8', 'T=5, ngridm=30, ny=3']
BASE = {'EMU_SANITIZE': '0', 'EGDST_ENV_TP': '1', 'EMU_WAVE': '4', 'EMU_ENV_BS': '16'}


def _run(script, env):
    e = dict(os.environ, **BASE, **env)
    r = subprocess.run([sys.executable, os.path.join(HERE, 'cpu_emu', script)] + ARGS, env=e, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'ok=True' in r.stdout and 'max_rel=0.00e+00' in r.stdout, r.stdout + r.stderr[-2000:]
    return r.stdout


@pytest.mark.parametrize('env', [
    {'EGDST_TP_LKCAP': '40'},                             # everything goes to the second tier
    {'EGDST_TP_LKCAP': '40', 'EGDST_TP_BIGCAP': '52'},    # second tier on, its list empty: this model's lists hold <= 40 or 53..60 points
    {'EGDST_TP_LKCAP': '40', 'EGDST_TP_BIG': '0'},        # leftover cells only
], ids=['second_tier', 'bigcap_52', 'leftover'])
def test_tail_launch_roles_bit_exact(env):
    out = _run('run_emu.py', env)
    done, left = eval(out.split('tp done/left')[1].strip())
    assert done + left > 0 and (done > 0 or env.get('EGDST_TP_BIG') == '0'), out
    if env.get('EGDST_TP_BIG') == '0' or env.get('EGDST_TP_BIGCAP'):
        assert left > 0, out
    if env.get('EGDST_TP_BIG') != '0':
        assert done > 0, out   # (the regular launch's with bigcap_52, the second tier's as well without it)


def _counts(out):
    """(done, left, in place), the same of the second solve, and the two lists' entries per period, from run_emu_tp_tail.py"""
    first = eval(out.split('tp done/left/in place')[1].split('second solve')[0].strip())
    again = eval(out.split('second solve')[1].split('listed per period')[0].strip())
    rest = eval(out.split('left over')[1].split('second tier')[0].strip())
    big = eval(out.split('second tier')[1].strip())
    return first, again, rest, big


def test_second_tier_cell_that_gives_up_is_done_in_place():
    """-DEG_TP_TAIL_GIVEUP_EVERY=2: every other second-tier entry gives up before it touches anything (none of the small examples
    has a second-tier cell that gives up by itself: with the 40-point budget all 32 are completed).  The workgroup that holds
    such a cell runs the envelope code on it there and then; it is counted as left over, as a listed cell was, and in the
    in-place counter.  A second solve on the same handle counts the same: tickets and counters are cleared once per solve."""
    (done0, left0, inplace0), _, _, _ = _counts(_run('run_emu_tp_tail.py', {'EGDST_TP_LKCAP': '40'}))
    assert inplace0 == 0 and done0 > 0
    first, again, _, _ = _counts(_run('run_emu_tp_tail.py', {'EGDST_TP_LKCAP': '40', 'EMU_EXTRA_FLAGS': '-DEG_TP_TAIL_GIVEUP_EVERY=2'}))
    done, left, inplace = first
    assert inplace > 0 and left == left0 + inplace and done == done0 - inplace, first
    assert again == first


BOTH = {'EGDST_TP_LKCAP': '20', 'EGDST_TP_BIGCAP': '52'}   # lists of up to 40 points are the second tier's, those of 53..60 are left over


def test_both_lists_filled_in_one_launch():
    """Four launches whose ticket range runs over four leftover cells and then four second-tier cells."""
    first, again, rest, big = _counts(_run('run_emu_tp_tail.py', BOTH))
    assert any(r > 0 and b > 0 for r, b in zip(rest, big)), (rest, big)
    done, left, inplace = first
    assert left == sum(rest) and inplace == 0 and done >= sum(big) > 0, (first, rest, big)
    assert again == first


def test_give_up_in_a_launch_with_both_lists():
    """the same launches with every other second-tier entry giving up: its index in the second list is the ticket less the
    leftover cells"""
    plain, _, rest, big = _counts(_run('run_emu_tp_tail.py', BOTH))
    first, again, rest2, big2 = _counts(_run('run_emu_tp_tail.py', dict(BOTH, EMU_EXTRA_FLAGS='-DEG_TP_TAIL_GIVEUP_EVERY=2')))
    assert (rest2, big2) == (rest, big)   # nothing is appended to either list
    assert first[2] == sum((b + 1) // 2 for b in big) > 0 and first[1] == plain[1] + first[2] and first[0] == plain[0] - first[2]
    assert again == first
