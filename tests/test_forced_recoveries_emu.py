"""The envelope step's rare recoveries in the CPU harness build, forced by the compile-time switches of the device code's checking
builds (egdst_kernels.hip) and held to the oracle bit for bit:
  -DEG_SEG_FAIL_EVERY=n                             the check of a cut walk's predictions fails: wave 0 walks the stream again;
  -DEG_TP_GIVEUP_EVERY=n -DEG_TP_GIVEUP_AT=13|14    a cell of the throughput path gives up after its stage-0 / stage-1 walk;
with -DENV_SEG_MINPTS=8, so that the small examples cut walks at four-lane waves and 16-thread workgroups.  No sanitizer here.
The first line of defence, on any machine; tests/test_gpu_forced_recoveries.py checks the device compilation."""
import functools
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
R8 = ('retirement8', 'T=5, ngridm=30, ny=3')         # eight states, two choices: 4 periods x 8 cells on the throughput path
OCC3 = ('occ3', 'T=6, ngridm=30, ngridmax=300, nthrhmax=100')   # one state, three choices (a cut walk needs 8 thresholds per segment)
RET2 = ('retirement2', 'T=20, ngridm=100, nthrhmax=100')        # one state, two choices, one cell whose list folds
BASE = {'EMU_SANITIZE': '0', 'EMU_WAVE': '4', 'EMU_ENV_BS': '16'}
MINPTS = '-DENV_SEG_MINPTS=8'
ENVS = {
    'k_envelope_lds': {'EGDST_ENV_TP': '0'},                         # run_walk<1>
    'k_envelope_global': {'EGDST_ENV_TP': '0', 'EGDST_LCAP': '64'},   # run_walk<0>: no stream fits the LDS
    'throughput': {'EGDST_ENV_TP': '1'},                              # run_walk<2>, the stream classified again
    'second_tier': {'EGDST_ENV_TP': '1', 'EGDST_TP_LKCAP': '40'},     # ... inside k_tp_tail
}


@functools.lru_cache(maxsize=None)
def _run(args, env_name, flags='', script='run_emu.py'):
    e = dict(os.environ, **BASE, **ENVS[env_name], EMU_EXTRA_FLAGS=(MINPTS + ' ' + flags).strip())
    r = subprocess.run([sys.executable, os.path.join(HERE, 'cpu_emu', script)] + list(args), env=e, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'ok=True' in r.stdout and 'max_rel=0.00e+00' in r.stdout, r.stdout + r.stderr[-2000:]
    return r.stdout


def _counts(out):
    """(merged, fallback), (done, left) from run_emu.py's line"""
    walks = eval(out.split('walks segmented/fallback')[1].split('tp done/left')[0].strip())
    tp = eval(out.split('tp done/left')[1].strip())
    return tuple(walks), tuple(tp)


@pytest.mark.parametrize('n', [1, 2])
@pytest.mark.parametrize('env', sorted(ENVS))
@pytest.mark.parametrize('args', [R8, OCC3], ids=['retirement8', 'occ3'])
def test_failed_predictions_are_walked_again(args, env, n):
    (m0, f0), tp0 = _counts(_run(args, env))
    assert m0 + f0 > 0, 'the shape cuts no walk in this configuration'
    (m, f), tp = _counts(_run(args, env, '-DEG_SEG_FAIL_EVERY=%d' % n))
    assert m + f == m0 + f0 and tp == tp0, ((m, f), (m0, f0), tp, tp0)   # the same cuts are planned; falling back gives no cell up
    if n == 1:
        assert m == 0 and f > 0
    else:
        assert m > 0 and f > 0


def _tail(out):
    """(done, left, in place) of the first and of the second solve, entries of the two lists, from run_emu_tp_tail.py"""
    first = eval(out.split('tp done/left/in place')[1].split('second solve')[0].strip())
    again = eval(out.split('second solve')[1].split('listed per period')[0].strip())
    rest = eval(out.split('left over')[1].split('second tier')[0].strip())
    big = eval(out.split('second tier')[1].strip())
    return tuple(first), tuple(again), sum(rest), sum(big)


GIVEUPS = [(R8, 'throughput', 14, 1), (R8, 'throughput', 14, 2), (R8, 'second_tier', 14, 1), (R8, 'second_tier', 14, 2),
           (OCC3, 'throughput', 14, 1), (OCC3, 'throughput', 14, 2),
           # site 13 needs a cell with a folded list, whose secondary envelope is the stage-0 walk: of the examples small enough for the
           # harness this one has one such cell (n = 2 would pass it by: the GPU file runs both on shapes with hundreds of them)
           (RET2, 'throughput', 13, 1)]


@pytest.mark.parametrize('args,env,at,n', GIVEUPS, ids=['%s-%s-%d-%d' % (g[0][0], g[1], g[2], g[3]) for g in GIVEUPS])
def test_cells_that_give_up_after_their_walk_are_redone(args, env, at, n):
    (done0, left0, inplace0), _, _, big0 = _tail(_run(args, env, script='run_emu_tp_tail.py'))
    assert inplace0 == 0 and done0 > 0 and (big0 > 0) == (env == 'second_tier')
    first, again, rest, big = _tail(_run(args, env, '-DEG_TP_GIVEUP_EVERY=%d -DEG_TP_GIVEUP_AT=%d' % (n, at), 'run_emu_tp_tail.py'))
    done, left, inplace = first
    assert again == first                                    # a second solve on the handle counts the same
    assert done + left == done0 + left0 and rest + inplace == left, (first, rest, big)
    if at == 13:
        assert left > left0 and done > 0                     # the cells with a folded list, and only they
    elif n == 1:
        assert done == 0
    else:
        assert done > 0 and left > 0
    if env == 'second_tier':
        assert inplace > 0                                   # done by the workgroup that holds the cell
    else:
        assert inplace == 0


@pytest.mark.parametrize('env', ['throughput', 'second_tier'])
def test_fall_back_inside_a_walk_whose_cell_then_gives_up(env):
    out = _run(R8, env, '-DEG_SEG_FAIL_EVERY=2 -DEG_TP_GIVEUP_EVERY=2 -DEG_TP_GIVEUP_AT=14')
    (m, f), (done, left) = _counts(out)
    assert m > 0 and f > 0 and done > 0 and left > 0, out
