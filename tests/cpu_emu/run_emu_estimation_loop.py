"""Harness build, no sanitizer: the estimation loop's solve -- one handle without history, egdst_set_params_dev /
egdst_solve_async / egdst_objective_dev chunk after chunk, the first chunk once more in reversed order at the end -- with the
objective and the two live periods of every chunk held to the oracle on bits (tests/estimation_loop_case.py).  Argument: the
case (CASES).  Nothing is preloaded."""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, os.path.join(ROOT, 'tests', 'cpu_emu'))
import numpy as np
import build_emu
from egdst_amd import examples, runtime, workloads
import estimation_loop_case as lc
from estimation_emu import write_modelspec


def perturbed(m, n, seed=21):
    p0 = m.param_vector()
    return p0[None] * (1 + 0.15 * np.random.default_rng(seed).uniform(-1, 1, (n, len(p0))))


def _c2():
    m, gen = workloads.c2(a0=0, ngridm=60, T=12, ny=5)
    return m, gen(12), 3


def _retirement8():
    m = examples.retirement8(T=5, ngridm=10)
    return m, perturbed(m, 8), 2


def _c4():
    m, gen = workloads.c4(ngridm=40, T=6, ny=3)
    return m, gen(8), 2


def _c4_short():
    """A solved table of a single-choice model has ngridm + 1 rows whatever the draw (the reference's adraw fills the grid),
    so on _c4 no table ever shrinks.  With a negative interest rate and a negative income the first period's table has two
    rows: the draws at index 1 of the first chunk and index 3 of the second, so that a slot goes from 41 rows to 2 within a
    solve (period 2 to period 0) and from one chunk to the next.  (With k_env1's loop that zeroes the rows past the new end
    switched off, this is the case that fails.)"""
    m, P, nchunks = _c4()
    P[1] = [-0.5, -1.0, 0.75]
    P[7] = [-0.5, -1.0, 0.0]
    return m, P, nchunks


# (model, draws, chunks of CHUNK); no draw fails in the oracle
CASES = {'c2': _c2, 'retirement8': _retirement8, 'c4': _c4, 'c4_short': _c4_short}
CHUNK = 4


def run_loop(lib, m, chunks):
    """the loop on one handle; the harness has no device: its "device" buffers are host arrays"""
    s = runtime.Solver(lib, m.descriptor(), ndraw=CHUNK, keep_history=False)
    res = []
    for P in chunks:
        obj = np.full((CHUNK, 2), np.nan)
        s.set_params_dev(P.ctypes.data)
        s.solve_async()
        s.objective_dev(obj.ctypes.data)
        res.append({'P': P, 'obj': obj, 'tabs': {it: lc.read_live_period_host(s, it) for it in (0, 1)}})
    s.sync(raise_on_error=False)
    st, wh = s.status()
    kept = runtime.Solver(lib, m.descriptor(), ndraw=CHUNK, keep_history=True)
    kept.set_params(chunks[-1])
    kept.solve(raise_on_error=False)
    last = {'status': st, 'where': wh, 'evals': s.evals()[1], 'where_kept': kept.status()[1],
            'strerror': lambda code: lib.lib.egdst_strerror(code).decode()}
    return res, last


if __name__ == '__main__':
    m, P, nchunks = CASES[sys.argv[1]]()
    lib = runtime.ModelLibrary(build_emu.build(write_modelspec(m), False, 1, False, 1))
    chunks = lc.chunks_then_first_reversed(P, CHUNK, nchunks)
    res, last = run_loop(lib, m, chunks)
    bad = lc.check(lc.OracleCache(m), res, [0] * len(chunks), last)
    shrunk = sum(int((res[-1]['tabs'][it]['len'] < res[-2]['tabs'][it]['len']).sum()) for it in (0, 1))
    print('estimation loop %s: %d chunks of %d draws, %d tables shorter in the last chunk than in the one before'
          % (sys.argv[1], len(chunks), CHUNK, shrunk))
    print('estimation loop problems: %d %s' % (len(bad), bad[:4]))
