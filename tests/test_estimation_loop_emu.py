"""The estimation loop's solve on the CPU harness (tests/cpu_emu), without a GPU: a handle without history, parameters by
egdst_set_params_dev, egdst_solve_async and egdst_objective_dev chunk after chunk, and after every chunk the objective and the
two live periods read where the handle keeps them (Solver.device_tables) -- lengths, rows and the zeros past a table's end --
equal to the oracle's on bits.  The harness library is loaded into python with no sanitizer (this file preloads nothing); the
GPU test with the same checker is tests/test_gpu_estimation_loop.py."""
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, 'cpu_emu')


@pytest.mark.parametrize('case', ['c2', 'retirement8', 'c4', 'c4_short'])
def test_loop_on_the_harness_against_the_oracle(case):
    """c2(a0=0, ngridm=60, T=12, ny=5) with gen(12) (two choices: k_envelope), retirement8(T=5, ngridm=10) with 8 perturbed
    draws (eight states), c4(ngridm=40, T=6, ny=3) with gen(8) (one choice: k_env1), in chunks of 4 and the first chunk once
    more in reversed order: no draw fails in the oracle, every draw of every chunk is compared, and the reversed chunk leaves
    tables shorter than the chunk before it did (or the zeros past the end would be checked on nothing).  Every solved table
    of c4 has ngridm + 1 rows, so c4_short replaces two of its draws by ones whose first period has two rows."""
    env = dict(os.environ, EMU_SANITIZE='0', EMU_EXTRA_FLAGS='')
    r = subprocess.run([sys.executable, os.path.join(EMU, 'run_emu_estimation_loop.py'), case], env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert 'estimation loop problems: 0 ' in r.stdout, r.stdout + r.stderr[-2000:]
    found = re.search(r'(\d+) tables shorter in the last chunk', r.stdout)
    assert found and (int(found.group(1)) > 0 or case == 'c4'), r.stdout
