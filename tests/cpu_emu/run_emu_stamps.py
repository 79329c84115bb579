"""Harness build, no sanitizer: a clock-stamp build (-DEGDST_STAMPS=wg: one stamp per completed cell, the cheapest set to emulate)
of retirement2 at T=8, ngridm=60 against the plain harness build of the same model: the same bits in every cell, stamps in the
slots of the set and in no other, and an empty guard record.  The harness clock counts its own reads, so a stamp that was taken
is a positive number.  Nothing is preloaded."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'cpu_emu'))
import build_emu  # noqa: E402
from egdst_amd import examples, runtime  # noqa: E402
from estimation_emu import write_modelspec  # noqa: E402

SET = 'wg'


def solve(model, flags):
    os.environ['EMU_EXTRA_FLAGS'] = flags
    lib = runtime.ModelLibrary(build_emu.build(write_modelspec(model), False, 1, False, 1))
    s = runtime.Solver(lib, model.descriptor(), ndraw=1, keep_history=True)
    s.set_params(model.param_vector())
    rc = s.solve(raise_on_error=False)
    return s, rc


if __name__ == '__main__':
    m = examples.retirement2(T=8, ngridm=60)
    bad = []
    plain, rc0 = solve(m, '')
    stamped, rc1 = solve(m, '-DEGDST_STAMPS=' + SET)
    if rc0 or rc1:
        bad.append('solve rc %d / %d' % (rc0, rc1))
    if not np.array_equal(plain.checksums(0), stamped.checksums(0)):
        bad.append('the stamp build computes other bits')
    if plain.solution(0).nevals != stamped.solution(0).nevals:
        bad.append('the stamp build counts other evaluations')
    if stamped.debug(0).any():
        bad.append('guard record %s' % stamped.debug(0).tolist())
    st = stamped.stamps(0)
    mine = {k: v for k, v in st.items() if k.startswith(SET + '.')}
    if not mine or not all(v > 0 for v in mine.values()):
        bad.append('slots of the set without a stamp: %s' % [k for k, v in mine.items() if v == 0])
    if any(v for k, v in st.items() if k not in mine):
        bad.append('stamps outside the set: %s' % [k for k, v in st.items() if v and k not in mine])
    try:
        plain.stamps(0)
        bad.append('the plain build hands out stamps')
    except runtime.EgdstRuntimeError:
        pass
    print('stamps', mine, 'walks segmented/fallback', stamped.walk_stats()[0].tolist())
    print('stamp build problems: %d %s' % (len(bad), bad[:3]))
