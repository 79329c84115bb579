"""The device against the recorded outputs of the reference's own programs (tests/golden/ref_*.npz), with no oracle in
between and no tolerance: solve, simulate and the accessor through the C ABI for the twelve example models and C5 at
T=20, ngridm=500; the first 256 C2 draws of the bench as one batch (same failing draws, same cells, same messages, the
solved draws by checksum); C1-C4 at full size by per-cell checksums, in the default build and in the batch build variants.
Reads tests/golden/ only."""
import os
import sys

import numpy as np
import pytest

from egdst_amd import build, runtime, workloads

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import make_golden_ref as G  # noqa: E402
from make_golden_big import BIG  # noqa: E402
from test_reference_fixtures import NFAIL, check_tables, model_with, same, same_text  # noqa: E402


def solver(m, P, flags=None):
    lib = build.build_model(m, extra_flags=flags) if flags else build.build_model(m)
    P = np.atleast_2d(np.asarray(P, dtype=np.float64))
    s = runtime.Solver(lib, m.descriptor(), ndraw=len(P), keep_history=True)
    s.set_params(P)
    s.solve(raise_on_error=False)
    return s


@pytest.mark.parametrize('name', sorted(G.MODELS))
def test_device_equals_the_recorded_reference(name):
    g = G.load('ref_%s.npz' % name)
    m = model_with(g, name)
    s = solver(m, g['params'])
    sol = s.solution(0)
    assert sol.status == 0, (sol.status, sol.err)
    check_tables(sol, g, name)
    for rt in (0, 1):
        assert same(s.simulate(g['init'], g['randstream'], rndtype=rt), g['sims%d' % rt]), '%s: panel, rndtype=%d' % (name, rt)
    for k in range(int(g['ncall'])):
        sw, args = int(g['call%d_sw' % k]), g['call%d_args' % k]
        assert same(s.call(sw, args), g['call%d_res' % k]), '%s: accessor case %d (switch %d)' % (name, k, sw)
    s.close()


@pytest.mark.parametrize('key', sorted(G.DRAW_SETS))
def test_device_fails_on_the_draws_the_reference_fails_on(key):
    g = G.load('ref_C2_draws.npz')
    m, gen = workloads.c2(a0=G.DRAW_SETS[key])
    P = gen(4096)[:G.NDRAWS]
    assert same(P, g[key + '_params'])
    failed = g[key + '_failed']
    assert int(failed.sum()) == NFAIL[key]
    s = solver(m, P)
    st = s.status()[0]
    assert same(st != 0, failed), (np.nonzero(st != 0)[0].tolist(), np.nonzero(failed)[0].tolist())
    for i in range(G.NDRAWS):
        what = 'C2 %s draw %d' % (key, i)
        ln, th = s.dims(i)
        if failed[i]:
            text = s.lib.lib.egdst_strerror(int(st[i])).decode()
            assert same_text(str(g[key + '_err'][i]), text), (what, text)
            assert G.fail_cell(ln, False) == tuple(g[key + '_cell'][i]), what
        assert same(ln, g[key + '_len'][i]) and same(th, g[key + '_thlen'][i]), what
        if not failed[i]:
            assert G.draw_checksum(s.checksums(i)) == g[key + '_checksum'][i], what
    s.close()


VARIANTS = [(n, None) for n in G.BIG_REF] + [('C2', workloads.BATCH_BUILD_FLAGS['C2']), ('C4', workloads.BATCH_BUILD_FLAGS['C4'])]


@pytest.mark.parametrize('name,flags', VARIANTS, ids=['%s-%s' % (n, 'batch' if f else 'default') for n, f in VARIANTS])
def test_device_equals_the_reference_checksums_at_full_size(name, flags):
    g = G.load('ref_big_%s.npz' % name)
    m, par = BIG[name][0]()
    s = solver(m, m.param_vector() if par is None else par, flags)
    assert s.status()[0][0] == 0
    ln, th = s.dims(0)
    assert same(ln, g['len']) and same(th, g['thlen'])
    bad = np.argwhere(s.checksums(0) != g['sums'])
    assert len(bad) == 0, ('cells (it, ist, column) whose checksum differs', bad[:8].tolist(), len(bad))
    s.close()
