"""The recorded outputs of the reference's own programs (tests/golden/ref_*.npz, written by tests/golden/make_golden_ref.py).

Always on, no reference needed: both builds of the CPU oracle -- the platform libm and include/egdst_math.h, which the GPU
runs too -- reproduce the recorded tables, panels, accessor results and failing draws EXACTLY.
Live only (reference sources present): regenerating a fixture gives the committed arrays, so a stale fixture cannot hide
behind the skip of tests/test_reference_parity.py.  The device is held to the same files by tests/test_gpu_reference.py.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import make_golden_ref as G  # noqa: E402
from make_golden_big import BIG, cell_sums  # noqa: E402
from oracle_harness import Oracle  # noqa: E402
import ref_harness  # noqa: E402

# the one message of the reference that has more than one line; the oracle and the device keep its first line
LONG_MESSAGE = 'Error:\nAll of the choices lead to -inf value functions for all values of money-at-hand!'
NFAIL = {'a0m5': 24, 'a0_0': 6}      # of the first 256 draws, in the reference


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f' and b.dtype.kind == 'f')


def same_text(recorded, ours):
    """The whole text, for every message but LONG_MESSAGE, of which the first line is kept on our side."""
    if recorded.startswith(LONG_MESSAGE + '\n'):
        return ours == LONG_MESSAGE
    return ours == recorded


def check_tables(sol, g, what):
    """sol: len, thlen, M, C, V, D, TH in the shared table layout, against a ref_<model>.npz."""
    assert same(sol.len, g['len']), (what, np.argwhere(sol.len != g['len'])[:5])
    assert same(sol.thlen, g['thlen']), (what, np.argwhere(sol.thlen != g['thlen'])[:5])
    nt, nst = g['len'].shape
    r = t = 0
    for it in range(nt):
        for ist in range(nst):
            n, k = int(g['len'][it, ist]), int(g['thlen'][it, ist])
            m, c, v = sol.M[it, ist, :n], sol.C[it, ist, :n], sol.V[it, ist, :n]
            assert same(np.stack([m, c, m - c, v], axis=1), g['mcav'][r:r + n]), '%s: [M C A V] of it=%d ist=%d' % (what, it, ist)
            assert same(np.stack([sol.D[it, ist, :k], sol.TH[it, ist, :k]], axis=1), g['dth'][t:t + k]), '%s: [D TH] of it=%d ist=%d' % (what, it, ist)
            r, t = r + n, t + k
    assert r == len(g['mcav']) and t == len(g['dth'])


def model_with(g, name):
    m = G.MODELS[name]()
    d = m.descriptor()
    for k in ('t0', 'T', 'ngridm', 'ngridmax', 'nthrhmax', 'ny', 'mmax', 'a0'):
        assert d[k] == g[k], (name, k)
    assert same(m.param_vector(), g['params'])
    return m


@pytest.mark.parametrize('native', [True, False], ids=['glibc', 'portable'])
@pytest.mark.parametrize('name', sorted(G.MODELS))
def test_oracle_equals_the_recorded_reference(name, native):
    g = G.load('ref_%s.npz' % name)
    m = model_with(g, name)
    O = Oracle(m, native_math=native)
    sol = O.solve(dbgout=True)
    assert sol.rc == 0, sol.err
    check_tables(sol, g, name)
    assert sol.dbgn == int(g['dbgn']) and same(np.asarray(sol.dbgout)[:sol.dbgn], g['dbgout'])
    assert same(G.init_rows(m), g['init']) and same(G.randstream(m, g['init']), g['randstream'])
    for rt in (0, 1):
        assert same(O.sim(sol, g['init'], g['randstream'], rt), g['sims%d' % rt]), '%s: panel, rndtype=%d' % (name, rt)
    cases = G.recorded_call_cases(m, sol.nt)
    assert len(cases) == int(g['ncall'])
    for k, (sw, args) in enumerate(cases):
        assert sw == int(g['call%d_sw' % k]) and same(args, g['call%d_args' % k])
        assert same(O.call(sol, sw, args), g['call%d_res' % k]), '%s: accessor case %d (switch %d)' % (name, k, sw)


@pytest.mark.parametrize('key,native,ndraw', [('a0m5', True, G.NDRAWS), ('a0_0', True, G.NDRAWS), ('a0m5', False, 64), ('a0_0', False, 96)])
def test_oracle_fails_on_the_draws_the_reference_fails_on(key, native, ndraw):
    """The first 256 C2 draws of the bench (the portable build: a leading part of them that holds failing draws)."""
    from egdst_amd import workloads
    g = G.load('ref_C2_draws.npz')
    m, gen = workloads.c2(a0=G.DRAW_SETS[key])
    P = gen(4096)[:G.NDRAWS]
    assert same(P, g[key + '_params'])
    assert int(g[key + '_failed'].sum()) == NFAIL[key]
    assert g[key + '_failed'][:ndraw].any()
    O = Oracle(m, native_math=native)
    for i in range(ndraw):
        sol = O.solve(params=P[i])
        what = 'C2 %s draw %d' % (key, i)
        assert bool(sol.err) == bool(g[key + '_failed'][i]), (what, sol.err, str(g[key + '_err'][i]))
        assert same_text(str(g[key + '_err'][i]), sol.err), (what, sol.err, str(g[key + '_err'][i]))
        if sol.err:
            assert G.fail_cell(sol.len, False) == tuple(g[key + '_cell'][i]), what
        assert same(sol.len, g[key + '_len'][i]) and same(sol.thlen, g[key + '_thlen'][i]), what
        assert G.draw_checksum(cell_sums(sol)) == g[key + '_checksum'][i], what


@pytest.mark.parametrize('name,native', [('C1', True), ('C1', False), ('C2', True), ('C2', False), ('C2_a0m5', True),
                                         ('C2_a0m5', False), ('C3', True), ('C3', False), ('C4', True)])
def test_oracle_equals_the_reference_checksums_at_full_size(name, native):
    g = G.load('ref_big_%s.npz' % name)
    m, par = BIG[name][0]()
    d = m.descriptor()
    for k in ('t0', 'T', 'ngridm', 'ngridmax', 'nthrhmax', 'ny', 'mmax', 'a0'):
        assert d[k] == g[k], (name, k)
    sol = Oracle(m, native_math=native).solve(par)
    assert sol.rc == 0, sol.err
    assert same(sol.len, g['len']) and same(sol.thlen, g['thlen'])
    bad = np.argwhere(cell_sums(sol) != g['sums'])
    assert len(bad) == 0, ('cells (it, ist, column) whose checksum differs', bad[:8].tolist(), len(bad))


def test_reference_checksums_equal_the_oracle_fixtures_at_full_size():
    """big_*.npz came from the oracle, ref_big_*.npz from the reference: the same rows, thresholds and checksums."""
    for name in G.BIG_REF:
        a, b = G.load('ref_big_%s.npz' % name), G.load('big_%s.npz' % name)
        for k in ('len', 'thlen', 'sums', 'lastM', 'params'):
            assert same(a[k], b[k]), (name, k)


@pytest.mark.skipif(not ref_harness.available(), reason='no reference sources (EGDST_REFERENCE_DIR): fixtures cannot be regenerated')
@pytest.mark.parametrize('fname', sorted(G.targets()))
def test_regenerated_fixture_equals_the_committed_one(fname):
    committed = G.load(fname)
    fresh = G.targets()[fname]()
    assert sorted(fresh) == sorted(committed.files)
    for k in committed.files:
        assert same(np.asarray(fresh[k]), committed[k]), (fname, k)
