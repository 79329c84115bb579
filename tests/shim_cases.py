"""What a run of the MEX shims is held to, shared by tests/test_shims_run.py (CPU harness library) and
tests/test_gpu_shims.py (MI355X): the recorded outputs, errors and warnings of the reference's own gateways
(tests/golden/ref_<model>.npz).  Reads tests/golden/ only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import make_golden_ref as G  # noqa: E402
import mex_object  # noqa: E402

RAND_SHORT = {0: 'Error: randstream is too short to be used for all requested simulations!',
              1: 'Error: randstream is too short even to be re-used for each simulated agent!'}
NOT_SOLVED = 'Error: the model has not yet been solved!'
NOT_FOUND = 'Solution not found in model.M'
INTERP = 'Error:\nError: At least two points are required for interpolation!'
MISSING = 'Solution missing for given it,ist..\n'
REFUSED_INDEX = 'Initial state index st(0) out of bounds! Moving to next simulation.\n'


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f' and b.dtype.kind == 'f')


class FixtureSolution:
    """The recorded cells of a ref_<model>.npz in the shape mex_object.properties() reads."""

    def __init__(self, g):
        self.len, self.thlen = g['len'], g['thlen']
        self.nt, self.nst = self.len.shape
        self._m, self._d = g['mcav'], g['dth']
        self._mo = np.concatenate([[0], np.cumsum(self.len.reshape(-1))])
        self._do = np.concatenate([[0], np.cumsum(self.thlen.reshape(-1))])

    def cell_M(self, it, ist):
        k = it * self.nst + ist
        return self._m[self._mo[k]:self._mo[k + 1]]

    def cell_D(self, it, ist):
        k = it * self.nst + ist
        return self._d[self._do[k]:self._do[k + 1]]


def fixture(name):
    """(recorded arrays, model, properties of the model object with the recorded cells, init and randstream)"""
    g = G.load('ref_%s.npz' % name)
    m = G.MODELS[name]()
    props = mex_object.properties(m, g['params'], FixtureSolution(g), g['init'], g['randstream'])
    return g, m, props


class EditedSolution:
    """A solution with the cells ``empty`` [(it, ist)] emptied and the M cells ``short`` cut to their first row."""

    def __init__(self, base, empty=(), short=()):
        self._b, self.nt, self.nst, self._short = base, base.nt, base.nst, set(short)
        self.len, self.thlen = base.len.copy(), base.thlen.copy()
        for c in empty:
            self.len[c] = self.thlen[c] = 0
        for c in short:
            self.len[c] = 1

    def cell_M(self, it, ist):
        return self._b.cell_M(it, ist)[:1] if (it, ist) in self._short else self._b.cell_M(it, ist)

    def cell_D(self, it, ist):
        return self._b.cell_D(it, ist)


def shim_models():
    """Every model whose shims the GPU tests load (__graft_entry__.build() builds them)."""
    from egdst_amd import workloads
    return [mk() for mk in G.MODELS.values()] + [workloads.c2(a0=G.DRAW_SETS['a0m5'])[0]]


def damaged_cells(g, m):
    """A solution of a model with one state per period (retirement2) that lacks a cell, or has a one-row cell, on the path
    of the second agent; the first agent's init row is refused.  (init, randstream, value-function rows,
    {label: (solution, index of the value-function row that reads the damaged cell)})."""
    sol = FixtureSolution(g)
    assert sol.nst == 1 and sol.nt > 4
    init = np.array([[0, 1.0], [1, 1.0], [2, 1.0]])
    rows = np.array([[m.t0, 1, 1.0], [m.t0 + 3, 1, 1.0], [m.t0 + 1, 1, 2.0]])
    return init, g['randstream'][:4 * sol.nt * len(init)], rows, {
        'empty': (EditedSolution(sol, empty=[(3, 0)]), 1), 'one_row': (EditedSolution(sol, short=[(0, 0)]), 0)}


def check_damaged_cells(label, sim, call, whole, hit):
    """What the shims do on damaged_cells() (diagnostics).  ``whole``: the accessor's result for the same
    rows on the undamaged solution."""
    # stated differences: no warning about the refused agent before the error (the reference has issued one), and a
    # one-row cell is a missing cell for the simulator (the reference raises the interpolation's message)
    assert (sim['rc'], sim['err'], sim['nwarn'], sim['warn']) == (1, NOT_FOUND, 0, ''), (label, sim['rc'], sim['err'], sim['warn'])
    assert call['rc'] == 0 and call['err'] == '', (label, call['err'])
    want = np.array(whole, dtype=float)
    if label == 'empty':
        want[hit] = np.nan
        assert (call['nwarn'], call['warn']) == (1, MISSING), (label, call['warn'])
    else:
        want[hit] = -1.0    # linter's return value on fewer than two points (egdst_lib.c:171)
        n = 2 * (len(want) - hit)   # the message is never cleared: twice for this row and for every later one
        assert (call['nwarn'], call['warn']) == (n, (INTERP + '\n') * n), (label, call['nwarn'], call['warn'])
    assert same(call['res'], want), (label, call['res'], want)


def parity_calls(g, m, cells):
    """Solver, both simulator panels, every recorded accessor case and the two with a wrong column count, the diagnostics:
    a randstream one number short and exactly long enough in both modes, an object without M and D."""
    nsim, nt = len(g['init']), g['len'].shape[0]
    calls = [{'gw': 'solver', 'drop': ['init', 'randstream'], 'cells': 'none'}]
    calls += [{'gw': 'simulator', 'rhs': [rt], 'cells': cells} for rt in (0, 1)]
    calls += [{'gw': 'call', 'rhs': [g['call%d_sw' % k], g['call%d_args' % k]], 'cells': cells} for k in range(int(g['ncall']))]
    calls += [{'gw': 'call', 'rhs': [g['xcall%d_sw' % k], g['xcall%d_args' % k]], 'cells': cells} for k in range(2)]
    for rt, need in ((0, 4 * nt * nsim), (1, 4 * nt)):
        calls.append({'gw': 'simulator', 'rhs': [rt], 'cells': cells, 'set': {'randstream': g['randstream'][:need - 1]}})
        calls.append({'gw': 'simulator', 'rhs': [rt], 'cells': cells, 'set': {'randstream': g['randstream'][:need]}})
    calls.append({'gw': 'simulator', 'rhs': [0], 'cells': 'none'})
    calls.append({'gw': 'call', 'rhs': [g['call0_sw'], g['call0_args']], 'cells': 'none'})
    return calls


def check_solver(r, g, what, nd):
    """``nd``: the model's number of discrete choices (the kink log has nt*nst*nd*2*nt rows)."""
    assert r['rc'] == 0 and r['err'] == '' and r['nwarn'] == 0 and r['warn'] == '', (what, r['rc'], r['err'], r['warn'])
    nt, nst = g['len'].shape
    assert r['ncells'] == nt * nst
    assert same(r['len'], g['len']), (what, 'cells are empty exactly where len == 0', np.argwhere(r['len'] != g['len'])[:5])
    assert same(r['thlen'], g['thlen']), (what, np.argwhere(r['thlen'] != g['thlen'])[:5])
    assert same(r['mcav'], g['mcav']), (what, 'rows of M')
    assert same(r['dth'], g['dth']), (what, 'rows of D')
    dbgn = int(g['dbgn'])
    assert r['dbgout'].shape == (nt * nst * nd * 2 * nt, 7), (what, r['dbgout'].shape)
    assert same(r['dbgout'][:dbgn], g['dbgout']), (what, 'dbgout')
    assert not r['dbgout'][dbgn:].any(), (what, 'dbgout past dbgn')


def check_parity(res, g, name, nd):
    """``res``: the results of parity_calls() in order."""
    it = iter(res)
    check_solver(next(it), g, name, nd)
    for rt in (0, 1):
        r = next(it)
        assert r['rc'] == 0 and r['err'] == '', (name, rt, r['err'])
        assert same(r['sims'], g['sims%d' % rt]), '%s: panel, rndtype=%d' % (name, rt)
        assert r['nwarn'] == int(g['sims%d_nwarn' % rt]) and r['warn'] == str(g['sims%d_warnings' % rt]), \
            '%s: simulator warnings, rndtype=%d: %d %r' % (name, rt, r['nwarn'], r['warn'][:300])
    for key in ['call%d' % k for k in range(int(g['ncall']))] + ['xcall0', 'xcall1']:
        r = next(it)
        assert r['rc'] == 0 and r['err'] == '', (name, key, r['err'])
        assert same(r['res'], g[key + '_res']), '%s: accessor %s (switch %d)' % (name, key, int(g[key + '_sw']))
        assert r['nwarn'] == int(g[key + '_nwarn']) and r['warn'] == str(g[key + '_warnings']), \
            '%s: accessor warnings of %s (switch %d): %d, recorded %d: %r' % (name, key, int(g[key + '_sw']), r['nwarn'],
                                                                              int(g[key + '_nwarn']), r['warn'][:300])
    for rt in (0, 1):
        r = next(it)
        assert r['rc'] == 1 and r['err'] == RAND_SHORT[rt], (name, 'short randstream', rt, r['rc'], r['err'])
        r = next(it)
        assert r['rc'] == 0 and r['err'] == '' and same(r['sims'], g['sims%d' % rt]), (name, 'exact randstream', rt, r['err'])
    for gw in ('simulator', 'call'):
        r = next(it)
        assert r['rc'] == 1 and r['err'] == NOT_SOLVED, (name, gw, 'object without M and D', r['rc'], r['err'])
