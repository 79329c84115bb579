"""The MEX shims (shims/*.c) RUN: each compiled with the runnable MEX host (oracle/mexhost/), linked to the CPU harness build
of the model's device code (tests/cpu_emu) and driven through ``ref_run`` exactly like the reference's own gateway
(tests/shim_harness.py; one fresh child process per model).  Outputs, gateway errors and warnings are held to the recorded
reference (tests/golden/ref_*.npz), to the live reference where its sources are present, and, for inputs on which the
reference reads past an array or dereferences a missing property, to gateway errors of the shims' own.
The same runs on the MI355X library: tests/test_gpu_shims.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mex_object  # noqa: E402
import ref_harness  # noqa: E402
import shim_cases as S  # noqa: E402
import shim_harness as H  # noqa: E402
from test_reference_fixtures import same_text  # noqa: E402

FIXTURE_MODELS = ['retirement2', 'occ3', 'model2', 'retirement8', 'retirement_hc', 'retirement_mortal', 'cake_normal']
OWN = {   # gateway errors of the shims' own, where the reference reads past an array or dereferences NULL
    'no_init': 'Error: the model object has no init or no randstream!',
    'cells': 'Error: the cells of M and D do not have the layout of a solution!',
    'call_inputs': 'Error in call(): the model, the switch and the arguments are needed!',
    'call_columns': 'Error in call(): every row of arguments starts with it and ist!',
}


@pytest.mark.parametrize('name', FIXTURE_MODELS)
def test_shims_equal_the_recorded_reference(name):
    """The solver shim's cells and dbgout; the simulator and accessor shims on the recorded cells: values, warnings
    (text, count, order), and the gateway errors for a short randstream and an unsolved object."""
    g, m, props = S.fixture(name)
    res = H.run(H.build_emu_for_model(m), props, S.parity_calls(g, m, 'props'), timeout=300)
    S.check_parity(res, g, name, m.nd)


@pytest.mark.skipif(not ref_harness.available(), reason='no reference sources (EGDST_REFERENCE_DIR)')
@pytest.mark.parametrize('name', ['retirement2', 'retirement_hc'])
def test_shims_equal_the_live_reference_call_by_call(name):
    """Both gateways get the same object (tests/mex_object.py) and are compared whole."""
    g, m, props = S.fixture(name)
    sol = S.FixtureSolution(g)
    R = ref_harness.Reference(m)
    nsim, nt = len(g['init']), sol.nt
    calls = S.parity_calls(g, m, 'props')
    res = H.run(H.build_emu_for_model(m), props, calls, timeout=300)
    ref = R.solve(params=g['params'], dbgout=True)
    r = res[0]
    assert ref.rc == 0 and r['rc'] == 0 and (r['warn'], r['nwarn']) == (ref.warnings, ref.nwarn)
    assert S.same(r['len'], ref.len) and S.same(r['thlen'], ref.thlen)
    assert S.same(r['mcav'], np.concatenate([ref.cell_M(it, ist) for it in range(nt) for ist in range(sol.nst)]))
    assert S.same(r['dth'], np.concatenate([ref.cell_D(it, ist) for it in range(nt) for ist in range(sol.nst)]))
    assert S.same(r['dbgout'], np.asarray(ref.dbgout))
    for c, r in zip(calls[1:], res[1:]):
        rs = c.get('set', {}).get('randstream', g['randstream'])
        given = sol if c['cells'] == 'props' else None
        if c['gw'] == 'simulator':
            q = R.sim(given, g['init'], rs, int(c['rhs'][0]), params=g['params'])
            ours = r.get('sims')
            theirs = q.sims
        else:
            q = R.call(given, int(c['rhs'][0]), c['rhs'][1], params=g['params'])
            ours, theirs = r.get('res'), q.res
        what = (name, c['gw'], [np.shape(a) for a in c['rhs']], len(rs))
        assert (r['rc'] != 0) == (theirs is None) and r['err'] == q.err, (what, r['rc'], r['err'], q.err)
        assert (r['warn'], r['nwarn']) == (q.warnings, q.nwarn), (what, r['warn'][:300], q.warnings[:300])
        if theirs is not None:
            assert S.same(ours, theirs), what


def _damaged_calls(g, m):
    init, rs, rows, cases = S.damaged_cells(g, m)
    sets = {k: mex_object.properties(m, g['params'], sol, init, rs) for k, (sol, _) in cases.items()}
    return init, rs, rows, cases, sets


def test_an_empty_and_a_one_row_cell_are_handled_as_stated():
    """A cell on an agent's path that is empty, or has one row, after a refused init row; the value function on that cell.
    The accessor does what the reference does, warnings included; the simulator ends in the reference's gateway error for a
    missing cell, without the warning about the refused agent (INTEGRATION.md states both differences; the live test below
    holds the reference to its side of them)."""
    g, m, props = S.fixture('retirement2')
    init, rs, rows, cases, sets = _damaged_calls(g, m)
    shims = H.build_emu_for_model(m)
    whole = H.run(shims, props, [{'gw': 'call', 'rhs': [6, rows]}], timeout=300)[0]
    assert whole['rc'] == 0 and whole['nwarn'] == 0 and np.isfinite(whole['res']).all()
    for label, (sol, hit) in cases.items():
        sim, call = H.run(shims, sets[label], [{'gw': 'simulator', 'rhs': [0]}, {'gw': 'call', 'rhs': [6, rows]}], timeout=300)
        S.check_damaged_cells(label, sim, call, whole['res'], hit)


@pytest.mark.skipif(not ref_harness.available(), reason='no reference sources (EGDST_REFERENCE_DIR)')
def test_the_live_reference_on_an_empty_and_a_one_row_cell():
    """The reference's side of the two stated differences, and the accessor whole."""
    g, m, props = S.fixture('retirement2')
    init, rs, rows, cases, sets = _damaged_calls(g, m)
    R = ref_harness.Reference(m)
    shims = H.build_emu_for_model(m)
    for label, (sol, hit) in cases.items():
        sim, call = H.run(shims, sets[label], [{'gw': 'simulator', 'rhs': [0]}, {'gw': 'call', 'rhs': [6, rows]}], timeout=300)
        q = R.sim(sol, init, rs, 0, params=g['params'])
        assert q.sims is None and sim['rc'] == 1
        assert q.err == (S.NOT_FOUND if label == 'empty' else S.INTERP) and sim['err'] == S.NOT_FOUND
        assert (q.nwarn, q.warnings) == (1, S.REFUSED_INDEX) and (sim['nwarn'], sim['warn']) == (0, '')
        c = R.call(sol, 6, rows, params=g['params'])
        assert (call['rc'], call['err'], call['nwarn'], call['warn']) == (0, c.err, c.nwarn, c.warnings), (label, call['warn'], c.warnings)
        assert S.same(call['res'], c.res), (label, call['res'], c.res)


def _failing_draw():
    """The first failing draw of the recorded C2 draws at a0 = -5 (tests/golden/ref_C2_draws.npz)."""
    from egdst_amd import workloads
    g = S.G.load('ref_C2_draws.npz')
    i = int(np.argmax(g['a0m5_failed']))
    assert g['a0m5_failed'][i]
    m, _ = workloads.c2(a0=S.G.DRAW_SETS['a0m5'])
    return g, i, m, mex_object.properties(m, g['a0m5_params'][i])


def check_failing_solve(r, g, i):
    """The reference's solver gateway does not raise when the solver fails (egdst_solver.c:237): clean return, one warning
    with the solver's message, the cells solved so far."""
    assert r['rc'] == 0 and r['err'] == '', (r['rc'], r['err'])
    assert r['nwarn'] == 1, (r['nwarn'], r['warn'])
    assert r['warn'].endswith('\n') and same_text(str(g['a0m5_err'][i]), r['warn'][:-1]), (r['warn'], str(g['a0m5_err'][i]))
    assert S.same(r['len'], g['a0m5_len'][i]) and S.same(r['thlen'], g['a0m5_thlen'][i])


def test_a_failing_solve_warns_once_and_returns_the_cells_solved_so_far():
    g, i, m, props = _failing_draw()
    res = H.run(H.build_emu_for_model(m), props, [{'gw': 'solver'}], timeout=600)
    check_failing_solve(res[0], g, i)


def test_malformed_objects_and_argument_counts_end_as_gateway_errors():
    """Host logic, the same on both machines.  What the live reference does with each case (tried on its own gateways, built
    by oracle/build_ref.py): without init, without randstream, and with two inputs to the accessor it dereferences NULL
    (SIGSEGV); with 3-column M cells or a one-column argument matrix it reads past the array and returns numbers; the
    argument-count cases are gateway errors, or for the accessor warnings, with the texts asserted here.  No case may end
    the child by a signal (H.run raises if one does)."""
    name = 'retirement2'
    g, m, props = S.fixture(name)
    M3 = [None if a is None else a[:, :3] for a in props['M']]
    a3 = g['call2_args']
    calls = [
        ({'gw': 'simulator', 'rhs': [0], 'drop': ['init']}, 1, OWN['no_init'], 0),
        ({'gw': 'simulator', 'rhs': [0], 'drop': ['randstream']}, 1, OWN['no_init'], 0),
        ({'gw': 'simulator', 'rhs': [0], 'cells': 'M3'}, 1, OWN['cells'], 0),
        ({'gw': 'call', 'rhs': [6, g['call5_args']], 'cells': 'M3'}, 1, OWN['cells'], 0),
        ({'gw': 'call', 'rhs': [3, a3[:, :1]]}, 1, OWN['call_columns'], 0),
        ({'gw': 'solver', 'nlhs': 0}, 1, 'Error: wrong number of outputs!', 0),
        ({'gw': 'solver', 'nlhs': 2}, 1, 'Error: wrong number of outputs!', 0),
        ({'gw': 'solver', 'nrhs': 2}, 1, 'Error: wrong number of inputs!', 0),
        ({'gw': 'solver', 'nrhs': 0}, 1, 'Error: wrong number of inputs!', 0),
        ({'gw': 'simulator', 'rhs': [0], 'nlhs': 0}, 1, 'Error: wrong number of outputs!', 0),
        ({'gw': 'simulator', 'rhs': [0], 'nlhs': 2}, 1, 'Error: wrong number of outputs!', 0),
        ({'gw': 'simulator', 'rhs': [0], 'nrhs': 1}, 1, 'Error: wrong number of inputs!', 0),
        ({'gw': 'simulator', 'rhs': [0], 'nrhs': 3}, 1, 'Error: wrong number of inputs!', 0),
        ({'gw': 'call', 'rhs': [3, a3], 'nlhs': 0}, 0, 'Error in call(): wrong number of outputs!\n', 1),
        ({'gw': 'call', 'rhs': [3, a3], 'nlhs': 2}, 0, 'Error in call(): wrong number of outputs!\n', 1),
        ({'gw': 'call', 'rhs': [3, a3], 'nrhs': 4}, 0, 'Error in call(): wrong number of inputs!\n', 1),
        ({'gw': 'call', 'rhs': [3, a3], 'nrhs': 2}, 1, OWN['call_inputs'], 1),
    ]
    props3 = dict(props, M=M3)
    shims = H.build_emu_for_model(m)
    res = H.run(shims, props, [dict(c, cells='props') for c, _, _, _ in calls if c.get('cells') != 'M3'], timeout=300)
    res3 = H.run(shims, props3, [dict(c, cells='props') for c, _, _, _ in calls if c.get('cells') == 'M3'], timeout=300)
    it, it3 = iter(res), iter(res3)
    for c, rc, text, nwarn in calls:
        r = next(it3 if c.get('cells') == 'M3' else it)
        assert r['rc'] == rc and r['nwarn'] == nwarn, (c['gw'], {k: v for k, v in c.items() if k != 'rhs'}, r['rc'], r['err'], r['warn'])
        assert (r['err'] if rc else r['warn']) == text, (c['gw'], r['err'], r['warn'])
        if rc == 0:   # the accessor goes on after its warning: the discount factors of the recorded case
            assert S.same(r['res'], g['call2_res'])
