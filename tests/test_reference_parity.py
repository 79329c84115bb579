"""Hold the CPU oracle to a LIVE build of the reference's own solver, simulator and accessor (oracle/build_ref.py).

Everything else in this suite is bit-for-bit against ``oracle/egdst_oracle.c``; this file is where the oracle itself is held
to the program it restates.  The requirement is equality: ``np.array_equal`` with NaNs matched, identical row counts and D
sequences, identical sets of failing draws.  Both programs are plain IEEE double on the same libm without contraction.

Skipped when there is neither a reference directory (``EGDST_REFERENCE_DIR``) nor libraries built earlier under
``oracle/_ref/``.

Sites where the reference's value is not a function of its inputs (evidence in DESIGN.md section 4); none of them is in a
solver table, a row count, a D sequence or a failing-draw set:
  * the accessor's value function at the TERMINAL period evaluates utility with ``id`` of whatever row went through the
    value-function routine before it (an uninitialised struct field for the first row).  The comparison there is still
    exact: the reference's number must equal the oracle's utility at that carried-over decision (`_terminal_rows`).
  * the cell the solver stores AFTER an error is a copy of its workspace under a stale length; cells computed before the
    error are compared exactly, the failing cell is identified and compared by position only (`_fail_cell`).
  * one error message of the reference has five lines; the oracle and the device keep its first line (`LONG_MESSAGE`).
    Every other message is compared in full.
  * with a continuous state, an init row whose continuous component is not at the first grid point makes the reference's
    simulator address another period's cell; the oracle refuses such a row (asserted in `test_simulator`).
"""
import time

import numpy as np
import pytest

from egdst_amd import examples, workloads
from call_cases import call_cases
from oracle_harness import Oracle
import ref_harness
from ref_harness import Reference

pytestmark = pytest.mark.skipif(
    not ref_harness.available(examples.retirement2()),
    reason='no reference sources (EGDST_REFERENCE_DIR) and no reference libraries under oracle/_ref/')

TABLES = ('M', 'C', 'V', 'D', 'TH')


def eq(a, b):
    return a is not None and b is not None and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# the one message of the reference that has more than one line; the oracle and the device keep its first line
LONG_MESSAGE = 'Error:\nAll of the choices lead to -inf value functions for all values of money-at-hand!'
NFAIL = {-5.0: 24, 0.0: 6}     # failing draws among the first 256 of the bench's C2 batch


def same_text(ref_err, orc_err):
    """The whole text for every message; of LONG_MESSAGE the oracle holds the first line only."""
    if ref_err.startswith(LONG_MESSAGE + '\n'):
        return orc_err == LONG_MESSAGE
    return orc_err == ref_err


def assert_same_solution(ref, orc, what, upto=None):
    """Row counts, every [M C A V] and [D TH] matrix of every (it, ist).  `upto`: only cells solved before that position."""
    nt, nst = ref.len.shape
    ncmp = 0
    for it in range(nt - 1, -1, -1):
        for ist in range(nst):
            if upto is not None and (it, ist) == upto:
                return ncmp
            assert ref.len[it, ist] == orc.len[it, ist], '%s: rows of it=%d ist=%d: %d vs %d' % (what, it, ist, ref.len[it, ist], orc.len[it, ist])
            assert ref.thlen[it, ist] == orc.thlen[it, ist], '%s: thresholds of it=%d ist=%d' % (what, it, ist)
            assert eq(ref.cell_M(it, ist), orc.cell_M(it, ist)), '%s: [M C A V] of it=%d ist=%d differs' % (what, it, ist)
            assert eq(ref.cell_D(it, ist), orc.cell_D(it, ist)), '%s: [D TH] of it=%d ist=%d differs' % (what, it, ist)
            if (it, ist) in getattr(ref, 'A', {}):       # the reference's own third column
                assert eq(ref.A[(it, ist)], orc.cell_M(it, ist)[:, 2]), '%s: A of it=%d ist=%d' % (what, it, ist)
            ncmp += 1
    assert upto is None, '%s: failing cell %s not reached' % (what, upto)
    return ncmp


def _fail_cell(sol, stores_failing_cell):
    """Position (it, ist) of the cell at which a failed solve stopped, in solving order (it down, ist up).  The reference
    stores the failing cell before it returns, the oracle does not."""
    nt, nst = sol.len.shape
    order = [(it, ist) for it in range(nt - 1, -1, -1) for ist in range(nst)]
    filled = [k for k, c in enumerate(order) if sol.len[c] > 0]
    last = filled[-1] if filled else -1
    assert filled == list(range(last + 1)), 'cells are not filled in solving order'
    return order[last] if stores_failing_cell else order[last + 1]


def assert_same_outcome(ref, orc, what):
    assert bool(ref.err) == bool(orc.err), '%s: reference %r, oracle %r' % (what, ref.err, orc.err)
    if not ref.err:
        assert_same_solution(ref, orc, what)
        return None
    assert same_text(ref.err, orc.err), (what, ref.err, orc.err)
    cell = _fail_cell(ref, True)
    assert cell == _fail_cell(orc, False), '%s: fails at %s in the reference, at %s in the oracle' % (what, cell, _fail_cell(orc, False))
    assert_same_solution(ref, orc, what, upto=cell)
    return cell


def assert_same_dbgout(ref, orc, what):
    assert ref.dbgn == orc.dbgn, '%s: dbgout rows %d vs %d' % (what, ref.dbgn, orc.dbgn)
    assert eq(np.asarray(ref.dbgout), np.asarray(orc.dbgout)), '%s: dbgout differs' % what


def _example(name):
    return examples.retirement8(T=5, ngridm=10) if name == 'retirement8' else examples.REGISTRY[name]()


# ------------------------------------------------------------------------------------------------ solver
@pytest.mark.parametrize('name', sorted(examples.REGISTRY))
def test_solver_example_models(name):
    """All twelve example models at their shipped sizes (retirement8, whose shipped size is the C5 stress size, at the
    size the suite builds it for: T=5, ngridm=10; its middle size is below)."""
    m = _example(name)
    ref = Reference(m).solve(dbgout=True)
    orc = Oracle(m, native_math=True).solve(dbgout=True)
    assert ref.err == '' and orc.err == ''
    assert ref.total_rows() > 0
    assert_same_solution(ref, orc, name)
    assert_same_dbgout(ref, orc, name)


def _c4_reduced():
    # C4 at full size (ngridm=65536, T=80, ny=21) costs about 20 s per solve in either CPU program; a quarter of the grid
    # keeps this file's wall time in minutes.  The full size is held through the checksums of tests/golden/big_C4*.npz.
    return workloads.c4(ngridm=16384)[0]


WORKLOADS = {
    'C1': lambda: workloads.c1()[0],
    'C2_a0m5': lambda: workloads.c2()[0],
    'C2_a0_0': lambda: workloads.c2(a0=0)[0],
    'C3': lambda: workloads.c3()[0],
    'C4_ngridm16384': _c4_reduced,
    'C5_T5_n10': lambda: workloads.c5(ngridm=10, T=5)[0],
    'C5_T20_n500': lambda: workloads.c5(ngridm=500, T=20)[0],
}


@pytest.mark.parametrize('name', sorted(WORKLOADS))
def test_solver_workloads(name):
    m = WORKLOADS[name]()
    t = time.perf_counter()
    ref = Reference(m).solve(dbgout=True)
    t_ref = time.perf_counter() - t
    orc = Oracle(m, native_math=True).solve(dbgout=True)
    print('%s: reference solve %.2f s, %d rows' % (name, t_ref, ref.total_rows()))
    assert ref.err == '' and orc.err == ''
    assert_same_solution(ref, orc, name)
    assert_same_dbgout(ref, orc, name)


# ------------------------------------------------------------------------------------------------ failing draws
@pytest.mark.parametrize('a0', [-5.0, 0.0])
def test_c2_failing_draws(a0):
    """The first 256 of the bench's own C2 draws: the draws that fail, the cell at which each fails and the message are
    the reference's; every solved draw matches in full."""
    m, draws = workloads.c2(a0=a0)
    par = draws(4096)[:256]
    R, O = Reference(m), Oracle(m, native_math=True)
    failed = {}
    for i, p in enumerate(par):
        ref, orc = R.solve(params=p), O.solve(params=p)
        cell = assert_same_outcome(ref, orc, 'C2 a0=%g draw %d' % (a0, i))
        if ref.err:
            failed[i] = (cell, ref.err)
    print('C2 a0=%g: %d of 256 draws fail in the reference and in the oracle: %s' % (a0, len(failed), sorted(failed)))
    assert len(failed) == NFAIL[a0]


def test_survey_recorded_case_retirement2_T100():
    """SURVEY.md recorded that retirement2 with a0=-5, T=100 aborted near it=65 in a stand-in build.  Whatever the live
    reference does with it, the oracle does the same."""
    for over in ({}, {'ngridm': 1000, 'ngridmax': 10000}):
        m = examples.retirement2(T=100, **over)
        ref, orc = Reference(m).solve(), Oracle(m, native_math=True).solve()
        cell = assert_same_outcome(ref, orc, 'retirement2 T=100 %s' % over)
        print('retirement2 a0=-5 T=100 %s: err=%r cell=%s' % (over, ref.err, cell))


# ------------------------------------------------------------------------------------------------ simulator
def _init_rows(m):
    """Every state index whose continuous components sit at their first grid point (the simulator's own convention for
    a starting index), each with cash below a0, at a0, inside, at mmax and beyond; plus indices outside [1, nst]."""
    sizes, strides = [int(v) for v in m.stm[:m.nnst]], [int(v) for v in m.stm[m.nnst:]]
    rows = []
    for ist in range(m.nst):
        if any(v.type == 'continuous' and (ist // strides[k]) % sizes[k] for k, v in enumerate(m.s)):
            continue
        for cash in (m.a0 - 1.0, m.a0, m.a0 + 0.25, 0.5 * (m.a0 + m.mmax), m.mmax, 1.5 * m.mmax):
            rows.append([ist + 1, cash])
    rows += [[0, 1.0], [m.nst + 1, 1.0]]
    return np.array(rows, dtype=float)


@pytest.mark.parametrize('name', ['retirement2', 'retirement_hc', 'retirement_mortal', 'cake_normal', 'occ3', 'model2',
                                  'deaton2', 'retirement8'])
def test_simulator(name):
    m = _example(name)
    R, O = Reference(m), Oracle(m, native_math=True)
    sol = R.solve()                      # the reference's own M / D
    assert sol.err == ''
    init = _init_rows(m)
    rs = np.random.default_rng(11).random(4 * m.nt * len(init))
    for rndtype in (0, 1):
        ref = R.sim(sol, init, rs, rndtype)
        assert ref.err == '' and ref.sims is not None
        orc = O.sim(sol, init, rs, rndtype)
        assert eq(ref.sims, orc), '%s rndtype=%d: sims differ' % (name, rndtype)
        assert np.isfinite(ref.sims[:, 0, 0]).sum() >= (len(init) - 2) // 2     # the in-range rows did simulate
        assert ref.nwarn >= 2                                                   # the out-of-range rows were refused
    # a randstream one number short of what each mode needs: the gateway raises, the oracle returns its refusal codes
    short0 = R.sim(sol, init, rs[:4 * m.nt * len(init) - 1], 0)
    short1 = R.sim(sol, init, rs[:4 * m.nt - 1], 1)
    assert short0.sims is None and 'randstream is too short' in short0.err
    assert short1.sims is None and 'randstream is too short' in short1.err
    with pytest.raises(RuntimeError, match='rc=-3'):
        O.sim(sol, init, rs[:4 * m.nt * len(init) - 1], 0)
    with pytest.raises(RuntimeError, match='rc=-2'):
        O.sim(sol, init, rs[:4 * m.nt - 1], 1)
    assert R.sim(sol, init, rs[:4 * m.nt], 1).err == ''                        # exactly enough is enough
    if any(v.type == 'continuous' for v in m.s):
        # a starting index whose continuous component is not the first grid point: the reference adds the component's
        # stride a second time and reads the cell of another period; the oracle refuses the call
        with pytest.raises(RuntimeError, match='rc=-4'):
            O.sim(sol, np.array([[m.nst, 1.0]]), rs, 0)


# ------------------------------------------------------------------------------------------------ accessor
def _terminal_rows(m, sol, args):
    """For a value-function call (switch 6): {row: decision index the reference evaluates utility with} for the rows of
    the terminal period.  egdst_call.c leaves `id` as the last row that went through its value-function routine left it
    (zero under the build's pin when there was none).
    Built from the solved tables and the arguments alone, never from the accessor's results.  Invariants: rows above mmax
    are answered before `id` is touched; a non-terminal row sets `id` to D[ith-1] with ith >= 1, which holds because the
    first threshold of every cell is -inf (asserted); call_cases puts bad it/ist only where the whole result is NaN or
    into cases of other switches, and such a call is recognised by its arguments (`_has_bad_index`)."""
    nt = sol.nt
    carried, out = 0, {}
    for i, (it, ist, cash) in enumerate(args):
        it, ist = int(it) - int(m.t0), int(ist) - 1
        if cash > m.mmax:
            continue
        if it == nt - 1:
            out[i] = carried
        else:
            th = sol.TH[it, ist, :sol.thlen[it, ist]]
            assert len(th) and cash >= th[0]
            ith = 0
            while ith < len(th) and cash >= th[ith]:
                ith += 1
            carried = int(sol.D[it, ist, ith - 1])
    return out


def _has_bad_index(m, sol, args):
    it, ist = args[:, 0] - m.t0, args[:, 1] - 1
    return bool(((it < 0) | (it > sol.nt - 1) | (ist < 0) | (ist > sol.nst - 1)).any())


def _extra_call_cases(m, sol):
    """Arguments below M(a0) and above the last grid point of every period/state, and every switch the gateway knows
    plus two it does not."""
    rows = []
    for it in range(sol.nt - 1):
        for ist in range(sol.nst):
            n = sol.len[it, ist]
            m1, mlast = sol.M[it, ist, 1], sol.M[it, ist, n - 1]
            for cash in (m.a0, 0.5 * (m.a0 + m1), m1, mlast, min(m.mmax, 0.5 * (mlast + m.mmax)), m.mmax):
                rows.append([it + m.t0, ist + 1, cash])
    cases = [(6, np.array(rows))]
    two = np.array([[m.t0, 1.0], [m.t0 + 1, float(m.nst)]])
    cases += [(sw, two) for sw in (0, 3, 7, -1)]
    return cases


@pytest.mark.parametrize('name', ['retirement2', 'retirement_hc', 'occ3', 'model2', 'retirement8', 'cake_normal'])
def test_call_accessor(name):
    m = _example(name)
    R, O = Reference(m), Oracle(m, native_math=True)
    sol = R.solve()
    assert sol.err == ''
    depends_on_id = not m.analyse_optim()['optim_UnoD']
    for k, (sw, args) in enumerate(call_cases(m, sol.nt, m.nst, m.nd) + _extra_call_cases(m, sol)):
        ref = R.call(sol, sw, args)
        orc = O.call(sol, sw, args)
        assert ref.err == '' and ref.res is not None
        expect = orc.copy()
        if sw == 6 and args.shape[1] == 3 and depends_on_id and not _has_bad_index(m, sol, args):
            for i, idc in _terminal_rows(m, sol, args).items():
                if idc != 0 and not np.isnan(orc[i]):
                    expect[i] = O.call(sol, 1, [[args[i, 0], args[i, 1], idc + 1, max(0.0, args[i, 2])]])[0]
        assert eq(ref.res, expect), '%s case %d (switch %d): %s' % (name, k, sw, np.argwhere(~((ref.res == expect) | (np.isnan(ref.res) & np.isnan(expect)))).ravel())
