"""The MEX shims (shims/*.c) run on the MI355X: each linked with the runnable MEX host (oracle/mexhost/) to the model's
libegdst.so by __graft_entry__.build() and driven like the reference's gateways (tests/shim_harness.py).  A gateway call
loads HIP, so every run is a fresh child process, one at a time; this process only reads tests/golden/ and compares.

    parity       per model: the solver shim, then the simulator and accessor shims on the cell arrays the solver shim returned,
                 read from the model object the MATLAB way; values, gateway errors and warnings equal the recorded reference
    failing draw the first failing C2 draw at a0 = -5, full size: clean return, one warning with the reference's text
    many calls   forty gateway calls in one process: same answers, no device memory left behind
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import shim_cases as S  # noqa: E402
import shim_harness as H  # noqa: E402
from test_shims_run import _failing_draw, check_failing_solve  # noqa: E402

MODELS = sorted(S.G.MODELS)
NCALLS = 40


@pytest.mark.parametrize('name', MODELS)
def test_shims_equal_the_recorded_reference_on_the_device(name):
    g, m, props = S.fixture(name)
    props.pop('M'), props.pop('D')    # the cells come from the solver shim
    res = H.run(H.find_for_model(m), props, S.parity_calls(g, m, 'solver'), timeout=60)
    S.check_parity(res, g, name, m.nd)


def test_a_failing_solve_warns_once_and_returns_the_cells_solved_so_far_on_the_device():
    """C2 at full size (T=60, 1000 grid points)."""
    g, i, m, props = _failing_draw()
    res = H.run(H.find_for_model(m), props, [{'gw': 'solver'}], timeout=60)
    check_failing_solve(res[0], g, i)


def test_forty_gateway_calls_in_one_process_leave_no_device_memory_behind():
    """What an estimation loop in MATLAB does: create, upload, work, destroy, again and again.  Calls cycle solver, simulator,
    accessor on retirement2.  Device memory in use (hipMemGetInfo) is read after call 2 and after call 40; then one live
    handle's footprint is measured in the same process as in-use memory with a handle minus without, the handle made as
    the shims make theirs (EGDST_STREAM_PER_THREAD).  A gateway call that kept its handle's memory would grow the in-use
    figure by that footprint per call, so growth over 38 calls must stay below ONE footprint (the runtime's own pools sit
    below it; DESIGN.md section 7 has the measured values)."""
    name = 'retirement2'
    g, m, props = S.fixture(name)
    cycle = [{'gw': 'solver', 'cells': 'none'}, {'gw': 'simulator', 'rhs': [0], 'cells': 'solver'},
             {'gw': 'call', 'rhs': [g['call5_sw'], g['call5_args']], 'cells': 'solver'}]
    props.pop('M'), props.pop('D')
    calls = [cycle[k % 3] for k in range(NCALLS)]
    calls[2:2] = [{'op': 'meminfo'}]
    calls += [{'op': 'meminfo'}, {'op': 'footprint'}]
    res = H.run(H.find_for_model(m), props, calls, timeout=120)
    mem2, mem40, fp = res[2], res[-2], res[-1]
    gate = res[:2] + res[3:-2]
    assert len(gate) == NCALLS and all(r['rc'] == 0 and r['err'] == '' for r in gate)
    S.check_solver(gate[0], g, name, m.nd)
    assert S.same(gate[1]['sims'], g['sims0']) and S.same(gate[2]['res'], g['call5_res'])
    for k in (NCALLS - 3, NCALLS - 2, NCALLS - 1):     # the last of each kind, the fortieth call among them
        for key in ('len', 'thlen', 'mcav', 'dth', 'dbgout', 'sims', 'res', 'warn', 'nwarn'):
            assert (key in gate[k]) == (key in gate[k % 3]) and (key not in gate[k] or S.same(gate[k][key], gate[k % 3][key])), (k, key)
    growth, footprint = int(mem40['in_use']) - int(mem2['in_use']), int(fp['footprint'])
    sim_ms = 1e3 * float(np.median([r['secs'] for k, r in enumerate(gate) if k % 3 == 1 and k > 3]))
    print('shim calls: in use after call 2: %d B, after call %d: %d B, growth %d B; one live handle: %d B (%d B left after destroy); '
          'median simulator gateway call %.2f ms' % (mem2['in_use'], NCALLS, mem40['in_use'], growth, footprint, fp['left'], sim_ms))
    assert footprint > 0, 'a live handle holds device memory'
    assert growth < footprint, (growth, footprint)
