"""Moments across two periods (egdst_simulate_batch_spec_lag) on the CPU harness (tests/cpu_emu), without a GPU: the estimation
step with lagged records in both regimes of the quantile kernel and over several slices of draws, loaded into python with no
sanitizer (this file preloads nothing); and the same code under AddressSanitizer / UBSan, leak check included, through a
stand-alone driver that links the sanitizer's runtime itself."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'cpu_emu'))
import estimation_emu as emu
INF = float('inf')


def _run_emu(flags):
    out = emu.run_runner('run_emu_lag_moments.py', flags, 'lag moment problems: 0')
    found = re.search(r'^lagged quantile regimes \(lds, global\): \((\d+), (\d+)\)  slices: (\d+)$', out, flags=re.M)
    assert found, out
    return tuple(int(x) for x in found.groups())


def test_lagged_quantiles_in_both_regimes_of_the_selection():
    """QNT_LDS_KEYS=64: a per-period quantile with a lagged condition (48 candidates) selects in LDS, a pooled one from global
    memory; 4 draws, 48 agents, both rndtype, means, counts and the objective with a full W bit-equal to the host mirror"""
    lds, glob, nslices = _run_emu('-DQNT_LDS_KEYS=64')
    assert lds > 0 and glob > 0 and nslices == 1


def test_lagged_moments_over_several_slices_of_draws():
    """a slice of two draws' paths makes the four draws take two slices (the runner derives the count from the flag and refuses
    a count below 2)"""
    from egdst_amd import moments as mo
    m = emu.occ3_case()
    nout = len(mo.columns(*mo._layout(m)))
    per_draw = 8 * nout * m.nt * emu.NSIM
    lds, glob, nslices = _run_emu('-DEG_SIM_SLICE_BYTES=%d' % (2 * per_draw))
    assert emu.NDRAW == 4 and emu.NSIM == 48 and nslices == 2 and lds > 0


@pytest.mark.skipif(not emu.sanitizer_runtime(), reason='g++ has no AddressSanitizer / UBSan runtime')
def test_stand_alone_driver_under_asan_and_ubsan(tmp_path):
    """The harness library built with -fsanitize=address,undefined and a driver with its own main linked against it: one occ3
    draw, 40 agents, generated uniforms, records of every kind with and without lags, a lead, lag nt - 1 and an empty record.
    Exit status 0, no report, the printed bits are those computed here from the oracle's paths for the replayed uniforms, and
    each of the three refusals the lags add answers EGDST_E_ARG."""
    import estimation_case
    from egdst_amd import moments as mo
    m = emu.occ3_case()
    exe = emu.build_driver(m, tmp_path)

    nsim, seed = 40, 2025
    nt = m.nt
    rng = np.random.default_rng(6)
    init = np.column_stack([np.ones(nsim), rng.uniform(m.a0, m.mmax, nsim)])
    spec = mo.MomentSpec([mo.mean('C'), mo.mean('C', where=('id', 0, 1, 1)), mo.cross('M', 'C'), mo.cross('C', 'C', lag=1),
                          mo.share('id', 1, periods=2), mo.transition('id', 0, 1), mo.median('M', periods=3),
                          mo.median('M', periods=3, where=('id', 0, 2, 1)), mo.quantile('C', 0.9, where=('id', 0, 2, 2)),
                          mo.cross('C', 'M', periods=(2, 4), lag=-1), mo.mean('C', periods=(0, nt - 2), where=('C', -INF, INF, -1)),   # leads
                          mo.cross('M', 'M', periods=nt - 1, lag=nt - 1), mo.share('id', 0, periods=0, where=('M', -INF, INF, -(nt - 1))),
                          mo.mean('C', where=('id', 9, 9, 1))], layout=m)
    rec = spec.pack_lag(nt, m)
    for kind in range(4):   # every kind with and without lags
        lagged = (rec['lag2'] != 0) | (rec['cond_lag'] != 0)
        assert ((rec['kind'] == kind) & lagged).any() and ((rec['kind'] == kind) & ~lagged).any(), kind
    assert (rec['lag2'] == nt - 1).any() and (rec['cond_lag'] == -(nt - 1)).any() and (rec['lag2'] < 0).any()
    par = m.param_vector()
    emu.write_case(tmp_path / 'case.txt', m, nsim, seed, init, rec)
    out = emu.run_driver(exe, 'lag', tmp_path / 'case.txt')
    assert 'solve rc=0' in out and out.count('refused rc=1') == 3 and 'accepted rc=0' in out, out
    assert not [ln for ln in out if ln.startswith('refused') and ln != 'refused rc=1'], out

    orc = emu.Oracle(m)
    sol = orc.solve(par)
    assert sol.rc == 0
    sims = orc.sim(sol, init, estimation_case.uniforms(seed, 4 * nt * nsim), rndtype=0, params=par)
    rm, rc = spec.evaluate(sims, block=1)
    nan_rows = [j for j in range(len(rec)) if rc[j] == 0]
    assert nan_rows == [len(rec) - 1]   # (nobody chooses 9)
    emu.assert_moments(out, rm, rc)   # (every line, bit for bit; a NaN's payload is not part of the contract)
