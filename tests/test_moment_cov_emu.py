"""The covariance of the moments (egdst_simulate_batch_spec_cov) on the CPU harness (tests/cpu_emu), without a GPU: the step with
its two kernels over one and over several slices of draws, loaded into python with no sanitizer (this file preloads nothing);
and the same code under AddressSanitizer / UBSan, leak check included, through a stand-alone driver that links the sanitizer's
runtime itself."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'cpu_emu'))
import estimation_emu as emu
INF = float('inf')


def _run_emu(flags):
    out = emu.run_runner('run_emu_moment_cov.py', flags, 'moment covariance problems: 0')
    found = re.search(r'^slices: (\d+)$', out, flags=re.M)
    assert found, out
    return int(found.group(1))


def test_covariance_on_the_harness_against_the_mirror():
    """occ3, 4 draws, 48 agents, both rndtype: Omega bit-equal to MomentSpec.covariance with the build's egdst_cov_parts() on the
    oracle's paths, NaN exactly on the empty record, mirror entries equal in bits, means and counts those of the step without
    the covariance"""
    assert _run_emu('') == 1


def test_covariance_over_several_slices_of_draws():
    """a slice that holds the paths of two draws but, once the padded scores count beside them, of one: the four draws take
    four slices (the runner derives the count from the flag and refuses a count below 2)"""
    import run_emu_moment_cov as rc
    from egdst_amd import moments as mo
    m = emu.occ3_case()
    nout = len(mo.columns(*mo._layout(m)))
    paths = 8 * nout * m.nt * emu.NSIM
    nmom = len(rc.cov_spec(m.nt, m))
    scores = 8 * emu.NSIM * (-(-nmom // emu.cov_tile()) * emu.cov_tile())
    assert 0 < scores and paths + scores <= 2 * paths < 2 * (paths + scores)
    assert _run_emu('-DEG_SIM_SLICE_BYTES=%d' % (2 * paths)) == 4


@pytest.mark.skipif(not emu.sanitizer_runtime(), reason='g++ has no AddressSanitizer / UBSan runtime')
def test_stand_alone_driver_under_asan_and_ubsan(tmp_path):
    """The harness library built with -fsanitize=address,undefined and a driver with its own main linked against it: one occ3
    draw, 40 agents, generated uniforms, records of every kind 0-2 with and without lags, an empty record, 13 records (below
    the tile's 32).  Exit status 0, no report, the printed bits of the moments and of Omega are those computed here from the
    oracle's paths for the replayed uniforms, and the two refusals the entry adds answer EGDST_E_ARG."""
    import estimation_case
    from egdst_amd import moments as mo
    m = emu.occ3_case()
    exe = emu.build_driver(m, tmp_path)

    nsim, seed = 40, 2025
    nt = m.nt
    rng = np.random.default_rng(6)
    init = np.column_stack([np.ones(nsim), rng.uniform(m.a0, m.mmax, nsim)])
    spec = mo.MomentSpec([mo.mean('C'), mo.mean('C', where=('id', 0, 1, 1)), mo.cross('M', 'C'), mo.cross('C', 'C', lag=1),
                          mo.share('id', 1, periods=2), mo.transition('id', 0, 1), mo.share('id', 0, periods=2),
                          mo.cross('C', 'M', periods=(2, 4), lag=-1), mo.mean('C', periods=(0, nt - 2), where=('C', -INF, INF, -1)),
                          mo.cross('M', 'M', periods=nt - 1, lag=nt - 1), mo.share('id', 0, periods=0, where=('M', -INF, INF, -(nt - 1))),
                          mo.mean('M', periods=3), mo.mean('C', where=('id', 9, 9, 1))], layout=m)
    rec = spec.pack_lag(nt, m)
    nmom = len(rec)
    assert nmom < emu.cov_tile()
    for kind in range(3):   # every kind with and without lags
        lagged = (rec['lag2'] != 0) | (rec['cond_lag'] != 0)
        assert ((rec['kind'] == kind) & lagged).any() and ((rec['kind'] == kind) & ~lagged).any(), kind
    par = m.param_vector()
    emu.write_case(tmp_path / 'case.txt', m, nsim, seed, init, rec)
    out = emu.run_driver(exe, 'cov', tmp_path / 'case.txt')
    assert 'solve rc=0' in out and 'same 1' in out, out[-40:]
    refused = [ln for ln in out if ln.startswith('refused')]
    assert len(refused) == 2 and all(ln.startswith('refused rc=1 egdst_simulate_batch_spec_cov') for ln in refused), refused
    assert 'moment %d:' % (nmom - 1) in refused[0] and 'quantile' in refused[0] and 'cov_dev' in refused[1]
    parts = int([ln for ln in out if ln.startswith('parts ')][0].split()[1])

    orc = emu.Oracle(m)
    sol = orc.solve(par)
    assert sol.rc == 0
    sims = orc.sim(sol, init, estimation_case.uniforms(seed, 4 * nt * nsim), rndtype=0, params=par)
    rm, rcnt, rv = spec.covariance(sims, block=1, parts=parts)
    assert [j for j in range(nmom) if rcnt[j] == 0] == [nmom - 1]   # (nobody chooses 9)

    emu.assert_moments(out, rm, rcnt)   # (every line, bit for bit; a NaN's payload is not part of the contract)
    got_v = emu.printed(out, 'cov')
    assert len(got_v) == nmom * nmom
    for g in got_v:
        j, k = int(g[0]), int(g[1])
        assert emu.same_bits(g[2], rv[j, k]), (j, k, g[2], emu.hexbits(rv[j, k]))
    assert np.isfinite(rv[:nmom - 1, :nmom - 1]).all() and (np.diag(rv)[:nmom - 1] > 0).all()
