"""Quantile records in the covariance of the moments (egdst_simulate_batch_spec_cov with banded kind-3 records) on the CPU
harness (tests/cpu_emu), without a GPU: the step with k_quantile_band in both regimes of the selection and over several slices
of draws, loaded into python with no sanitizer (this file preloads nothing); and the same code under AddressSanitizer / UBSan,
leak check included, through the stand-alone driver of the estimation step, which links the sanitizer's runtime itself."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'cpu_emu'))
import estimation_emu as emu
INF = float('inf')


def _run_emu(flags):
    out = emu.run_runner('run_emu_quantile_cov.py', flags, 'quantile covariance problems: 0')
    found = re.search(r'^quantile regimes \(lds, global\): \((\d+), (\d+)\)  slices: (\d+)$', out, flags=re.M)
    assert found, out
    return tuple(int(x) for x in found.groups())


def test_banded_quantiles_on_the_harness_against_the_mirror():
    """occ3, 4 draws, 48 agents, both rndtype, as built (every record's keys fit LDS): Omega bit-equal to MomentSpec.covariance
    on the oracle's paths, NaN exactly where the mirror's scores are, means and counts those of the step without the
    covariance, with and without the bandwidth in the records"""
    lds, glob, nslices = _run_emu('')
    assert lds > 0 and glob == 0 and nslices == 1


def test_both_regimes_of_the_selection():
    """QNT_LDS_KEYS=64: the 48 agents of a per-period record are selected in LDS, the pooled records from global memory"""
    lds, glob, nslices = _run_emu('-DQNT_LDS_KEYS=64')
    assert lds > 0 and glob > 0 and nslices == 1


def test_banded_quantiles_over_several_slices_of_draws():
    """a slice that holds the paths of two draws but, once the padded scores count beside them, of one: four slices"""
    import run_emu_quantile_cov as rq
    from egdst_amd import moments as mo
    m = emu.occ3_case()
    nout = len(mo.columns(*mo._layout(m)))
    paths = 8 * nout * m.nt * emu.NSIM
    nmom = len(rq.quantile_cov_spec(m.nt, m))
    scores = 8 * emu.NSIM * (-(-nmom // emu.cov_tile()) * emu.cov_tile())
    assert 0 < scores and paths + scores <= 2 * paths < 2 * (paths + scores)
    lds, glob, nslices = _run_emu('-DEG_SIM_SLICE_BYTES=%d' % (2 * paths))
    assert nslices == 4 and lds > 0


@pytest.mark.skipif(not emu.sanitizer_runtime(), reason='g++ has no AddressSanitizer / UBSan runtime')
def test_stand_alone_driver_under_asan_and_ubsan(tmp_path):
    """The harness library built with -fsanitize=address,undefined and the driver with its own main, mode cov: one occ3 draw, 40
    agents, generated uniforms, records of kinds 0-2 and banded quantiles (per period, pooled, conditional with a lag, on the
    tied column, an empty one).  Exit status 0, no report, the printed bits of the moments and of Omega are those computed here
    from the oracle's paths, and the two refusals answer as before: a quantile without a bandwidth and a null cov_dev."""
    import estimation_case
    from egdst_amd import moments as mo
    m = emu.occ3_case()
    exe = emu.build_driver(m, tmp_path)

    nsim, seed = 40, 2026
    nt = m.nt
    rng = np.random.default_rng(6)
    init = np.column_stack([np.ones(nsim), rng.uniform(m.a0, m.mmax, nsim)])
    spec = mo.MomentSpec([mo.mean('C'), mo.median('M', periods=2, bandwidth=0.2), mo.cross('C', 'C', lag=1),
                          mo.quantile('C', 0.25, bandwidth=0.1), mo.share('id', 1, periods=2),
                          mo.quantile('M', 0.75, periods=(1, nt - 1), where=('id', 0, 1, 1), bandwidth=0.2),
                          mo.median('id', bandwidth=0.05), mo.transition('id', 0, 1),
                          mo.median('V', where=('id', 9, 9), bandwidth=0.25), mo.mean('M', periods=3)], layout=m)
    rec = spec.pack_lag(nt, m)
    nmom = len(rec)
    assert (rec['kind'] == 3).sum() == 5 and (rec['hi'][rec['kind'] == 3] > 0).all()
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
    assert [j for j in range(nmom) if rcnt[j] == 0] == [8]   # (nobody chooses 9)

    emu.assert_moments(out, rm, rcnt)   # (every line, bit for bit; a NaN's payload is not part of the contract)
    got_v = emu.printed(out, 'cov')
    assert len(got_v) == nmom * nmom
    for g in got_v:
        j, k = int(g[0]), int(g[1])
        assert emu.same_bits(g[2], rv[j, k]), (j, k, g[2], emu.hexbits(rv[j, k]))
    nan = np.isnan(np.diag(rv))
    assert list(np.nonzero(nan)[0]) == [8] and np.isfinite(rv[np.ix_(~nan, ~nan)]).all()
    assert (np.diag(rv)[[1, 3, 5]] > 0).all()   # (the quantile rows carry a variance)
