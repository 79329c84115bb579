"""The covariance of the moments (egdst_simulate_batch_spec_cov) on the CPU harness (tests/cpu_emu), without a GPU: the step with
its two kernels over one and over several slices of draws, loaded into python with no sanitizer (this file preloads nothing);
and the same code under AddressSanitizer / UBSan, leak check included, through a stand-alone driver that links the sanitizer's
runtime itself."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU = os.path.join(HERE, 'cpu_emu')
sys.path.insert(0, EMU)
INF = float('inf')


def _run_emu(flags):
    env = dict(os.environ, EMU_SANITIZE='0', EMU_EXTRA_FLAGS=flags)
    r = subprocess.run([sys.executable, os.path.join(EMU, 'run_emu_moment_cov.py')], env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'moment covariance problems: 0' in r.stdout, r.stdout + r.stderr[-2000:]
    found = re.search(r'^slices: (\d+)$', r.stdout, flags=re.M)
    assert found, r.stdout
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
    m = rc.occ3_case()
    nout = len(mo.columns(*mo._layout(m)))
    paths = 8 * nout * m.nt * rc.NSIM
    nmom = len(rc.cov_spec(m.nt, m))
    scores = 8 * rc.NSIM * (-(-nmom // rc.cov_tile()) * rc.cov_tile())
    assert 0 < scores and paths + scores <= 2 * paths < 2 * (paths + scores)
    assert _run_emu('-DEG_SIM_SLICE_BYTES=%d' % (2 * paths)) == 4


def _sanitizer_runtime():
    for name in ('libasan.so', 'libubsan.so'):
        p = subprocess.run(['g++', '-print-file-name=' + name], capture_output=True, text=True).stdout.strip()
        if not (os.path.isabs(p) and os.path.exists(p)):
            return False
    return True


@pytest.mark.skipif(not _sanitizer_runtime(), reason='g++ has no AddressSanitizer / UBSan runtime')
def test_stand_alone_driver_under_asan_and_ubsan(tmp_path):
    """The harness library built with -fsanitize=address,undefined and a driver with its own main linked against it: one occ3
    draw, 40 agents, generated uniforms, records of every kind 0-2 with and without lags, an empty record, 13 records (below
    the tile's 32).  Exit status 0, no report, the printed bits of the moments and of Omega are those computed here from the
    oracle's paths for the replayed uniforms, and the two refusals the entry adds answer EGDST_E_ARG."""
    import build_emu
    import estimation_case
    import run_emu_moment_cov as rc
    from egdst_amd import moments as mo
    from oracle_harness import Oracle
    m = rc.occ3_case()
    lib = build_emu.build(rc.write_modelspec(m), 'address', 1, False, 1)
    exe = str(tmp_path / 'emu_cov_main')
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    '-fno-omit-frame-pointer', os.path.join(EMU, 'emu_cov_main.cpp'), lib, '-Wl,-rpath,' + os.path.dirname(lib),
                    '-pthread', '-o', exe], check=True)

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
    assert nmom < rc.cov_tile()
    for kind in range(3):   # every kind with and without lags
        lagged = (rec['lag2'] != 0) | (rec['cond_lag'] != 0)
        assert ((rec['kind'] == kind) & lagged).any() and ((rec['kind'] == kind) & ~lagged).any(), kind
    desc = m.descriptor()
    ngridmax = desc['ngridmax'] if desc['ngridmax'] > desc['ngridm'] else 2 * desc['ngridm']

    def num(a):
        return ' '.join('inf' if v == INF else '-inf' if v == -INF else '%.17g' % v for v in np.asarray(a, dtype=np.float64).ravel())
    par = m.param_vector()
    lines = ['%d %d %d %d %d %d %.17g %.17g %d' % (desc['t0'], desc['T'], desc['ngridm'], ngridmax, desc['nthrhmax'], desc['ny'],
                                                    desc['mmax'], desc['a0'], len(par)),
             num(desc['quadrature']), num(par), '%d %d' % (nsim, seed), num(init.T), '%d' % nmom]
    names = mo.MOMENT_LAG_DTYPE.names
    lines += ['%d %d %d %d %d %d %s %d %d' % (tuple(int(r[k]) for k in names[:6]) + (num([r[k] for k in names[6:10]]),)
                                              + tuple(int(r[k]) for k in names[10:])) for r in rec]
    case = tmp_path / 'case.txt'
    case.write_text('\n'.join(lines) + '\n')
    r = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=900)   # (leak detection stays on)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert 'ERROR: AddressSanitizer' not in r.stderr and 'ERROR: LeakSanitizer' not in r.stderr and 'runtime error' not in r.stderr, \
        r.stderr[-3000:]
    out = r.stdout.splitlines()
    assert 'solve rc=0' in out and 'same 1' in out, r.stdout[-2000:]
    refused = [ln for ln in out if ln.startswith('refused')]
    assert len(refused) == 2 and all(ln.startswith('refused rc=1 egdst_simulate_batch_spec_cov') for ln in refused), refused
    assert 'moment %d:' % (nmom - 1) in refused[0] and 'quantile' in refused[0] and 'cov_dev' in refused[1]
    parts = int([ln for ln in out if ln.startswith('parts ')][0].split()[1])

    orc = Oracle(m)
    sol = orc.solve(par)
    assert sol.rc == 0
    sims = orc.sim(sol, init, estimation_case.uniforms(seed, 4 * nt * nsim), rndtype=0, params=par)
    rm, rcnt, rv = spec.covariance(sims, block=1, parts=parts)
    assert [j for j in range(nmom) if rcnt[j] == 0] == [nmom - 1]   # (nobody chooses 9)

    def hexbits(x):
        return '%016x' % int(np.array([x], dtype=np.float64).view(np.uint64)[0])

    def same(got, want):   # a NaN's payload is not part of the contract
        g = np.array([int(got, 16)], dtype=np.uint64).view(np.float64)[0]
        return math.isnan(g) if math.isnan(want) else got == hexbits(want)
    got_m = [ln.split() for ln in out if ln.startswith('moment ')]
    assert len(got_m) == nmom
    for j, g in enumerate(got_m):
        assert g[1:3] == [str(j), str(rcnt[j])] and same(g[3], rm[j]), (j, g)
    got_v = [ln.split() for ln in out if ln.startswith('cov ')]
    assert len(got_v) == nmom * nmom
    for g in got_v:
        j, k = int(g[1]), int(g[2])
        assert same(g[3], rv[j, k]), (j, k, g[3], hexbits(rv[j, k]))
    assert np.isfinite(rv[:nmom - 1, :nmom - 1]).all() and (np.diag(rv)[:nmom - 1] > 0).all()
