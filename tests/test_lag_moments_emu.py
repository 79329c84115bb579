"""Moments across two periods (egdst_simulate_batch_spec_lag) on the CPU harness (tests/cpu_emu), without a GPU: the estimation
step with lagged records in both regimes of the quantile kernel and over several slices of draws, loaded into python with no
sanitizer (this file preloads nothing); and the same code under AddressSanitizer / UBSan, leak check included, through a
stand-alone driver that links the sanitizer's runtime itself."""
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
    r = subprocess.run([sys.executable, os.path.join(EMU, 'run_emu_lag_moments.py')], env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'lag moment problems: 0' in r.stdout, r.stdout + r.stderr[-2000:]
    found = re.search(r'^lagged quantile regimes \(lds, global\): \((\d+), (\d+)\)  slices: (\d+)$', r.stdout, flags=re.M)
    assert found, r.stdout
    return tuple(int(x) for x in found.groups())


def test_lagged_quantiles_in_both_regimes_of_the_selection():
    """QNT_LDS_KEYS=64: a per-period quantile with a lagged condition (48 candidates) selects in LDS, a pooled one from global
    memory; 4 draws, 48 agents, both rndtype, means, counts and the objective with a full W bit-equal to the host mirror"""
    lds, glob, nslices = _run_emu('-DQNT_LDS_KEYS=64')
    assert lds > 0 and glob > 0 and nslices == 1


def test_lagged_moments_over_several_slices_of_draws():
    """a slice of two draws' paths makes the four draws take two slices (the runner derives the count from the flag and refuses
    a count below 2)"""
    import run_emu_lag_moments as rl
    from egdst_amd import moments as mo
    m = rl.occ3_case()
    nout = len(mo.columns(*mo._layout(m)))
    per_draw = 8 * nout * m.nt * rl.NSIM
    lds, glob, nslices = _run_emu('-DEG_SIM_SLICE_BYTES=%d' % (2 * per_draw))
    assert rl.NDRAW == 4 and rl.NSIM == 48 and nslices == 2 and lds > 0


def _sanitizer_runtime():
    for name in ('libasan.so', 'libubsan.so'):
        p = subprocess.run(['g++', '-print-file-name=' + name], capture_output=True, text=True).stdout.strip()
        if not (os.path.isabs(p) and os.path.exists(p)):
            return False
    return True


@pytest.mark.skipif(not _sanitizer_runtime(), reason='g++ has no AddressSanitizer / UBSan runtime')
def test_stand_alone_driver_under_asan_and_ubsan(tmp_path):
    """The harness library built with -fsanitize=address,undefined and a driver with its own main linked against it: one occ3
    draw, 40 agents, generated uniforms, records of every kind with and without lags, a lead, lag nt - 1 and an empty record.
    Exit status 0, no report, the printed bits are those computed here from the oracle's paths for the replayed uniforms, and
    each of the three refusals the lags add answers EGDST_E_ARG."""
    import build_emu
    import estimation_case
    import run_emu_lag_moments as rl
    from egdst_amd import build, codegen
    from egdst_amd import moments as mo
    from oracle_harness import Oracle
    m = rl.occ3_case()
    text = codegen.generate_modelspec(m)
    d = os.path.join(build.MODELS_DIR, build.model_tag(m, text))
    os.makedirs(d, exist_ok=True)
    spec_h = os.path.join(d, 'modelspec.h')
    if not os.path.exists(spec_h) or open(spec_h).read() != text:
        open(spec_h, 'w').write(text)
    lib = build_emu.build(d, 'address', 1, False, 1)
    exe = str(tmp_path / 'emu_lag_main')
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    '-fno-omit-frame-pointer', os.path.join(EMU, 'emu_lag_main.cpp'), lib, '-Wl,-rpath,' + os.path.dirname(lib),
                    '-pthread', '-o', exe], check=True)

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
    desc = m.descriptor()
    ngridmax = desc['ngridmax'] if desc['ngridmax'] > desc['ngridm'] else 2 * desc['ngridm']

    def num(a):
        return ' '.join('inf' if v == INF else '-inf' if v == -INF else '%.17g' % v for v in np.asarray(a, dtype=np.float64).ravel())
    par = m.param_vector()
    lines = ['%d %d %d %d %d %d %.17g %.17g %d' % (desc['t0'], desc['T'], desc['ngridm'], ngridmax, desc['nthrhmax'], desc['ny'],
                                                    desc['mmax'], desc['a0'], len(par)),
             num(desc['quadrature']), num(par), '%d %d' % (nsim, seed), num(init.T), '%d' % len(rec)]
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
    assert 'solve rc=0' in out and out.count('refused rc=1') == 3 and 'accepted rc=0' in out, r.stdout
    assert not [ln for ln in out if ln.startswith('refused') and ln != 'refused rc=1'], r.stdout

    orc = Oracle(m)
    sol = orc.solve(par)
    assert sol.rc == 0
    sims = orc.sim(sol, init, estimation_case.uniforms(seed, 4 * nt * nsim), rndtype=0, params=par)
    rm, rc = spec.evaluate(sims, block=1)
    want = ['moment %d %d %016x' % (j, rc[j], int(np.array([rm[j]]).view(np.uint64)[0])) for j in range(len(rec))]
    got = [ln for ln in out if ln.startswith('moment ')]
    nan_rows = [j for j in range(len(rec)) if rc[j] == 0]
    assert nan_rows == [len(rec) - 1]   # (nobody chooses 9)
    for j, (g, w) in enumerate(zip(got, want)):
        if j in nan_rows:   # a NaN's payload is not part of the contract
            assert g.split()[:3] == w.split()[:3] and math.isnan(np.array([int(g.split()[3], 16)], dtype=np.uint64).view(np.float64)[0])
        else:
            assert g == w, (j, g, w)
    assert len(got) == len(want)
