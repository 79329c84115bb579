"""k_quantiles on the CPU harness (tests/cpu_emu), without a GPU: the estimation step with quantile moments in both regimes of
the kernel and over several slices of draws, loaded into python with no sanitizer (this file preloads nothing); and the same
code under AddressSanitizer / UBSan, leak check included, through a stand-alone driver that links the sanitizer's runtime
itself."""
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


def _run_emu(flags):
    env = dict(os.environ, EMU_SANITIZE='0', EMU_EXTRA_FLAGS=flags)
    r = subprocess.run([sys.executable, os.path.join(EMU, 'run_emu_quantiles.py')], env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'quantile problems: 0' in r.stdout, r.stdout + r.stderr[-2000:]
    found = re.search(r'^quantile regimes \(lds, global\): \((\d+), (\d+)\)  slices: (\d+)$', r.stdout, flags=re.M)
    assert found, r.stdout
    return tuple(int(x) for x in found.groups())


def test_both_regimes_of_the_selection():
    """QNT_LDS_KEYS=64: the 48 agents of one period are selected in LDS, pooled periods from global memory"""
    lds, glob, nslices = _run_emu('-DQNT_LDS_KEYS=64')
    assert lds > 0 and glob > 0 and nslices == 1


def test_quantiles_over_several_slices_of_draws():
    """the paths of one draw are 8 bytes * nout columns * 7 periods (t0 = 0 .. T = 6) * 48 agents; a slice of two of them
    makes the four draws take two slices (the runner derives the count from the flag and refuses a count below 2)"""
    import run_emu_quantiles as rq
    m = rq.occ3_case()
    from egdst_amd import moments as mo
    nout = len(mo.columns(*mo._layout(m)))
    per_draw = 8 * nout * m.nt * rq.NSIM
    lds, glob, nslices = _run_emu('-DEG_SIM_SLICE_BYTES=%d' % (2 * per_draw))
    assert rq.NDRAW == 4 and nslices == 2 and lds > 0


def _sanitizer_runtime():
    for name in ('libasan.so', 'libubsan.so'):
        p = subprocess.run(['g++', '-print-file-name=' + name], capture_output=True, text=True).stdout.strip()
        if not (os.path.isabs(p) and os.path.exists(p)):
            return False
    return True


def _keys(x):
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))


@pytest.mark.skipif(not _sanitizer_runtime(), reason='g++ has no AddressSanitizer / UBSan runtime')
def test_stand_alone_driver_under_asan_and_ubsan(tmp_path):
    """The harness library built with -fsanitize=address,undefined and a driver with its own main linked against it: one occ3
    draw, the estimation step with generated uniforms on a handful of quantile records, egdst_quantile_eval on a small
    array.  Exit status 0, no report, and the printed bits are those computed here from the oracle's paths for the
    replayed uniforms."""
    import build_emu
    import estimation_case
    import run_emu_quantiles as rq
    from egdst_amd import build, codegen
    from egdst_amd import moments as mo
    from oracle_harness import Oracle
    m = rq.occ3_case()
    text = codegen.generate_modelspec(m)
    d = os.path.join(build.MODELS_DIR, build.model_tag(m, text))
    os.makedirs(d, exist_ok=True)
    spec_h = os.path.join(d, 'modelspec.h')
    if not os.path.exists(spec_h) or open(spec_h).read() != text:
        open(spec_h, 'w').write(text)
    lib = build_emu.build(d, 'address', 1, False, 1)
    exe = str(tmp_path / 'emu_quantile_main')
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    '-fno-omit-frame-pointer', os.path.join(EMU, 'emu_quantile_main.cpp'), lib, '-Wl,-rpath,' + os.path.dirname(lib),
                    '-pthread', '-o', exe], check=True)

    nsim, seed = 40, 2024
    rng = np.random.default_rng(6)
    init = np.column_stack([np.ones(nsim), rng.uniform(m.a0, m.mmax, nsim)])
    spec = mo.MomentSpec([mo.median('C', periods=1), mo.quantile('M', 0.25, periods=3), mo.quantile('A', 0.9), mo.median('id'),
                          mo.mean('C'), mo.quantile('C', 1 / 3, where=('id', 1, 2)), mo.median('V', where=('id', 9, 9))], layout=m)
    rec = spec.pack(m.nt, m)
    assert rec['kind'][0] == 3
    x = rng.normal(size=301)
    x[::7] = np.nan
    x[5], x[6], x[8] = -0.0, 0.0, -np.inf
    p = np.array([0.01, 0.5, 1 / 3, 0.99, np.nextafter(1, 0)])
    desc = m.descriptor()
    ngridmax = desc['ngridmax'] if desc['ngridmax'] > desc['ngridm'] else 2 * desc['ngridm']
    num = lambda a: ' '.join('%.17g' % v for v in np.asarray(a, dtype=np.float64).ravel())   # noqa: E731
    par = m.param_vector()
    lines = ['%d %d %d %d %d %d %.17g %.17g %d' % (desc['t0'], desc['T'], desc['ngridm'], ngridmax, desc['nthrhmax'], desc['ny'],
                                                    desc['mmax'], desc['a0'], len(par)),
             num(desc['quadrature']), num(par), '%d %d' % (nsim, seed), num(init.T), '%d' % len(rec)]
    lines += ['%d %d %d %d %d %d %s' % (tuple(int(r[k]) for k in mo.MOMENT_DTYPE.names[:6]) + (num([r[k] for k in mo.MOMENT_DTYPE.names[6:]]),))
              for r in rec]
    lines += ['%d' % len(x), num(x), '%d' % len(p), num(p)]
    case = tmp_path / 'case.txt'
    case.write_text('\n'.join(lines) + '\n')
    r = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=900)   # (leak detection stays on)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert 'ERROR: AddressSanitizer' not in r.stderr and 'ERROR: LeakSanitizer' not in r.stderr and 'runtime error' not in r.stderr, \
        r.stderr[-3000:]
    out = r.stdout.splitlines()
    assert 'solve rc=0' in out and 'refused rc=1' in out, r.stdout

    orc = Oracle(m)
    sol = orc.solve(par)
    assert sol.rc == 0
    sims = orc.sim(sol, init, estimation_case.uniforms(seed, 4 * m.nt * nsim), rndtype=0, params=par)
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
    assert len(got) == len(want) and (rc[:4] > 0).all()
    v = x[~np.isnan(x)]
    ks = np.sort(_keys(v))
    for i, pi in enumerate(p):
        key = ks[min(max(math.ceil(pi * float(len(v))), 1), len(v)) - 1]
        u = int(key) & ((1 << 63) - 1) if int(key) >> 63 else ~int(key) & ((1 << 64) - 1)
        assert 'eval %d %d %016x' % (i, len(v), u) in out, (i, r.stdout)
