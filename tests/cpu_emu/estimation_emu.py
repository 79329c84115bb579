"""What the CPU-harness runners and tests of the estimation step share (run_emu_quantiles / _lag_moments / _moment_cov and
test_quantile_emu / test_lag_moments_emu / test_moment_cov_emu): the harness build of a model, the occ3 case with its solved
batch of draws and the oracle's panels, and the stand-alone driver emu_estimation_main.cpp under AddressSanitizer / UBSan.
Nothing here preloads anything: the driver links the sanitizer's runtime itself."""
import math
import os
import re
import subprocess
import sys
import types
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, 'tests'), HERE) if p not in sys.path]
import numpy as np
import build_emu
from egdst_amd import build, codegen, examples, runtime
from egdst_amd import moments as mo
from oracle_harness import Oracle
import estimation_case

NSIM, NDRAW = 48, 4


# ---- build

def write_modelspec(m):
    """the model's directory under egdst_amd/_models with its modelspec.h (left alone when it is already that text, so that
    build_emu.build, which compares mtimes, keeps the library it has)"""
    text = codegen.generate_modelspec(m)
    d = os.path.join(build.MODELS_DIR, build.model_tag(m, text))
    os.makedirs(d, exist_ok=True)
    spec_h = os.path.join(d, 'modelspec.h')
    if not os.path.exists(spec_h) or open(spec_h).read() != text:
        open(spec_h, 'w').write(text)
    return d


# ---- case

def occ3_case():
    return examples.occ3(T=6, ngridm=30, ngridmax=100)


def flag(name, default):
    m = re.search(r'-D%s=(\d+)' % name, os.environ.get('EMU_EXTRA_FLAGS', ''))
    return int(m.group(1)) if m else default


def full_w(n, seed=11):
    a = np.random.default_rng(seed).normal(size=(n, n))
    return (a @ a.T) / n


def cov_tile():
    """COV_T, the records per side of k_moment_cov's tile: the scores of a draw are padded to a multiple of it"""
    text = open(os.path.join(ROOT, 'egdst_amd', 'csrc', 'egdst_kernels.hip')).read()
    return int(re.search(r'^#define COV_T (\d+)', text, flags=re.M).group(1))


def solved_batch():
    """occ3 on the harness build EMU_SANITIZE asks for ('0': none), NDRAW perturbed parameter rows solved, NSIM agents: m, lib, s
    (the Solver), P, init, st (the draws' status), orc (the oracle) and rng, which the runner goes on drawing from"""
    san = os.environ.get('EMU_SANITIZE', '0')
    m = occ3_case()
    lib = runtime.ModelLibrary(build_emu.build(write_modelspec(m), {'0': False}.get(san, san), 1, False, 1))
    rng = np.random.default_rng(4)
    P = m.param_vector()[None] * (1 + 0.15 * rng.uniform(-1, 1, (NDRAW, len(m.param_vector()))))
    s = runtime.Solver(lib, m.descriptor(), ndraw=NDRAW, keep_history=True)
    s.set_params(P)
    s.solve(raise_on_error=False)
    init = np.column_stack([np.ones(NSIM), rng.uniform(m.a0, m.mmax, NSIM)])
    return types.SimpleNamespace(m=m, lib=lib, s=s, P=P, init=init, st=s.status()[0], orc=Oracle(m), rng=rng)


def slices(b, bad, scores=0):
    """the slices of draws estimation_step takes, from the arithmetic of the library: a draw's paths and, with the covariance, its
    `scores` records padded to the tile; a build with EG_SIM_SLICE_BYTES that leaves one slice goes into bad"""
    per_draw = 8 * b.lib.nout * b.s.nt * NSIM + (8 * NSIM * (-(-scores // cov_tile()) * cov_tile()) if scores else 0)
    slice_ = max(1, min(NDRAW, flag('EG_SIM_SLICE_BYTES', 2 << 30) // per_draw))
    nslices = -(-NDRAW // slice_)
    if 'EG_SIM_SLICE_BYTES' in os.environ.get('EMU_EXTRA_FLAGS', '') and nslices < 2:
        bad.append('EG_SIM_SLICE_BYTES is set but the %d draws take %d slice' % (NDRAW, nslices))
    return nslices


def oracle_panels(b, seed, rndtype):
    """(draw, panel) for every draw of the batch: the oracle's paths [NSIM, nt, nout] for the host replay of the uniforms of
    `seed`, or None where the oracle fails"""
    rs = estimation_case.uniforms(seed, 4 * b.s.nt * (1 if rndtype == 1 else NSIM))
    for dr in range(NDRAW):
        sol = b.orc.solve(b.P[dr])
        yield dr, b.orc.sim(sol, b.init, rs, rndtype=rndtype, params=b.P[dr]) if sol.rc == 0 else None


def run_runner(script, flags, passed):
    """stdout of a runner beside this file on the plain harness build with EMU_EXTRA_FLAGS = flags, which must hold `passed`"""
    env = dict(os.environ, EMU_SANITIZE='0', EMU_EXTRA_FLAGS=flags)
    r = subprocess.run([sys.executable, os.path.join(HERE, script)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert passed in r.stdout, r.stdout + r.stderr[-2000:]
    return r.stdout


# ---- the stand-alone driver

def sanitizer_runtime():
    for name in ('libasan.so', 'libubsan.so'):
        p = subprocess.run(['g++', '-print-file-name=' + name], capture_output=True, text=True).stdout.strip()
        if not (os.path.isabs(p) and os.path.exists(p)):
            return False
    return True


def build_driver(m, tmp_path):
    """emu_estimation_main, with its own main, linked against the ASan / UBSan harness library of m, with the same sanitizers"""
    lib = build_emu.build(write_modelspec(m), 'address', 1, False, 1)
    exe = str(tmp_path / 'emu_estimation_main')
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    '-fno-omit-frame-pointer', os.path.join(HERE, 'emu_estimation_main.cpp'), lib, '-Wl,-rpath,' + os.path.dirname(lib),
                    '-pthread', '-o', exe], check=True)
    return exe


def write_case(path, m, nsim, seed, init, rec, quantile=None):
    """the case file of emu_case.h: the model, the agents, the records (either dtype; written in the 12-field lag form) and,
    with quantile = (x, p), the section egdst_quantile_eval reads"""
    desc = m.descriptor()
    ngridmax = desc['ngridmax'] if desc['ngridmax'] > desc['ngridm'] else 2 * desc['ngridm']
    num = lambda a: ' '.join('%.17g' % v for v in np.asarray(a, dtype=np.float64).ravel())   # noqa: E731  (inf, -inf, nan: as scanf reads them)
    par = m.param_vector()
    lines = ['%d %d %d %d %d %d %.17g %.17g %d' % (desc['t0'], desc['T'], desc['ngridm'], ngridmax, desc['nthrhmax'], desc['ny'],
                                                    desc['mmax'], desc['a0'], len(par)),
             num(desc['quadrature']), num(par), '%d %d' % (nsim, seed), num(init.T), '%d' % len(rec)]
    names = mo.MOMENT_LAG_DTYPE.names
    lines += ['%d %d %d %d %d %d %s %d %d' % (tuple(int(r[k]) for k in names[:6]) + (num([r[k] for k in names[6:10]]),)
                                              + tuple(int(r[k]) for k in names[10:])) for r in mo.convert_records(rec, mo.MOMENT_LAG_DTYPE)]
    if quantile is not None:
        x, p = quantile
        lines += ['%d' % len(x), num(x), '%d' % len(p), num(p)]
    path.write_text('\n'.join(lines) + '\n')


def run_driver(exe, mode, case):
    """the lines the driver prints: it must end with status 0 and without a report of a sanitizer"""
    r = subprocess.run([exe, mode, str(case)], capture_output=True, text=True, timeout=900)   # (leak detection stays on)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert 'ERROR: AddressSanitizer' not in r.stderr and 'ERROR: LeakSanitizer' not in r.stderr and 'runtime error' not in r.stderr, \
        r.stderr[-3000:]
    return r.stdout.splitlines()


def printed(out, word):
    """the fields after `word` of the lines that begin with it: ('moment', j, count, bits), ('cov', j, k, bits), ('eval', i, count, bits)"""
    return [ln.split()[1:] for ln in out if ln.startswith(word + ' ')]


def hexbits(x):
    return '%016x' % int(np.array([x], dtype=np.float64).view(np.uint64)[0])


def same_bits(got, want):
    """do the printed bits `got` (hex) hold the float `want`?  A NaN's payload is not part of the contract"""
    g = np.array([int(got, 16)], dtype=np.uint64).view(np.float64)[0]
    return math.isnan(g) if math.isnan(want) else got == hexbits(want)


def assert_moments(out, means, counts):
    """the driver's `moment` lines are these means and counts, bit for bit"""
    got = printed(out, 'moment')
    assert len(got) == len(means)
    for j, g in enumerate(got):
        assert g[:2] == [str(j), str(counts[j])] and same_bits(g[2], means[j]), (j, g, hexbits(means[j]))
