"""The policy at a data panel's observations (egdst_policy_batch) on the CPU harness (tests/cpu_emu), without a GPU: every draw
against the mirror, several slices of draws, a solution imported with a missing cell and every refusal, loaded into
python with no sanitizer (this file preloads nothing); and the same code under AddressSanitizer / UBSan, leak check included,
through a stand-alone driver that links the sanitizer's runtime itself."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'cpu_emu'))
import estimation_emu as emu
import build_emu
from egdst_amd import datafit

NOBS = 349   # what the runner's case comes to: 336 present pairs of the 48 agents' panel and 13 points off it


def _run_emu(flags):
    out = emu.run_runner('run_emu_policy.py', flags, 'policy problems: 0')
    found = re.search(r'^policy cells: (\d+)  slices: (\d+)$', out, flags=re.M)
    nobs = re.search(r'^policy: (\d+) observations \((\d+) on the panel, (\d+) off it\)', out, flags=re.M)
    ref = re.search(r'^policy refusals: (\d+) of (\d+)$', out, flags=re.M)
    assert found and nobs and ref, out
    assert int(nobs.group(1)) == NOBS and int(nobs.group(2)) > 300 and int(nobs.group(3)) >= 12, out
    return tuple(int(x) for x in found.groups()), tuple(int(x) for x in ref.groups())


def test_every_draw_against_the_mirror_and_every_refusal():
    """the default harness build: predictions of every draw bit-equal to policy_mirror on that draw's oracle solution, ssr and
    hits to fit_mirror with the build's egdst_policy_parts(), both residuals; the imported missing cell; each of the 17 refused
    calls on occ3 answers EGDST_E_ARG naming the observation or the argument, the handle then gives the bits it gave before
    them, and a solved retirement_hc (a continuous state) is refused with a message that says so: 18 refusals"""
    (ncell, nslices), (ok, tried) = _run_emu('')
    assert ncell >= 6 and nslices == 1
    assert ok == tried == 18


def test_several_slices_of_draws():
    """a budget of two draws' terms (12 bytes per observation and draw) makes the four draws take two slices (the runner
    derives the count from the flag and refuses a count below 2)"""
    (ncell, nslices), (ok, tried) = _run_emu('-DEG_POL_SLICE_BYTES=%d' % (2 * 12 * NOBS))
    assert emu.NDRAW == 4 and nslices == 2 and ok == tried


@pytest.mark.skipif(not emu.sanitizer_runtime(), reason='g++ has no AddressSanitizer / UBSan runtime')
def test_stand_alone_driver_under_asan_and_ubsan(tmp_path):
    """The harness library built with -fsanitize=address,undefined and emu_policy_main, with its own main, linked against it
    with the same sanitizers: one occ3 draw, the oracle's panel of 40 agents and points at a0, at mmax and above it, some without
    consumption, choice or weight.  Exit status 0, no report, and the printed bits are the mirror's."""
    import estimation_case
    m = emu.occ3_case()
    lib = build_emu.build(emu.write_modelspec(m), 'address', 1, False, 1)
    exe = str(tmp_path / 'emu_policy_main')
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    '-fno-omit-frame-pointer', os.path.join(HERE, 'cpu_emu', 'emu_policy_main.cpp'), lib, '-Wl,-rpath,' + os.path.dirname(lib),
                    '-pthread', '-o', exe], check=True)
    nsim, nt = 40, m.nt
    rng = np.random.default_rng(8)
    init = np.column_stack([np.ones(nsim), rng.uniform(m.a0, m.mmax, nsim)])
    par = m.param_vector()
    orc = emu.Oracle(m)
    sol = orc.solve(par)
    assert sol.rc == 0
    panel = orc.sim(sol, init, estimation_case.uniforms(31, 4 * nt * nsim), rndtype=0, params=par)
    on = datafit.Observations.from_panel(panel, m)
    extra = [(0, 0, m.a0), (nt - 1, 0, m.mmax), (2, 0, 3 * m.mmax), (1, 0, float(sol.M[1, 0, 1]))]
    n = len(on) + len(extra)
    cons = np.concatenate([on.cons, np.full(len(extra), 0.5)])
    ids = np.concatenate([on.id, np.zeros(len(extra), dtype=np.int32)])
    w = rng.uniform(0.5, 2, n)
    cons[rng.choice(n, n // 8, replace=False)] = np.nan
    ids[rng.choice(n, n // 6, replace=False)] = -1
    w[rng.choice(n, n // 7, replace=False)] = 0.0
    obs = datafit.Observations(np.concatenate([on.it, [e[0] for e in extra]]), np.concatenate([on.ist, [e[1] for e in extra]]),
                               np.concatenate([on.cash, [e[2] for e in extra]]), id=ids, cons=cons, w=w)
    rec = obs.pack()
    # the case file: the solver part as estimation_emu.write_case writes it, then the observations
    desc = m.descriptor()
    ngridmax = desc['ngridmax'] if desc['ngridmax'] > desc['ngridm'] else 2 * desc['ngridm']
    num = lambda a: ' '.join('%.17g' % v for v in np.asarray(a, dtype=np.float64).ravel())   # noqa: E731
    lines = ['%d %d %d %d %d %d %.17g %.17g %d' % (desc['t0'], desc['T'], desc['ngridm'], ngridmax, desc['nthrhmax'], desc['ny'],
                                                    desc['mmax'], desc['a0'], len(par)), num(desc['quadrature']), num(par), '%d' % n]
    lines += ['%d %d %d %.17g %.17g %.17g' % (r['it'], r['ist'], r['id'], r['cash'], r['cons'], r['w']) for r in rec]
    (tmp_path / 'case.txt').write_text('\n'.join(lines) + '\n')

    r = subprocess.run([exe, str(tmp_path / 'case.txt')], capture_output=True, text=True, timeout=900)   # (leak detection stays on)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert 'ERROR: AddressSanitizer' not in r.stderr and 'ERROR: LeakSanitizer' not in r.stderr and 'runtime error' not in r.stderr, \
        r.stderr[-3000:]
    out = r.stdout.splitlines()
    assert 'solve rc=0' in out and 'same 1' in out, out[:5]
    parts = int(emu.printed(out, 'parts')[0][0])
    assert parts == 1
    refused = [ln for ln in out if ln.startswith('refused')]
    assert len(refused) == 4 and all(ln.startswith('refused rc=1 egdst_policy_batch') for ln in refused), refused
    assert 'observation %d: reserved' % (n - 1) in refused[0] and 'observation 0: cash' in refused[1]

    rc, ri, rv = datafit.policy_mirror(sol, obs, call=lambda sw, a: orc.call(sol, sw, a, params=par), t0=m.t0)
    got = emu.printed(out, 'obs')
    assert len(got) == n
    for k, g in enumerate(got):
        assert g[:2] == [str(k), str(ri[k])] and emu.same_bits(g[2], rc[k]) and emu.same_bits(g[3], rv[k]), (k, g, rc[k], rv[k])
    assert (rec['cash'] > m.mmax).any() and (rec['cash'] == m.a0).any() and (ri >= 0).all()
    fits = emu.printed(out, 'fit')
    assert len(fits) == 2
    for resid, g in enumerate(fits):
        ssr, hits = datafit.fit_mirror(obs, rc, ri, resid=resid, block=parts)
        assert g[0] == str(resid) and emu.same_bits(g[1], ssr) and g[2] == str(hits), (g, ssr, hits)
        assert hits > 0
