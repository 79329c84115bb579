"""The data panel attached to a handle and evaluated inside the solve (egdst_attach_panel, egdst_fit_dev, egdst_get_fit) on the
CPU harness (tests/cpu_emu), without a GPU: a handle without history with 1 and 2 draw groups, and one with history, against
datafit.fit_mirror on every draw's oracle solution, both residuals, two solves back to back; the lifetime of the fit and every
refusal, loaded into python with no sanitizer (this file preloads nothing); and the same code under AddressSanitizer / UBSan,
leak check included, through a stand-alone driver that links the sanitizer's runtime itself.

The flag -1 (an observation in a cell with fewer than 2 rows, which makes a draw's ssr NaN) cannot be reached here: no shipped
model solves with a missing cell, and imported solutions are not served by this door (egdst_fit_dev answers
EGDST_E_NOT_SOLVED).  That branch of the reduction stands on k_policy_fit's existing coverage (test_policy_fit_emu's imported
missing cell through egdst_policy_batch): the reduction exists once."""
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


def test_every_draw_against_the_mirror_back_to_back_and_every_refusal():
    """occ3, emu.NDRAW draws, the 349 observations of the policy runner: without history with 1 and 2 groups and with history,
    resid 0 and 1, two solves enqueued back to back (the second with the draws reversed) and one synchronisation -- every
    (chunk, draw) is fit_mirror's bits with the build's one partial sum; the six stations of the fit's lifetime (no panel,
    no solve yet, both outputs NULL, a refused attach keeps the fit, after the detach, after an import); the 16 refused
    attaches on occ3 and the one on retirement_hc"""
    out = emu.run_runner('run_emu_attached.py', '', 'attached problems: 0')
    head = re.search(r'^attached: (\d+) observations .* (\d+) \(draw, chunk\) pairs compared$', out, flags=re.M)
    life = re.search(r'^attached lifetime: (\d+) of (\d+)$', out, flags=re.M)
    ref = re.search(r'^attached refusals: (\d+) of (\d+)$', out, flags=re.M)
    assert head and life and ref, out
    assert int(head.group(1)) == 349 and int(head.group(2)) == 2 * 2 * 2 * 2 * emu.NDRAW
    assert life.groups() == ('6', '6') and ref.groups() == ('17', '17')


@pytest.mark.skipif(not emu.sanitizer_runtime(), reason='g++ has no AddressSanitizer / UBSan runtime')
def test_stand_alone_driver_under_asan_and_ubsan(tmp_path):
    """The harness library built with -fsanitize=address,undefined and emu_attached_main, with its own main, linked against it
    with the same sanitizers: two occ3 draws in two groups on a handle without history, the oracle's panel of 40 agents and points
    at a0, at mmax and above it, some without consumption, choice or weight.  Exit status 0, no report, the printed bits are the
    mirror's in both solves and both draws, the refusals are answered and a panel left attached is freed with the handle."""
    import estimation_case
    m = emu.occ3_case()
    lib = build_emu.build(emu.write_modelspec(m), 'address', 1, False, 1)
    exe = str(tmp_path / 'emu_attached_main')
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    '-fno-omit-frame-pointer', os.path.join(HERE, 'cpu_emu', 'emu_attached_main.cpp'), lib, '-Wl,-rpath,' + os.path.dirname(lib),
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
    parts = int(emu.printed(out, 'parts')[0][0])
    assert parts == 1
    assert [ln for ln in out if ln.startswith('early')] == ['early rc=1', 'early rc=40'], out[:6]
    assert 'host 0 1' in out and 'host 1 1' in out and 'again 1' in out and 'detached rc=1' in out, out[-8:]
    refused = [ln for ln in out if ln.startswith('refused')]
    assert len(refused) == 3 and all(ln.startswith('refused rc=1 egdst_attach_panel') for ln in refused), refused
    assert 'observation %d: reserved' % (n - 1) in refused[0] and 'observation 0: cash' in refused[1] and 'resid' in refused[2]

    rc, ri, _ = datafit.policy_mirror(sol, obs, call=lambda sw, a: orc.call(sol, sw, a, params=par), t0=m.t0)
    fits = emu.printed(out, 'fit')
    assert len(fits) == 2 * 2 * 2
    want = {resid: datafit.fit_mirror(obs, rc, ri, resid=resid, block=parts) for resid in (0, 1)}
    assert want[0][1] > 0 and np.isfinite(want[0][0])
    seen = set()
    for g in fits:
        resid, k, d = int(g[0]), int(g[1]), int(g[2])
        seen.add((resid, k, d))
        ssr, hits = want[resid]
        assert emu.same_bits(g[3], ssr) and g[4] == str(hits), (g, ssr, hits)
    assert len(seen) == 8
