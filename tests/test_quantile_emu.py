"""k_quantiles on the CPU harness (tests/cpu_emu), without a GPU: the estimation step with quantile moments in both regimes of
the kernel and over several slices of draws, loaded into python with no sanitizer (this file preloads nothing); and the same
code under AddressSanitizer / UBSan, leak check included, through a stand-alone driver that links the sanitizer's runtime
itself."""
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'cpu_emu'))
import estimation_emu as emu


def _run_emu(flags):
    out = emu.run_runner('run_emu_quantiles.py', flags, 'quantile problems: 0')
    found = re.search(r'^quantile regimes \(lds, global\): \((\d+), (\d+)\)  slices: (\d+)$', out, flags=re.M)
    assert found, out
    return tuple(int(x) for x in found.groups())


def test_both_regimes_of_the_selection():
    """QNT_LDS_KEYS=64: the 48 agents of one period are selected in LDS, pooled periods from global memory"""
    lds, glob, nslices = _run_emu('-DQNT_LDS_KEYS=64')
    assert lds > 0 and glob > 0 and nslices == 1


def test_quantiles_over_several_slices_of_draws():
    """the paths of one draw are 8 bytes * nout columns * 7 periods (t0 = 0 .. T = 6) * 48 agents; a slice of two of them
    makes the four draws take two slices (the runner derives the count from the flag and refuses a count below 2)"""
    m = emu.occ3_case()
    from egdst_amd import moments as mo
    nout = len(mo.columns(*mo._layout(m)))
    per_draw = 8 * nout * m.nt * emu.NSIM
    lds, glob, nslices = _run_emu('-DEG_SIM_SLICE_BYTES=%d' % (2 * per_draw))
    assert emu.NDRAW == 4 and nslices == 2 and lds > 0


def _keys(x):
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))


@pytest.mark.skipif(not emu.sanitizer_runtime(), reason='g++ has no AddressSanitizer / UBSan runtime')
def test_stand_alone_driver_under_asan_and_ubsan(tmp_path):
    """The harness library built with -fsanitize=address,undefined and a driver with its own main linked against it: one occ3
    draw, the estimation step with generated uniforms on a handful of quantile records, egdst_quantile_eval on a small
    array.  Exit status 0, no report, and the printed bits are those computed here from the oracle's paths for the
    replayed uniforms."""
    import estimation_case
    from egdst_amd import moments as mo
    m = emu.occ3_case()
    exe = emu.build_driver(m, tmp_path)

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
    par = m.param_vector()
    emu.write_case(tmp_path / 'case.txt', m, nsim, seed, init, rec, quantile=(x, p))
    out = emu.run_driver(exe, 'spec', tmp_path / 'case.txt')
    assert 'solve rc=0' in out and 'refused rc=1' in out, out

    orc = emu.Oracle(m)
    sol = orc.solve(par)
    assert sol.rc == 0
    sims = orc.sim(sol, init, estimation_case.uniforms(seed, 4 * m.nt * nsim), rndtype=0, params=par)
    rm, rc = spec.evaluate(sims, block=1)
    nan_rows = [j for j in range(len(rec)) if rc[j] == 0]
    assert nan_rows == [len(rec) - 1]   # (nobody chooses 9)
    emu.assert_moments(out, rm, rc)   # (every line, bit for bit; a NaN's payload is not part of the contract)
    assert (rc[:4] > 0).all()
    v = x[~np.isnan(x)]
    ks = np.sort(_keys(v))
    for i, pi in enumerate(p):
        key = ks[min(max(math.ceil(pi * float(len(v))), 1), len(v)) - 1]
        u = int(key) & ((1 << 63) - 1) if int(key) >> 63 else ~int(key) & ((1 << 64) - 1)
        assert 'eval %d %d %016x' % (i, len(v), u) in out, (i, out)
