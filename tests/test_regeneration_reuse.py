"""k_fixup regenerates a guess stream from the probe's hand-over and takes the grid kernel's rows while its guesses are the grid
kernel's (EG_FIX_REUSE, egdst_kernels.hip): the results must be those of the build that regenerates every stream from its first
call (-DEG_FIX_REUSE=0) and of the oracle, bit for bit, with the same evaluation counts."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from egdst_amd import workloads  # noqa: E402

# the checking builds of the GPU test below (__graft_entry__.build() compiles them): the C2 batch build with the regeneration
# statistics (dbg ints 4, 7-11, 14 per draw), with and without the reuse
FIXSTAT = ['-DEGDST_FIXSTAT']
BUILD_VARIANTS = [(lambda: workloads.c2()[0], workloads.BATCH_BUILD_FLAGS['C2'] + FIXSTAT),
                  (lambda: workloads.c2()[0], workloads.BATCH_BUILD_FLAGS['C2'] + FIXSTAT + ['-DEG_FIX_REUSE=0'])]


def _asan():
    r = subprocess.run(['gcc', '-print-file-name=libasan.so'], capture_output=True, text=True)
    p = r.stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.mark.skipif(_asan() is None, reason='libasan not found')
def test_regenerated_streams_are_asan_clean_and_equal_with_and_without_reuse():
    """Full-size C2 at a0 = -5, three draws with 12 regenerated streams, one of which re-bases at every call up to the runaway
    guard (10 000 calls, 9 996 kept points): both builds under ASan+UBSan, each equal to the oracle."""
    env = dict(os.environ, LD_PRELOAD=_asan(), ASAN_OPTIONS='detect_leaks=0', EMU_SANITIZE='address', EMU_NGRIDM='1000', EMU_T='60',
               EGDST_TRACE_FIXUP='1')
    r = subprocess.run([sys.executable, os.path.join(HERE, 'cpu_emu', 'run_emu_fix_reuse.py'), '3', '0'], env=env,
                       capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'ERROR: AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('draw ')]
    assert len(lines) == 3
    for ln in lines:
        assert 'on_same_as_oracle=True off_same_as_oracle=True' in ln, ln
        f = ln.split()
        assert f[3].split('/')[0] == f[3].split('/')[1], ln                           # regenerated streams
        assert f[5].split('/')[0] == f[5].split('/')[1], ln                           # status
        assert f[7].split('/')[0] == f[7].split('/')[1], ln                           # evaluations
    assert 'regenerated streams: 12' in r.stdout, r.stdout
    ends = [ln for ln in r.stderr.splitlines() if ln.startswith('fixup end')]
    assert len(ends) == 24, r.stderr[-3000:]
    taken = [int(ln.rsplit('taken=', 1)[1]) for ln in ends]
    assert sum(taken[:12]) > 0 and sum(taken[12:]) == 0, taken                          # (the reuse build runs first)
    assert any('ncalls=10000' in ln for ln in ends[:12])


def _solve(lib, m, P):
    from egdst_amd import runtime
    s = runtime.Solver(lib, m.descriptor(), ndraw=len(P), keep_history=True)
    s.set_params(P)
    s.solve(raise_on_error=False)
    st, ev = s.status()[0].copy(), s.evals()[1].copy()
    sums = np.stack([s.checksums(d) for d in range(len(P))])
    dbg = np.stack([s.debug(d) for d in range(len(P))]).astype(np.int64)
    reg = s.regenerations().copy()
    s.close()
    return st, ev, sums, dbg, reg


@pytest.mark.gpu
@pytest.mark.parametrize('a0', [-5.0, 0.0])
def test_reuse_equals_full_regeneration_on_the_c2_batch_build(a0):
    from egdst_amd import build
    m, gen = workloads.c2(a0=a0)
    P = gen(512)
    on = _solve(build.build_model(m, extra_flags=BUILD_VARIANTS[0][1]), m, P)
    off = _solve(build.build_model(m, extra_flags=BUILD_VARIANTS[1][1]), m, P)
    assert np.array_equal(on[0], off[0])                      # status per draw
    assert np.array_equal(on[1], off[1])                      # evaluations per draw
    assert np.array_equal(on[2], off[2])                      # checksums of every cell (M, C, V, TH, D)
    assert np.array_equal(on[4], off[4]) and on[4].sum() > 0  # the same streams regenerated
    assert on[3][:, 14].sum() > 0 and off[3][:, 14].sum() == 0  # grid rows taken
    assert on[3][:, 11].sum() == off[3][:, 11].sum()          # streams counted by the statistics
    print('a0=%g: %d regenerated streams; per stream: taken rows %.0f, guesses evaluated in batches %.0f against %.0f, calls taken '
          'over from the probe %.1f, ticks %.0f against %.0f us' % (
              a0, on[3][:, 11].sum(), on[3][:, 14].sum() / on[3][:, 11].sum(), on[3][:, 7].sum() / on[3][:, 11].sum(),
              off[3][:, 7].sum() / off[3][:, 11].sum(), on[3][:, 4].sum() / on[3][:, 11].sum(),
              ((on[3][:, 12] & 0xffffffff) + (on[3][:, 13] << 32)).sum() * 1e-2 / on[3][:, 11].sum(),
              ((off[3][:, 12] & 0xffffffff) + (off[3][:, 13] << 32)).sum() * 1e-2 / off[3][:, 11].sum()))
