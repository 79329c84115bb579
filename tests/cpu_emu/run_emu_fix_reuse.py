"""Harness build: C2 at the surveyed credit limit a0 = -5 (reduced sizes), a batch of draws whose guess streams k_fixup
regenerates, solved by the default build (k_fixup starts at the probe's hand-over and takes the grid kernel's rows) and by the
build that regenerates every stream from its first call (-DEG_FIX_REUSE=0): every table, status and evaluation count of the
two must equal the oracle's bit for bit.
   python tests/cpu_emu/run_emu_fix_reuse.py <ndraw> <first draw>      (EMU_SANITIZE=address for ASan+UBSan)"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, os.path.join(ROOT, 'tests', 'cpu_emu'))
import numpy as np
import build_emu
from egdst_amd import runtime, workloads
from estimation_emu import write_modelspec
from oracle_harness import Oracle
from parity import compare


def solve(lib, m, P):
    s = runtime.Solver(lib, m.descriptor(), ndraw=len(P), keep_history=True)
    s.set_params(P)
    s.solve(raise_on_error=False)
    out = [s.solution(i) for i in range(len(P))], s.status()[0].copy(), s.evals()[1].copy(), s.regenerations().copy()
    s.close()
    return out


if __name__ == '__main__':
    nd = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    d0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    m, gen = workloads.c2(a0=-5.0, ngridm=int(os.environ.get("EMU_NGRIDM", 300)), T=int(os.environ.get("EMU_T", 20)), ny=10)
    P = gen(d0 + nd)[d0:]
    d = write_modelspec(m)
    san = os.environ.get('EMU_SANITIZE', '0')
    san = {'0': False}.get(san, san)
    res = {}
    for flag in ('', '-DEG_FIX_REUSE=0'):
        os.environ['EMU_EXTRA_FLAGS'] = flag   # (build_emu.build names the library after its flags)
        res[flag] = solve(runtime.ModelLibrary(build_emu.build(d, san, 1, False, 1)), m, P)
    os.environ.pop('EMU_EXTRA_FLAGS')
    (sa, st_a, ev_a, rg_a), (sb, st_b, ev_b, rg_b) = res[''], res['-DEG_FIX_REUSE=0']
    orc = Oracle(m)
    for i in range(nd):
        ref = orc.solve(P[i])
        ok_ref, rep = compare(sa[i], ref, 0.0, 0.0)
        ok_ab, rep_ab = compare(sb[i], ref, 0.0, 0.0)
        print('draw %d regenerated %d/%d status %d/%d/%d evals %d/%d/%d on_same_as_oracle=%s off_same_as_oracle=%s %s' % (
            d0 + i, rg_a[i], rg_b[i], st_a[i], st_b[i], ref.rc, ev_a[i], ev_b[i], ref.nevals, ok_ref, ok_ab,
            (rep['problems'] + rep_ab['problems'])[:2]))
    print('regenerated streams: %d' % int(rg_a.sum()))
