"""Recorded outputs of the reference's own programs (oracle/build_ref.py), as fixtures that reach machines without it.

    python tests/golden/make_golden_ref.py [name ...]        # all: a few minutes (C4 at full size: one ~25 s solve)

Needs the reference sources (EGDST_REFERENCE_DIR).  Data only: what the reference's solver, simulator and accessor wrote.

  ref_<model>.npz      the twelve example models and C5 at T=10, ngridm=200: descriptor, parameters, len/thlen, the rows of
                       M, C, A, V and of D, TH of all cells back to back (cell order: it up, ist up), dbgout rows, the
                       simulator's panels for both rndtype with their init / randstream, the accessor's results case by case;
                       the warnings of every simulator and accessor call (count and text), and two accessor calls with a
                       wrong column count (xcall<k>_*)
  ref_C2_draws.npz     the first 256 C2 draws of the bench at a0=-5 and at a0=0: parameters, which draws fail, at which cell,
                       with which text; len/thlen of every draw and one checksum per draw
  ref_big_<case>.npz   C1, C2, C2_a0m5, C3, C4 at full size in the layout of big_*.npz (per-cell index-weighted checksums)

The accessor's value-function cases are recorded with their terminal-period rows FIRST: the reference evaluates those rows
with the decision of the last non-terminal row before them, and no such row then precedes them.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from egdst_amd import examples, workloads  # noqa: E402
from call_cases import call_cases  # noqa: E402
from make_golden_big import BIG, cell_sums  # noqa: E402

MODELS = dict({k: (lambda k=k: examples.retirement8(T=5, ngridm=10) if k == 'retirement8' else examples.REGISTRY[k]())
               for k in examples.REGISTRY}, C5_T10_n200=lambda: workloads.c5(ngridm=200, T=10)[0])
BIG_REF = ('C1', 'C2', 'C2_a0m5', 'C3', 'C4')
NDRAWS = 256
DRAW_SETS = {'a0m5': -5.0, 'a0_0': 0.0}


def init_rows(m):
    """Every state index whose continuous components sit at their first grid point, each with cash below a0, at a0,
    inside, at mmax and beyond; plus indices outside [1, nst]."""
    sizes, strides = [int(v) for v in m.stm[:m.nnst]], [int(v) for v in m.stm[m.nnst:]]
    rows = []
    for ist in range(m.nst):
        if any(v.type == 'continuous' and (ist // strides[k]) % sizes[k] for k, v in enumerate(m.s)):
            continue
        for cash in (m.a0 - 1.0, m.a0, m.a0 + 0.25, 0.5 * (m.a0 + m.mmax), m.mmax, 1.5 * m.mmax):
            rows.append([ist + 1, cash])
    rows += [[0, 1.0], [m.nst + 1, 1.0]]
    return np.array(rows, dtype=float)


def randstream(m, init):
    return np.random.default_rng(11).random(4 * m.nt * len(init))


def recorded_call_cases(m, nt):
    """tests/call_cases.py; value-function cases with their terminal-period rows moved to the front (module docstring)."""
    out = []
    for sw, args in call_cases(m, nt, m.nst, m.nd):
        if sw == 6 and args.shape[1] == 3:
            term = args[:, 0] == m.t0 + nt - 1
            args = np.concatenate([args[term], args[~term]])
        out.append((sw, args))
    return out


def wrong_column_cases(m):
    """Accessor calls whose argument matrix has the wrong number of columns: utility without consumption, value function
    without cash.  The reference warns once and leaves zeros."""
    it, ist = np.full(5, float(m.t0)), np.ones(5)
    return [(1, np.column_stack([it, ist, np.ones(5)])), (6, np.column_stack([it, ist]))]


def flat(sol):
    """Rows of all cells back to back."""
    nt, nst = sol.len.shape
    cells = [(it, ist) for it in range(nt) for ist in range(nst)]
    mcav = np.concatenate([sol.cell_M(it, ist) for it, ist in cells]) if cells else np.zeros((0, 4))
    dth = np.concatenate([sol.cell_D(it, ist) for it, ist in cells]) if cells else np.zeros((0, 2))
    return mcav, dth


def draw_checksum(sums):
    """One wrapping uint64 per draw from the [nt, nst, 5] cell checksums (each weighted by its position)."""
    s = np.ascontiguousarray(sums, dtype=np.uint64).reshape(-1)
    w = 2 * np.arange(s.size, dtype=np.uint64) + np.uint64(1)
    with np.errstate(over='ignore'):
        return (s * w).sum(dtype=np.uint64)


def fail_cell(ln, stores_failing_cell):
    """(it, ist) at which a failed solve stopped, in solving order (it down, ist up).  The reference stores the failing
    cell before it returns; the oracle and the device do not."""
    nt, nst = ln.shape
    order = [(it, ist) for it in range(nt - 1, -1, -1) for ist in range(nst)]
    filled = [k for k, c in enumerate(order) if ln[c] > 0]
    last = filled[-1] if filled else -1
    assert filled == list(range(last + 1)), 'cells are not filled in solving order'
    return order[last] if stores_failing_cell else order[last + 1]


def model_arrays(name):
    from ref_harness import Reference
    m = MODELS[name]()
    R = Reference(m)
    sol = R.solve(dbgout=True)
    assert sol.err == '', sol.err
    d = m.descriptor()
    mcav, dth = flat(sol)
    out = dict(t0=d['t0'], T=d['T'], ngridm=d['ngridm'], ngridmax=d['ngridmax'], nthrhmax=d['nthrhmax'], ny=d['ny'],
               mmax=d['mmax'], a0=d['a0'], params=m.param_vector(), len=sol.len, thlen=sol.thlen, mcav=mcav, dth=dth,
               dbgout=np.ascontiguousarray(np.asarray(sol.dbgout)[:sol.dbgn]), dbgn=np.int64(sol.dbgn))
    init = init_rows(m)
    rs = randstream(m, init)
    out['init'], out['randstream'] = init, rs
    for rt in (0, 1):
        r = R.sim(sol, init, rs, rt)
        assert r.err == '' and r.sims is not None
        out['sims%d' % rt] = r.sims
        out['sims%d_nwarn' % rt], out['sims%d_warnings' % rt] = np.int64(r.nwarn), np.array(r.warnings)
    cases = recorded_call_cases(m, sol.nt)
    out['ncall'] = np.int64(len(cases))
    for k, (sw, args) in enumerate(cases):
        r = R.call(sol, sw, args)
        assert r.err == '' and r.res is not None
        out['call%d_sw' % k], out['call%d_args' % k], out['call%d_res' % k] = np.int64(sw), args, r.res
        out['call%d_nwarn' % k], out['call%d_warnings' % k] = np.int64(r.nwarn), np.array(r.warnings)
    for k, (sw, args) in enumerate(wrong_column_cases(m)):
        r = R.call(sol, sw, args)
        assert r.err == '' and r.res is not None
        out['xcall%d_sw' % k], out['xcall%d_args' % k], out['xcall%d_res' % k] = np.int64(sw), args, r.res
        out['xcall%d_nwarn' % k], out['xcall%d_warnings' % k] = np.int64(r.nwarn), np.array(r.warnings)
    return out


def draws_arrays():
    from ref_harness import Reference
    out = {}
    for key, a0 in DRAW_SETS.items():
        m, gen = workloads.c2(a0=a0)
        P = gen(4096)[:NDRAWS]
        R = Reference(m)
        nt = m.nt
        ln, th = np.zeros((NDRAWS, nt, m.nst), np.int32), np.zeros((NDRAWS, nt, m.nst), np.int32)
        failed, cell, chk, texts = np.zeros(NDRAWS, bool), np.full((NDRAWS, 2), -1, np.int64), np.zeros(NDRAWS, np.uint64), []
        for i, p in enumerate(P):
            sol = R.solve(params=p)
            if sol.err:
                failed[i] = True
                cell[i] = fail_cell(sol.len, True)
                sol.len[tuple(cell[i])] = 0          # the failing cell itself holds no result
                sol.thlen[tuple(cell[i])] = 0
            texts.append(sol.err)
            ln[i], th[i] = sol.len, sol.thlen
            chk[i] = draw_checksum(cell_sums(sol))
        out.update({key + '_params': P, key + '_failed': failed, key + '_cell': cell, key + '_len': ln, key + '_thlen': th,
                    key + '_checksum': chk, key + '_err': np.array(texts)})
    return out


def big_arrays(name):
    from ref_harness import Reference
    m, par = BIG[name][0]()
    sol = Reference(m).solve(params=par)
    assert sol.err == '', sol.err
    d = m.descriptor()
    nt, nst = sol.len.shape
    lastM = np.zeros((nt, nst))
    for it in range(nt):
        for ist in range(nst):
            if sol.len[it, ist]:
                lastM[it, ist] = sol.M[it, ist, sol.len[it, ist] - 1]
    return dict(t0=d['t0'], T=d['T'], ngridm=d['ngridm'], ngridmax=d['ngridmax'], nthrhmax=d['nthrhmax'], ny=d['ny'],
                mmax=d['mmax'], a0=d['a0'], params=np.asarray(m.param_vector() if par is None else par, dtype=np.float64),
                len=sol.len, thlen=sol.thlen, sums=cell_sums(sol), lastM=lastM)


def targets():
    t = {'ref_%s.npz' % k: (lambda k=k: model_arrays(k)) for k in MODELS}
    t['ref_C2_draws.npz'] = draws_arrays
    t.update({'ref_big_%s.npz' % k: (lambda k=k: big_arrays(k)) for k in BIG_REF})
    return t


def load(fname):
    return np.load(os.path.join(HERE, fname))


if __name__ == '__main__':
    T = targets()
    for fname in (['ref_%s.npz' % a if not a.endswith('.npz') else a for a in sys.argv[1:]] or sorted(T)):
        arrays = T[fname]()
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **arrays)
        print('%s: %d bytes' % (fname, os.path.getsize(path)), flush=True)
