"""Shared by the CPU-harness test and the GPU test of the estimation loop's solve: one handle without history (two ping-pong
periods), parameters already on the device, egdst_set_params_dev / egdst_solve_async / egdst_objective_dev chunk after chunk.
In that mode only status, counters and the objective leave the device, so the tests read the two live periods where the
handle keeps them (Solver.device_tables) and hold them to the oracle: the chunks of draws, the readers of the live periods,
and the comparison, which is on bits throughout."""
import ctypes as C

import numpy as np

COLS = ('M', 'C', 'V')


def chunks_then_first_reversed(P, chunk, nchunks):
    """P[0:chunk], P[chunk:2 chunk], ... and the first chunk once more in reversed order: other draws at every index from one
    chunk to the next, so the tables of a slot shrink and grow, and a draw that fails follows one that solves at its index"""
    out = [np.ascontiguousarray(P[c * chunk:(c + 1) * chunk]) for c in range(nchunks)]
    assert all(len(p) == chunk for p in out)
    return out + [np.ascontiguousarray(out[0][::-1])]


class OracleCache:
    """the oracle's solution of every distinct parameter vector, solved once"""

    def __init__(self, model):
        from oracle_harness import Oracle
        self.orc = Oracle(model)
        self.model = model
        self._sols = {}

    def solve(self, p):
        p = np.ascontiguousarray(p, dtype=np.float64)
        key = p.tobytes()
        if key not in self._sols:
            self._sols[key] = self.orc.solve(p)
        return self._sols[key]


def _shapes(solver):
    return (solver.ndraw, solver.lib.info.nst)


def read_live_period_host(solver, it):
    """{'M', 'C', 'V': [ndraw, nst, stride], 'len': [ndraw, nst]} copied from a CPU-harness handle, whose "device" pointers are
    host addresses"""
    pm, pc, pv, pl, stride = solver.device_tables(it)
    nd, nst = _shapes(solver)
    out = {k: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), shape=(nd, nst, stride)).copy()
           for k, p in zip(COLS, (pm, pc, pv))}
    out['len'] = np.ctypeslib.as_array(C.cast(pl, C.POINTER(C.c_int)), shape=(nd, nst)).copy()
    return out


class _DeviceArray:
    """device memory that torch did not allocate, as torch.as_tensor takes it (zero-copy)"""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {'shape': tuple(shape), 'typestr': typestr, 'data': (int(ptr), False), 'strides': None,
                                         'version': 2}


def snapshot_live_period_device(solver, it, stream):
    """the same as device tensors: views of the handle's tables cloned under `stream` (the handle's), so that the copy follows
    the solve enqueued before it and precedes the one enqueued after it, without a host synchronisation"""
    import torch
    pm, pc, pv, pl, stride = solver.device_tables(it)
    nd, nst = _shapes(solver)
    with torch.cuda.stream(stream):
        out = {k: torch.as_tensor(_DeviceArray(p, (nd, nst, stride), '<f8'), device='cuda').clone()
               for k, p in zip(COLS, (pm, pc, pv))}
        out['len'] = torch.as_tensor(_DeviceArray(pl, (nd, nst), '<i4'), device='cuda').clone()
    return out


def to_host(snapshot):
    return {k: v.cpu().numpy() for k, v in snapshot.items()}


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def check(cache, chunks, expect_failed, last=None):
    """chunks: per chunk a dict with 'P' [chunk, nparam], 'obj' [chunk, 2] and 'tabs' {0: .., 1: ..}, the live periods as the
    readers above return them (host arrays), all taken after that chunk's solve.  expect_failed: the draws per chunk that the
    oracle fails, asserted here from the oracle alone.  last: for the chunk read back last a dict with 'status', 'where',
    'evals' of the handle, 'strerror' (status -> text) and 'where_kept', the `where` of a kept-history solve of the same draws.
    Returns the list of problems (empty = pass); no tolerance anywhere."""
    refs = [[cache.solve(p) for p in ch['P']] for ch in chunks]
    failed = [sum(int(r.rc != 0) for r in rs) for rs in refs]
    assert failed == list(expect_failed), ('draws the oracle fails, per chunk', failed, expect_failed)
    bad, compared = [], 0
    for c, (ch, rs) in enumerate(zip(chunks, refs)):
        obj = np.asarray(ch['obj'], dtype=np.float64)
        assert obj.shape == (len(rs), 2)
        for d, ref in enumerate(rs):
            at = 'chunk %d draw %d' % (c, d)
            if ref.rc != 0:
                if not np.isnan(obj[d]).all():
                    bad.append('%s: the oracle fails (%s), objective %r' % (at, ref.err.strip(), obj[d].tolist()))
                continue
            compared += 1
            want = np.array([ref.V[0, 0, 1], ref.C[0, 0, 1]])
            if not _same(obj[d], want):
                bad.append('%s: objective %r, oracle %r' % (at, obj[d].tolist(), want.tolist()))
            for it in (0, 1):
                tab = ch['tabs'][it]
                stride = tab['M'].shape[2]
                assert stride == ref.M.shape[2], (stride, ref.M.shape)
                for ist in range(ref.len.shape[1]):
                    n = int(ref.len[it, ist])
                    if int(tab['len'][d, ist]) != n:
                        bad.append('%s it %d ist %d: len %d, oracle %d' % (at, it, ist, tab['len'][d, ist], n))
                        continue
                    for col in COLS:
                        row = tab[col][d, ist]
                        if not _same(row[:n], getattr(ref, col)[it, ist, :n]):
                            k = np.nonzero(row[:n].view(np.int64) != getattr(ref, col)[it, ist, :n].view(np.int64))[0]
                            bad.append('%s it %d ist %d: %s differs in %d of %d rows, first %d' % (at, it, ist, col, len(k), n, k[0]))
                        tail = row[n:].view(np.int64)
                        if tail.any():
                            k = np.nonzero(tail)[0]
                            bad.append('%s it %d ist %d: %s has %d non-zero rows past its end %d, first %d = %r'
                                       % (at, it, ist, col, len(k), n, n + k[0], float(row[n + k[0]])))
    assert compared == sum(len(rs) for rs in refs) - sum(failed) and compared > 0
    if last is not None:
        rs = refs[-1]
        st, wh, ev = last['status'], last['where'], last['evals']
        for d, ref in enumerate(rs):
            at = 'last chunk draw %d' % d
            if ref.rc == 0:
                if st[d] != 0 or int(ev[d]) != ref.nevals:
                    bad.append('%s: status %d, %d evaluations, oracle solves with %d' % (at, st[d], ev[d], ref.nevals))
                continue
            if st[d] == 0 or last['strerror'](int(st[d])).strip() != ref.err.strip():
                bad.append('%s: status %d, oracle %r' % (at, st[d], ref.err.strip()))
            if tuple(wh[d]) != tuple(last['where_kept'][d]):
                bad.append('%s: fails at %r, the kept-history solve at %r' % (at, tuple(wh[d]), tuple(last['where_kept'][d])))
    return bad
