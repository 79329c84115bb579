"""The fit to micro data: observations of a data panel for egdst_policy_batch (include/egdst.h), and the host mirrors the tests
hold the device to -- the policy in numpy from an exported solution, operation for operation as the device's bracket search and
interpolation (csrc/egdst_device.h: eg_bracket, eg_lerp; csrc/egdst_kernels.hip: eg_policy_at), and the fit in the summation
order of the contract.  Nothing here runs on the estimation path: Solver.policy_batch does.

The same observations can stay on a handle (egdst_attach_panel: Solver.attach_panel, fit_dev, fit): every solve then evaluates them
period by period while the period's table is live, so the fit needs no history and no host synchronisation -- the form for an
estimation loop over a large batch.  Its ssr and hits are egdst_policy_batch's bit for bit, so fit_mirror below is the contract
of both doors; the predictions themselves (cons, id, vf) remain policy_batch's."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

# egdst_obs: 40 bytes, no padding
OBS_DTYPE = np.dtype([('it', '<i4'), ('ist', '<i4'), ('id', '<i4'), ('reserved', '<i4'), ('cash', '<f8'), ('cons', '<f8'), ('w', '<f8')])
assert OBS_DTYPE.itemsize == 40

# columns of a simulated path that a panel is read by (egdst_simulate: the first 11 are the same for every model)
COL_M, COL_C, COL_VF, COL_ID, COL_IST = 0, 1, 3, 4, 5


class Observations:
    """Observed households: period `it` and state `ist` (0-based), cash-in-hand, and what may be missing -- the choice `id`
    (0-based; -1 or None: not observed), consumption `cons` (NaN or None: not observed) and the weight `w` in the fit (None: 1)."""

    def __init__(self, it, ist, cash, id=None, cons=None, w=None):   # noqa: A002  (the field's name in egdst_obs)
        self.cash = np.atleast_1d(np.asarray(cash, dtype=np.float64)).reshape(-1).copy()
        n = self.cash.size

        def col(a, dtype, default):
            a = np.full(n, default, dtype=dtype) if a is None else np.atleast_1d(np.asarray(a)).reshape(-1).astype(dtype)
            if a.size == 1 and n > 1:
                a = np.repeat(a, n)
            if a.size != n:
                raise ValueError('Observations: a column has %d entries for %d observations' % (a.size, n))
            return a.copy()
        self.it, self.ist = col(it, np.int32, 0), col(ist, np.int32, 0)
        self.id = col(id, np.int32, -1)
        self.cons = col(cons, np.float64, np.nan)
        self.w = col(w, np.float64, 1.0)

    def __len__(self):
        return self.cash.size

    @classmethod
    def from_panel(cls, panel, layout=None, w=None):
        """every present (agent, period) pair of a `sims`-shaped panel [nsim, nt, nout] -- simulated by the library, by the
        oracle, or real data laid out that way -- in agent order, within an agent in period order: the state from column 5,
        cash from column 0, the choice from column 4 and consumption from column 1.  A pair is present when its cash is not NaN.
        layout (a model or a library's info) is only checked against the panel's width."""
        panel = np.asarray(panel, dtype=np.float64)
        if panel.ndim != 3 or panel.shape[2] < 11:
            raise ValueError('from_panel: the panel is not [nsim, nt, nout >= 11]')
        if layout is not None:
            from . import moments
            nout = 11 + sum(moments._layout(layout))
            if panel.shape[2] != nout:
                raise ValueError('from_panel: the panel has %d columns, the layout %d' % (panel.shape[2], nout))
        ia, it = np.nonzero(~np.isnan(panel[:, :, COL_M]))
        row = panel[ia, it]
        choice = np.where(np.isnan(row[:, COL_ID]), -1, row[:, COL_ID]).astype(np.int32)
        return cls(it, row[:, COL_IST].astype(np.int32), row[:, COL_M], id=choice, cons=row[:, COL_C], w=w)

    def pack(self):
        """the 40-byte records egdst_policy_batch takes"""
        rec = np.zeros(len(self), dtype=OBS_DTYPE)
        for f in ('it', 'ist', 'id', 'cash', 'cons', 'w'):
            rec[f] = getattr(self, f)
        return rec


def records(obs):
    """contiguous OBS_DTYPE records of an Observations or of an array of that dtype"""
    if isinstance(obs, Observations):
        return obs.pack()
    rec = np.ascontiguousarray(obs)
    if rec.dtype != OBS_DTYPE or rec.ndim != 1:
        raise ValueError('expected datafit.Observations or a 1-d array of datafit.OBS_DTYPE')
    return rec


# ---- the policy, as the device computes it

def _bracket(x, g, n):
    """eg_bracket(x, g, n, 0) for a vector of x on one column: the reference's bisection (bxsearch_common, egdst_lib.c:136-166),
    every lane stepping as the scalar loop does"""
    lo = np.ones(x.size, dtype=np.int64)
    hi = np.full(x.size, n - 2, dtype=np.int64)
    below, above = x < g[1], x >= g[n - 2]
    asc = bool(g[0] <= g[n - 1])
    run = ~below & ~above & (hi - lo > 1)
    while run.any():
        mid = (hi + lo) // 2
        up = (g[mid] > x) if asc else np.zeros(x.size, dtype=bool)
        hi = np.where(run & up, mid, hi)
        lo = np.where(run & ~up, mid, lo)
        run = run & (hi - lo > 1)
    return np.where(below, 0, np.where(above, n - 2, lo))


def _lerp(x, g0, g1, f0, f1):
    """eg_lerp: f1 (x - g0) / (g1 - g0) + f0 (g1 - x) / (g1 - g0), every operation rounded"""
    with np.errstate(all='ignore'):
        return f1 * (x - g0) / (g1 - g0) + f0 * (g1 - x) / (g1 - g0)


def policy_mirror(tables, obs, call=None, t0=1):
    """(c, id, vf) at every observation from one draw's exported solution (`tables`: the arrays of Solver.solution / the
    oracle's: M, C, V [nt, nst, rows], D, TH [nt, nst, nthrhmax], len, thlen [nt, nst]), as eg_policy_at computes them.  Below the
    first endogenous point the value is u(c) + discount * V[0], which needs the model's functions: call(sw, args) with
    egdst_call's conventions (sw 1 utility on rows (period, state, decision, c), sw 3 discount on rows (period, state); period as
    the model counts it from t0, state and decision 1-based) -- Solver.call or the oracle's.  An observation whose cell has
    fewer than two rows reads NaN / -1 / NaN."""
    rec = records(obs)
    n = len(rec)
    c, vf, ids = np.full(n, np.nan), np.full(n, np.nan), np.full(n, -1, dtype=np.int32)
    cell = rec['it'].astype(np.int64) * tables.len.shape[1] + rec['ist']
    for key in np.unique(cell):
        who = np.nonzero(cell == key)[0]
        it, ist = int(rec['it'][who[0]]), int(rec['ist'][who[0]])
        ln, th = int(tables.len[it, ist]), int(tables.thlen[it, ist])
        if ln < 2:
            continue
        M, Cc, V = tables.M[it, ist], tables.C[it, ist], tables.V[it, ist]
        TH, D = tables.TH[it, ist], tables.D[it, ist]
        x = rec['cash'][who]
        i = _bracket(x, M, ln)
        ci = _lerp(x, M[i], M[i + 1], Cc[i], Cc[i + 1])
        # the threshold scan: j = the number of leading thresholds that are not above x
        if th > 0:
            ok = x[:, None] >= TH[None, :th]
            j = np.where(ok.all(axis=1), th, ok.argmin(axis=1))
        else:
            j = np.zeros(x.size, dtype=np.int64)
        di = D[np.maximum(j - 1, 0)].astype(np.int32)
        vi = _lerp(x, M[i], M[i + 1], V[i], V[i + 1])
        low = (x < M[1]) & (V[0] > -np.inf)
        if low.any():
            if call is None:
                raise ValueError('policy_mirror: an observation lies below the first endogenous point: the value there needs `call`')
            k = np.nonzero(low)[0]
            per, st = np.full(k.size, it + t0, dtype=np.float64), np.full(k.size, ist + 1, dtype=np.float64)
            u = np.asarray(call(1, np.column_stack([per, st, di[k] + 1.0, ci[k]])))
            df = np.asarray(call(3, np.column_stack([per, st])))
            vi[k] = u + df * V[0]
        c[who], ids[who], vf[who] = ci, di, vi
    return c, ids, vf


# ---- the fit, in the order of the contract

_HOST_MATH = None


def host_log(x):
    """eg_log of include/egdst_math.h on the host, the device's bits: the header compiled by gcc with -ffp-contract=off, as
    tests/test_math_vs_libm.py compiles it (the library is kept beside the model libraries)"""
    global _HOST_MATH
    if _HOST_MATH is None:
        from . import build
        d = os.path.join(build.MODELS_DIR, '_hostmath')
        os.makedirs(d, exist_ok=True)
        inc = os.path.join(build.HERE, '..', 'include')
        so, src = os.path.join(d, 'libegdst_hostmath.so'), os.path.join(d, 'hostmath.c')
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(os.path.join(inc, 'egdst_math.h')):
            tmp = '%s.tmp.%d' % (so, os.getpid())
            with open(src, 'w') as f:
                f.write('#include "egdst_math.h"\nvoid egdst_host_log(int n, const double *x, double *out)\n'
                        '{\n    for (int i = 0; i < n; i++) out[i] = eg_log(x[i]);\n}\n')
            subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-I', inc, src, '-o', tmp, '-lm'], check=True)
            os.replace(tmp, so)
        _HOST_MATH = C.CDLL(so)
        _HOST_MATH.egdst_host_log.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.zeros_like(x)
    _HOST_MATH.egdst_host_log(x.size, x.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double)))
    return out


def fit_terms(obs, cons, resid, log=host_log):
    """(term, counts): w (r r) per observation, two rounded products, and which observations enter the sum (consumption observed,
    weight not zero); r = cons_k - c_k, or for resid = 1 log(cons_k) - log(c_k) with the device's log"""
    rec = records(obs)
    cons = np.asarray(cons, dtype=np.float64)
    with np.errstate(all='ignore'):
        r = (log(rec['cons']) - log(cons)) if resid else (rec['cons'] - cons)
        term = rec['w'] * (r * r)
    return term, ~np.isnan(rec['cons']) & (rec['w'] != 0.0)


def fit_mirror(obs, cons, ids, resid=0, block=256, failed=False, log=host_log):
    """(ssr, hits) of one draw from its predictions (cons, ids: what the device or policy_mirror gives) in the order of
    egdst_policy_batch: partial t of `block` adds the terms of the observations k = t (mod block) that count in ascending k, then
    the tree p[t] += p[t + o] for o = block/2 .. 1.  An observation without a policy (id -1) makes ssr NaN; a failed draw is
    (NaN, -1).  block = the library's policy_parts gives the device's bits."""
    if failed:
        return np.nan, -1
    if block < 1 or block & (block - 1):
        raise ValueError('fit_mirror: block is not a power of two')
    rec = records(obs)
    ids = np.asarray(ids)
    term, counts = fit_terms(rec, cons, resid, log)
    rounds = -(-len(rec) // block)
    tt = np.zeros(rounds * block)
    cc = np.zeros(rounds * block, dtype=bool)
    tt[:len(rec)], cc[:len(rec)] = term, counts
    p = np.zeros(block)
    with np.errstate(all='ignore'):
        for q in range(rounds):
            row, use = tt[q * block:(q + 1) * block], cc[q * block:(q + 1) * block]
            p = np.where(use, p + row, p)
        o = block // 2
        while o >= 1:
            p[:o] = p[:o] + p[o:2 * o]
            o //= 2
    hits = int(((rec['id'] >= 0) & (rec['id'] == ids)).sum())
    return (np.nan if (ids < 0).any() else float(p[0])), hits
