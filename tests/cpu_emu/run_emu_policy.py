"""Harness build, no sanitizer: the policy at a data panel's observations (egdst_policy_batch) on 4 perturbed occ3 draws.  The
observations are the oracle's panel of draw 0 (48 agents) and off-path points -- cash exactly at a0 and at mmax, at a table's
M[1], at an interior grid value, just below a threshold -- some without consumption, some without a choice, some with weight 0.
Every draw's predictions are held to datafit.policy_mirror on that draw's own oracle solution, ssr and hits to
datafit.fit_mirror with the build's egdst_policy_parts(), for both residuals; then a solution imported with a missing cell, and
every refusal, the one for a model with continuous states on a harness build of retirement_hc.  EMU_EXTRA_FLAGS chooses what the build exercises: -DEG_POL_SLICE_BYTES=... makes the draws take several slices of
terms.  Nothing is preloaded."""
import copy
import os

import numpy as np
import estimation_emu as emu
from estimation_emu import NDRAW, flag
from egdst_amd import datafit, runtime
from estimation_case import bits_equal, uniforms


def off_path(m, sol, nt):
    """(it, ist, cash) of the points no simulated agent stands on, from the tables of one solution"""
    pts = []
    for it in (0, nt // 2, nt - 1):
        ist = 0
        ln, th = int(sol.len[it, ist]), int(sol.thlen[it, ist])
        M, TH = sol.M[it, ist], sol.TH[it, ist]
        pts += [(it, ist, m.a0), (it, ist, m.mmax), (it, ist, M[1]), (it, ist, M[ln // 2])]
        pts += [(it, ist, np.nextafter(TH[j], -np.inf)) for j in range(th) if m.a0 < TH[j] < np.inf][:2]
    return [p for p in pts if m.a0 <= p[2]]


def observations(b, sols):
    panel = b.orc.sim(sols[0], b.init, uniforms(77, 4 * b.s.nt * len(b.init)), rndtype=0, params=b.P[0])
    on = datafit.Observations.from_panel(panel, b.lib.info)
    off = off_path(b.m, sols[0], b.s.nt)
    it = np.concatenate([on.it, [p[0] for p in off]])
    ist = np.concatenate([on.ist, [p[1] for p in off]])
    cash = np.concatenate([on.cash, [p[2] for p in off]])
    ids = np.concatenate([on.id, np.zeros(len(off), dtype=np.int32)])
    cons = np.concatenate([on.cons, np.full(len(off), 0.75)])
    n = len(cash)
    w = b.rng.uniform(0.5, 2.0, n)
    cons[b.rng.choice(n, n // 7, replace=False)] = np.nan
    ids[b.rng.choice(n, n // 5, replace=False)] = -1
    w[b.rng.choice(n, n // 6, replace=False)] = 0.0
    return datafit.Observations(it, ist, cash, id=ids, cons=cons, w=w), len(on), len(off)


def run(s, obs, resid, fit=True):
    n = len(obs)
    cons, vf, ids = np.zeros((s.ndraw, n)), np.zeros((s.ndraw, n)), np.zeros((s.ndraw, n), dtype=np.int32)
    ssr, hits = np.zeros(s.ndraw), np.zeros(s.ndraw, dtype=np.int32)
    s.policy_batch(obs, resid=resid, cons_dev=cons.ctypes.data, id_dev=ids.ctypes.data, vf_dev=vf.ctypes.data,
                   ssr_dev=ssr.ctypes.data if fit else None, hits_dev=hits.ctypes.data if fit else None)
    return cons, ids, vf, ssr, hits


def compare(tag, got, tables, obs, call, t0, parts, resid, bad):
    cons, ids, vf, ssr, hits = got
    rc, ri, rv = datafit.policy_mirror(tables, obs, call=call, t0=t0)
    if not (bits_equal(cons, rc) and np.array_equal(ids, ri) and bits_equal(vf, rv)):
        bad.append('%s: predictions differ (cons %d, id %d, vf %d)' % (tag, (~((cons == rc) | (np.isnan(cons) & np.isnan(rc)))).sum(), (ids != ri).sum(),
                                                                   (~((vf == rv) | (np.isnan(vf) & np.isnan(rv)))).sum()))
    rs, rh = datafit.fit_mirror(obs, rc, ri, resid=resid, block=parts)
    if not bits_equal(ssr, rs) or hits != rh:
        bad.append('%s resid %d: ssr %r vs %r, hits %d vs %d' % (tag, resid, ssr, rs, hits, rh))
    return rs, rh


def refusals(s, obs, m):
    """every refusal of egdst_policy_batch: (answered EGDST_E_ARG with the observation's index in the message, tried)"""
    rec = obs.pack()
    k = len(rec) // 2
    n = len(rec)
    out = np.zeros((s.ndraw, n))
    cases = []
    for field, value in (('it', -1), ('it', s.nt), ('ist', -1), ('ist', s.lib.info.nst), ('id', -2), ('id', s.lib.info.nd), ('reserved', 1),
                         ('cash', np.nan), ('cash', np.nextafter(m.a0, -np.inf)), ('cash', -np.inf), ('w', np.nan), ('w', -1.0)):
        r = rec.copy()
        r[field][k] = value
        cases.append((r, 0, out.ctypes.data, 'observation %d:' % k))
    r = rec.copy()
    r['cons'][k] = 0.0
    cases += [(r, 1, out.ctypes.data, 'observation %d:' % k), (rec, 2, out.ctypes.data, 'resid'), (rec, -1, out.ctypes.data, 'resid'),
              (rec, 0, None, 'no output'), (rec[:0], 0, out.ctypes.data, '')]
    ok = 0
    for r, resid, ptr, word in cases:
        try:
            s.policy_batch(r, resid=resid, cons_dev=ptr, want=())
        except runtime.EgdstRuntimeError as e:
            ok += int(e.code == 1 and word in str(e))
    return ok, len(cases)


def continuous_refusal():
    """(code, message) of egdst_policy_batch on a solved handle of a model with a continuous state (retirement_hc, a small grid,
    the same harness build): the one refusal that takes a library of its own"""
    from egdst_amd import examples
    import build_emu
    mc = examples.retirement_hc(T=4, ngridm=20, ngridmax=100)
    san = os.environ.get('EMU_SANITIZE', '0')
    libc = runtime.ModelLibrary(build_emu.build(emu.write_modelspec(mc), {'0': False}.get(san, san), 1, False, 1))
    sc = runtime.Solver(libc, mc.descriptor(), ndraw=1, keep_history=True)
    sc.set_params(mc.param_vector())
    if sc.solve(raise_on_error=False) != 0:
        return -1, 'the model does not solve on the harness'
    out = np.zeros((1, 2))
    try:
        sc.policy_batch(datafit.Observations([0, 1], [0, 0], [mc.a0 + 1.0, mc.a0 + 2.0], cons=[0.5, 0.5]), cons_dev=out.ctypes.data)
    except runtime.EgdstRuntimeError as e:
        return e.code, str(e)
    return 0, 'accepted'


if __name__ == '__main__':
    b = emu.solved_batch()
    lib, s, st, m = b.lib, b.s, b.st, b.m
    bad = []
    parts = lib.policy_parts
    if parts != 1:
        bad.append('the harness library reports %d parts' % parts)
    sols = [b.orc.solve(p) for p in b.P]
    if sols[0].rc != 0:
        raise SystemExit('the oracle fails on draw 0')
    obs, n_on, n_off = observations(b, sols)
    nobs = len(obs)
    # the slices, from the arithmetic of the library
    cells = sorted(set(zip(obs.it.tolist(), obs.ist.tolist())))
    nslices = -(-NDRAW // max(1, min(NDRAW, flag('EG_POL_SLICE_BYTES', 1 << 30) // (12 * nobs))))
    if 'EG_POL_SLICE_BYTES' in os.environ.get('EMU_EXTRA_FLAGS', '') and nslices < 2:
        bad.append('EG_POL_SLICE_BYTES is set but the %d draws take %d slice' % (NDRAW, nslices))
    solved = finite = 0
    before = None
    for resid in (0, 1):
        got = run(s, obs, resid)
        before = got if resid == 0 else before
        for d in range(NDRAW):
            g = tuple(a[d] for a in got)
            if sols[d].rc != 0:
                if st[d] == 0 or not (np.isnan(g[0]).all() and (g[1] == -1).all() and np.isnan(g[2]).all() and np.isnan(g[3]) and g[4] == -1):
                    bad.append('draw %d: the oracle fails, device status %d' % (d, st[d]))
                continue
            solved += 1
            rs, rh = compare('draw %d' % d, g, sols[d], obs, lambda sw, a, d=d: b.orc.call(sols[d], sw, a, params=b.P[d]), m.t0, parts, resid, bad)
            finite += int(np.isfinite(rs) and rs > 0 and rh > 0)
        only = run(s, obs, resid, fit=False)   # the predictions alone are the same bits
        if not all(bits_equal(x, y) for x, y in zip(only[:3], got[:3])):
            bad.append('resid %d: the predictions without the fit differ' % resid)
    if solved < 2 * NDRAW or finite < 2:   # (the oracle solves all four draws of this case: every (draw, resid) pair is compared)
        bad.append('only %d solved (draw, resid) pairs, %d with a finite positive ssr and hits' % (solved, finite))
    # a solved draw with a missing cell: imported, draw 1 of a second handle loses a cell that observations stand in
    s2 = runtime.Solver(lib, m.descriptor(), ndraw=2, keep_history=True)
    s2.set_params(b.P[[0, 0]])
    hole = copy.deepcopy(sols[0])
    it_h, ist_h = int(obs.it[n_on // 2]), int(obs.ist[n_on // 2])
    hole.len[it_h, ist_h] = 0
    hole.thlen[it_h, ist_h] = 0
    s2.set_solution(sols[0], 0)
    s2.set_solution(hole, 1)
    call0 = lambda sw, a: b.orc.call(sols[0], sw, a, params=b.P[0])   # noqa: E731
    got = run(s2, obs, 0)
    compare('imported draw 0', tuple(a[0] for a in got), sols[0], obs, call0, m.t0, parts, 0, bad)
    rs, rh = compare('imported draw 1', tuple(a[1] for a in got), hole, obs, call0, m.t0, parts, 0, bad)
    in_hole = (obs.it == it_h) & (obs.ist == ist_h)
    if not (np.isnan(rs) and np.isnan(got[3][1]) and rh > 0 and (got[1][1][in_hole] == -1).all() and np.isnan(got[0][1][in_hole]).all()
            and in_hole.sum() > 0 and np.isfinite(got[3][0])):
        bad.append('the missing cell: ssr %r, hits %d' % (got[3][1], got[4][1]))
    ref_ok, ref_n = refusals(s, obs, m)
    again = run(s, obs, 0)   # against the resid-0 results taken BEFORE the refused calls
    if not all(bits_equal(x, y) for x, y in zip(again, before)):
        bad.append('the handle gives other bits after the refusals')
    cont_code, cont_msg = continuous_refusal()
    if cont_code != 1 or 'continuous' not in cont_msg:
        bad.append('a model with continuous states: code %d, %r' % (cont_code, cont_msg))
    ref_ok, ref_n = ref_ok + int(cont_code == 1 and 'continuous' in cont_msg), ref_n + 1
    print('policy: %d observations (%d on the panel, %d off it), draw status %s' % (nobs, n_on, n_off, list(st)))
    print('policy cells: %d  slices: %d' % (len(cells), nslices))
    print('policy refusals: %d of %d' % (ref_ok, ref_n))
    print('policy problems: %d %s' % (len(bad), bad[:3]))
