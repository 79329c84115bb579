"""Harness build, no sanitizer: the data panel attached to a handle and evaluated inside the solve (egdst_attach_panel,
egdst_fit_dev, egdst_get_fit) on the 4 perturbed occ3 draws of the estimation runners.  The observations are run_emu_policy's: the
oracle's panel of draw 0 and off-path points, some without consumption, some without a choice, some with weight 0.  The handle
keeps NO history (two ping-pong periods), with 1 and with 2 draw groups: per draw ssr and hits are held to datafit.fit_mirror with
the build's egdst_policy_parts() on datafit.policy_mirror's predictions from that draw's own oracle solution, for both residuals
(each a re-attach), over two solves enqueued back to back with the draws reversed in the second and one synchronisation at the
end; then the same numbers through the kept-history door egdst_policy_batch, a single observation, the lifetime of the fit (no
panel, no solve yet, an import, a detach) and every refusal, after which the handle fits with the bits it gave before.  Nothing
is preloaded."""
import os

import numpy as np
import estimation_emu as emu
from estimation_emu import NDRAW
from egdst_amd import datafit, runtime
from estimation_case import bits_equal
from run_emu_policy import observations


def mirror(b, sols, obs, resid, parts):
    """(ssr, hits) per draw from the oracle's solutions"""
    out = []
    for d in range(NDRAW):
        c, ids, _ = datafit.policy_mirror(sols[d], obs, call=lambda sw, a, d=d: b.orc.call(sols[d], sw, a, params=b.P[d]), t0=b.m.t0)
        out.append(datafit.fit_mirror(obs, c, ids, resid=resid, block=parts))
    return np.array([o[0] for o in out]), np.array([o[1] for o in out], dtype=np.int32)


def loop(s, chunks):
    """set_params_dev / solve_async / fit_dev per chunk into slices of its own, one sync at the end (the harness's "device" memory
    is host memory)"""
    ssr, hits = np.full((len(chunks), s.ndraw), -7.0), np.full((len(chunks), s.ndraw), -7, dtype=np.int32)
    for c, P in enumerate(chunks):
        s.set_params_dev(P.ctypes.data)
        s.solve_async()
        s.fit_dev(ssr[c].ctypes.data, hits[c].ctypes.data)
    rc = s.sync(raise_on_error=False)
    return ssr, hits, rc


def refused(call, code, word):
    try:
        call()
    except runtime.EgdstRuntimeError as e:
        return int(e.code == code and word in str(e))
    return 0


def refusals(s, obs, m):
    """every refusal of egdst_attach_panel: (answered EGDST_E_ARG with the observation's index or the argument named, tried)"""
    rec = obs.pack()
    k = len(rec) // 2
    cases = []
    for field, value in (('it', -1), ('it', s.nt), ('ist', -1), ('ist', s.lib.info.nst), ('id', -2), ('id', s.lib.info.nd), ('reserved', 1),
                         ('cash', np.nan), ('cash', np.nextafter(m.a0, -np.inf)), ('cash', -np.inf), ('w', np.nan), ('w', -1.0)):
        r = rec.copy()
        r[field][k] = value
        cases.append((r, 0, 'observation %d:' % k))
    r = rec.copy()
    r['cons'][k] = 0.0
    cases += [(r, 1, 'observation %d:' % k), (rec, 2, 'resid'), (rec, -1, 'resid'), (rec[:0], 0, '')]
    return sum(refused(lambda: s.attach_panel(r, resid=resid), 1, word) for r, resid, word in cases), len(cases)


def continuous_refusal():
    """egdst_attach_panel on a model with a continuous state (retirement_hc, the same harness build): refused, and says why"""
    from egdst_amd import examples
    import build_emu
    mc = examples.retirement_hc(T=4, ngridm=20, ngridmax=100)
    san = os.environ.get('EMU_SANITIZE', '0')
    libc = runtime.ModelLibrary(build_emu.build(emu.write_modelspec(mc), {'0': False}.get(san, san), 1, False, 1))
    sc = runtime.Solver(libc, mc.descriptor(), ndraw=1, keep_history=False)
    obs = datafit.Observations([0, 1], [0, 0], [mc.a0 + 1.0, mc.a0 + 2.0], cons=[0.5, 0.5])
    return refused(lambda: sc.attach_panel(obs), 1, 'continuous')


if __name__ == '__main__':
    b = emu.solved_batch()
    lib, m = b.lib, b.m
    bad = []
    parts = lib.policy_parts
    if parts != 1:
        bad.append('the harness library reports %d parts' % parts)
    sols = [b.orc.solve(p) for p in b.P]
    if any(sol.rc for sol in sols):
        raise SystemExit('the oracle fails on a draw')
    obs, n_on, n_off = observations(b, sols)
    chunks = [np.ascontiguousarray(b.P), np.ascontiguousarray(b.P[::-1])]
    compared = 0
    want = {}
    for resid in (0, 1):
        want[resid] = mirror(b, sols, obs, resid, parts)
        kept_ssr, kept_hits = np.zeros(NDRAW), np.zeros(NDRAW, dtype=np.int32)
        b.s.policy_batch(obs, resid=resid, ssr_dev=kept_ssr.ctypes.data, hits_dev=kept_hits.ctypes.data)   # (the kept-history door, solved with b.P)
        if not (bits_equal(kept_ssr, want[resid][0]) and np.array_equal(kept_hits, want[resid][1])):
            bad.append('resid %d: the kept-history door and the mirror differ' % resid)
    if not (np.isfinite(want[0][0]).all() and (want[0][1] > 0).all() and want[0][0][0] >= 0):
        bad.append('the mirror\'s fit is not finite: %r' % (want[0],))
    for groups in (1, 2):
        for keep in (False, True):
            s = runtime.Solver(lib, m.descriptor(), ndraw=NDRAW, keep_history=keep)
            s.set_groups(groups)
            for resid in (0, 1):
                s.attach_panel(obs, resid=resid)
                ssr, hits, rc = loop(s, chunks)
                ws, wh = want[resid]
                for c, rev in enumerate((False, True)):
                    es, eh = (ws[::-1], wh[::-1]) if rev else (ws, wh)
                    if rc or not (bits_equal(ssr[c], es) and np.array_equal(hits[c], eh)):
                        bad.append('groups %d history %d resid %d chunk %d: rc %d ssr %r vs %r, hits %r vs %r' % (groups, keep, resid, c, rc, ssr[c], es, hits[c], eh))
                    compared += NDRAW
                hs, hh = s.fit()   # the host form: the last solve's
                if not (bits_equal(hs, ws[::-1]) and np.array_equal(hh, wh[::-1])):
                    bad.append('groups %d history %d resid %d: egdst_get_fit differs' % (groups, keep, resid))
            s.close()
    # one observation (every period but one without a launch), lifetime and refusals on a handle without history
    s = runtime.Solver(lib, m.descriptor(), ndraw=NDRAW, keep_history=False)
    s.set_groups(2)
    out_s, out_h = np.zeros(NDRAW), np.zeros(NDRAW, dtype=np.int32)
    life = refused(lambda: s.fit_dev(out_s.ctypes.data, out_h.ctypes.data), 1, 'panel')
    one = datafit.Observations(obs.it[:1], obs.ist[:1], obs.cash[:1], id=obs.id[:1], cons=[0.75], w=[1.5])
    s.attach_panel(one)
    life += refused(lambda: s.fit_dev(out_s.ctypes.data, out_h.ctypes.data), 40, '')
    s.set_params(b.P)
    s.solve()
    w1 = mirror(b, sols, one, 0, parts)
    g1 = s.fit()
    if not (bits_equal(g1[0], w1[0]) and np.array_equal(g1[1], w1[1])):
        bad.append('one observation: %r vs %r' % (g1, w1))
    life += refused(lambda: s.fit_dev(None, None), 1, '')
    s.attach_panel(obs)
    s.solve()
    before = s.fit()
    if not (bits_equal(before[0], want[0][0]) and np.array_equal(before[1], want[0][1])):
        bad.append('after the re-attach: %r' % (before,))
    ref_ok, ref_n = refusals(s, obs, m)
    s.fit_dev(out_s.ctypes.data, None)   # (a refused attach keeps the panel and its fit)
    life += int(bits_equal(out_s, before[0]))
    s.solve()
    again = s.fit()
    if not (bits_equal(again[0], before[0]) and np.array_equal(again[1], before[1])):
        bad.append('the handle fits with other bits after the refusals')
    obj = s.objective()
    s.detach_panel()
    life += refused(lambda: s.fit(), 1, 'panel')
    s.solve()
    if not bits_equal(s.objective(), obj):
        bad.append('the objective after the detach differs')
    s.close()
    # an import: the kept-history handle has a fit, then a solution is imported
    k = runtime.Solver(lib, m.descriptor(), ndraw=NDRAW, keep_history=True)
    k.set_params(b.P)
    k.attach_panel(obs)
    k.solve()
    if not bits_equal(k.fit()[0], want[0][0]):
        bad.append('the kept-history handle\'s fit differs')
    k.set_solution(sols[0], 1)
    life += refused(lambda: k.fit(), 40, '')
    k.solve()
    if not bits_equal(k.fit()[0], want[0][0]):
        bad.append('the fit after the import and a solve differs')
    k.close()
    cont = continuous_refusal()
    print('attached: %d observations (%d on the panel, %d off it), %d (draw, chunk) pairs compared' % (len(obs), n_on, n_off, compared))
    print('attached lifetime: %d of 6' % life)
    print('attached refusals: %d of %d' % (ref_ok + cont, ref_n + 1))
    print('attached problems: %d %s' % (len(bad), bad[:3]))
