"""The host side of the fit to micro data (egdst_amd/datafit.py), without a GPU: the policy mirror against the reference
simulator's own policy() -- every present (agent, period) pair of the oracle's panels must reproduce the panel's consumption,
choice and value bit for bit -- the fit mirror against a plain loop in the contract's summation order, and the record layout."""
import ctypes
import functools
import math

import numpy as np
import pytest

from egdst_amd import datafit, examples
from oracle_harness import Oracle
from estimation_case import bits_equal, uniforms

MODELS = {
    'occ3': (lambda: examples.occ3(T=6, ngridm=30, ngridmax=100), 48, 0.0),   # (the small case of tests/cpu_emu/estimation_emu.py)
    'retirement_mortal': (lambda: examples.retirement_mortal(), 300, 0.5),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    make, nsim, off = MODELS[name]
    m = make()
    orc = Oracle(m)
    sol = orc.solve()
    assert sol.rc == 0
    rng = np.random.default_rng(12)
    init = np.column_stack([np.ones(nsim), rng.uniform(m.a0 - off, m.mmax + off, nsim)])
    panel = orc.sim(sol, init, uniforms(9, 4 * m.nt * nsim), rndtype=0)
    return m, orc, sol, panel


@pytest.mark.parametrize('name', list(MODELS))
def test_policy_mirror_is_the_simulators_policy(name):
    """policy_mirror at (period, state of column 5, cash of column 0) of every present pair equals columns 1 (C), 4 (id) and 3
    (vf) of the oracle's panel, which the reference's simulator fills from the same policy()"""
    m, orc, sol, panel = _case(name)
    obs = datafit.Observations.from_panel(panel, m)
    present = ~np.isnan(panel[:, :, 0])
    assert len(obs) == present.sum() > 200
    c, ids, vf = datafit.policy_mirror(sol, obs, call=lambda sw, a: orc.call(sol, sw, a), t0=m.t0)
    rows = panel[present]   # (agent order, within an agent period order: from_panel's)
    assert bits_equal(obs.cash, rows[:, 0]) and np.array_equal(obs.ist, rows[:, 5].astype(np.int32))
    assert bits_equal(c, rows[:, 1])
    assert np.array_equal(ids, rows[:, 4].astype(np.int32))
    assert bits_equal(vf, rows[:, 3])
    # what the case exercises: points below the first endogenous point (the value there is u(c) + discount V[0]) and above it
    first = np.array([sol.M[it, ist, 1] for it, ist in zip(obs.it, obs.ist)])
    assert (obs.cash < first).any() and (obs.cash >= first).any()
    if name == 'occ3':
        assert (obs.cash > m.mmax).any() and len(set(ids.tolist())) > 1   # (agents grow past mmax: the tables are extrapolated)
    else:
        assert np.isnan(panel[:, :, 0]).any()   # (agents that die, and agents that never have a value)


def _loop(rec, cons, ids, resid, block):
    """ssr and hits as the contract words them, one observation at a time"""
    p = [0.0] * block
    hits, missing = 0, False
    for k in range(len(rec)):
        if ids[k] < 0:
            missing = True
            continue
        if rec['id'][k] >= 0 and rec['id'][k] == ids[k]:
            hits += 1
        if math.isnan(rec['cons'][k]) or rec['w'][k] == 0.0:
            continue
        if resid:
            r = float(datafit.host_log(np.array([rec['cons'][k]]))[0]) - float(datafit.host_log(np.array([cons[k]]))[0])
        else:
            r = float(rec['cons'][k]) - float(cons[k])
        rr = r * r
        p[k % block] = p[k % block] + float(rec['w'][k]) * rr
    o = block // 2
    while o >= 1:
        for t in range(o):
            p[t] = p[t] + p[t + o]
        o //= 2
    return (math.nan if missing else p[0]), hits


@pytest.mark.parametrize('resid', [0, 1])
@pytest.mark.parametrize('nobs', [1, 255, 256, 257, 700])
def test_fit_mirror_against_a_plain_loop(nobs, resid):
    rng = np.random.default_rng(100 + nobs)
    obs = datafit.Observations(rng.integers(0, 5, nobs), rng.integers(0, 3, nobs), rng.uniform(0, 5, nobs), id=rng.integers(-1, 3, nobs),
                               cons=rng.uniform(0.1, 3, nobs), w=rng.uniform(0.1, 2, nobs))
    if nobs > 1:
        obs.cons[rng.choice(nobs, nobs // 6, replace=False)] = np.nan
        obs.w[rng.choice(nobs, nobs // 5, replace=False)] = 0.0
    rec = obs.pack()
    cons = rng.uniform(0.1, 3, nobs)
    ids = rng.integers(0, 3, nobs).astype(np.int32)
    for block in (256, 4, 1):
        ssr, hits = datafit.fit_mirror(obs, cons, ids, resid=resid, block=block)
        want = _loop(rec, cons, ids, resid, block)
        assert bits_equal(ssr, want[0]) and hits == want[1], (block, ssr, want)
    assert nobs == 1 or (ssr > 0 and 0 < hits < nobs)
    # an observation without a policy makes ssr NaN and leaves the other hits; a failed draw is (NaN, -1)
    ids[0] = -1
    ssr2, hits2 = datafit.fit_mirror(obs, cons, ids, resid=resid, block=256)
    assert math.isnan(ssr2) and (hits2, ) == _loop(rec, cons, ids, resid, 256)[1:]
    assert datafit.fit_mirror(obs, cons, ids, resid=resid, failed=True) == pytest.approx((math.nan, -1), nan_ok=True)


def test_records_are_40_bytes():
    class Obs(ctypes.Structure):   # egdst_obs of include/egdst.h
        _fields_ = [('it', ctypes.c_int), ('ist', ctypes.c_int), ('id', ctypes.c_int), ('reserved', ctypes.c_int),
                    ('cash', ctypes.c_double), ('cons', ctypes.c_double), ('w', ctypes.c_double)]
    assert ctypes.sizeof(Obs) == 40 == datafit.OBS_DTYPE.itemsize
    for f in datafit.OBS_DTYPE.names:
        assert datafit.OBS_DTYPE.fields[f][1] == getattr(Obs, f).offset
    rec = datafit.Observations([1, 2], [0, 1], [0.5, 1.5], id=[1, -1], cons=[0.25, np.nan]).pack()
    assert rec.dtype == datafit.OBS_DTYPE and rec.nbytes == 80 and rec.flags['C_CONTIGUOUS']
    assert (rec['reserved'] == 0).all() and rec['id'].tolist() == [1, -1] and rec['w'].tolist() == [1.0, 1.0] and np.isnan(rec['cons'][1])
