"""Moments across two periods (egdst_moment_lag, egdst_amd/moments.py) without a GPU: the record layout against the C
compiler's, pack_lag and the periods=None rule, every refusal, and MomentSpec.evaluate against a brute-force evaluation
written out here in the contract's order (include/egdst.h) -- plain loops over partial, agent and period."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from egdst_amd import moments as mo

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INF = float('inf')
LAYOUT = (1, 1, 3)   # nout = 16
NSIM, NT = 23, 6


def test_lag_record_layout_is_the_c_struct(tmp_path):
    src = tmp_path / 'layout.c'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "egdst.h"\nint main(void) {\n'
                   '    printf("%d %d", (int)sizeof(egdst_moment_lag), (int)sizeof(egdst_moment));\n' +
                   ''.join('    printf(" %%d", (int)offsetof(egdst_moment_lag, %s));\n' % f for f in mo.MOMENT_LAG_DTYPE.names) +
                   '    return 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == mo.MOMENT_LAG_DTYPE.itemsize == 64 and out[1] == mo.MOMENT_DTYPE.itemsize == 56
    assert out[2:] == [mo.MOMENT_LAG_DTYPE.fields[f][1] for f in mo.MOMENT_LAG_DTYPE.names]
    assert mo.MOMENT_LAG_DTYPE.names == mo.MOMENT_DTYPE.names + ('lag2', 'cond_lag')
    for f in mo.MOMENT_DTYPE.names:   # the first 56 bytes are egdst_moment
        assert mo.MOMENT_LAG_DTYPE.fields[f] == mo.MOMENT_DTYPE.fields[f]


def test_pack_lag_fields_and_the_pooled_period_range():
    nt = 10
    spec = mo.MomentSpec([mo.cross('C', 'M', lag=1), mo.cross('C', 'M', lag=-2), mo.cross('M', 'M', periods=nt - 1, lag=nt - 1),
                          mo.mean('C', where=('id', 1, 2, 3)), mo.mean('C', where=('id', 1, 2, -1)),
                          mo.cross('A', 'V', lag=2, where=('id', 0, 0, -3)), mo.transition('id', 0, 2), mo.transition('id', 2, 1, periods=4, lag=3),
                          mo.quantile('C', 0.9, periods=(4, 6), where=('id', 1, 2, 2)), mo.cross('M', 'C', periods=(3, 7), lag=-1),
                          mo.mean('C'), mo.mean('C', where=('id', 1, 1, 0))], layout=LAYOUT)
    assert spec.lagged
    rec = spec.pack_lag(nt)
    assert rec.dtype == mo.MOMENT_LAG_DTYPE
    first, last = list(rec['it_first']), list(rec['it_last'])
    # periods=None: first = max(0, lags in use), last = nt - 1 + min(0, lags in use)
    assert (first[0], last[0]) == (1, 9) and (first[1], last[1]) == (0, 7) and (first[2], last[2]) == (9, 9)
    assert (first[3], last[3]) == (3, 9) and (first[4], last[4]) == (0, 8) and (first[5], last[5]) == (2, 6)
    assert (first[6], last[6]) == (1, 9) and (first[7], last[7]) == (4, 4) and (first[8], last[8]) == (4, 6)
    assert (first[9], last[9]) == (3, 7) and (first[10], last[10]) == (0, 9) and (first[11], last[11]) == (0, 9)
    assert list(rec['lag2']) == [1, -2, 9, 0, 0, 2, 0, 0, 0, -1, 0, 0]
    assert list(rec['cond_lag']) == [0, 0, 0, 3, -1, -3, 1, 3, 2, 0, 0, 0]
    # a transition is the share of `to` among those at `frm` lag periods before
    assert tuple(rec[6])[:6] == (mo.SHARE, 4, 4, 1, 9, 4) and tuple(rec[6])[6:] == (2.0, 2.0, 0.0, 0.0, 0, 1)
    assert tuple(rec[7])[:6] == (mo.SHARE, 4, 4, 4, 4, 4) and tuple(rec[7])[6:] == (1.0, 1.0, 2.0, 2.0, 0, 3)
    assert tuple(rec[5])[:3] == (mo.CROSS, 2, 3) and tuple(rec[8])[:3] == (mo.QUANTILE, 1, 1)


def test_pack_refuses_a_lagged_spec_and_names_pack_lag():
    for item in (mo.cross('C', 'M', lag=1), mo.mean('C', where=('id', 0, 0, -1)), mo.transition('id', 0, 1)):
        spec = mo.MomentSpec([mo.mean('C'), item], layout=LAYOUT)
        assert spec.lagged
        with pytest.raises(ValueError, match='pack_lag'):
            spec.pack(NT)
        assert len(spec.pack_lag(NT)) == 2


def test_a_spec_without_lags_packs_the_same_either_way():
    spec = mo.MomentSpec([mo.mean('C'), mo.cross('M', 'C', periods=(1, 3), where=('st1', 0, 1)), mo.share('id', 1, periods=2),
                          mo.quantile('A', 0.25, where=('id', 1, 2, 0)), mo.cross('C', 'C', lag=0)], layout=LAYOUT)
    assert not spec.lagged and not mo.MomentSpec([], layout=LAYOUT).lagged
    a, b = spec.pack(NT), spec.pack_lag(NT)
    assert a.dtype == mo.MOMENT_DTYPE and b.dtype == mo.MOMENT_LAG_DTYPE
    for f in mo.MOMENT_DTYPE.names:
        assert np.array_equal(a[f], b[f]), f
    assert a.tobytes() == b''.join(r.tobytes()[:56] for r in b)
    assert not b['lag2'].any() and not b['cond_lag'].any()


def _plain_and_lagged():
    plain = mo.MomentSpec([mo.mean('C'), mo.cross('M', 'C', periods=(1, 3), where=('st1', 0, 1)), mo.share('id', 1, periods=2),
                           mo.quantile('A', 0.25, where=('id', 1, 2))], layout=LAYOUT)
    return plain, mo.MomentSpec(plain + [mo.cross('C', 'C', lag=1), mo.transition('id', 0, 1)], layout=LAYOUT)


@pytest.mark.parametrize('form', ['spec', 'lagged spec', 'MOMENT_DTYPE', 'MOMENT_LAG_DTYPE', 'list of tuples'])
def test_lag_records_of_what_a_caller_may_pass(form):
    """lag_records: the records, byte for byte those of pack / pack_lag, and the entry they need -- the one that takes
    egdst_moment_lag for a spec with a lag and for an array of MOMENT_LAG_DTYPE (zero lags or not), the other one otherwise"""
    plain, lagged = _plain_and_lagged()
    given, want, door = {'spec': (plain, plain.pack_lag(NT), False),
                         'lagged spec': (lagged, lagged.pack_lag(NT), True),
                         'MOMENT_DTYPE': (plain.pack(NT), plain.pack_lag(NT), False),
                         'MOMENT_LAG_DTYPE': (plain.pack_lag(NT), plain.pack_lag(NT), True),
                         'list of tuples': ([tuple(r) for r in plain.pack(NT)], plain.pack_lag(NT), False)}[form]
    rec, lag = mo.lag_records(given, NT, layout=LAYOUT)
    assert lag is door
    assert rec.dtype == mo.MOMENT_LAG_DTYPE and rec.flags['C_CONTIGUOUS'] and rec.shape == (len(want),)
    assert rec.tobytes() == want.tobytes()
    if not door:   # what the entry without lags is sent
        narrow = mo.convert_records(rec, mo.MOMENT_DTYPE)
        assert narrow.dtype == mo.MOMENT_DTYPE and narrow.tobytes() == plain.pack(NT).tobytes()


def test_convert_records_widens_with_zero_lags_and_refuses_to_drop_a_lag():
    plain, lagged = _plain_and_lagged()
    a, b = plain.pack(NT), plain.pack_lag(NT)
    assert mo.convert_records(a, mo.MOMENT_LAG_DTYPE).tobytes() == b.tobytes()
    assert mo.convert_records(b, mo.MOMENT_DTYPE).tobytes() == a.tobytes()
    assert mo.convert_records(a, mo.MOMENT_DTYPE).tobytes() == a.tobytes() and mo.convert_records(b[::-1], mo.MOMENT_LAG_DTYPE).flags['C_CONTIGUOUS']
    for field in ('lag2', 'cond_lag'):
        r = b.copy()
        r[field][len(r) - 1] = -1
        with pytest.raises(ValueError, match='lag'):
            mo.convert_records(r, mo.MOMENT_DTYPE)
    with pytest.raises(ValueError, match='lag'):
        mo.convert_records(lagged.pack_lag(NT), mo.MOMENT_DTYPE)


@pytest.mark.parametrize('item', [
    mo.Moment(mo.MEAN, 'C', lag=1), mo.Moment(mo.SHARE, 'id', lo=1.0, hi=1.0, lag=-1), mo.Moment(mo.QUANTILE, 'C', lo=0.5, lag=2),
    mo.cross('C', 'M', lag=NT), mo.cross('C', 'M', lag=-NT), mo.mean('C', where=('id', 0, 0, NT)),
    mo.cross('C', 'M', lag=3, where=('id', 0, 0, -3)),                                    # nothing between first 3 and last 2
    mo.cross('C', 'M', periods=0, lag=1), mo.cross('C', 'M', periods=(0, NT - 1), lag=-1), mo.cross('C', 'M', periods=NT - 1, lag=-1),
    mo.mean('C', periods=(0, 3), where=('id', 0, 0, 1)), mo.mean('C', periods=(2, NT - 1), where=('id', 0, 0, -1)),
    mo.transition('id', 0, 1, periods=0), mo.transition('id', 0, 1, periods=1, lag=2),
    mo.cross('C', 'M', lag=2 ** 31), mo.cross('C', 'M', periods=2, lag=-2 ** 31), mo.mean('C', periods=3, where=('id', 0, 0, 2 ** 40)),
    mo.cross('C', 'M', lag=1.0), mo.cross('C', 'M', lag=True), mo.cross('C', 'M', lag='1'), mo.mean('C', where=('id', 0, 0, 0.5)),
    mo.mean('C', where=('id', 0, 0, 1, 1)), mo.mean('C', where=('id', 1, 0, 1)), mo.mean('C', where=('bad', 0, 0, 1))])
def test_bad_lags_raise_before_the_library(item):
    spec = mo.MomentSpec([item], layout=LAYOUT)
    with pytest.raises(ValueError):
        spec.pack_lag(NT)
    with pytest.raises(ValueError):
        spec.evaluate(np.zeros((3, NT, 16)))


# ---- evaluate against plain loops ----

def _panel():
    """23 agents, 6 periods, 16 columns: values with ties, both zeros and both infinities; agent 4 is NaN everywhere, agent 9
    from period 3 on, agent 15 in period 2 only"""
    rng = np.random.default_rng(12)
    sims = np.full((NSIM, NT, 16), np.nan)
    sims[:, :, 0] = np.round(rng.normal(2, 2, (NSIM, NT)) * 2) / 2          # M: halves, many ties, both signs
    sims[:, :, 1] = np.round(rng.uniform(0, 3, (NSIM, NT)) * 4) / 4         # C: quarters
    sims[:, :, 2] = sims[:, :, 0] - sims[:, :, 1]                            # A
    sims[:, :, 3] = rng.normal(0, 5, (NSIM, NT))                             # V
    sims[:, :, 4] = rng.integers(0, 3, (NSIM, NT))                           # id
    sims[:, :, 5] = 1.0
    sims[:, :, 11] = rng.integers(0, 2, (NSIM, NT))                          # st1
    sims[2, 1, 0], sims[3, 1, 0], sims[2, 4, 1], sims[7, 0, 1], sims[11, 5, 1] = 0.0, -0.0, -0.0, 0.0, -0.0
    sims[5, 2, 3], sims[6, 3, 3], sims[12, 0, 3], sims[13, 5, 3], sims[20, 4, 3] = INF, -INF, -INF, INF, INF
    sims[4] = np.nan
    sims[9, 3:] = np.nan
    sims[15, 2] = np.nan
    return sims


def _spec():
    return mo.MomentSpec([
        mo.cross('C', 'M', lag=1), mo.cross('C', 'M', lag=-1), mo.cross('M', 'M', periods=NT - 1, lag=NT - 1),   # (lag nt - 1)
        mo.cross('C', 'C', lag=-2, where=('id', 0, 1, 1)), mo.cross('A', 'C', periods=(2, 4), lag=2, where=('st1', 1, 1, -1)),
        mo.mean('C', where=('id', 1, 1, 1)), mo.mean('C', where=('id', 1, 2, -1)), mo.mean('M', periods=(2, 4), where=('V', -INF, INF, 2)),
        mo.mean('C', periods=(0, NT - 2), where=('C', -INF, INF, -1)),                              # survivors into the next period
        mo.share('id', 1, periods=0, where=('V', -INF, 0.0, -(NT - 1))), mo.share('M', 0.0, 2.0, where=('id', 2, 2, 2)),
        mo.transition('id', 0, 1), mo.transition('id', 1, 0, periods=3), mo.transition('id', 2, 2, lag=2), mo.transition('id', 0, 0, lag=-1),
        mo.quantile('C', 0.5, where=('id', 0, 1, 1)), mo.quantile('V', 0.9, periods=(1, 3), where=('C', -INF, INF, -2)),
        mo.median('M', periods=4, where=('id', 1, 1, 1)), mo.quantile('V', 0.05, where=('V', -INF, INF, 3)),
        mo.mean('C', where=('id', 9, 9, 1)), mo.median('C', where=('id', 9, 9, -1)),                # nothing satisfies these
        mo.mean('C'), mo.share('id', 1, periods=2), mo.median('M'), mo.cross('M', 'C', where=('id', 0, 1))], layout=LAYOUT)


def _bits(x):
    return struct.unpack('<Q', struct.pack('<d', x))[0]


def _key(x):
    u = _bits(x)
    return (~u) & (2 ** 64 - 1) if u >> 63 else u | (1 << 63)


def brute_force(sims, rec, block):
    """the definition of include/egdst.h in plain loops: partial t adds the agents i = t (mod block) ascending, within an
    agent the periods ascending; then the tree over the partials.  A quantile sorts the keys of the qualifying values."""
    means, counts = [], []
    for q in rec:
        kind, col, col2, cc = int(q['kind']), int(q['col']), int(q['col2']), int(q['cond_col'])
        part = [0.0] * block
        n = 0
        values = []
        for t in range(block):
            for i in range(t, len(sims), block):
                for it in range(int(q['it_first']), int(q['it_last']) + 1):
                    v = float(sims[i][it][col])
                    if math.isnan(v):
                        continue
                    if cc >= 0:
                        c = float(sims[i][it - int(q['cond_lag'])][cc])
                        if not (float(q['cond_lo']) <= c <= float(q['cond_hi'])):
                            continue
                    x = v
                    if kind == 1:
                        w = float(sims[i][it - int(q['lag2'])][col2])
                        if math.isnan(w):
                            continue
                        x = np.float64(v) * np.float64(w)
                    elif kind == 2:
                        x = 1.0 if float(q['lo']) <= v <= float(q['hi']) else 0.0
                    n += 1
                    if kind == 3:
                        values.append(v)
                    else:
                        part[t] = float(np.float64(part[t]) + np.float64(x))
        counts.append(n)
        if n == 0:
            means.append(float('nan'))
        elif kind == 3:
            t_ = float(q['lo']) * float(n)
            k = min(max(int(math.ceil(t_)), 1), n)
            means.append(sorted(values, key=_key)[k - 1])
        else:
            o = block // 2
            while o > 0:
                for t in range(o):
                    part[t] = float(np.float64(part[t]) + np.float64(part[t + o]))
                o //= 2
            means.append(float(np.float64(part[0]) / np.float64(n)))
    return means, counts


@pytest.mark.parametrize('block', [1, 4, 256])
def test_evaluate_is_the_brute_force_in_the_contract_order(block):
    sims, spec = _panel(), _spec()
    assert np.isnan(sims[4]).all() and np.isnan(sims[9, 3:]).all() and not np.isnan(sims[9, :3, :5]).any()
    assert np.isnan(sims[15, 2]).all() and not np.isnan(sims[15, [1, 3], :5]).any()
    rec = spec.pack_lag(NT)
    assert (rec['lag2'] > 0).any() and (rec['lag2'] < 0).any() and (rec['cond_lag'] > 0).any() and (rec['cond_lag'] < 0).any()
    assert (np.abs(rec['lag2']) == NT - 1).any() and (np.abs(rec['cond_lag']) == NT - 1).any()
    assert ((rec['kind'] == 3) & (rec['cond_lag'] != 0)).any()
    with np.errstate(invalid='ignore', over='ignore'):
        want_m, want_c = brute_force(sims, rec, block)
    got_m, got_c = spec.evaluate(sims, block=block)
    assert [int(c) for c in got_c] == want_c
    for j, (g, w) in enumerate(zip(got_m, want_m)):
        if want_c[j] == 0 or math.isnan(w):
            assert math.isnan(g), j
        else:
            assert _bits(float(g)) == _bits(w), (j, g, w)
    empty = [j for j, c in enumerate(want_c) if c == 0]
    assert empty == [19, 20]
    # the lags do something: the condition of record 8 meets the NaNs of agents 9 (dead from 3) and 15 (period 2), and the
    # unlagged counterpart of a lagged record counts other pairs
    present = sum(1 for i in range(NSIM) for it in range(NT - 1) if not math.isnan(sims[i, it, 1]))
    assert want_c[8] == present - 2 and want_c[0] < want_c[21]
    # values: both zeros and an infinity are picked by some quantile's population, and the sums are not all NaN
    assert sum(1 for j, w in enumerate(want_m) if want_c[j] and not math.isnan(w)) >= len(rec) - 4


def test_zero_lag_records_evaluate_as_before():
    """the same moments with and without explicit zero lags: the same bits"""
    sims = _panel()
    a = mo.MomentSpec([mo.cross('C', 'M'), mo.mean('C', where=('id', 1, 1)), mo.median('V', where=('id', 0, 1))], layout=LAYOUT)
    b = mo.MomentSpec([mo.cross('C', 'M', lag=0), mo.mean('C', where=('id', 1, 1, 0)), mo.median('V', where=('id', 0, 1, 0))], layout=LAYOUT)
    (ma, ca), (mb, cb) = a.evaluate(sims), b.evaluate(sims)
    assert np.array_equal(ca, cb) and ma.tobytes() == mb.tobytes() and (ca > 0).all()
