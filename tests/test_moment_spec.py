"""User-defined moments of the estimation step (egdst_simulate_batch_spec, egdst_amd/moments.py) without a GPU: the record
layout against the C compiler's, column names, validation, MomentSpec.evaluate against an independent masked computation,
and the kernels themselves under AddressSanitizer on the CPU harness (tests/cpu_emu)."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from egdst_amd import examples
from egdst_amd import moments as mo

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_record_layout_is_the_c_struct(tmp_path):
    src = tmp_path / 'layout.c'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "egdst.h"\nint main(void) {\n'
                   '    printf("%d", (int)sizeof(egdst_moment));\n' +
                   ''.join('    printf(" %%d", (int)offsetof(egdst_moment, %s));\n' % f for f in mo.MOMENT_DTYPE.names) +
                   '    return 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == mo.MOMENT_DTYPE.itemsize == 56
    assert out[1:] == [mo.MOMENT_DTYPE.fields[f][1] for f in mo.MOMENT_DTYPE.names]


@pytest.mark.parametrize('make', [examples.occ3, examples.retirement2, examples.retirement_hc])
def test_column_names_follow_the_simulator_labels(make):
    m = make()
    labels = m.make_simlabels()
    names = mo.columns(*mo._layout(m))
    assert len(names) == len(labels)
    for k, lab in enumerate(labels):   # '12 Human capital (st1)': the token in brackets, where the label has one
        if lab.endswith(')'):
            assert lab[lab.rindex('(') + 1:-1] == names[k], (k, lab)
    spec = mo.MomentSpec([mo.mean(n) for n in names] + [mo.share('id', 1, periods=3), mo.cross('C', 'eq1', periods=(2, 5), where=('st1', 0, 1))],
                         layout=m)
    rec = spec.pack(m.nt)
    assert list(rec['col'][:len(names)]) == list(range(len(names)))
    assert tuple(rec[-2])[:6] == (2, 4, 4, 3, 3, -1) and (rec[-2]['lo'], rec[-2]['hi']) == (1.0, 1.0)
    assert tuple(rec[-1])[:6] == (1, 1, names.index('eq1'), 2, 5, names.index('st1'))
    assert (rec[-1]['cond_lo'], rec[-1]['cond_hi']) == (0.0, 1.0)
    assert tuple(rec[0])[3:5] == (0, m.nt - 1)   # periods=None pools every period


def test_occ3_sector_shares_resolve():
    m = examples.occ3()
    rec = mo.MomentSpec([mo.share('id', k, periods=it) for it in range(m.nt) for k in range(3)], layout=m).pack(m.nt)
    assert np.all(rec['kind'] == 2) and np.all(rec['col'] == 4)
    assert np.array_equal(rec['lo'], np.tile([0.0, 1.0, 2.0], m.nt)) and np.array_equal(rec['lo'], rec['hi'])
    assert np.array_equal(rec['it_first'], np.repeat(np.arange(m.nt), 3)) and np.array_equal(rec['it_first'], rec['it_last'])


@pytest.mark.parametrize('item', [
    mo.mean('X'), mo.mean('st2'), mo.mean('eq4'), mo.mean(16), mo.mean(-1), mo.mean(2.0), mo.cross('C', 'nope'),
    mo.mean('C', periods=41), mo.mean('C', periods=-1), mo.mean('C', periods=(5, 4)), mo.mean('C', periods=(0, 41)),
    mo.mean('C', periods='all'), mo.mean('C', where=('id', 1)), mo.mean('C', where=('bad', 0, 1)),
    mo.mean('C', where=('id', 2, 1)), mo.share('id', 2, 1), mo.Moment(3, 'C'), 'C'])
def test_bad_moments_raise_before_the_library(item):
    m = examples.occ3()   # nout 16, nt 41
    with pytest.raises(ValueError):
        mo.MomentSpec([item], layout=m).pack(m.nt)


def test_empty_spec_and_missing_layout_raise():
    with pytest.raises(ValueError):
        mo.MomentSpec([], layout=(0, 1, 0)).pack(5)
    with pytest.raises(ValueError):
        mo.MomentSpec([mo.mean('st1')]).pack(5)
    assert mo.MomentSpec([mo.mean('C'), mo.mean(12)]).pack(5)['col'].tolist() == [1, 12]   # base tokens and indices need none
    with pytest.raises(ValueError):   # the panel has fewer columns than the index
        mo.MomentSpec([mo.mean(12)]).evaluate(np.zeros((3, 5, 12)))


def _panel(seed, nsim, nt, nout, holes=0.2):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(nsim, nt, nout)) * rng.uniform(0.1, 100, nout)
    x[..., 4] = rng.integers(0, 3, (nsim, nt))
    x[rng.random((nsim, nt, nout)) < holes] = np.nan
    dead = rng.integers(0, nt + 1, nsim)                    # agents that leave the panel: NaN from then on
    x[np.arange(nt)[None, :] >= dead[:, None]] = np.nan
    return x


def _masked(sims, q):
    """independent: moment q of the panel by masks and np.mean"""
    f, l_ = int(q['it_first']), int(q['it_last']) + 1
    v = sims[:, f:l_, q['col']]
    ok = ~np.isnan(v)
    if q['cond_col'] >= 0:
        c = sims[:, f:l_, q['cond_col']]
        with np.errstate(invalid='ignore'):
            ok &= (c >= q['cond_lo']) & (c <= q['cond_hi'])
    if q['kind'] == 1:
        v = v * sims[:, f:l_, q['col2']]
        ok &= ~np.isnan(v)
    elif q['kind'] == 2:
        v = ((v >= q['lo']) & (v <= q['hi'])).astype(float)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return (np.mean(v[ok]) if ok.any() else np.nan), int(ok.sum())


@pytest.mark.parametrize('seed,nsim', [(1, 1), (2, 255), (3, 700), (4, 1000)])
def test_evaluate_agrees_with_a_masked_computation(seed, nsim):
    nt, nout = 9, 14
    sims = _panel(seed, nsim, nt, nout)
    items = [mo.mean(c, periods=it) for it in range(nt) for c in (0, 1, 13)]
    items += [mo.share('id', k, periods=(2, 6)) for k in range(3)] + [mo.share(1, -0.5, 0.5)]
    items += [mo.mean('C', where=('id', k, k)) for k in range(3)] + [mo.cross('M', 'C'), mo.cross('M', 'M', periods=(0, 4))]
    items += [mo.mean(12, periods=(3, 8), where=('A', -10, 10)), mo.cross('V', 'u', periods=8, where=(11, 0, 1e9))]
    spec = mo.MomentSpec(items, layout=(1, 1, 1))
    rec = spec.pack(nt)
    for block in (1, 256, 64):
        means, counts = spec.evaluate(sims, block=block)
        for j, q in enumerate(rec):
            rm, rc = _masked(sims, q)
            assert counts[j] == rc, (block, j)
            assert np.isnan(means[j]) == np.isnan(rm), (block, j)
            if rc:
                assert abs(means[j] - rm) <= 1e-13 * max(1.0, abs(rm)), (block, j, means[j], rm)


def test_evaluate_is_the_per_period_cell_sum_order():
    """a kind-0 moment of one period is the k_moments order: per thread t the agents t, t+B, ... then the tree"""
    sims = _panel(9, 600, 3, 12)
    spec = mo.MomentSpec([mo.mean(0, periods=1)])
    v = sims[:, 1, 0]
    p = np.zeros(256)
    for t in range(256):
        acc = 0.0
        for i in range(t, 600, 256):
            if v[i] == v[i]:
                acc += v[i]
        p[t] = acc
    o = 128
    while o:
        for t in range(o):
            p[t] += p[t + o]
        o //= 2
    n = int((~np.isnan(v)).sum())
    means, counts = spec.evaluate(sims)
    assert counts[0] == n and means[0] == p[0] / n


def test_objective_order_and_empty_moments():
    rng = np.random.default_rng(0)
    n = 7
    means, target = rng.normal(size=n), rng.normal(size=n)
    counts = np.full(n, 5)
    w = rng.uniform(0, 2, n)
    w[2] = 0
    e = means - target
    acc = 0.0
    for k in range(n):   # k_moment_objective with a diagonal: weight * e * e in cell order
        if w[k] != 0:
            acc += w[k] * e[k] * e[k]
    assert mo.objective(means, counts, target, w) == acc      # a vector is the diagonal: the same bits
    A = rng.normal(size=(n, n))
    W = A @ A.T
    W[3, :] = W[:, 3] = 0
    ref = 0.0
    for j in range(n):
        if W[j].any():
            r = 0.0
            for k in range(n):
                if W[j, k] != 0:
                    r += W[j, k] * e[k]
            ref += e[j] * r
    assert mo.objective(means, counts, target, W) == ref
    c = counts.copy()
    c[3] = 0          # untouched by W: no effect
    assert mo.objective(means, c, target, W) == ref
    c[4] = 0
    assert np.isnan(mo.objective(means, c, target, W))
    with pytest.raises(ValueError):
        mo.objective(means, counts, target, np.eye(n + 1))


def _asan():
    r = subprocess.run(['gcc', '-print-file-name=libasan.so'], capture_output=True, text=True)
    p = r.stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.mark.skipif(_asan() is None, reason='libasan not found')
def test_moment_spec_kernels_under_asan():
    """egdst_simulate_batch_spec under ASan: occ3 draws, every moment kind, a full W -- means and counts bit-equal to
    MomentSpec.evaluate(block=1) on the oracle's paths for the same uniforms, the objective bit-equal to moments.objective,
    malformed records refused with code 1."""
    env = dict(os.environ, LD_PRELOAD=_asan(), ASAN_OPTIONS='detect_leaks=0', EMU_SANITIZE='address')
    r = subprocess.run([sys.executable, os.path.join(HERE, 'cpu_emu', 'run_emu_moment_spec.py')], env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'moment spec problems: 0' in r.stdout, r.stdout + r.stderr[-2000:]
    assert 'ERROR: AddressSanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-3000:]
