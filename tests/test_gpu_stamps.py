"""The clock-stamp builds (-DEGDST_STAMPS=<set>, egdst_device.h) on the GPU, one set on each side of the envelope step: the
set that stamps the segmented walk inside k_envelope and the walk set of the throughput path.  A stamp build computes what the
default build computes, its stamps land in the slots of its own set and nowhere else, and the record of a tripped guard
(egdst_get_debug) stays empty: the stamps have an array of their own."""
import numpy as np
import pytest

from egdst_amd import build, runtime, workloads

pytestmark = pytest.mark.gpu


def _model():
    # two choices, 300 grid points each: ~600 sorted points per cell, above 2 x ENV_SEG_MINPTS = 384, so walks are cut
    return workloads.c2(a0=0, ngridm=300, T=5)


# (model factory, extra hipcc flags): compiled in-tree by __graft_entry__.build(), like the variants of test_gpu_parity.py
BUILD_VARIANTS = [(lambda: _model()[0], ['-DEGDST_STAMPS=seg']), (lambda: _model()[0], ['-DEGDST_STAMPS=tpwalk'])]


def _solve(flags, P):
    m = _model()[0]
    lib = build.build_model(m, extra_flags=flags)
    s = runtime.Solver(lib, m.descriptor(), ndraw=len(P), keep_history=True)
    s.set_params(P)
    assert s.solve(raise_on_error=False) == 0
    return s


def _check(stamped, plain, ndraw, owner):
    assert np.array_equal(stamped.status()[0], plain.status()[0])
    total = {}
    for d in range(ndraw):
        assert np.array_equal(stamped.checksums(d), plain.checksums(d)), d   # M, C, V, TH, D of every cell
        assert not stamped.debug(d).any(), (d, stamped.debug(d).tolist())
        for name, v in stamped.stamps(d).items():
            total[name] = total.get(name, 0) + v
    print(total)
    mine = {k: v for k, v in total.items() if k.startswith(owner + '.')}
    assert mine and all(v > 0 for v in mine.values()), mine
    assert all(v == 0 for k, v in total.items() if k not in mine), total
    with pytest.raises(runtime.EgdstRuntimeError):
        plain.stamps(0)   # (the default build has no stamps, and says so)


def test_segmented_walk_stamps_in_k_envelope(monkeypatch):
    monkeypatch.setenv('EGDST_ENV_TP', '0')
    m = _model()[0]
    P = m.param_vector()[None]
    s, p = _solve(['-DEGDST_STAMPS=seg'], P), _solve([], P)
    merged, fallback = s.walk_stats()[0]
    assert merged >= 1, (merged, fallback)   # (at least one walk was cut and merged: every slot of the set has been stamped)
    _check(s, p, 1, 'seg')
    s.close(), p.close()


def test_throughput_path_walk_stamps(monkeypatch):
    monkeypatch.setenv('EGDST_ENV_TP', '1')   # (read when the handle is created)
    P = _model()[1](8)
    s, p = _solve(['-DEGDST_STAMPS=tpwalk'], P), _solve([], P)
    assert s.tp_stats()[:, 0].sum() > 0   # cells the throughput path completed
    _check(s, p, 8, 'tpwalk')
    s.close(), p.close()
