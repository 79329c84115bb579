"""bench.py --dump-outputs: the arrays of the last timed step as finite float64 .npy files, a fixed sample of the draws when
they exceed the size limit."""
import os

import numpy as np

import bench


def _chunks(n, nchunks):
    rng = np.random.default_rng(3)
    st = rng.integers(0, 3, n).astype(np.int32)
    wh = rng.integers(0, 9, (n, 2)).astype(np.int32)
    ev = rng.integers(0, 1 << 40, n)
    cr = rng.integers(0, 1 << 20, n)
    parts = np.array_split(np.arange(n), nchunks)
    return [(st[p], wh[p], ev[p], cr[p]) for p in parts], (st, wh, ev, cr)


def test_every_draw_in_order_as_float64(tmp_path):
    chunks, (st, wh, ev, cr) = _chunks(100, 3)
    obj = np.random.default_rng(4).random((100, 2))
    obj[st != 0] = np.nan                 # (the solver's objective of a failed draw)
    bench.dump_outputs(str(tmp_path), obj, chunks, 0, 1)
    assert sorted(os.listdir(tmp_path)) == ['evals.npy', 'evals_credited.npy', 'objective.npy', 'status.npy', 'status_where.npy']
    assert 0 < (st != 0).sum() < len(st)
    for name, want in (('objective', np.where(np.isnan(obj), 0.0, obj)), ('status', st), ('status_where', wh), ('evals', ev), ('evals_credited', cr)):
        a = np.load(tmp_path / (name + '.npy'))
        assert a.dtype == np.float64 and a.shape == want.shape and np.all(np.isfinite(a)), name
        assert np.array_equal(a, want.astype(np.float64)), name


def test_a_large_batch_is_a_fixed_sample_within_the_limit(tmp_path):
    n, limit = 5000, 64 * 1000
    chunks, (st, _, ev, _) = _chunks(n, 4)
    obj = np.random.default_rng(5).random((n, 2))
    obj[st != 0] = np.nan
    for d, rank in (('a', 1), ('b', 1)):
        bench.dump_outputs(str(tmp_path / d), obj, chunks, rank, 2, limit=limit)
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == sorted(f + '_rank1.npy' for f in ('draw_index', 'evals', 'evals_credited', 'objective', 'status', 'status_where'))
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in files) <= limit // 2 + 128 * len(files)   # (+ the .npy headers)
    for f in files:
        assert np.array_equal(np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f))
    idx = np.load(tmp_path / 'a' / 'draw_index_rank1.npy').astype(np.int64)
    assert len(idx) == limit // 2 // 64 and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / 'a' / 'objective_rank1.npy'), np.where(np.isnan(obj), 0.0, obj)[idx])
    assert np.array_equal(np.load(tmp_path / 'a' / 'evals_rank1.npy'), ev[idx].astype(np.float64))
    assert np.array_equal(np.load(tmp_path / 'a' / 'status_rank1.npy'), st[idx].astype(np.float64))
