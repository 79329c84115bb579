"""k_quantiles on synthetic values through egdst_quantile_eval: every size around the wave, the workgroup and the LDS / global
threshold, value sets with ties, NaNs, signed zeros, infinities and denormals; the bits must be those of a sort of the keys
written out here."""
import functools
import math

import numpy as np
import pytest
import torch  # noqa: F401  (first: the model libraries then bind torch's HIP runtime)

from egdst_amd import build, examples, runtime

pytestmark = pytest.mark.gpu

PS = np.array([0.01, 0.25, 0.5, 0.75, 0.99, 1 / 3, np.nextafter(0, 1), np.nextafter(1, 0)])
SETS = ['normal', 'equal', 'two_values', 'descending', 'normal_with_nan', 'specials']


@functools.lru_cache(maxsize=None)
def _lib():
    return build.build_model(examples.deaton1())


def _keys(x):
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))


def _values(kind, n, rng):
    if kind == 'normal':
        return rng.normal(size=n)
    if kind == 'equal':
        return np.full(n, -1.75)
    if kind == 'two_values':
        return rng.choice([3.5, -2.0], n)
    if kind == 'descending':
        return np.arange(n, 0, -1.0)
    if kind == 'normal_with_nan':
        x = rng.normal(size=n)
        x[rng.random(n) < 0.2] = np.nan
        return x
    tiny = np.nextafter(0, 1)
    return rng.choice([0.0, -0.0, np.inf, -np.inf, tiny, -tiny, np.finfo(np.float64).max, 1.0], n)


def _sizes():
    q = _lib().quantile_lds_keys
    return [1, 2, 63, 64, 65, 255, 256, 257, q - 1, q, q + 1, 100003]


def test_the_default_build_reports_its_lds_threshold():
    """QNT_LDS_KEYS is read from the library (egdst_quantile_lds_keys); the default build gathers up to 2048 keys, so that
    the sizes below straddle the threshold between the two regimes of the kernel."""
    assert _lib().quantile_lds_keys == 2048


@pytest.mark.parametrize('kind', SETS)
def test_selection_equals_a_sort_of_the_keys(kind):
    lib = _lib()
    rng = np.random.default_rng(SETS.index(kind))
    for n in _sizes():
        x = _values(kind, n, rng)
        out, count = lib.quantile_eval(x, PS)
        v = x[~np.isnan(x)]
        assert count == len(v), (kind, n)
        if len(v) == 0:
            assert np.isnan(out).all(), (kind, n)
            continue
        ks = np.sort(_keys(v))
        want = np.array([ks[min(max(math.ceil(p * float(len(v))), 1), len(v)) - 1] for p in PS])
        assert not np.isnan(out).any() and np.array_equal(_keys(out), want), (kind, n, out)


def test_all_nan_gives_nan_and_count_zero():
    out, count = _lib().quantile_eval(np.full(300, np.nan), PS)
    assert count == 0 and np.isnan(out).all()


def test_empty_arguments_are_refused():
    lib = _lib()
    for x, p in ((np.zeros(0), PS), (np.zeros(5), np.zeros(0)), (np.zeros(5), np.array([0.5, 1.0]))):
        with pytest.raises(runtime.EgdstRuntimeError) as e:
            lib.quantile_eval(x, p)
        assert e.value.code == 1
