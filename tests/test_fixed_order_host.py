"""The numpy replay of the summaries' fixed reduction order (tests/fixed_order.py) is a sum, is exact on integers, and is an
order of its own: tests/test_gpu_fixed_order.py, which holds the GPU's summaries to it bit for bit, can tell orders apart."""
import math

import numpy as np
import pytest

import fixed_order as F

SIZES = (1, 63, 64, 65, 255, 256, 257, 16384, 16385, 16641)


@pytest.mark.parametrize("n", SIZES)
def test_the_replay_is_a_sum(n):
    v = np.random.default_rng(n).normal(size=n) * 10.0 ** np.random.default_rng(n + 1).integers(-6, 6, size=n)
    assert abs(F.reduce(v, np.add) - math.fsum(v)) <= n * 2.0 ** -53 * np.abs(v).sum()
    assert F.reduce(np.abs(v), np.fmax) == np.abs(v).max()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_integers_are_exact(n, dtype):
    u = np.random.default_rng(n).integers(0, 100000, size=n).astype(dtype)
    assert F.reduce(u, np.add) == u.sum(dtype=np.uint64) and F.reduce(u, np.maximum) == u.max()


def test_one_value_passes_unchanged():
    assert F.reduce(np.array([-0.375]), np.add) == -0.375 and F.reduce(np.array([7], np.uint32), np.maximum) == 7


@pytest.mark.parametrize("n", [1000, 16641])
def test_the_order_matters_and_is_neither_numpys_nor_left_to_right(n):
    # 1e16 + 1 rounds back to 1e16: what survives of the ones depends on which values meet first
    v = np.tile(np.array([1e16, 1.0, -1e16, 1.0]), n // 4 + 1)[:n]
    left_to_right = 0.0
    for x in v:
        left_to_right += x
    r = F.reduce(v, np.add)
    assert r != np.sum(v) and r != left_to_right
    assert abs(r - math.fsum(v)) <= n * 2.0 ** -53 * np.abs(v).sum()
