"""The scene of ring_scene.py makes the shared ring walk do everything it can do, in every grid the GPU tests build over it: the
row loop runs more than once, a step has whole-row and side runs, the block grows at least three times and is clipped by the
grid's edge.  Checked on a CPU model of the grids and of the walk (no GPU)."""
import numpy as np
import pytest

import outlier_restate as R
import ring_scene as S


@pytest.fixture(scope="module")
def sorted_dist():
    P = S.scene().astype(np.float64)
    far = P[S.N_PATCH:]
    return np.sort(np.linalg.norm(far[:, None] - P[None], axis=2), axis=1)    # [:, 0] = 0: the point itself


@pytest.mark.parametrize("k", [1, 8, 16, 64])
def test_knn_walks_of_the_isolated_points(sorted_dist, k):
    """normals (the point itself included: the k-th key is the (k-1)-th other point) and outliers (left out: the k-th other)"""
    P = S.scene()
    cell, dims = S.knn_grid(P, k)
    for i in range(S.N_FAR):
        for need in {sorted_dist[i, max(k - 1, 1)], sorted_dist[i, k]}:
            steps = S.walk(P, P[S.N_PATCH + i], cell, dims, need)
            assert S.does_everything(steps), (k, i, steps)


@pytest.mark.parametrize("d", S.RADII)
def test_distance_walks_of_the_isolated_probes(d):
    T = S.scene()
    cell, dims = S.distance_grid(T, d)
    for q in S.PROBES:
        nn = np.linalg.norm(T.astype(np.float64) - q, axis=1).min()
        assert nn > S.GAP and S.RADII[0] < S.GAP < S.RADII[1]
        steps = S.walk(T, q, cell, dims, min(nn, d))
        assert S.does_everything(steps), (d, q, steps)


@pytest.mark.parametrize("k", [1, 16, 64])
def test_no_mean_distance_sits_on_the_threshold(k):
    """what test_gpu_outliers.py asserts before it compares keep flags"""
    P = S.scene()
    ref = R.statistical(P, k, 1.0, keys=R.neighbours(P, kmax=64)[0])
    assert R.nearest_gap(ref["m"], ref["threshold"]) > 1e-9
