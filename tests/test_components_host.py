"""The restatement of the connected components (tests/components_restate.py) pinned without a GPU: against a plain-Python
breadth-first search over the float32 predicate, its two edge paths against each other, and the library's documented defaults."""
from collections import deque

import numpy as np

import plade_amd
import components_restate as CR

F32 = np.float32


def bfs_components(P, r):
    """label (ids in order of the smallest index) by a breadth-first search, one float32 predicate at a time."""
    X = np.asarray(P, F32)[:, :3]
    n = len(X)
    r2 = F32(r) * F32(r)

    def near(i, j):
        dx, dy, dz = X[i, 0] - X[j, 0], X[i, 1] - X[j, 1], X[i, 2] - X[j, 2]
        return F32(F32(F32(dx * dx) + F32(dy * dy)) + F32(dz * dz)) < r2

    label = [-1] * n
    c = 0
    for s in range(n):                       # ascending: a new component is met at its smallest index
        if label[s] >= 0:
            continue
        label[s] = c
        todo = deque([s])
        while todo:
            i = todo.popleft()
            for j in range(n):
                if label[j] < 0 and j != i and near(i, j):
                    label[j] = c
                    todo.append(j)
        c += 1
    return np.asarray(label, np.int32)


def test_restatement_against_breadth_first_search():
    rng = np.random.default_rng(11)
    for n, r in ((1, 0.1), (2, 0.5), (60, 0.12), (150, 0.08), (150, 0.2)):
        P = rng.random((n, 3)).astype(F32)
        P[n // 2] = P[0]                     # a duplicate
        ref = bfs_components(P, r)
        out = CR.components(P, r)
        assert np.array_equal(out["label"], ref)
        assert np.array_equal(out["size"], np.bincount(ref).astype(np.uint32))
        assert out["components"] == ref.max() + 1 and out["kept"] == n and out["largest"] == np.bincount(ref).max()


def test_selection_rule():
    size = np.array([5, 1, 9, 5, 2, 9], np.uint32)
    assert CR.select(size).all()
    assert np.array_equal(CR.select(size, min_size=2), [1, 0, 1, 1, 1, 1])
    assert np.array_equal(CR.select(size, min_size=2, max_size=5), [1, 0, 0, 1, 1, 0])
    assert np.array_equal(CR.select(size, keep_largest=1), [0, 0, 1, 0, 0, 0])          # the tie at 9: the smaller id
    assert np.array_equal(CR.select(size, keep_largest=3), [1, 0, 1, 0, 0, 1])          # the tie at 5: the smaller id
    assert np.array_equal(CR.select(size, max_size=5, keep_largest=2), [1, 0, 0, 1, 0, 0])
    assert np.array_equal(CR.select(size, min_size=10, keep_largest=2), [0] * 6)


def test_both_edge_paths_agree_on_5k():
    rng = np.random.default_rng(5)
    P = (rng.random((5000, 3)) * np.array([4.0, 3.0, 0.05])).astype(F32)   # a noisy slab: about 13 points within r
    r = 0.1
    a, b = CR.edges_brute(P, r), CR.edges_kdtree(P, r)
    assert len(a) > 20000 and np.array_equal(a, b)
    la, lb = CR.labels_from_edges(len(P), a), CR.labels_from_edges(len(P), b)
    assert np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1])


def test_default_params():
    assert plade_amd.component_default_params() == {"radius": 0.0, "min_size": 1, "max_size": 0, "keep_largest": 0}
    assert set(("plade_component_default_params", "plade_label_components", "plade_cloud_filter_components_dev")) <= set(plade_amd.ABI_SYMBOLS)
