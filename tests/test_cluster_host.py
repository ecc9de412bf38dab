"""The restatement of the candidate clustering (tests/cluster_restate.py) pinned without a GPU: against a plain-Python search over
the two float32 predicates, against the oracle's ClusterTransformation on every candidate set the GPU tests use
(tests/cluster_cases.py), and against the labels recorded from the FLANN composition (tests/golden/g10_cluster.npz).  And the
candidate sets themselves: each must reach the part of the spatial hash it is aimed at."""
import os
from collections import deque

import numpy as np
import pytest

import cluster_cases as CC
import cluster_restate as KR

F32 = np.float32
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def bfs_clusters(t, e, r, gate):
    """cluster_of (ids in order of the smallest member) by a breadth-first search, one float32 predicate at a time."""
    T, E = np.asarray(t, F32), np.asarray(e, F32)
    n = len(T)
    r2, g = F32(float(F32(r)) * float(F32(r))), F32(gate)

    def sq(a, b):
        d0, d1, d2 = a[0] - b[0], a[1] - b[1], a[2] - b[2]
        return F32(F32(F32(d0 * d0) + F32(d1 * d1)) + F32(d2 * d2))

    label = [-1] * n
    c = 0
    for s in range(n):
        if label[s] >= 0:
            continue
        label[s] = c
        todo = deque([s])
        while todo:
            i = todo.popleft()
            for j in range(n):
                if label[j] < 0 and j != i and sq(T[i], T[j]) < r2 and sq(E[i], E[j]) < g:
                    label[j] = c
                    todo.append(j)
        c += 1
    return np.asarray(label, np.int32), c


def test_restatement_against_breadth_first_search():
    rng = np.random.default_rng(2)
    with np.errstate(invalid="ignore"):
        for n, r, gate in ((1, 0.1, 0.01), (2, 0.9, 0.5), (80, 0.15, 0.02), (160, 0.12, 0.01), (160, 0.3, 0.004)):
            t = rng.random((n, 3)).astype(F32)
            e = (rng.normal(0, 0.05, (n, 3))).astype(F32)
            t[n // 2], e[n // 2] = t[0], e[0]      # an exact duplicate
            if n > 100:
                e[7, 2] = np.nan                  # no edge to anything
            want = bfs_clusters(t, e, r, gate)
            got = KR.cluster(t, e, r, gate)
            assert got[1] == want[1] and np.array_equal(got[0], want[0])
            assert 1 < want[1] < n or n <= 2


def test_r2_is_pcl_r2():
    # float(double(r) * double(r)) with r a float: the double product of two floats is exact, so this is the one rounding of
    # float(r) * float(r) as well -- the threshold is taken from the float the seam receives, never from the Python double
    for r in (0.06, 0.07, 0.11, 0.13, 1e-3, 37.5):
        assert KR.r2_of(r) == F32(np.float64(F32(r)) ** 2) == F32(r) * F32(r)
    assert KR.r2_of(0.5) == F32(0.25) and KR.r2_of(0.0) == 0 and np.isinf(KR.r2_of(np.inf))


def test_both_edge_paths_agree():
    for name in ("mixed_5000", "wide_x", "lattice"):
        t, e, r, gate = CC.case(name)
        a, b = KR.edges_brute(t, e, r, gate), KR.edges_kdtree(t, e, r, gate)
        assert len(a) >= 700 and np.array_equal(a, b), name


@pytest.mark.parametrize("name", CC.NAMES)
def test_restatement_equals_the_oracle(oracle, name):
    t, e, r, gate = CC.case(name)
    lab, n = CC.reference(name)
    lab_o, n_o = oracle.cluster_transforms(t, e, r, gate)
    assert n == n_o and np.array_equal(lab, lab_o)
    seeds = np.array([np.flatnonzero(lab == c)[0] for c in range(n)])
    assert (np.diff(seeds) > 0).all()         # cluster c is the one with the c-th smallest seed


def test_restatement_equals_the_recorded_flann_composition():
    g = np.load(os.path.join(G, "g10_cluster.npz"), allow_pickle=False)
    names = str(g["names"]).split(";")
    assert len(names) >= 4
    for name in names:
        lab, n = KR.cluster(g[f"{name}_t"], g[f"{name}_euler"], float(g[f"{name}_dist"]), float(g[f"{name}_angle"]))
        assert n == int(g[f"{name}_n"]) and np.array_equal(lab, g[f"{name}_cluster_of"]), name


# ---- the candidate sets are what they are meant to be ----------------------------------------------------------------------
def test_mixed_sets_reach_both_walks_of_the_edge_kernel():
    """Window lengths 5 (only the lane's own 16-entry walk), 17 (one entry left for the wavefront), 80 (one full step of 64) and 81
    (a second step of one entry) all occur, and each blob is split in two by the gate."""
    for m in (255, 256, 257, 5000):
        t, e, r, gate = CC.case(f"mixed_{m}")
        assert len(t) == m
        assert set(CC.BLOBS) <= set(CC.x_window_counts(t, r).tolist()), m
        lab, n = CC.reference(f"mixed_{m}")
        size = np.bincount(lab)
        for nb in CC.BLOBS:
            assert nb // 2 in size and nb - nb // 2 in size, (m, nb)
        assert (size == 1).sum() >= 20 and (size == 2).sum() >= 10        # isolated ones; duplicates that joined
    assert CC.reference("mixed_1")[1] == 1 and CC.reference("mixed_2")[1] == 1
    lab, n = CC.reference("mixed_5000")
    assert n > 500 and np.bincount(lab).max() > 100
    assert CC.case("mixed_5000")[0].min() < -2


def test_expected_partitions_of_the_constructed_sets():
    assert CC.reference("dense")[1] == 5
    assert CC.x_window_counts(*CC.case("dense")[0::2]).min() == 3000
    lab, n = CC.reference("chain")
    assert n == 1 and not lab.any()
    t, e, r, gate = CC.case("chain_cut")
    lab, n = CC.reference("chain_cut")
    assert n == 2 and sorted(np.bincount(lab)) == [1499, 2501]
    p = np.random.default_rng(CC.CHAIN_SEED).permutation(len(t))
    i, j = np.flatnonzero(p == 2500), np.flatnonzero(p == 2501)          # the cut link is r exactly: float32 d^2 == r^2
    assert KR.pair_d2(t, i, j)[0] == KR.r2_of(r) and lab[i[0]] != lab[j[0]]
    for name, want in (("r_apart", 2), ("r_joined", 1), ("gate_apart", 2), ("gate_joined", 1), ("same_spot_one", 1),
                       ("same_spot_two", 2), ("r_zero", 257), ("r_inf", 3)):
        assert CC.reference(name)[1] == want, name
    lab, n = CC.reference("nan_euler")
    assert n == 2 and lab.tolist() == [0, 1, 0, 0]
    lab, n = CC.reference("lattice")
    assert 2 <= n < 729 and len(lab) == 1458           # the partners chain the lattice points along their rows


def test_frame_and_order_cases_are_the_same_candidates():
    t, e, r, gate = CC.case("mixed_5000")
    ts = CC.case("shifted_5000")[0]
    assert np.abs(ts - (t.astype(np.float64) + [1000, -2000, 500])).max() < 2e-4 and not np.array_equal(ts - ts[0], t - t[0])
    p = np.random.default_rng(CC.PERM_SEED).permutation(len(t))
    assert np.array_equal(CC.case("permuted_5000")[0], t[p])
    # the partition does not depend on the order: same sets, renumbered by smallest member
    lab, n = CC.reference("mixed_5000")
    lab_p, n_p = CC.reference("permuted_5000")
    assert n == n_p
    first = np.full(n, len(t))
    np.minimum.at(first, lab[p], np.arange(len(t)))
    rank = np.empty(n, np.int64)
    rank[np.argsort(first)] = np.arange(n)
    assert np.array_equal(lab_p, rank[lab[p]])


@pytest.mark.parametrize("axis", (0, 1, 2))
def test_wide_spread_defeats_a_float32_cell_coordinate(axis):
    """The wide-spread set is only worth its GPU time while a float32 cell coordinate, floorf((t - mn) * (1.f / cell)) + 1, sends
    pairs that are within the radius two or more cells apart -- out of reach of the probe of +-1 cell.  At least 10 of the 3000
    pairs must do so; in float64 none may."""
    name = "wide_" + "xyz"[axis]
    t, e, r, gate = CC.case(name)
    n = CC.WIDE_PAIRS
    assert len(t) == 2 * n + 1
    a, b = np.arange(1, n + 1), np.arange(n + 1, 2 * n + 1)
    assert (KR.pair_d2(t, a, b) < KR.r2_of(r)).all()
    mn, cell = CC.grid_of(t, r)
    assert cell == F32(r) * F32(1.001)                                   # no doubling yet: about 10^6 cells
    assert 0.9e6 < (t[:, axis].max() - t[:, axis].min()) / cell < 1.1e6
    c32, c64 = CC.cells_f32(t, r), CC.cells_f64(t, r)
    apart32 = np.abs(c32[a] - c32[b]).max(1)
    assert (apart32 >= 2).sum() >= 10, int((apart32 >= 2).sum())
    assert np.abs(c64[a] - c64[b]).max() <= 1
    lab, k = CC.reference(name)
    assert k == n + 1 and np.array_equal(lab, np.concatenate([[0], np.arange(1, n + 1), np.arange(1, n + 1)]))


def test_far_set_doubles_the_cell_and_fills_the_key():
    t, e, r, gate = CC.case("far_63bit")
    mn, cell = CC.grid_of(t, r)
    assert cell == F32(r) * F32(1.001) * F32(32)
    ext = t.max(0).astype(np.float64) - t.min(0)
    bits = [int(np.ceil(np.log2(x / float(cell) + 4))) for x in ext]
    assert bits == [21, 21, 21]
    n = CC.WIDE_PAIRS
    lab, k = CC.reference("far_63bit")
    assert k == n + 1 and np.array_equal(lab, np.concatenate([[0], np.arange(1, n + 1), np.arange(1, n + 1)]))
