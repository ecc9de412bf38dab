"""The candidate-clustering stage (plade_amd/csrc/k_cluster.hip: k_t_keys, k_cell_spans, k_cluster_edges, k_flatten and the
compaction of the seeds, behind the seam plade_cluster_transforms) against the brute-force restatement tests/cluster_restate.py.
Every comparison is exact equality of (cluster_of, n_clusters): no tolerance, no candidate left out.  The candidate sets are those
of tests/cluster_cases.py; tests/test_cluster_host.py pins the restatement on each of them against the oracle, and shows that each
reaches the part of the spatial hash it is aimed at."""
import numpy as np
import pytest

import plade_amd
import cluster_cases as CC

pytestmark = pytest.mark.gpu


def run(ctx, name):
    t, e, r, gate = CC.case(name)
    lab, n = ctx.cluster_transforms(t, e, r, gate)
    want, want_n = CC.reference(name)
    bad = np.flatnonzero(lab != want)
    assert n == want_n and len(bad) == 0, (name, n, want_n, len(bad), bad[:8].tolist())
    return lab, n


@pytest.mark.parametrize("m", (1, 2, 255, 256, 257, 5000))
def test_sizes_of_mixed_content(ctx, m):
    """Blobs whose row window holds 5, 17, 80 and 81 candidates (the lane's own 16-entry walk; one entry, one full step of 64, and a
    second step of one entry left to the wavefront), each split by the gate; isolated candidates; exact duplicates that join and
    that do not; at 5000 a slab of random candidates besides.  255 / 256 / 257: the last workgroup of the per-candidate kernels."""
    run(ctx, f"mixed_{m}")


def test_one_dense_cell_three_times(ctx):
    """3000 candidates in one cell, five clusters by the gate: spans of thousands, every union contended.  The result does not depend on
    the order the edges are found in: three runs, one answer."""
    first, n = run(ctx, "dense")
    assert n == 5
    for _ in range(2):
        lab, n2 = run(ctx, "dense")
        assert n2 == n and np.array_equal(lab, first)


def test_chain_of_4000(ctx):
    """4000 candidates 0.99 r apart in shuffled order: one cluster, parent chains as deep as they get.  With one link of exactly r
    (float32 d^2 == r^2, strict <): two."""
    lab, n = run(ctx, "chain")
    assert n == 1 and not lab.any()
    lab, n = run(ctx, "chain_cut")
    assert n == 2 and sorted(np.bincount(lab).tolist()) == [1499, 2501]


def test_both_predicates_are_strict(ctx):
    assert run(ctx, "r_apart")[0].tolist() == [0, 1]        # x = 0 and x = 0.5 at r = 0.5
    assert run(ctx, "r_joined")[0].tolist() == [0, 0]       # x = nextafter(0.5, 0)
    assert run(ctx, "gate_apart")[0].tolist() == [0, 1]     # Euler difference 0.5 at gate 0.25
    assert run(ctx, "gate_joined")[0].tolist() == [0, 0]    # gate nextafter(0.25, 1)
    assert run(ctx, "nan_euler")[0].tolist() == [0, 1, 0, 0]


def test_far_frame(ctx):
    """5000 candidates around the origin, negative coordinates included, moved by (1000, -2000, 500): the partition of the moved
    candidates as the restatement sees them."""
    run(ctx, "shifted_5000")


def test_permuted_input_gives_the_permuted_partition(ctx):
    lab_p, n = run(ctx, "permuted_5000")
    lab, n0 = run(ctx, "mixed_5000")
    p = np.random.default_rng(CC.PERM_SEED).permutation(len(lab))
    assert n == n0
    # the same sets of candidates, renumbered by their smallest member in the new order
    first = np.full(n, len(lab))
    np.minimum.at(first, lab[p], np.arange(len(lab)))
    rank = np.empty(n, np.int64)
    rank[np.argsort(first)] = np.arange(n)
    assert np.array_equal(lab_p, rank[lab[p]])


def test_candidates_on_multiples_of_the_cell_edge(ctx):
    run(ctx, "lattice")


def test_zero_extent(ctx):
    lab, n = run(ctx, "same_spot_one")
    assert n == 1 and not lab.any()
    lab, n = run(ctx, "same_spot_two")
    assert n == 2 and np.array_equal(lab, np.arange(1000) % 2)


@pytest.mark.parametrize("axis", "xyz")
def test_wide_spread(ctx, axis):
    """r = 0.06 over an extent of 60 000, 10^6 cells on one axis: 3000 pairs just inside the radius, each a cluster of its own next
    to the anchor.  A float32 cell coordinate sends 23 of the pairs two cells apart, where the probe of +-1 cell never looks
    (tests/test_cluster_host.py): 3024 clusters instead of 3001."""
    lab, n = run(ctx, f"wide_{axis}")
    k = CC.WIDE_PAIRS
    assert n == k + 1 and np.array_equal(lab, np.concatenate([[0], np.arange(1, k + 1), np.arange(1, k + 1)]))


def test_beyond_the_doubling_bound(ctx):
    """The same pairs with the anchor 4 10^6 away on all three axes: the cell doubles five times, 21 bits per axis, a 63-bit key."""
    lab, n = run(ctx, "far_63bit")
    assert n == CC.WIDE_PAIRS + 1


def test_degenerate_thresholds(ctx):
    lab, n = run(ctx, "r_zero")                      # nothing is closer than 0, duplicates included
    assert n == 257 and np.array_equal(lab, np.arange(257))
    lab, n = run(ctx, "r_inf")                       # everything is: the gate alone decides
    assert n == 3


@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_non_finite_translation_is_an_error(ctx, bad):
    t, e, r, gate = CC.case("mixed_257")
    t = t.copy()
    t[200, 1] = bad
    with pytest.raises(plade_amd.PladeError, match="not finite"):
        ctx.cluster_transforms(t, e, r, gate)
    run(ctx, "mixed_257")                            # the context is as good as before
