"""The consistent normal orientation on the GPU (plade_orient_normals / plade_cloud_orient_normals_dev, plade_amd/csrc/k_orient.hip)
against the restatement of its semantics (tests/orient_restate.py: the float32 graph, the edge keys, Kruskal's forest with a parity
bit, the anchors).  flip, label, the rows as bit patterns, components, flipped, unoriented, tree_edges and tree_key_sum are compared
exactly: the forest is unique under the total order of the edges, so there is no tolerance anywhere in this file.  rounds is the one
field that belongs to the GPU's iteration: it has to lie in [1, ceil(log2 n) + 1].
"""
import ctypes
import math

import numpy as np
import pytest

import plade_amd
import grid_shapes as GS
import orient_restate as OR
from outlier_restate import flann_d2
from conftest import ORIENTED

pytestmark = pytest.mark.gpu

F32 = np.float32
VOTE, EXTREME = plade_amd.ORIENT_VOTE, plade_amd.ORIENT_EXTREME
SUMMARY = ("n", "unoriented", "components", "flipped", "tree_edges", "tree_key_sum")
STATS = ("orient_grid_s", "orient_rounds_s", "orient_finish_s", "orient_rounds", "orient_components", "orient_flipped", "orient_grid_dx",
         "orient_grid_dy", "orient_grid_dz", "orient_grid_cell")
SIZES = (1, 2, 63, 64, 65, 257, 4099)
RADII = (1.5, 3.0, 10.0)               # x the mean point spacing of OR.sheet (1)

# the messages of the errors
E_EMPTY = "orient_normals: the cloud is empty (n = 0)"
E_NULL = "plade_orient_normals: NULL cloud"
E_NULL_DEV = "plade_cloud_orient_normals_dev: NULL cloud"
E_FINITE = "the point cloud contains non-finite coordinates (NaN or infinity)"
E_RADIUS = "orient_normals: radius must be finite and > 0, its fp32 square finite and not below FLT_MIN"
E_MODE = "orient_normals: mode must be 0 (vote) or 1 (extreme point)"
E_INWARD = "orient_normals: inward must be 0 or 1"
E_VIEW = "orient_normals: the viewpoint must be finite"
E_DIR = "orient_normals: the direction must be finite"
E_DIR0 = "orient_normals: the direction must not be zero"


@pytest.fixture(scope="module")
def octx():
    c = plade_amd.Context(0, **ORIENTED)
    yield c
    c.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same(got, ref):
    rows, info = got
    for k in SUMMARY:
        assert info[k] == ref[k], (k, info[k], ref[k])
    assert 1 <= info["rounds"] <= math.ceil(math.log2(ref["n"])) + 1, info["rounds"]
    assert np.array_equal(info["flip"].view(np.uint8), ref["flip"])
    assert info["label"].dtype == np.int32 and same_bits(info["label"], ref["label"])
    assert rows.dtype == F32 and same_bits(rows.view(np.uint32), ref["rows"].view(np.uint32))


def check(ctx, rows, radius, resident=True, **kw):
    """the host form twice and the resident form against the restatement.  Returns (restated, info of the host form)"""
    rows = np.ascontiguousarray(rows, F32)
    ref = OR.orient(rows, radius, **kw)
    got = ctx.orient_consistent(rows, radius, **kw)
    info = got[1]
    print(f"n {len(rows)} radius {float(radius):.6g} {kw}: " + ", ".join(f"{k} {info[k]} ({ref[k]})" for k in SUMMARY) +
          f", rounds {info['rounds']}")
    assert_same(got, ref)
    s = ctx.stats()
    assert all(k in s for k in STATS), [k for k in STATS if k not in s]
    assert (s["orient_rounds"], s["orient_components"], s["orient_flipped"]) == (info["rounds"], info["components"], info["flipped"])
    assert_same(ctx.orient_consistent(rows, radius, **kw), ref)                  # a second call on the same context: the same bits
    if resident:
        c = ctx.upload(rows)
        try:
            out, dinfo = ctx.orient_consistent_dev(c, radius, info=True, **kw)
            try:
                assert out.n == len(rows)
                assert_same((out.download(), dinfo), ref)
            finally:
                out.free()
        finally:
            c.free()
    return ref, info


def one_side(rows, truth):
    """+1 / -1: every valid normal of the oriented rows is `truth` or every one is -truth (else 0)"""
    d = np.einsum("ij,ij->i", rows[:, 3:6].astype(np.float64), np.asarray(truth, np.float64))
    return 1 if (d > 0).all() else -1 if (d < 0).all() else 0


# ---- seeded sheets: sizes around the wavefront and the workgroup, several workgroups; three densities of the graph ---------------
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("n", SIZES)
def test_sheets_random_normals(octx, n, radius):
    check(octx, OR.with_normals(OR.sheet(n), OR.random_normals(n)), radius)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("n", SIZES)
def test_sheets_flipped_normals(octx, n, radius):
    """analytic normals (+z, tilted a little by seeded noise so that the keys differ) flipped at random"""
    N = np.tile(np.asarray([0, 0, 1], np.float64), (n, 1)) + 0.05 * np.random.default_rng(4).normal(size=(n, 3))
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    rows = OR.with_normals(OR.sheet(n), OR.random_flips(N))
    ref, info = check(octx, rows, radius, viewpoint=(0.0, 0.0, 50.0))
    lab = ref["label"]
    for c in range(ref["components"]):                             # every component on one side; the large ones face the viewpoint
        assert one_side(ref["rows"][lab == c], N[lab == c]) != 0
    if radius == 10.0 and n > 2:
        assert ref["components"] == 1 and one_side(ref["rows"], N) == 1


# ---- anchors -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shell():
    P, U = OR.sphere(3000)
    return OR.with_normals(P, OR.random_flips(U)), U


def test_sphere_extreme_is_outward_and_inward_the_opposite(octx, shell):
    rows, U = shell
    ref, info = check(octx, rows, 1.5, mode=EXTREME)
    assert ref["components"] == 1 and one_side(ref["rows"], U) == 1
    ref_in, _ = check(octx, rows, 1.5, mode=EXTREME, inward=1)
    assert one_side(ref_in["rows"], U) == -1 and np.array_equal(ref_in["flip"], ref["flip"] ^ 1)
    down, _ = check(octx, rows, 1.5, mode=EXTREME, direction=(0.3, -2.0, -0.5), resident=False)
    assert one_side(down["rows"], U) == 1                          # another direction, another anchor, the same side


def test_sphere_vote_from_inside_and_outside(octx, shell):
    rows, U = shell
    inside, _ = check(octx, rows, 1.5, viewpoint=(1.0, -2.0, 0.5))
    assert one_side(inside["rows"], U) == -1                       # toward a viewpoint inside the shell
    flipped, _ = check(octx, rows, 1.5, viewpoint=(1.0, -2.0, 0.5), inward=1, resident=False)
    assert one_side(flipped["rows"], U) == 1
    far, _ = check(octx, rows, 1.5, viewpoint=(0.0, 0.0, 1000.0), resident=False)
    assert far["components"] == 1 and one_side(far["rows"], U) != 0   # one side, whichever half of the shell outvotes the other


def test_two_components_one_votes_to_toggle(octx):
    """two sheets far apart, both with +z normals on every point: the viewpoint is above the first and below the second, so the
    second toggles as a whole"""
    A, B = OR.sheet(300, seed=6), OR.sheet(200, seed=7)
    B[:, 0] += 100.0
    B[:, 2] += 40.0
    rows = OR.with_normals(np.concatenate([A, B]), np.tile(np.asarray([0, 0, 1], F32), (500, 1)))
    ref, info = check(octx, rows, 3.0, viewpoint=(50.0, 8.0, 20.0))
    assert ref["components"] == 2 and not ref["flip"][:300].any() and ref["flip"][300:].all()
    assert (ref["label"][:300] == 0).all() and (ref["label"][300:] == 1).all()


def test_vote_tie_toggles_nothing(octx):
    """four collinear points, the viewpoint in the plane through the middle that the normals cross: two face it, two do not"""
    rows = np.zeros((4, 6), F32)
    rows[:, 0] = [-1.5, -0.5, 0.5, 1.5]
    rows[:, 3] = 1.0
    for first in (1.0, -1.0):
        rows[0, 3] = first
        ref, info = check(octx, rows, 1.1, viewpoint=(0.0, 5.0, 0.0))
        assert ref["components"] == 1 and ref["flip"].tolist() == [0, int(first < 0), int(first < 0), int(first < 0)]
        ref_in, _ = check(octx, rows, 1.1, viewpoint=(0.0, 5.0, 0.0), inward=1, resident=False)
        assert np.array_equal(ref_in["flip"], ref["flip"] ^ 1)


def test_crease_of_90_degrees(octx):
    """a floor and a wall that meet at x = 0: |dot| = 0 across the crease, the forest crosses it once, and both end up facing the
    viewpoint inside the corner"""
    g = np.stack(np.meshgrid(np.arange(1, 21), np.arange(20), indexing="ij"), -1).reshape(-1, 2).astype(np.float64) * 0.5
    floor = np.c_[g[:, 0], g[:, 1], np.zeros(len(g))]
    wall = np.c_[np.zeros(len(g)), g[:, 1], g[:, 0]]
    P = np.concatenate([floor, wall]).astype(F32)
    N = np.concatenate([np.tile([0.0, 0, 1], (len(g), 1)), np.tile([1.0, 0, 0], (len(g), 1))])
    rows = OR.with_normals(P, OR.random_flips(N, seed=8))
    ref, info = check(octx, rows, 0.75, viewpoint=(5.0, 5.0, 5.0))
    assert ref["components"] == 1 and one_side(ref["rows"], N) == 1
    assert (OR.weighted_edges(rows, 0.75)[2][-1] == OR.KEY_TOP) and ref["tree_key_sum"] == (ref["tree_edges"] - 1) * OR.KEY_FLAT + OR.KEY_TOP


# ---- ties, duplicates, the radius ---------------------------------------------------------------------------------------------------
def test_lattice_with_identical_normals_is_all_ties(octx):
    g = np.stack(np.meshgrid(np.arange(30), np.arange(31), np.arange(2), indexing="ij"), -1).reshape(-1, 3)
    perm = np.random.default_rng(10).permutation(len(g))           # (the index order is not the scan order)
    rows = OR.with_normals(g[perm].astype(F32), np.tile(np.asarray([0, 0, -1], F32), (len(g), 1)))
    ref, info = check(octx, rows, 1.2, viewpoint=(0.0, 0.0, 9.0))
    assert ref["components"] == 1 and ref["tree_key_sum"] == ref["tree_edges"] * OR.KEY_FLAT and ref["flip"].all()
    lo, hi, key, s = OR.weighted_edges(rows, 1.2)
    assert (key == OR.KEY_FLAT).all() and len(lo) > 2 * len(g)


def test_exact_duplicates(octx):
    P = OR.sheet(200, seed=12)
    P = np.concatenate([P, P[:50], P[:50]])
    rows = OR.with_normals(P, OR.random_normals(len(P), seed=13))
    ref, info = check(octx, rows, 1.5)
    assert ref["unoriented"] == 0
    same = OR.with_normals(np.zeros((70, 3), F32), OR.random_normals(70, seed=14))   # one place, seventy points
    ref, info = check(octx, same, 0.5)
    assert ref["components"] == 1 and ref["tree_edges"] == 69


def test_pair_exactly_at_the_radius_and_one_ulp_closer(octx):
    r = 0.75
    rows = np.zeros((2, 6), F32)
    rows[1, 0] = r
    rows[0, 5], rows[1, 5] = 1.0, -1.0
    assert flann_d2(rows[:1, :3], rows[1:, :3])[0, 0] == F32(r) * F32(r)
    ref, info = check(octx, rows, r, viewpoint=(0.0, 0.0, 3.0))
    assert ref["components"] == 2 and ref["tree_edges"] == 0 and ref["flip"].tolist() == [0, 1] and info["rounds"] == 1
    rows[1, 0] = np.nextafter(F32(r), F32(0))
    ref, info = check(octx, rows, r, viewpoint=(0.0, 0.0, 3.0))
    assert ref["components"] == 1 and ref["tree_edges"] == 1 and ref["tree_key_sum"] == OR.KEY_FLAT and info["rounds"] == 2
    assert ref["flip"].tolist() == [0, 1]                          # anchored on point 0, both then face the viewpoint


def test_radius_below_the_smallest_gap_and_above_the_diameter(octx):
    P = OR.sheet(257)
    rows = OR.with_normals(P, OR.random_normals(257, seed=15))
    d = flann_d2(P, P)
    np.fill_diagonal(d, np.inf)
    ref, info = check(octx, rows, 0.99 * float(np.sqrt(d.min())))
    assert ref["components"] == 257 and ref["tree_edges"] == 0 and info["rounds"] == 1
    assert np.array_equal(ref["label"], np.arange(257, dtype=np.int32))
    ref, info = check(octx, rows, 100.0)                           # the diagonal of the sheet is 23: the complete graph
    assert ref["components"] == 1 and ref["tree_edges"] == 256


# ---- invalid normals -----------------------------------------------------------------------------------------------------------------
def test_invalid_normals_are_left_alone(octx):
    n = 600
    rows = OR.with_normals(OR.sheet(n, seed=16), OR.random_normals(n, seed=17))
    w = rows.view(np.uint32)
    w[5::7, 3] = np.uint32(0x7FC00000) + np.arange(len(w[5::7]), dtype=np.uint32) + np.uint32(1)   # NaNs with a payload
    rows[3::11, 4] = np.inf
    rows[2::13, 5] = -np.inf
    rows[1::17, 3] = 1e19
    rows[8::19, 4] = -1.0000001e18
    rows[9::23, 5] = 1e18                                          # (valid: the bound is <=)
    rows[0, 3:] = 0.0                                              # length 0: valid, every key 0x7F800000
    rows[4, 3:] = [-0.0, 0.0, -0.0]
    ok = OR.valid_points(rows)
    assert 150 < (~ok).sum() < 300 and ok[0] and ok[4] and ok[9]
    for mode in (VOTE, EXTREME):
        ref, info = check(octx, rows, 2.0, mode=mode)
        assert ref["unoriented"] == (~ok).sum() and (ref["label"][~ok] == -1).all() and not ref["flip"][~ok].any()
        assert same_bits(ref["rows"][~ok].view(np.uint32), rows[~ok].view(np.uint32))


def test_cloud_without_a_valid_point(octx):
    rows = OR.with_normals(OR.sheet(100, seed=18), np.full((100, 3), np.nan, F32))
    rows[::2, 4] = np.inf
    for mode in (VOTE, EXTREME):
        ref, info = check(octx, rows, 2.0, mode=mode)
        assert (info["unoriented"], info["components"], info["flipped"], info["tree_edges"], info["rounds"]) == (100, 0, 0, 0, 1)


def test_normals_of_length_zero(octx):
    rows = OR.with_normals(OR.sheet(300, seed=19), np.zeros((300, 3), F32))
    ref, info = check(octx, rows, 2.0)
    assert ref["flipped"] == 0 and ref["tree_key_sum"] == ref["tree_edges"] * OR.KEY_TOP
    ref, info = check(octx, rows, 2.0, inward=1, mode=EXTREME)     # flipped zeros: the sign bits say so
    assert ref["flipped"] == 300 and np.signbit(ref["rows"][:, 3:]).all()


# ---- the grid shapes of DESIGN.md section 22 ----------------------------------------------------------------------------------------
def test_single_row_grid(octx):
    P = GS.cloud("row0")
    rows = OR.with_normals(P, OR.random_normals(len(P), seed=20))
    check(octx, rows, GS.R)
    s = octx.stats()
    assert (s["orient_grid_dy"], s["orient_grid_dz"]) == (1, 1) and s["orient_grid_dx"] > 100
    sorted_line = OR.with_normals(P, np.tile(np.asarray([0, 1, 0], F32), (len(P), 1)))
    ref, info = check(octx, sorted_line, GS.R, resident=False)     # all ties on a sorted scan line: every point picks its predecessor
    assert ref["components"] == 1 and info["rounds"] <= 3


def test_one_cell_thick_grid(octx):
    P = GS.cloud("sheet2")
    check(octx, OR.with_normals(P, OR.random_normals(len(P), seed=21)), GS.R)
    s = octx.stats()
    assert s["orient_grid_dz"] == 1 and s["orient_grid_dx"] > 1 and s["orient_grid_dy"] > 1


def test_capped_grid(octx):
    rng = np.random.default_rng(9)
    clump = 0.02 * rng.random((200, 3))
    far = clump[::-1] + 1e4 / np.sqrt(3.0)                         # 1e4 away along the diagonal: every axis is long
    P = np.ascontiguousarray(np.concatenate([clump, far]).astype(F32))
    radius = 2e-3
    ref, info = check(octx, OR.with_normals(P, OR.random_normals(400, seed=22)), radius)
    assert 2 <= ref["components"] < 400
    s = octx.stats()
    dims = (s["orient_grid_dx"], s["orient_grid_dy"], s["orient_grid_dz"])
    assert GS.is_capped(s["orient_grid_cell"], dims, GS.radius_cell(P, r=radius)), (s["orient_grid_cell"], dims)


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def test_errors(octx):
    rows = OR.with_normals(OR.sheet(300), OR.random_normals(300))
    ref = OR.orient(rows, 2.0)
    nan, inf = rows.copy(), rows.copy()
    nan[17, 1] = np.nan
    inf[299, 2] = np.inf
    bad = float("nan")
    cases = [(np.zeros((0, 6), F32), {"radius": 2.0}, E_EMPTY), (nan, {"radius": 2.0}, E_FINITE), (inf, {"radius": 2.0}, E_FINITE)]
    cases += [(rows, {"radius": r}, E_RADIUS) for r in (0.0, -1.0, bad, 1e30, 1e-30, float("inf"))]
    cases += [(rows, {"radius": 2.0, "mode": m}, E_MODE) for m in (2, -1)]
    cases += [(rows, {"radius": 2.0, "inward": i}, E_INWARD) for i in (2, -1)]
    cases += [(rows, {"radius": 2.0, "viewpoint": (0.0, bad, 0.0)}, E_VIEW), (rows, {"radius": 2.0, "viewpoint": (float("inf"), 0.0, 0.0)}, E_VIEW),
              (rows, {"radius": 2.0, "mode": EXTREME, "direction": (0.0, 0.0, bad)}, E_DIR),
              (rows, {"radius": 2.0, "direction": (0.0, -float("inf"), 0.0)}, E_DIR),
              (rows, {"radius": 2.0, "mode": EXTREME, "direction": (0.0, -0.0, 0.0)}, E_DIR0)]
    for arr, kw, msg in cases:
        with pytest.raises(plade_amd.PladeError) as e:
            octx.orient_consistent(arr, **kw)
        assert e.value.code == plade_amd.PLADE_EINVAL and str(e.value).endswith(": " + msg), (kw, str(e.value))
        assert_same(octx.orient_consistent(rows, 2.0), ref)        # the next call on the same context succeeds
    # a NULL cloud and the defaults (no radius) through the C ABI itself
    prm = plade_amd._orient_params(2.0, VOTE, 0, (0, 0, 0), (0, 0, 1))
    summ = plade_amd.OrientSummary()
    L, h = octx.L, octx.h
    rc = L.plade_orient_normals(h, None, 10, ctypes.byref(prm), None, None, None, ctypes.byref(summ))
    assert rc == plade_amd.PLADE_EINVAL and L.plade_last_error(h).decode() == E_NULL
    rc = L.plade_orient_normals(h, rows.ctypes.data, len(rows), None, None, None, None, ctypes.byref(summ))
    assert rc == plade_amd.PLADE_EINVAL and L.plade_last_error(h).decode() == E_RADIUS
    out = ctypes.c_void_p()
    rc = L.plade_cloud_orient_normals_dev(h, None, ctypes.byref(prm), ctypes.byref(out), None, None, ctypes.byref(summ))
    assert rc == plade_amd.PLADE_EINVAL and L.plade_last_error(h).decode() == E_NULL_DEV and not out.value
    c = octx.upload(rows)
    try:
        with pytest.raises(plade_amd.PladeError) as e:
            octx.orient_consistent_dev(c, 0.0)
        assert e.value.code == plade_amd.PLADE_EINVAL and str(e.value).endswith(": " + E_RADIUS)
    finally:
        c.free()
    # every output is optional; in place
    rc = L.plade_orient_normals(h, rows.ctypes.data, len(rows), ctypes.byref(prm), None, None, None, ctypes.byref(summ))
    assert rc == 0 and all(getattr(summ, k) == ref[k] for k in SUMMARY)
    assert L.plade_orient_normals(h, rows.ctypes.data, len(rows), ctypes.byref(prm), None, None, None, None) == 0
    own = rows.copy()
    assert L.plade_orient_normals(h, own.ctypes.data, len(own), ctypes.byref(prm), own.ctypes.data, None, None, None) == 0
    assert same_bits(own.view(np.uint32), ref["rows"].view(np.uint32))


def test_defaults():
    assert plade_amd.orient_default_params() == {"radius": 0.0, "mode": 0, "inward": 0, "viewpoint": (0.0, 0.0, 0.0),
                                                 "direction": (0.0, 0.0, 1.0)}
