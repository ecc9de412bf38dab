"""FPFH descriptors and their feature-space match on the GPU (plade_cloud_fpfh / plade_match_features and their resident forms,
plade_amd/csrc/k_fpfh.hip) against the numpy restatement of their semantics (tests/fpfh_restate.py: brute force over all pairs, the
fp64 expressions of fpfh.h term for term).

The histograms, the pair counts and the described flags bit for bit on every point none of whose counted pairs has a feature within
1e-9 of a bin edge (atan2 is the only inexact operation between the kernel and numpy: a few ulps of 1e-16; the test asserts on the
restatement alone that this excludes at most 1 % of the points -- here none).  W and R within 1e-12 relative per entry (a few hundred
positive fp64 terms at 2^-53 each, three orders of margin).  The descriptor bit for bit from the GPU's own H, c, W and R, and within
one fp32 ulp of the restatement's.  The match is integers and fp32 bit patterns: equal to the restatement exactly.
"""
import ctypes

import numpy as np
import pytest

import plade_amd
import fpfh_restate as F
from plade_amd.synth import sample_scene
from conftest import ORIENTED
from test_fpfh_host import LATTICE_R, check_lattice, lattice, match_table

pytestmark = pytest.mark.gpu

RADII = (0.04, 0.08)                # in units of the diagonal D
INT_KEYS = ("spfh", "pairs", "described_mask")
ALL_KEYS = INT_KEYS + ("raw",)


@pytest.fixture(scope="module")
def fctx():
    c = plade_amd.Context(0, **ORIENTED)
    yield c
    c.close()


def diag(P):
    return float(np.linalg.norm(P[:, :3].max(0).astype(np.float64) - P[:, :3].min(0).astype(np.float64)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_result(x, y):
    """two (desc, info) results of Context.fpfh with per_point and seams: every array and the summary, bit for bit"""
    (d0, i0), (d1, i1) = x[:2], y[:2]
    scal = ("n", "described", "mean_pairs", "max_pairs")
    return (same_bits(d0, d1) and all(same_bits(i0[k], i1[k]) for k in ALL_KEYS)
            and all(np.float64(i0[k]).tobytes() == np.float64(i1[k]).tobytes() for k in scal))


@pytest.fixture(scope="module")
def scene():
    A = np.ascontiguousarray(sample_scene(6000, scene_seed=3, sample_seed=4))
    return A, diag(A)


@pytest.fixture(scope="module")
def restated(scene):
    A, D = scene
    return [F.fpfh(A, f * D) for f in RADII]


@pytest.fixture(scope="module")
def computed(scene, fctx):
    A, D = scene
    return [fctx.fpfh(A, f * D, seams=True) for f in RADII]


def check_integers(got, ref, label=""):
    """H, c and the described flags of a GPU result against a restatement, on the points that are not edge_near"""
    info = got[1]
    ok = ~ref["edge_near"]
    assert info["spfh"].dtype == np.uint32 and info["pairs"].dtype == np.uint32
    assert np.array_equal(info["spfh"][ok], ref["spfh"][ok]), label
    assert np.array_equal(info["pairs"][ok], ref["pairs"][ok]), label
    assert np.array_equal(info["described_mask"][ok], ref["described"][ok]), label
    assert (info["spfh"].astype(np.int64).reshape(len(ok), 3, 11).sum(axis=2) == info["pairs"][:, None]).all(), label


def check_sums(got, ref, label=""):
    """W, R, the descriptor and the summary of a GPU result (seams=True) against a restatement"""
    desc, info = got
    m = info["described_mask"]
    ok = ~ref["edge_reach"]
    raw = info["raw"]
    assert (np.abs(raw[ok] - ref["raw"][ok]) <= 1e-12 * ref["raw"][ok]).all(), label
    assert (raw[~m] == 0).all() and np.isnan(desc[~m]).all() and not np.isnan(desc[m]).any(), label
    own = F.descriptor(info["spfh"], info["pairs"], m, raw)
    assert desc.dtype == np.float32 and same_bits(desc, own), label
    both = ok & m
    a, b = desc[both], ref["desc"][both]
    assert (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))).all(), label
    blocks = desc[m].astype(np.float64).reshape(int(m.sum()), 3, 11)
    assert (np.abs(blocks.sum(axis=2) - 100.0) < 1e-3).all(), label
    s = F.summary(info["pairs"], m)
    assert (info["n"], info["described"], info["max_pairs"], info["mean_pairs"]) == (s["n"], s["described"], s["max_pairs"], s["mean_pairs"]), label


# ---- 1: the histograms on a scene ---------------------------------------------------------------------------------------------------
def test_histograms_on_a_scene(scene, restated, computed):
    A, D = scene
    assert abs(D - 13.20) < 0.01
    for f, ref, got in zip(RADII, restated, computed):
        assert ref["edge_near"].sum() <= 0.01 * len(A), f          # (on the restatement alone)
        check_integers(got, ref, f)
    # what the figures were when the test was written: counted pairs, median and largest c, points with c < 5
    assert [r["counted_pairs"] for r in restated] == [123638, 533316]
    assert [int(np.median(g[1]["pairs"])) for g in computed] == [16, 71] and [g[1]["max_pairs"] for g in computed] == [84, 245]
    assert [int((g[1]["pairs"] < 5).sum()) for g in computed] == [82, 4]


# ---- 2: the weighted sums and the descriptor ------------------------------------------------------------------------------------------
def test_weighted_sums_and_descriptor(restated, computed):
    for f, ref, got in zip(RADII, restated, computed):
        check_sums(got, ref, f)
        assert 0 < got[1]["described"] < got[1]["n"]


# ---- 3: the radius boundary, coincident points, missing axes, parallel pairs -------------------------------------------------------
def boundary_cloud():
    """Five groups 16 units apart, every coordinate dyadic, r = 0.25; the expected pair counts at min_pairs = 1."""
    up = (0.0, 0.0, 1.0)
    below = float(np.nextafter(np.float32(0.25), np.float32(0.0)))
    rows = [
        ((0.0, 0.0, 0.0), up), ((0.0, 0.25, 0.0), up),                                   # 0, 1: exactly r apart: out
        ((16.0, 0.0, 0.0), up), ((16.0, below, 0.0), up),                                # 2, 3: one fp32 ulp nearer: in
        ((32.0, 0.0, 0.0), up), ((32.0, 0.0, 0.0), up), ((32.0, 0.125, 0.0), up),        # 4, 5 coincide; 6 sees both
        ((48.0, 0.0, 0.0), up), ((48.0, 0.125, 0.0), (0.0, np.nan, 1.0)), ((48.0, -0.125, 0.0), (0.0, 0.0, 0.0)),
        ((48.125, 0.0, 0.0), (0.0, 0.0, 2.5)),                                           # 7 .. 10: 8 and 9 have no axis
        ((64.0, 0.0, 0.0), up), ((64.0, 0.0, 0.125), up),                                # 11, 12: dp is parallel to n1
    ]
    cloud = np.array([p + n for p, n in rows], np.float32)
    return np.ascontiguousarray(cloud), [0, 0, 1, 1, 1, 1, 2, 1, 0, 0, 1, 0, 0]


def test_radius_boundary_coincident_points_missing_axes_parallel_pairs(fctx):
    cloud, pairs = boundary_cloud()
    ref = F.fpfh(cloud, 0.25, min_pairs=1)
    assert list(ref["pairs"]) == pairs and not ref["edge_near"].any()
    got = fctx.fpfh(cloud, 0.25, min_pairs=1, seams=True)
    assert list(got[1]["pairs"]) == pairs
    assert list(got[1]["described_mask"]) == [c >= 1 for c in pairs]
    check_integers(got, ref)
    check_sums(got, ref)
    assert np.isnan(got[0][[8, 9]]).all() and (got[1]["spfh"][[8, 9]] == 0).all()
    assert (got[1]["described"], got[1]["max_pairs"], got[1]["mean_pairs"]) == (7, 2, 8.0 / 7.0)
    # min_pairs = 2: point 6 alone is described, none of its neighbours is: W = 0, the descriptor is its own histogram
    ref2 = F.fpfh(cloud, 0.25, min_pairs=2)
    got2 = fctx.fpfh(cloud, 0.25, min_pairs=2, seams=True)
    check_integers(got2, ref2)
    check_sums(got2, ref2)
    assert list(np.nonzero(got2[1]["described_mask"])[0]) == [6] and (got2[1]["raw"] == 0).all()
    assert (got2[0][6, [5, 16, 27]] == 100).all() and got2[0][6].sum() == 300


# ---- 4: the smallest shapes -------------------------------------------------------------------------------------------------------
def test_one_and_two_points(fctx):
    cloud = lattice()
    for n in (1, 2):
        desc, info = fctx.fpfh(cloud[:n], LATTICE_R, seams=True)
        assert desc.shape == (n, 33) and np.isnan(desc).all() and not info["described_mask"].any()
        assert list(info["pairs"]) == [0, 1, 1][n - 1:2 * n - 1] and (info["raw"] == 0).all()
        assert (info["n"], info["described"], info["max_pairs"], info["mean_pairs"]) == (n, 0, n - 1, 0.0)
    desc, info = fctx.fpfh(cloud[:2], LATTICE_R, min_pairs=1)
    assert info["described"] == 2 and (desc[:, [5, 16, 27]] == 100).all() and desc.sum() == 600


@pytest.mark.parametrize("shape", ["257", "one_cell", "far"])
def test_small_shapes(fctx, shape):
    cloud = lattice()
    radius = LATTICE_R
    if shape == "257":                       # one lane past a workgroup
        cloud = cloud[:257]
    elif shape == "one_cell":                # 8 x 8 points of pitch 2^-5: the extent is below the cell of r = 0.25
        cloud, radius = np.ascontiguousarray(cloud.reshape(32, 32, 6)[:8, :8].reshape(64, 6)), 0.25
    else:                                    # 1 000 units off the origin (1000 + k / 32 is a float32)
        cloud[:, 0] += np.float32(1000.0)
    ref = F.fpfh(cloud, radius)
    assert not ref["edge_near"].any()
    got = fctx.fpfh(cloud, radius, seams=True)
    check_integers(got, ref, shape)
    check_sums(got, ref, shape)
    if shape == "far":
        check_lattice({"spfh": got[1]["spfh"], "pairs": got[1]["pairs"], "described": got[1]["described_mask"], "desc": got[0]})
    if shape == "one_cell":
        assert float((cloud[:, :3].max(0) - cloud[:, :3].min(0)).max()) < 1.03 * radius and got[1]["max_pairs"] > 36


# ---- 5: a permutation of the rows -------------------------------------------------------------------------------------------------
def test_permutation(scene, computed, fctx):
    A, D = scene
    perm = np.random.default_rng(11).permutation(len(A))
    desc, info = fctx.fpfh(np.ascontiguousarray(A[perm]), RADII[0] * D, seams=True)
    for k in INT_KEYS:
        assert same_bits(info[k], computed[0][1][k][perm]), k
    assert np.allclose(info["raw"], computed[0][1]["raw"][perm], rtol=1e-12, atol=0)


# ---- 6: determinism ---------------------------------------------------------------------------------------------------------------
def test_same_bits_on_every_run_context_and_entry_point(scene, computed, fctx):
    A, D = scene
    r = RADII[0] * D
    assert same_result(fctx.fpfh(A, r, seams=True), computed[0])
    other = plade_amd.Context(0, **ORIENTED)
    try:
        assert same_result(other.fpfh(A, r, seams=True), computed[0])
    finally:
        other.close()
    cloud = fctx.upload(A)
    try:
        res = fctx.fpfh_dev(cloud, r, seams=True, resident=True)
        assert same_result(res, computed[0]) and res[2].n == len(A)
        res[2].free()
        assert same_result(fctx.fpfh_dev(cloud, r, seams=True), computed[0])
    finally:
        cloud.free()
    s = fctx.stats()
    assert all(k in s for k in ("fpfh_grid_s", "fpfh_spfh_s", "fpfh_weight_s")) and s["fpfh_described"] == computed[0][1]["described"]


# ---- 7: the match -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tables(scene, computed, fctx):
    A, D = scene
    B = np.ascontiguousarray(sample_scene(6000, scene_seed=3, sample_seed=5))
    S, T = computed[1][0], fctx.fpfh(B, RADII[1] * D)[0]
    assert np.isnan(S[:, 0]).any()
    return S, T


def check_match(ctx, S, T, label=""):
    nn, d2 = F.nearest2(S, T)
    back, _ = F.nearest2(T, S)
    counts = []
    for mutual, ratio in ((True, 0.0), (False, 0.0), (True, 0.9), (False, 0.9)):
        corr, info = ctx.match_features(S, T, mutual=mutual, max_ratio=ratio)
        want = F.keep(nn, d2, back, mutual, ratio)
        assert same_bits(info["nn"], nn) and same_bits(info["d2"], d2) and same_bits(info["back"], back), (label, mutual, ratio)
        assert info["complete"] and info["n_corr"] == len(want) and same_bits(corr, want), (label, mutual, ratio)
        counts.append(len(want))
    return counts


def test_match_scene(tables, fctx):
    S, T = tables
    counts = check_match(fctx, S, T, "scene")
    assert counts[1] == int((~np.isnan(S[:, 0])).sum()) and 0 < counts[2] < counts[0] < counts[1] and counts[2] < counts[3] < counts[1]
    assert fctx.stats()["feat_match_s"] > 0


def test_match_small_shapes(tables, fctx):
    S, T = tables
    vs, vt = np.nonzero(~np.isnan(S[:, 0]))[0], np.nonzero(~np.isnan(T[:, 0]))[0]
    check_match(fctx, S[:65], T[:129], "65 x 129")
    check_match(fctx, S[:300], T[:plade_amd.FEAT_CHUNK + 1], "one target past a chunk")
    check_match(fctx, S[:plade_amd.FEAT_CHUNK + 1], T[:300], "one query past a chunk")
    corr, info = fctx.match_features(S[vs[:1]], T[vt[:1]], max_ratio=0.5)           # no second neighbour: kept
    assert corr.tolist() == [[0, 0]] and np.isnan(info["d2"][0, 1]) and info["d2"][0, 0] == F.delta(S[vs[:1]], T[vt[:1]])[0, 0]
    check_match(fctx, S[vs[:1]], T[vt[:1]], "1 x 1")


def test_match_ties_nan_rows_and_capacity(tables, fctx):
    S, T = tables
    hs, ht = match_table()
    check_match(fctx, hs, ht, "hand-made")
    assert fctx.match_features(hs, ht, mutual=False)[0].tolist() == [[0, 0], [2, 3], [3, 6], [4, 0], [5, 0]]
    # duplicated rows resolve to the smaller index
    dup = np.ascontiguousarray(np.concatenate([T[:200], T[:200]]))
    corr, info = fctx.match_features(T[:200], dup, mutual=False)
    v = ~np.isnan(T[:200, 0])
    assert np.array_equal(info["nn"][v], np.nonzero(v)[0]) and (info["d2"][v] == 0).all() and (info["nn"][~v] == -1).all()
    check_match(fctx, T[:200], dup, "duplicates")
    # nothing valid on one side
    corr, info = fctx.match_features(S[:70], np.full((5, 33), np.nan, np.float32))
    assert len(corr) == 0 and info["n_corr"] == 0 and (info["nn"] == -1).all() and (info["back"] == -1).all() and np.isnan(info["d2"]).all()
    # a capacity that is too small: PLADE_ECAP, the exact number, the first pairs
    full, finfo = fctx.match_features(S[:300], T[:300], mutual=False)
    assert finfo["n_corr"] > 3
    part, pinfo = fctx.match_features(S[:300], T[:300], mutual=False, cap=3)
    assert not pinfo["complete"] and pinfo["n_corr"] == finfo["n_corr"] and same_bits(part, full[:3])
    n_corr = ctypes.c_uint64()
    s300, t300 = np.ascontiguousarray(S[:300]), np.ascontiguousarray(T[:300])
    buf = np.full((3, 2), -7, np.int32)
    prm = plade_amd.FeatureMatchParams(0, 0.0)
    rc = fctx.L.plade_match_features(fctx.h, s300.ctypes.data, 300, t300.ctypes.data, 300, ctypes.byref(prm), None, None, None,
                                     buf.ctypes.data, 3, ctypes.byref(n_corr))
    assert rc == plade_amd.PLADE_ECAP and n_corr.value == finfo["n_corr"] and same_bits(buf, full[:3])
    rc = fctx.L.plade_match_features(fctx.h, s300.ctypes.data, 300, t300.ctypes.data, 300, ctypes.byref(prm), None, None, None, None, 0,
                                     ctypes.byref(n_corr))
    assert rc == 0 and n_corr.value == finfo["n_corr"]                              # no list wanted: the number alone


def test_match_resident(scene, tables, fctx):
    A, D = scene
    S, T = tables
    ca = fctx.upload(A)
    cb = fctx.upload(np.ascontiguousarray(sample_scene(6000, scene_seed=3, sample_seed=5)))
    try:
        fa = fctx.fpfh_dev(ca, RADII[1] * D, resident=True)[2]
        fb = fctx.fpfh_dev(cb, RADII[1] * D, resident=True)[2]
        for kw in ({}, {"mutual": False, "max_ratio": 0.9}):
            c0, i0 = fctx.match_features(S, T, **kw)
            c1, i1 = fctx.match_features_dev(fa, fb, **kw)
            assert same_bits(c0, c1) and i0["n_corr"] == i1["n_corr"] and all(same_bits(i0[k], i1[k]) for k in ("nn", "d2", "back"))
        fa.free(); fb.free()
    finally:
        ca.free(); cb.free()


# ---- 8: errors ----------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(fctx):
    cloud = lattice()
    L, h = fctx.L, fctx.h

    def refused(call, word):
        with pytest.raises(plade_amd.PladeError) as e:
            call()
        assert e.value.code == plade_amd.PLADE_EINVAL and word in str(e.value), str(e.value)

    for r in (0.0, -1.0, float("nan"), float("inf"), 1e-30, 1e30):
        refused(lambda: fctx.fpfh(cloud, r), "radius")
    for m in (0, -3):
        refused(lambda: fctx.fpfh(cloud, LATTICE_R, min_pairs=m), "min_pairs")
    for bad in (np.nan, np.inf):
        c = cloud.copy()
        c[17, 1] = bad
        refused(lambda: fctx.fpfh(c, LATTICE_R), "finite")
    prm, summ = plade_amd.FpfhParams(LATTICE_R, 5, 0), plade_amd.FpfhSummary()
    refused(lambda: fctx._check(L.plade_cloud_fpfh(h, cloud.ctypes.data, 0, ctypes.byref(prm), None, None, None, None, None,
                                                   ctypes.byref(summ))), "empty")
    refused(lambda: fctx._check(L.plade_cloud_fpfh(h, None, 5, ctypes.byref(prm), None, None, None, None, None, ctypes.byref(summ))), "NULL")
    refused(lambda: fctx._check(L.plade_cloud_fpfh(h, cloud.ctypes.data, 5, None, None, None, None, None, None, ctypes.byref(summ))), "NULL")
    refused(lambda: fctx._check(L.plade_cloud_fpfh(h, cloud.ctypes.data, 5, ctypes.byref(prm), None, None, None, None, None, None)), "NULL")
    refused(lambda: fctx._check(L.plade_cloud_fpfh_dev(h, None, ctypes.byref(prm), None, None, None, None, None, None, ctypes.byref(summ))), "NULL")
    S, T = match_table()
    n_corr = ctypes.c_uint64()
    for ratio in (-0.5, float("nan"), float("inf")):
        refused(lambda: fctx.match_features(S, T, max_ratio=ratio), "max_ratio")
    refused(lambda: fctx._check(L.plade_match_features(h, None, 6, T.ctypes.data, 7, None, None, None, None, None, 0, ctypes.byref(n_corr))), "NULL")
    refused(lambda: fctx._check(L.plade_match_features(h, S.ctypes.data, 6, T.ctypes.data, 7, None, None, None, None, None, 0, None)), "NULL")
    refused(lambda: fctx._check(L.plade_match_features(h, S.ctypes.data, 0, T.ctypes.data, 7, None, None, None, None, None, 0,
                                                       ctypes.byref(n_corr))), "empty")
    refused(lambda: fctx._check(L.plade_match_features_dev(h, None, None, None, None, None, None, None, 0, ctypes.byref(n_corr))), "NULL")
    with pytest.raises(ValueError):
        fctx.fpfh(cloud[:, :3], LATTICE_R)
    with pytest.raises(ValueError):
        fctx.match_features(S[:, :8], T)
    # and a good call afterwards
    desc, info = fctx.fpfh(cloud, LATTICE_R)
    check_lattice({"spfh": fctx.fpfh(cloud, LATTICE_R, seams=True)[1]["spfh"], "pairs": info["pairs"], "described": info["described_mask"],
                   "desc": desc})
    assert fctx.match_features(S, T)[0].tolist() == [[2, 3], [3, 6], [4, 0]]
