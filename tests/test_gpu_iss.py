"""ISS keypoints on the GPU (plade_cloud_keypoints_iss and its resident form, plade_features_select, plade_register_keypoints;
plade_amd/csrc/k_keypoints.hip) against the numpy restatement of their semantics (tests/iss_restate.py).

The counts are exact.  The scatter is an fp64 sum in the order of the grid walk: within the sequential-sum bound of the restatement.
Everything behind it is checked on the GPU's own previous stage, where it is an exact function of it: the eigenvalues against the
restated closed form on the GPU's scatter (only acos and cos differ: within 4 E + 4 ulp of the long-double values, E = what the
float64 restatement itself loses against long double on these inputs), the salient test on the GPU's eigenvalues and the
suppression on the GPU's saliencies bit for bit.  Against the fully independent restatement the flags are equal wherever a last-bit
difference cannot matter (iss_restate's `unsure`: nothing on these inputs).
"""
import ctypes

import numpy as np
import pytest

import plade_amd
import grid_shapes as GS
import iss_cases
import iss_restate as I
import fpfh_restate as F
import corr_pose_restate as P
from conftest import ORIENTED

pytestmark = pytest.mark.gpu

CASES = iss_cases.gpu_cases()
IDS = ["%s-rs%.3f-g%.3f" % (c[0], c[2], c[4]) for c in CASES]
ARRAYS = ("keypoint", "saliency", "eigenvalues", "count", "nms_count", "scatter")


@pytest.fixture(scope="module")
def kctx():
    c = plade_amd.Context(0, **ORIENTED)
    yield c
    c.close()


@pytest.fixture(scope="module")
def computed(kctx):
    """(index, info) of the four inputs, with the seam"""
    return [kctx.iss_keypoints(cl, rs, rn, g, g, seams=True) for _, cl, rs, rn, g in CASES]


@pytest.fixture(scope="module")
def host_loss():
    """E: the largest |l_float64 - l_longdouble| / l1 of the restated closed form over the four inputs"""
    E = 0.0
    for name, cl, rs, rn, g in CASES:
        out = iss_cases.restated(name, rs, rn, g)
        Ld = I.eigenvalues(out["scatter"], out["count"], np.longdouble)
        ok = Ld[:, 0] > 0
        E = max(E, float((np.abs(out["eigenvalues"][ok].astype(np.longdouble) - Ld[ok]).max(axis=1) / Ld[ok, 0]).max()))
    print("E (float64 against long double, all four inputs):", E)
    return E


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_result(x, y, keys=ARRAYS):
    (i0, a), (i1, b) = x, y
    return same_bits(i0, i1) and all(same_bits(a[k], b[k]) for k in keys if k in a) and all(
        a[k] == b[k] for k in ("n", "salient", "keypoints", "max_count", "n_keypoints", "complete"))


def check_against_restatement(got, ref, min_neighbours=5, gamma=0.975, flags=True):
    """items 1, 2, 4, 5 and 6 on one result"""
    index, info = got
    n = len(ref["count"])
    assert np.array_equal(info["count"], ref["count"]) and np.array_equal(info["nms_count"], ref["nms_count"])        # 1
    assert (np.abs(info["scatter"] - ref["scatter"]) <= I.moment_bound(ref["count"], ref["abs_terms"])).all()         # 2
    sal, s = I.salient_test(info["eigenvalues"], info["count"], gamma, gamma)                                         # 4
    assert same_bits(info["saliency"], s)
    key, m = I.suppress(info["saliency"], *ref["nms_pairs"], n, min_neighbours)                                       # 5
    assert np.array_equal(info["keypoint"], key) and np.array_equal(index, np.nonzero(key)[0]) and index.dtype == np.uint32
    assert info["n_keypoints"] == key.sum() == info["keypoints"] and info["complete"]
    assert (info["n"], info["salient"], info["max_count"]) == (n, int(sal.sum()), int(ref["count"].max()))
    if flags:                                                                                                         # 6
        sure = ~ref["unsure"]
        assert ref["unsure"].mean() <= 0.01
        assert np.array_equal(sal[sure], ref["salient"][sure]) and np.array_equal(info["keypoint"][sure], ref["keypoint"][sure])


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_against_the_restatement(kctx, computed, host_loss, k):
    name, cl, rs, rn, g = CASES[k]
    ref = iss_cases.restated(name, rs, rn, g)
    index, info = computed[k]
    assert not ref["unsure"].any()                            # on the restatement alone: these inputs exclude nothing
    check_against_restatement(computed[k], ref, gamma=g)
    assert np.array_equal(index, ref["index"])
    # 3: the eigenvalues against the restated closed form on the GPU's own scatter and counts, in long double
    Ld = I.eigenvalues(info["scatter"], info["count"], np.longdouble)
    L = info["eigenvalues"]
    ok = Ld[:, 0] > 0
    assert (L[~ok] == 0).all() and (L[:, 0] >= L[:, 1]).all() and (L[:, 1] >= L[:, 2]).all()
    worst = float((np.abs(L[ok].astype(np.longdouble) - Ld[ok]).max(axis=1) / Ld[ok, 0]).max())
    three = info["count"][ok] >= 3
    print(IDS[k], I.summary(ref), "GPU eigenvalues against long double, worst |dl| / l1:", worst, "over c >= 3:",
          float((np.abs(L[ok].astype(np.longdouble) - Ld[ok]).max(axis=1) / Ld[ok, 0])[three].max()), "bound", 4 * host_loss + 4 * 2.0 ** -52)
    assert worst <= 4 * host_loss + 4 * 2.0 ** -52
    # E is set by the scene's 16 points with one neighbour: l2 = l3 = 0 is a double root, where acos turns an ulp of r into 1e-8 of
    # phi.  From three points on the same rule with the restatement's loss over those points alone (1.2e-14) asks much more.
    E3 = 0.0
    for nm, _, a_, b_, g_ in CASES:
        o = iss_cases.restated(nm, a_, b_, g_)
        m3 = (o["count"] >= 3) & (o["eigenvalues"][:, 0] > 0)
        l3 = I.eigenvalues(o["scatter"][m3], o["count"][m3], np.longdouble)
        E3 = max(E3, float((np.abs(o["eigenvalues"][m3].astype(np.longdouble) - l3).max(axis=1) / l3[:, 0]).max()))
    assert float((np.abs(L[ok].astype(np.longdouble) - Ld[ok]).max(axis=1) / Ld[ok, 0])[three].max()) <= 4 * E3 + 4 * 2.0 ** -52, E3
    st = kctx.stats()
    assert {"iss_grid_s", "iss_scatter_s", "iss_nms_s", "iss_salient", "iss_keypoints"} <= set(st)


def test_stats_name_the_last_call(kctx):
    name, cl, rs, rn, g = CASES[0]
    index, info = kctx.iss_keypoints(cl, rs, rn, g, g, per_point=False)
    st = kctx.stats()
    assert st["iss_salient"] == info["salient"] and st["iss_keypoints"] == info["keypoints"] == len(index)
    assert st["iss_grid_s"] > 0 and st["iss_scatter_s"] > 0 and st["iss_nms_s"] > 0
    assert "keypoint" not in info and "scatter" not in info


# ---- 7: the radii are strict, in fp32 -------------------------------------------------------------------------------------------------
def test_a_neighbour_at_the_radius_is_out_and_one_ulp_nearer_is_in(kctx):
    near = np.nextafter(np.float32(0.25), np.float32(0))
    P3 = np.array([[0, 0, 0], [0.25, 0, 0], [-near, 0, 0], [0, 0, 0.25], [0, -near, 0]], np.float32)
    assert near < 0.25 and np.float32(near * near) < np.float32(0.0625)
    for rs, rn, c0, m0 in ((0.25, 0.25, 3, 3), (0.25, 0.0, 3, 3), (0.5, 0.25, 5, 3), (0.25, 0.5, 3, 5)):
        index, info = kctx.iss_keypoints(P3, rs, rn, seams=True)
        ref = I.iss(P3, rs, rn)
        check_against_restatement((index, info), ref)
        assert info["count"][0] == c0 and info["nms_count"][0] == m0, (rs, rn)      # rows 2 and 4 are in, rows 1 and 3 are not


def test_zero_non_max_radius_is_the_salient_radius(kctx, computed):
    name, cl, rs, rn, g = CASES[0]
    assert rn == rs
    assert same_result(kctx.iss_keypoints(cl, rs, 0.0, g, g, seams=True), computed[0])


def test_ties_and_min_neighbours(kctx):
    """a coincident pair has one saliency: the smaller index is the keypoint; min_neighbours counts the OTHER points within rn"""
    cloud = iss_cases.tie_cloud()
    a, b = iss_cases.TIE_PAIR
    for mn, want in ((1, True), (2, False)):
        index, info = kctx.iss_keypoints(cloud, 1.0, 0.5, min_neighbours=mn, seams=True)
        ref = I.iss(cloud, 1.0, 0.5, min_neighbours=mn)
        check_against_restatement((index, info), ref, min_neighbours=mn, flags=False)
        assert info["saliency"][a] == info["saliency"][b] > 0 and same_bits(info["scatter"][a], info["scatter"][b])
        assert info["nms_count"][a] == 2 and bool(info["keypoint"][a]) == want and not info["keypoint"][b]
        assert np.array_equal(info["keypoint"], ref["keypoint"])
        assert info["count"][iss_cases.TIE_LONELY] == 2 and info["saliency"][iss_cases.TIE_LONELY] == 0


# ---- 8: small and degenerate sizes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, 3))
def test_tiny_clouds_have_nothing_salient(kctx, n):
    cloud = np.random.default_rng(n).uniform(0, 0.2, (n, 3)).astype(np.float32)
    index, info = kctx.iss_keypoints(cloud, 1.0, min_neighbours=1, seams=True)
    check_against_restatement((index, info), I.iss(cloud, 1.0, min_neighbours=1), min_neighbours=1)
    assert (info["count"] == n).all() and info["salient"] == 0 and len(index) == 0 and not info["keypoint"].any()


def test_257_points_one_cell_and_far_from_the_origin(kctx):
    rng = np.random.default_rng(257)
    cloud = rng.uniform(0, 1, (257, 3)).astype(np.float32)
    ref = I.iss(cloud, 0.3)
    check_against_restatement(kctx.iss_keypoints(cloud, 0.3, seams=True), ref)
    assert ref["salient"].sum() > 100 and 0 < ref["keypoint"].sum() < 60
    # every point inside one cell: everybody is everybody's neighbour
    tiny = (cloud * np.float32(2.0 ** -6)).astype(np.float32)
    index, info = kctx.iss_keypoints(tiny, 1.0, seams=True)
    check_against_restatement((index, info), I.iss(tiny, 1.0))
    assert (info["count"] == 257).all() and (info["nms_count"] == 257).all() and len(index) <= 1
    # dyadic coordinates 1 000 units off the origin: the differences are the same numbers, so are the flags
    dy = (rng.integers(0, 128, (300, 3)) * 2.0 ** -6).astype(np.float32)
    far = dy + np.float32(1000.0)
    assert np.array_equal((far - np.float32(1000.0)), dy)
    i0, a = kctx.iss_keypoints(dy, 0.5, seams=True)
    i1, b = kctx.iss_keypoints(far, 0.5, seams=True)
    check_against_restatement((i0, a), I.iss(dy, 0.5))
    assert np.array_equal(i0, i1) and len(i0) > 0 and all(np.array_equal(a[k], b[k]) for k in ("count", "nms_count", "keypoint"))
    assert np.array_equal(a["saliency"] > 0, b["saliency"] > 0)


@pytest.mark.parametrize("name", GS.SHAPES)
def test_grid_shapes(kctx, name):
    cloud = GS.cloud(name)
    ref = I.iss(cloud, GS.R)
    index, info = kctx.iss_keypoints(cloud, GS.R, seams=True)
    check_against_restatement((index, info), ref)
    if name != "capped":
        assert info["salient"] == 0 and len(index) == 0 and (info["saliency"] == 0).all()      # a line, a plane: flat by arithmetic
    else:
        assert info["salient"] > 0 and info["count"][-3:].tolist() == [1, 2, 2]
        st = kctx.stats()
        assert st["iss_grid_cell"] >= 4.0 * GS.radius_cell(cloud)


# ---- 9, 10, 11 --------------------------------------------------------------------------------------------------------------------------
def test_permuting_the_rows_permutes_the_answer(kctx, computed):
    name, cl, rs, rn, g = CASES[0]
    perm = np.random.default_rng(9).permutation(len(cl))
    index, info = kctx.iss_keypoints(np.ascontiguousarray(cl[perm]), rs, rn, g, g)
    first = computed[0][1]
    assert np.array_equal(info["count"], first["count"][perm]) and np.array_equal(info["nms_count"], first["nms_count"][perm])
    assert np.array_equal(info["keypoint"], first["keypoint"][perm]) and np.array_equal(info["saliency"] > 0, first["saliency"][perm] > 0)
    assert np.array_equal(index, np.nonzero(first["keypoint"][perm])[0])


def test_identical_bits(kctx, computed):
    name, cl, rs, rn, g = CASES[1]
    first = computed[1]
    assert same_result(kctx.iss_keypoints(cl, rs, rn, g, g, seams=True), first)
    other = plade_amd.Context(0, **ORIENTED)
    try:
        assert same_result(other.iss_keypoints(cl, rs, rn, g, g, seams=True), first)
    finally:
        other.close()
    c = kctx.upload(cl)
    try:
        assert same_result(kctx.iss_keypoints_dev(c, rs, rn, g, g, seams=True), first)
    finally:
        c.free()
    xyz = np.ascontiguousarray(cl[:, :3])                    # another stride: the same points, the same grid
    assert same_result(kctx.iss_keypoints(xyz, rs, rn, g, g, seams=True), first)


def test_a_small_capacity(kctx, computed):
    name, cl, rs, rn, g = CASES[0]
    full, finfo = computed[0]
    part, pinfo = kctx.iss_keypoints(cl, rs, rn, g, g, cap=7)
    assert len(full) > 7 and not pinfo["complete"] and pinfo["n_keypoints"] == len(full) and same_bits(part, full[:7])
    prm, summ, total = plade_amd.IssParams(rs, rn, g, g, 5, 0), plade_amd.IssSummary(), ctypes.c_uint64()
    buf = np.full(7, 0xffffffff, np.uint32)
    args = [kctx.h, cl.ctypes.data, len(cl), 6, ctypes.byref(prm), None, buf.ctypes.data, 7, ctypes.byref(total), None, None, None, None,
            None, ctypes.byref(summ)]
    assert kctx.L.plade_cloud_keypoints_iss(*args) == plade_amd.PLADE_ECAP and total.value == len(full) and same_bits(buf, full[:7])
    assert summ.keypoints == len(full)
    args[6], args[7] = None, 0                               # no list wanted: the number alone
    assert kctx.L.plade_cloud_keypoints_iss(*args) == 0 and total.value == len(full)


# ---- 12: errors -------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(kctx, computed):
    name, cl, rs, rn, g = CASES[0]
    L, h = kctx.L, kctx.h

    def refused(call, word):
        with pytest.raises(plade_amd.PladeError) as e:
            call()
        assert e.value.code == plade_amd.PLADE_EINVAL and word in str(e.value), str(e.value)

    for r in (0.0, -1.0, float("nan"), float("inf"), 1e-30, 1e30):
        refused(lambda: kctx.iss_keypoints(cl, r), "salient_radius")
    for r in (-1.0, float("nan"), float("inf"), 1e-30, 1e30):
        refused(lambda: kctx.iss_keypoints(cl, rs, r), "non_max_radius")
    for bad in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        refused(lambda: kctx.iss_keypoints(cl, rs, gamma21=bad), "gamma")
        refused(lambda: kctx.iss_keypoints(cl, rs, gamma32=bad), "gamma")
    for m in (0, -3):
        refused(lambda: kctx.iss_keypoints(cl, rs, min_neighbours=m), "min_neighbours")
    for bad in (np.nan, np.inf):
        c = cl.copy()
        c[17, 1] = bad
        refused(lambda: kctx.iss_keypoints(c, rs), "finite")
    prm, summ, total = plade_amd.IssParams(rs, rn, g, g, 5, 0), plade_amd.IssSummary(), ctypes.c_uint64()
    args = [h, cl.ctypes.data, len(cl), 6, ctypes.byref(prm), None, None, 0, ctypes.byref(total), None, None, None, None, None,
            ctypes.byref(summ)]
    for k, v, word in ((1, None, "NULL"), (4, None, "NULL"), (14, None, "NULL"), (2, 0, "empty"), (3, 2, "stride")):
        a = list(args); a[k] = v
        refused(lambda: kctx._check(L.plade_cloud_keypoints_iss(*a)), word)
    refused(lambda: kctx._check(L.plade_cloud_keypoints_iss_dev(h, None, ctypes.byref(prm), None, None, 0, None, None, None, None, None, None,
                                                                ctypes.byref(summ))), "NULL")
    with pytest.raises(ValueError):
        kctx.iss_keypoints(cl[:, :2], rs)
    assert same_result(kctx.iss_keypoints(cl, rs, rn, g, g, seams=True), computed[0])


# ---- 13: the rows of a resident table at the keypoints ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def terrain_tables(kctx):
    """the terrain pair resident, its descriptors on the host and on the device"""
    tg, sr, T = iss_cases.terrain()
    cs, ct = kctx.upload(sr), kctx.upload(tg)
    ds, i_s, fs = kctx.fpfh_dev(cs, iss_cases.TERRAIN["radius"], resident=True)
    dt, i_t, ft = kctx.fpfh_dev(ct, iss_cases.TERRAIN["radius"], resident=True)
    yield dict(cs=cs, ct=ct, ds=ds, dt=dt, fs=fs, ft=ft, i_s=i_s, i_t=i_t)
    fs.free(); ft.free(); cs.free(); ct.free()


def test_select_features(kctx, computed, terrain_tables):
    t = terrain_tables
    index = computed[2][0]
    rows = np.ascontiguousarray(t["ds"][index])
    sel = kctx.select_features(t["fs"], index)
    try:
        assert sel.n == len(index)
        # bit for bit: against the table they were taken from every valid row finds itself (or an identical row) at distance 0 ...
        corr, info = kctx.match_features_dev(sel, t["fs"], mutual=False)
        valid = ~np.isnan(rows[:, 0])
        assert valid.sum() > 200 and (info["d2"][valid, 0] == 0).all() and (info["nn"][~valid] == -1).all()
        assert same_bits(t["ds"][info["nn"][valid]], rows[valid])
        # ... and the match of the selected table is the match of the gathered host rows
        for kw in ({}, {"mutual": False, "max_ratio": 0.9}):
            c0, i0 = kctx.match_features(rows, t["dt"], **kw)
            c1, i1 = kctx.match_features_dev(sel, t["ft"], **kw)
            assert same_bits(c0, c1) and i0["n_corr"] == i1["n_corr"] > 0 and all(same_bits(i0[k], i1[k]) for k in ("nn", "d2", "back"))
        twice = t["fs"].select([5, 5, 0])                     # any list of rows: repeats, any order
        try:
            c2, i2 = kctx.match_features_dev(twice, t["fs"], mutual=False)
            assert twice.n == 3 and same_bits(i2["d2"], kctx.match_features(t["ds"][[5, 5, 0]], t["ds"], mutual=False)[1]["d2"])
        finally:
            twice.free()
    finally:
        sel.free()
    for bad in ([len(t["ds"])], [0, 1, 2 ** 31], []):
        with pytest.raises(plade_amd.PladeError) as e:
            kctx.select_features(t["fs"], bad)
        assert e.value.code == plade_amd.PLADE_EINVAL and "plade_features_select" in str(e.value)
    with pytest.raises(ValueError):
        kctx.select_features(t["fs"], [-1])


# ---- 14, 15: the keypoints in front of the match ------------------------------------------------------------------------------------------
def chained_by_hand(ctx, t, sr, tg, seed=0, mutual=True):
    """ISS, the selection, the match and the pose as public calls; the list in original source indices"""
    K = iss_cases.TERRAIN
    index, ki = ctx.iss_keypoints_dev(t["cs"], K["salient_radius"], K["non_max_radius"])
    sel = ctx.select_features(t["fs"], index)
    try:
        corr, mi = ctx.match_features_dev(sel, t["ft"], mutual=mutual)
    finally:
        sel.free()
    corr = corr.copy()
    corr[:, 0] = index[corr[:, 0]].astype(np.int32)
    return index, ki, corr, ctx.estimate_pose_dev(t["cs"], t["ct"], corr, K["inlier_dist"], seed=seed)


def test_register_keypoints_is_the_chain(kctx, terrain_tables):
    tg, sr, T = iss_cases.terrain()
    t, K = terrain_tables, iss_cases.TERRAIN
    for seed, mutual in ((0, True), (3, False)):
        index, ki, corr, (Tc, ci) = chained_by_hand(kctx, t, sr, tg, seed, mutual)
        Tr, ri = kctx.register_keypoints(tg, sr, K["radius"], K["inlier_dist"], K["salient_radius"], K["non_max_radius"], seed=seed,
                                         mutual=mutual)
        Td, rd = kctx.register_keypoints_dev(t["ct"], t["cs"], K["radius"], K["inlier_dist"], K["salient_radius"], K["non_max_radius"],
                                             seed=seed, mutual=mutual)
        for Tx, x in ((Tr, ri), (Td, rd)):
            assert same_bits(x["corr"], corr) and x["n_corr"] == len(corr) and x["corr"][:, 0].max() >= len(index)
            assert same_bits(Tx, Tc) and same_bits(x["T64"], ci["T64"]) and x["ok"] == ci["ok"]
            for k in ("hypotheses", "scored", "best_hypothesis", "best_count", "inliers", "refinements", "failure", "rmse", "fitness"):
                assert np.float64(x[k]).tobytes() == np.float64(ci[k]).tobytes(), k
            assert x["iss"] == {k: ki[k] for k in ("n", "salient", "keypoints", "max_count")}
            for k in ("n", "described", "mean_pairs", "max_pairs"):
                assert x["fpfh_src"][k] == t["i_s"][k] and x["fpfh_tgt"][k] == t["i_t"][k]


def test_register_keypoints_without_keypoints_fails_like_too_few(kctx):
    tg, sr, T = iss_cases.terrain()
    K = iss_cases.TERRAIN
    Tr, ri = kctx.register_keypoints(tg, sr, K["radius"], K["inlier_dist"], K["salient_radius"], K["non_max_radius"], min_neighbours=5000)
    assert not ri["ok"] and ri["failure"] == plade_amd.PLADE_CORR_POSE_TOO_FEW and ri["n_corr"] == 0 and ri["iss"]["keypoints"] == 0
    assert np.array_equal(Tr, np.eye(4, dtype=np.float32)) and ri["fpfh_src"]["n"] == len(sr)
    with pytest.raises(plade_amd.PladeError) as e:
        kctx.register_keypoints(tg, sr, K["radius"], K["inlier_dist"], 0.0)
    assert e.value.code == plade_amd.PLADE_EINVAL and "salient_radius" in str(e.value)


def test_end_to_end_on_the_terrain_pair(kctx, computed, terrain_tables):
    """15: the restated chain on the CPU first, then the GPU's pose within the bounds of the full chain (2 degrees, 0.1), from a match
    that ran on fewer than 5 % of the source rows"""
    tg, sr, T = iss_cases.terrain()
    K = iss_cases.TERRAIN
    ref = iss_cases.restated("terrain", K["salient_radius"], K["non_max_radius"], 0.975)
    fs, ft = F.fpfh(sr, K["radius"]), F.fpfh(tg, K["radius"])
    m = F.match(fs["desc"][ref["index"]], ft["desc"], mutual=True)
    corr = m["corr"].astype(np.int32)
    corr[:, 0] = ref["index"][corr[:, 0]]
    Sc, Qc = P.packed(np.ascontiguousarray(sr[:, :3]), np.ascontiguousarray(tg[:, :3]), corr)
    est = P.estimate(Sc, Qc, K["inlier_dist"], seed=0, H=65536)
    rot, tr = P.pose_error(est["T"], T)
    print("restated chain: keypoints", len(ref["index"]), "correspondences", len(corr), "rot", rot, "trans", tr)
    assert est["ok"] and rot < 0.5 and tr < 0.06              # (0.38 degrees and 0.044)
    Tg, info = kctx.register_keypoints(tg, sr, K["radius"], K["inlier_dist"], K["salient_radius"], K["non_max_radius"], hypotheses=65536,
                                       seed=0, mutual=True)
    assert info["ok"], info["reason"]
    rot, tr = P.pose_error(info["T64"], T)
    share = info["iss"]["keypoints"] / len(sr)
    print("GPU: keypoints", info["iss"]["keypoints"], "share", share, "correspondences", info["n_corr"], "inliers", info["inliers"],
          "rot", rot, "trans", tr)
    assert rot < 2.0 and tr < 0.1
    assert share < 0.05 and info["iss"]["keypoints"] == len(computed[2][0])
    Ti, ii = kctx.refine_icp(tg, sr, Tg)
    rot2, tr2 = P.pose_error(Ti, T)
    print("after ICP: rot", rot2, "trans", tr2)
    assert rot2 < 2.0 and tr2 < 0.1
