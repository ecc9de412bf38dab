"""M3C2 distances on the GPU (plade_cloud_m3c2 / plade_cloud_m3c2_dev, plade_amd/csrc/k_m3c2.hip) against the numpy restatement of
their semantics (tests/m3c2_restate.py: brute force over all points, the fp64 expressions of m3c2.h term for term).

Counts and the valid flag bit for bit; S1 and S2 within 1e-12 of the sum of the absolute values of their terms (a few hundred
fp64 terms at 2^-53 each: four orders of margin); the derived values from the GPU's own counts and moments to 1e-14 relative (a
handful of correctly rounded fp64 operations each); the distance against the restatement within 1e-12 (sum|t|_A / c_A +
sum|t|_B / c_B); the significance flags equal wherever the restated | |distance| - lod | is at least 1e-9 L (the test asserts on
the restatement alone that this excludes at most 1 % of the valid core points -- here none).
"""
import ctypes

import numpy as np
import pytest

import plade_amd
import m3c2_restate as M
from plade_amd.synth import _faces, make_pair, random_se3, sample_scene
from conftest import ORIENTED
from test_m3c2_host import PITCH, PLANE_L, PLANE_R, PLANE_REG, check_planes, planes

pytestmark = pytest.mark.gpu

MIN_POINTS = 4
SCENE_PARAMS = ((0.01, 0.04), (0.02, 0.04), (0.03, 0.08))      # (R, L) in units of the diagonal D
LONG_PARAMS = ((0.01, 0.2), (0.005, 0.5))
AXES6 = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))


@pytest.fixture(scope="module")
def mctx():
    c = plade_amd.Context(0, **ORIENTED)
    yield c
    c.close()


def diag(P):
    return float(np.linalg.norm(P[:, :3].max(0).astype(np.float64) - P[:, :3].min(0).astype(np.float64)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_result(x, y):
    """two (distance, info) results of Context.m3c2 with per_point and moments: every array and the summary, bit for bit"""
    (d0, i0), (d1, i1) = x, y
    keys = ("lod", "significant_mask", "count", "sigma", "moments")
    scal = ("m", "valid", "significant", "mean", "rms", "max", "max_count")
    return (same_bits(d0, d1) and all(same_bits(i0[k], i1[k]) for k in keys)
            and all(np.float64(i0[k]).tobytes() == np.float64(i1[k]).tobytes() for k in scal))


def moved_pair(tilted):
    """A = the scene sampled with seed 4, B = the same scene sampled with seed 5 with the face of 7th-largest support (ties: the
    smaller face id) moved 5 cm along its normal."""
    A = np.ascontiguousarray(sample_scene(20000, scene_seed=3, sample_seed=4, tilted=tilted))
    B, lb = sample_scene(20000, scene_seed=3, sample_seed=5, tilted=tilted, return_labels=True)
    support = np.bincount(lb[lb >= 0])
    fid = int(np.argsort(-support, kind="stable")[6])
    nrm = np.asarray(_faces(3, 8, tilted=tilted)[fid][3], np.float64)
    B = np.ascontiguousarray(B)
    B[lb == fid, :3] = (B[lb == fid, :3].astype(np.float64) + 0.05 * nrm).astype(np.float32)
    return A, B


def check_against(got, ref, L, label=""):
    """counts, valid, moments, distance and flags of a GPU result (moments=True) against a restatement (checks 1, 3 and 4)"""
    dist, info = got
    assert info["count"].dtype == np.uint32 and np.array_equal(info["count"], ref["count"]), label
    valid = ~np.isnan(dist)
    assert np.array_equal(valid, ref["valid"]) and info["valid"] == int(ref["valid"].sum()), label
    err = np.abs(info["moments"] - ref["moments"])
    print(f"{label} moments: max err / mag = {np.max(err / np.maximum(ref['mag'], 1e-300)):.3e}")
    assert (err <= 1e-12 * ref["mag"]).all(), label
    v = ref["valid"]
    c = ref["count"][v].astype(np.float64)
    bound = 1e-12 * (ref["mag"][v, 0] / c[:, 0] + ref["mag"][v, 2] / c[:, 1])
    derr = np.abs(dist[v] - ref["distance"][v])
    print(f"{label} distance: max err = {derr.max() if len(derr) else 0.0:.3e}")
    assert (derr <= bound).all(), label
    band = np.abs(np.abs(ref["distance"][v]) - ref["lod"][v]) >= 1e-9 * L
    assert (~band).sum() <= 0.01 * v.sum(), label                    # (on the restatement alone)
    assert np.array_equal(info["significant_mask"][v][band], ref["significant"][v][band]), label
    assert not info["significant_mask"][~v].any() and np.isnan(info["lod"][~v]).all() and np.isnan(info["sigma"][~v]).all(), label


def check_derived(got, has_axis, min_points=MIN_POINTS, reg_error=0.0):
    """distance, lod, sigma and significant recomputed from the GPU's own counts and moments (check 4)"""
    dist, info = got
    mo, cnt = info["moments"], info["count"]
    own = M.derive(has_axis, cnt[:, 0], mo[:, 0], mo[:, 1], cnt[:, 1], mo[:, 2], mo[:, 3], min_points, reg_error)
    v = own["valid"]
    assert np.array_equal(v, ~np.isnan(dist))

    def close(a, b):
        return (np.abs(a - b) <= 1e-14 * np.abs(b)).all()
    assert close(dist[v], own["distance"][v]) and close(info["lod"][v], own["lod"][v]) and close(info["sigma"][v], own["sigma"][v])
    assert np.array_equal(info["significant_mask"], v & (np.abs(np.where(v, dist, 0.0)) > np.where(v, info["lod"], 0.0)))


class Scene:
    """The two 20k clouds, their core points, the restatement at every (R, L) and the GPU's answer at each (computed once, never
    changed)."""
    def __init__(self, ctx, tilted, params, random_normals):
        self.A, self.B = moved_pair(tilted)
        self.D = diag(self.A)
        self.core = np.ascontiguousarray(self.A[::10])
        if random_normals:
            rng = np.random.default_rng(7)
            v = rng.normal(size=(len(self.core), 3))
            v /= np.linalg.norm(v, axis=1, keepdims=True)
            self.core[:, 3:] = (v * rng.uniform(0.5, 2.0, len(self.core))[:, None]).astype(np.float32)
        self.params = [(r * self.D, l * self.D) for r, l in params]
        self.ref = M.m3c2(self.core, self.A, self.B, self.params, min_points=MIN_POINTS)
        self.gpu = [ctx.m3c2(self.core, self.A, self.B, R, L, min_points=MIN_POINTS, moments=True) for R, L in self.params]


@pytest.fixture(scope="module")
def scene(mctx):
    return Scene(mctx, False, SCENE_PARAMS, False)


@pytest.fixture(scope="module")
def tilted(mctx):
    return Scene(mctx, True, LONG_PARAMS, True)


# ---- 1, 3, 4. counts, moments and derived values on a scene ----------------------------------------------------------------------
@pytest.mark.parametrize("t", [0, 1, 2])
def test_counts_moments_and_flags_of_a_20k_scene(scene, t):
    ref, (R, L) = scene.ref[t], scene.params[t]
    ca = ref["count"][:, 0]
    print(f"D = {scene.D:.2f}, (R, L) = {SCENE_PARAMS[t]} D: valid {ref['valid'].sum()}, median c_A {np.median(ca):.0f}, max c_A {ca.max()}, "
          f"significant {ref['significant'].sum()}")
    assert abs(scene.D - 13.20) < 0.005
    assert (int(ref["valid"].sum()), int(np.median(ca)), int(ca.max())) == ((859, 5, 45), (1969, 16, 113), (1994, 46, 260))[t]
    check_against(scene.gpu[t], ref, L, f"scene {t}")
    check_derived(scene.gpu[t], ref["has_axis"])
    band = np.abs(np.abs(ref["distance"]) - ref["lod"])[ref["valid"]] >= 1e-9 * L
    assert band.all()                                               # on these inputs the band excludes nothing
    assert scene.gpu[t][1]["max_count"] == int(ref["count"].max()) and scene.gpu[t][1]["m"] == 2000


# ---- 2. long thin cylinders in arbitrary directions ------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [0, 1])
def test_long_thin_cylinders_in_arbitrary_directions(tilted, t):
    ref, (R, L) = tilted.ref[t], tilted.params[t]
    ca = ref["count"][:, 0]
    print(f"(R, L) = {LONG_PARAMS[t]} D: median c_A {np.median(ca):.0f}, max c_A {ca.max()}, min c_A {ca.min()}")
    assert ca.min() > 0
    check_against(tilted.gpu[t], ref, L, f"tilted {t}")
    check_derived(tilted.gpu[t], ref["has_axis"])


def test_axis_aligned_cylinders(mctx, tilted):
    """the six axis-aligned normals on the first 500 core points: a cover that is wrong for one dominant axis shows here"""
    R, L = tilted.params[0]
    core = np.concatenate([tilted.core[:500]] * 6)
    core[:, 3:] = np.repeat(np.asarray(AXES6, np.float32), 500, axis=0)
    core = np.ascontiguousarray(core)
    ref = M.m3c2(core, tilted.A, tilted.B, [(R, L)], min_points=MIN_POINTS)[0]
    got = mctx.m3c2(core, tilted.A, tilted.B, R, L, min_points=MIN_POINTS, moments=True)
    assert ref["count"][:, 0].min() > 0
    check_against(got, ref, L, "axes")
    # opposite normals: the same cylinder, the opposite sign
    d = got[0].reshape(6, 500)
    for k in (0, 2, 4):
        assert np.array_equal(got[1]["count"][500 * k:500 * (k + 1)], got[1]["count"][500 * (k + 1):500 * (k + 2)])
        v = ~np.isnan(d[k])
        assert np.allclose(d[k][v], -d[k + 1][v], rtol=0, atol=1e-12)


# ---- 5. exact boundaries ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("roll", [0, 1, 2])
def test_points_exactly_on_the_boundary(mctx, roll):
    """dyadic coordinates, the normal along +z (rolled to x and y): rho exactly R is out, one fp32 ulp nearer is in; |t| exactly L
    is in, one ulp beyond is out"""
    R, L = 0.375, 0.5
    one, f = np.float32(1), np.float32
    near = np.nextafter(f(R), f(0))
    far = np.nextafter(f(L), one)
    pts = np.array([[R, 0, 0.125], [near, 0, 0.125], [0, R, -0.25], [0, -near, -0.25], [0, 0, L], [0, 0, far], [0, 0, -L], [0, 0, -far],
                    [0.25, 0.25, 0.0625]], np.float32)
    inside = np.array([0, 1, 0, 1, 1, 0, 1, 0, 1], bool)
    core = np.array([[0, 0, 0, 0, 0, 2.0]], np.float32)
    pts = np.ascontiguousarray(np.roll(pts, roll, axis=1))
    core[0, :3] = np.roll(core[0, :3], roll)
    core[0, 3:] = np.roll(core[0, 3:], roll)
    for k in range(len(pts)):                                        # each point alone with an inside one, then all together
        two = np.ascontiguousarray(pts[[k, 8]])
        d, info = mctx.m3c2(core, two, two, R, L, min_points=2, moments=True)
        assert list(info["count"][0]) == [1 + int(inside[k])] * 2, (roll, k)
    d, info = mctx.m3c2(core, pts, pts[inside], R, L, min_points=2, moments=True)
    assert list(info["count"][0]) == [5, 5]
    t = np.roll(pts[inside], -roll, axis=1)[:, 2].astype(np.float64)
    assert info["moments"][0, 0] == t.sum() and info["moments"][0, 1] == (t * t).sum() and d[0] == 0.0
    ref = M.m3c2(core, pts, pts[inside], [(R, L)], min_points=2)[0]
    assert list(ref["count"][0]) == [5, 5]


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_two_exact_planes_bit_for_bit(mctx, sign):
    core, A, B = planes((0.0, 0.0, sign))
    d, info = mctx.m3c2(core, A, B, PLANE_R, PLANE_L, reg_error=PLANE_REG, moments=True)
    check_planes({"distance": d, "lod": info["lod"], "significant": info["significant_mask"], "count": info["count"]}, sign)
    assert (info["sigma"] == 0).all() and (info["moments"][:, 0] == 0).all()
    assert (info["moments"][:, 2] == sign * info["count"][:, 1] * PITCH).all()
    assert (info["m"], info["valid"], info["significant"], info["mean"], info["rms"], info["max"], info["max_count"]) == (
        586, 586, 586, sign * PITCH, PITCH, PITCH, 129)


# ---- 6. the transform ------------------------------------------------------------------------------------------------------------
def test_compared_cloud_in_another_frame(mctx, scene):
    R, L = scene.params[1]
    T = random_se3(41).astype(np.float32)
    Ti = np.linalg.inv(T.astype(np.float64))
    Bo = np.ascontiguousarray(scene.B.copy())
    Bo[:, :3] = (scene.B[:, :3].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
    ref = M.m3c2(scene.core, scene.A, Bo, [(R, L)], T=T, min_points=MIN_POINTS)[0]
    got = mctx.m3c2(scene.core, scene.A, Bo, R, L, T=T, min_points=MIN_POINTS, moments=True)
    check_against(got, ref, L, "frame")
    assert ref["valid"].sum() > 1900


def test_no_transform_is_the_identity_matrix(mctx, scene):
    R, L = scene.params[1]
    eye = mctx.m3c2(scene.core, scene.A, scene.B, R, L, T=np.eye(4, dtype=np.float32), min_points=MIN_POINTS, moments=True)
    assert same_result(eye, scene.gpu[1])


# ---- 7. the edges of the grids ---------------------------------------------------------------------------------------------------
def test_compared_cloud_cropped_to_half_the_scene(mctx, scene):
    """core points lie outside B's grid and cylinders cross its edge"""
    R, L = scene.params[1]
    half = np.ascontiguousarray(scene.B[scene.B[:, 0] < 0.0])
    ref = M.m3c2(scene.core, scene.A, half, [(R, L)], min_points=MIN_POINTS)[0]
    got = mctx.m3c2(scene.core, scene.A, half, R, L, min_points=MIN_POINTS, moments=True)
    check_against(got, ref, L, "cropped")
    assert 0 < (ref["count"][:, 1] == 0).sum() < len(scene.core) and 0 < ref["valid"].sum()
    # ... and with long oblique cylinders that enter and leave the grid
    Rl, Ll = 0.01 * scene.D, 0.2 * scene.D
    core = scene.core[::4].copy()
    rng = np.random.default_rng(9)
    core[:, 3:] = rng.normal(size=(len(core), 3)).astype(np.float32)
    ref = M.m3c2(core, scene.A, half, [(Rl, Ll)], min_points=MIN_POINTS)[0]
    check_against(mctx.m3c2(core, scene.A, half, Rl, Ll, min_points=MIN_POINTS, moments=True), ref, Ll, "cropped, oblique")


def test_scene_far_from_the_origin(mctx, scene):
    """100 D away the shift is not exact in fp32: the restatement is that of the shifted floats"""
    R, L = scene.params[1]
    shift = (100.0 * scene.D / np.sqrt(3.0)) * np.ones(3)
    A, B = scene.A.copy(), scene.B.copy()
    A[:, :3] = (scene.A[:, :3].astype(np.float64) + shift).astype(np.float32)
    B[:, :3] = (scene.B[:, :3].astype(np.float64) + shift).astype(np.float32)
    core = np.ascontiguousarray(A[::10])
    ref = M.m3c2(core, A, B, [(R, L)], min_points=MIN_POINTS)[0]
    check_against(mctx.m3c2(core, A, B, R, L, min_points=MIN_POINTS, moments=True), ref, L, "shifted")
    assert ref["valid"].sum() > 1800


def test_one_core_point_one_reference_point_and_coincident_points(mctx, scene):
    R, L = scene.params[1]
    one = np.ascontiguousarray(scene.core[123:124])
    ref = M.m3c2(one, scene.A, scene.B, [(R, L)], min_points=MIN_POINTS)[0]
    check_against(mctx.m3c2(one, scene.A, scene.B, R, L, min_points=MIN_POINTS, moments=True), ref, L, "m = 1")
    # n_A = 1: the core point's own point; never valid at min_points >= 2
    a1 = np.ascontiguousarray(scene.A[1230:1231])
    d, info = mctx.m3c2(one, a1, scene.B, R, L, min_points=2, moments=True)
    assert info["count"][0, 0] == 1 and info["count"][0, 1] == ref["count"][0, 1] and np.isnan(d[0]) and info["valid"] == 0
    assert np.isnan(info["mean"]) and np.isnan(info["rms"]) and np.isnan(info["max"]) and info["significant"] == 0
    assert info["moments"][0, 0] == 0.0 and info["moments"][0, 1] == 0.0
    # 50 coincident points in each cloud, 2^-4 apart along the normal
    pa = np.tile(np.array([[0.25, 4.0, -1.5]], np.float32), (50, 1))
    pb = pa.copy()
    pb[:, 2] += np.float32(0.0625)
    core = np.array([[0.25, 4.0, -1.5, 0, 0, 1]], np.float32)
    d, info = mctx.m3c2(core, pa, pb, 0.5, 1.0, moments=True)
    assert list(info["count"][0]) == [50, 50] and d[0] == 0.0625 and (info["sigma"] == 0).all() and info["lod"][0] == 0.0
    assert info["significant_mask"][0] and list(info["moments"][0]) == [0.0, 0.0, 50 * 0.0625, 50 * 0.0625 ** 2]


def test_core_points_without_an_axis(mctx, scene):
    R, L = scene.params[1]
    core = scene.core.copy()
    core[17, 4] = np.nan
    core[40, 3:] = 0.0
    core[77, 3] = np.inf
    core = np.ascontiguousarray(core)
    d, info = mctx.m3c2(core, scene.A, scene.B, R, L, min_points=MIN_POINTS, moments=True)
    bad = [17, 40, 77]
    assert (info["count"][bad] == 0).all() and (info["moments"][bad] == 0).all()
    assert np.isnan(d[bad]).all() and np.isnan(info["lod"][bad]).all() and np.isnan(info["sigma"][bad]).all()
    assert not info["significant_mask"][bad].any()
    keep = np.ones(len(core), bool)
    keep[bad] = False
    d0, i0 = scene.gpu[1]
    assert same_bits(d[keep], d0[keep]) and same_bits(info["count"][keep], i0["count"][keep]) and same_bits(info["moments"][keep], i0["moments"][keep])
    assert info["valid"] == int((~np.isnan(d)).sum())


# ---- 8. the same bits ------------------------------------------------------------------------------------------------------------
def test_same_bits_from_every_entry_point(mctx, scene):
    R, L = scene.params[1]
    kw = dict(min_points=MIN_POINTS, reg_error=0.003, moments=True)
    first = mctx.m3c2(scene.core, scene.A, scene.B, R, L, **kw)
    assert same_result(mctx.m3c2(scene.core, scene.A, scene.B, R, L, **kw), first)
    other = plade_amd.Context(0)
    try:
        assert same_result(other.m3c2(scene.core, scene.A, scene.B, R, L, **kw), first)
    finally:
        other.close()
    # xyz rows and wider rows
    assert same_result(mctx.m3c2(scene.core, np.ascontiguousarray(scene.A[:, :3]), np.ascontiguousarray(scene.B[:, :4]), R, L, **kw), first)
    made = [mctx.upload(x) for x in (scene.core, scene.A, scene.B)]
    try:
        assert same_result(mctx.m3c2_dev(made[0], made[1], made[2], R, L, **kw), first)
        whole = mctx.m3c2(scene.A, scene.A, scene.B, R, L, **kw)
        assert same_result(mctx.m3c2_dev(made[1], made[1], made[2], R, L, **kw), whole)
        assert same_bits(whole[0][::10], first[0]) and same_bits(whole[1]["moments"][::10], first[1]["moments"])
    finally:
        for c in made:
            c.free()
    st = mctx.stats()
    assert {"m3c2_grid_s", "m3c2_walk_s", "m3c2_reduce_s", "m3c2_valid"} <= set(st) and st["m3c2_valid"] == whole[1]["valid"]


# ---- 9. the summary --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [0, 1, 2])
def test_summary_is_numpy_on_the_per_point_outputs(scene, t):
    d, info = scene.gpu[t]
    want = M.summary(d, info["significant_mask"], info["count"])
    assert (info["m"], info["valid"], info["significant"], info["max"], info["max_count"]) == (
        want["m"], want["valid"], want["significant"], want["max"], want["max_count"])
    assert abs(info["rms"] - want["rms"]) <= 1e-12 * want["rms"] and abs(info["mean"] - want["mean"]) <= 1e-12 * abs(want["mean"])
    assert 0 < info["significant"] < info["valid"]


def test_per_point_outputs_are_optional(mctx, scene):
    R, L = scene.params[1]
    d, info = mctx.m3c2(scene.core, scene.A, scene.B, R, L, min_points=MIN_POINTS, per_point=False)
    assert same_bits(d, scene.gpu[1][0]) and "count" not in info and "moments" not in info
    assert info["rms"] == scene.gpu[1][1]["rms"] and info["valid"] == scene.gpu[1][1]["valid"]


# ---- 10. refusals ----------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_the_context_usable(mctx, scene):
    core, A, B = scene.core[:300], np.ascontiguousarray(scene.A[:3000, :3]), np.ascontiguousarray(scene.B[:3000, :3])
    core = np.ascontiguousarray(core)
    kw = dict(radius=0.3, depth=0.6)
    good = mctx.m3c2(core, A, B, moments=True, **kw)

    def spoil(X, v, col=1):
        Y = X.copy()
        Y[17, col] = v
        return Y
    Tn = np.eye(4, dtype=np.float32)
    Tn[1, 3] = np.nan
    Ti = np.eye(4, dtype=np.float32)
    Ti[0, 0] = np.inf
    e3 = np.zeros((0, 3), np.float32)
    cases = [(core, e3, B, kw), (core, A, e3, kw),
             (spoil(core, np.nan), A, B, kw), (spoil(core, np.inf, 2), A, B, kw), (core, spoil(A, np.nan), B, kw), (core, spoil(A, -np.inf, 0), B, kw),
             (core, A, spoil(B, np.nan), kw), (core, A, spoil(B, np.inf, 2), kw),
             (core, A, B, dict(kw, T=Tn)), (core, A, B, dict(kw, T=Ti)),
             (core, A, B, dict(kw, radius=0.0)), (core, A, B, dict(kw, radius=-1.0)), (core, A, B, dict(kw, radius=np.nan)),
             (core, A, B, dict(kw, radius=np.inf)), (core, A, B, dict(kw, radius=1e200)),          # R * R is not finite
             (core, A, B, dict(kw, depth=0.0)), (core, A, B, dict(kw, depth=-0.5)), (core, A, B, dict(kw, depth=np.nan)),
             (core, A, B, dict(kw, depth=np.inf)),
             (core, A, B, dict(kw, reg_error=-1e-9)), (core, A, B, dict(kw, reg_error=np.nan)), (core, A, B, dict(kw, reg_error=np.inf)),
             (core, A, B, dict(kw, min_points=1)), (core, A, B, dict(kw, min_points=0)), (core, A, B, dict(kw, min_points=-3))]
    for c, a, b, k in cases:
        with pytest.raises(plade_amd.PladeError) as e:
            mctx.m3c2(c, a, b, **k)
        assert e.value.code == plade_amd.PLADE_EINVAL and str(e.value).split(": ", 1)[1], k
        assert same_result(mctx.m3c2(core, A, B, moments=True, **kw), good)      # the next call on the same context succeeds
    # a B that leaves the fp32 range under T
    Tb = np.eye(4, dtype=np.float32)
    Tb[0, 0] = 3e38
    with pytest.raises(plade_amd.PladeError) as e:
        mctx.m3c2(core, A, B, T=Tb, **kw)
    assert e.value.code == plade_amd.PLADE_EINVAL
    # through the C ABI itself: m = 0, stride < 3, NULL clouds, params and summary
    L_ = mctx.L
    prm = plade_amd.M3c2Params()
    L_.plade_m3c2_default_params(ctypes.byref(prm))
    summ = plade_amd.M3c2Summary()
    pc, pa, pb = core.ctypes.data, A.ctypes.data, B.ctypes.data

    def call(c=pc, m=len(core), a=pa, na=len(A), sa=3, b=pb, nb=len(B), sb=3, p=ctypes.byref(prm), s=ctypes.byref(summ)):
        return L_.plade_cloud_m3c2(mctx.h, c, m, a, na, sa, b, nb, sb, None, p, None, None, None, None, None, None, s)
    assert call() == plade_amd.PLADE_EINVAL and b"radius" in L_.plade_last_error(mctx.h)   # the defaults carry no radius
    prm.radius = 0.3
    assert call() == plade_amd.PLADE_EINVAL and b"depth" in L_.plade_last_error(mctx.h)    # ... and no depth
    prm.depth = 0.6
    assert call() == plade_amd.PLADE_OK
    for bad, word in ((dict(m=0), b"empty"), (dict(na=0), b"empty"), (dict(nb=0), b"empty"), (dict(sa=2), b"stride"), (dict(sb=2), b"stride"),
                      (dict(c=None), b"NULL"), (dict(a=None), b"NULL"), (dict(b=None), b"NULL"), (dict(p=None), b"NULL"), (dict(s=None), b"NULL")):
        assert call(**bad) == plade_amd.PLADE_EINVAL and word in L_.plade_last_error(mctx.h), bad
    made = [mctx.upload(scene.A[:3000])]
    try:
        h = made[0].h
        rc = L_.plade_cloud_m3c2_dev(mctx.h, h, None, h, None, ctypes.byref(prm), None, None, None, None, None, None, ctypes.byref(summ))
        assert rc == plade_amd.PLADE_EINVAL and b"NULL" in L_.plade_last_error(mctx.h)
        rc = L_.plade_cloud_m3c2_dev(mctx.h, h, h, h, None, None, None, None, None, None, None, None, ctypes.byref(summ))
        assert rc == plade_amd.PLADE_EINVAL and b"NULL" in L_.plade_last_error(mctx.h)
        with pytest.raises(plade_amd.PladeError):
            mctx.m3c2_dev(made[0], made[0], made[0], -1.0, 0.5)
    finally:
        for c in made:
            c.free()
    assert same_result(mctx.m3c2(core, A, B, moments=True, **kw), good)


# ---- 11. the chain ---------------------------------------------------------------------------------------------------------------
def test_chain_registration_then_m3c2(mctx):
    """registration_dev -> evaluate_registration -> m3c2_dev on a 100k pair whose source has one face displaced by 5 cm (the face of
    7th-largest support in the source); core points = every 200th target point, resident.  The flags against the restatement;
    the shares of significant core points on and off the moved face are printed, none is fixed in advance."""
    tg, sr, Tgt, tl, sl = make_pair(100000, seed=0, return_labels=True)
    support = np.bincount(sl[sl >= 0])
    fid = int(np.argsort(-support, kind="stable")[6])
    nrm = np.linalg.inv(Tgt)[:3, :3] @ np.asarray(_faces(1000, 8)[fid][3], np.float64)          # in the source's frame
    sr = np.ascontiguousarray(sr)
    sr[sl == fid, :3] = (sr[sl == fid, :3].astype(np.float64) + 0.05 * nrm).astype(np.float32)
    D = diag(tg)
    R, L = 0.01 * D, 0.04 * D
    core = np.ascontiguousarray(tg[::200])
    made = [mctx.upload(x) for x in (tg, sr, core)]
    try:
        ok, T = mctx.registration_dev(made[0], made[1])
        assert ok
        rmse = mctx.evaluate_registration(tg, sr, T, 0.01 * D)["rmse"]
        got = mctx.m3c2_dev(made[2], made[0], made[1], R, L, T=T, reg_error=rmse, moments=True)
    finally:
        for c in made:
            c.free()
    ref = M.m3c2(core, tg, sr, [(R, L)], T=T, min_points=MIN_POINTS, reg_error=rmse)[0]
    check_against(got, ref, L, "chain")
    check_derived(got, ref["has_axis"], reg_error=rmse)
    d, info = got
    on = (tl[::200] == fid) & ref["valid"]
    off = (tl[::200] != fid) & ref["valid"]
    print(f"|T - T_gt| = {np.linalg.norm(T.astype(np.float64) - Tgt):.4f}, rmse {rmse:.4e}, valid {info['valid']} of {info['m']}, "
          f"significant {info['significant']}; on the moved face {info['significant_mask'][on].sum()} of {on.sum()}, "
          f"off it {info['significant_mask'][off].sum()} of {off.sum()}; mean {info['mean']:.4e}, rms {info['rms']:.4e}, max {info['max']:.4e}")
    assert info["valid"] > 0
