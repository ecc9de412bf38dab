"""Multi-scale normals and dimensionality features on the GPU (plade_cloud_scale_features / plade_cloud_scale_normals_dev,
plade_amd/csrc/k_scales.hip) against the numpy restatement of their semantics (tests/scales_restate.py: fp32 brute force for the
distances, fp64 sums in ascending j, the closed-form eigenvalues expression for expression, numpy's eigh for the normals).

Counts, fitted flags and the summary bit for bit; every moment within 1e-12 of the sum of the absolute values of its terms (a few
hundred fp64 terms at 2^-53 each: four orders of margin, the bound of test_gpu_smooth.py); the eigenvalues against the restated closed
form in long double on the GPU's OWN moments and counts within 4 E + 4 * 2^-52 of l1, E = the float64 restatement's own loss against
long double measured here (the rule of test_gpu_iss.py); chosen, features and the chosen normal recomputed from the GPU's own
per-scale outputs bit for bit (divisions and comparisons are exact functions), and chosen against the full restatement outside its
unsure set; per-scale normals within 1e-4 rad of eigh where the restated (l2 - l3) / trace exceeds 1e-3 (the numbers of
test_gpu_normals.py / test_gpu_smooth.py for the same solver).

The scene (8000 points, radii 0.02 .. 0.08 D), checked on the CPU: median counts 6 / 23 / 50 / 92, max 330; every scale is chosen by
both modes; the fitted shares are 0.61 .. 0.9996; no query is unsure; no fitted scale has (l2 - l3) / trace < 1e-3.
"""
import ctypes

import numpy as np
import pytest

import grid_shapes as G
import plade_amd
import scales_restate as R
from plade_amd.synth import sample_scene
from conftest import ORIENTED
from test_smooth_host import plane

pytestmark = pytest.mark.gpu

FRACTIONS = (0.02, 0.04, 0.06, 0.08)   # of the diagonal D
MIN_NB = 6
PER_SCALE = ("count", "fitted_mask", "eigenvalues", "normals", "moments")
ARRAYS = ("chosen", "features") + PER_SCALE
MESSAGES = {
    "empty": "the cloud is empty (n = 0)", "stride": "stride must be >= 3 floats",
    "stride6": "orient = 1 reads the rows' normals: stride must be >= 6 floats", "scales": "the number of scales must be 1 .. 8",
    "radius": "every radius must be finite and > 0, and its fp32 square finite and not below FLT_MIN",
    "ascending": "the fp32 squares of the radii must be strictly ascending", "min_nb": "min_neighbours must be >= 3",
    "mode": "mode must be 0 (planarity) or 1 (surface variation)", "orient": "orient must be 0 or 1",
    "viewpoint": "the viewpoint must be finite", "k0": "the query list is empty (k = 0)", "index": "a query index is >= n",
    "order": "the query indices must be strictly ascending", "coordinate": "non-finite coordinates",
}


@pytest.fixture(scope="module")
def sctx():
    c = plade_amd.Context(0, **ORIENTED)
    yield c
    c.close()


def diag(P):
    return float(np.linalg.norm(P[:, :3].max(0).astype(np.float64) - P[:, :3].min(0).astype(np.float64)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_but_nan(a, b):
    """the same NaN positions, the same bits everywhere else"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(na, nb) and same_bits(np.where(na, 0, a), np.where(nb, 0, b))


def same_result(x, y, keys=ARRAYS):
    (n0, a), (n1, b) = x, y
    return same_bits(n0, n1) and all(same_bits(a[k], b[k]) for k in keys if k in a or k in b) and all(
        a[k] == b[k] for k in ("queries", "fitted", "chosen_hist", "max_count"))


def own_choice(info, mode):
    """chosen, features and normal recomputed from the GPU's own per-scale eigenvalues, normals and fitted flags"""
    F = R.features(info["eigenvalues"])
    chosen = R.choose(R.criterion(F, mode), info["fitted_mask"])
    return chosen, R.pick(F, chosen), R.pick(info["normals"], chosen)


def check(got, ref, mode, S, max_unsure=0.01):
    """what every input must satisfy: counts, flags, summary, moments, the choice from the GPU's own outputs and against the restatement"""
    nrm, info = got
    assert info["count"].dtype == np.uint32 and np.array_equal(info["count"], ref["count"])
    assert np.array_equal(info["fitted_mask"], ref["fitted"])
    assert (np.abs(info["moments"] - ref["moments"]) <= 1e-12 * ref["mag"]).all()
    L = info["eigenvalues"]
    assert (L[..., 0] >= L[..., 1]).all() and (L[..., 1] >= L[..., 2]).all() and (L[..., 2] >= 0).all()
    chosen, feat, normal = own_choice(info, mode)
    assert info["chosen"].dtype == np.int32 and np.array_equal(info["chosen"], chosen)
    assert same_but_nan(info["features"], feat) and same_but_nan(nrm, normal)
    assert np.isnan(info["normals"][~info["fitted_mask"]]).all() and not np.isnan(info["normals"][info["fitted_mask"]]).any()
    want = R.summary(info["chosen"], ref["count"], S)
    assert {k: info[k] for k in want} == want
    sure = ~ref["unsure"]
    assert ref["unsure"].mean() <= max_unsure                          # on the restatement alone
    assert np.array_equal(info["chosen"][sure], ref["chosen"][sure])


def angles(a, b):
    """between two arrays of unit vectors, sign-free"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), np.abs((a * b).sum(-1)))


class Scene8k:
    """The 8k scene, its restatement and the GPU's answer in both modes (computed once, never changed)."""
    def __init__(self, ctx):
        self.P = np.ascontiguousarray(sample_scene(8000, scene_seed=3, sample_seed=4))
        self.D = diag(self.P)
        self.radii = [np.float32(f * self.D) for f in FRACTIONS]
        self.ref = [R.scales(self.P, self.radii, mode=0, min_neighbours=MIN_NB)]
        m1 = dict(self.ref[0])
        m1["criterion"] = R.criterion(m1["features"], 1)
        m1["chosen"] = R.choose(m1["criterion"], m1["fitted"])
        m1["unsure"] = R.unsure(m1["criterion"], m1["fitted"], m1["count"], m1["eigenvalues"], MIN_NB)
        m1["normal"], m1["chosen_features"] = R.pick(m1["normals"], m1["chosen"]), R.pick(m1["features"], m1["chosen"])
        self.ref.append(m1)
        self.gpu = [ctx.scale_features(self.P, self.radii, mode=m, min_neighbours=MIN_NB, moments=True) for m in (0, 1)]


@pytest.fixture(scope="module")
def s8k(sctx):
    return Scene8k(sctx)


# ---- 1. the scene against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_the_scene_against_the_restatement(s8k, mode):
    ref, (nrm, info) = s8k.ref[mode], s8k.gpu[mode]
    print(f"mode {mode}: median counts {np.median(ref['count'], axis=0)}, max {ref['count'].max()}, fitted shares "
          f"{ref['fitted'].mean(0)}, chosen {np.bincount(ref['chosen'] + 1, minlength=5)}, unsure {ref['unsure'].sum()}")
    assert not ref["unsure"].any()                                     # on the restatement alone: this scene excludes nothing
    assert (np.bincount(ref["chosen"] + 1, minlength=5) > 0).all()     # every scale, and "none", is chosen
    assert ((0 < ref["fitted"].sum(0)) & (ref["fitted"].sum(0) < len(s8k.P))).all()      # both branches at every scale
    check((nrm, info), ref, mode, 4)
    assert np.array_equal(info["chosen"], ref["chosen"])
    rel = np.abs(info["moments"] - ref["moments"])[ref["mag"] > 0] / ref["mag"][ref["mag"] > 0]
    print(f"mode {mode}: worst |moment - restated| / sum |terms| {rel.max():.3e}")


def test_eigenvalues_against_long_double_on_the_gpus_own_moments(s8k):
    ref, (_, info) = s8k.ref[0], s8k.gpu[0]
    Lr = R.eigenvalues(ref["moments"], ref["count"], np.longdouble)
    okr = Lr[..., 0] > 0
    E = float((np.abs(ref["eigenvalues"][okr].astype(np.longdouble) - Lr[okr]).max(axis=-1) / Lr[okr][:, 0]).max())
    Ld = R.eigenvalues(info["moments"], info["count"], np.longdouble)
    ok = Ld[..., 0] > 0
    L = info["eigenvalues"]
    assert (L[~ok] == 0).all()
    worst = float((np.abs(L[ok].astype(np.longdouble) - Ld[ok]).max(axis=-1) / Ld[ok][:, 0]).max())
    print("E (float64 restatement against long double):", E, "GPU worst |dl| / l1:", worst, "bound", 4 * E + 4 * 2.0 ** -52)
    assert worst <= 4 * E + 4 * 2.0 ** -52


def test_per_scale_normals_against_eigh(s8k):
    ref, (_, info) = s8k.ref[0], s8k.gpu[0]
    f = ref["fitted"]
    clear = f & (ref["gap"] > 1e-3)
    assert (f & ~clear).sum() <= 0.01 * f.sum()                        # on the restatement alone
    n_gpu = info["normals"].astype(np.float64)
    ang = angles(n_gpu[clear], ref["normals"][clear])
    print(f"excluded {(f & ~clear).sum()} of {f.sum()}, max angle {ang.max():.3e}")
    assert ang.max() <= 1e-4
    assert np.abs(np.linalg.norm(n_gpu[f], axis=-1) - 1.0).max() <= 1e-6
    to_view = -np.repeat(s8k.P[:, None, :3].astype(np.float64), 4, axis=1)       # viewpoint 0 0 0
    assert ((to_view[f] * n_gpu[f]).sum(-1) >= -1e-6 * np.linalg.norm(to_view[f], axis=-1)).all()


# ---- 2. orientation ---------------------------------------------------------------------------------------------------------------
def test_both_orientation_rules(sctx, s8k):
    P = s8k.P.copy()
    P[0::7, 3:] = np.nan                                               # not finite: the viewpoint decides
    P[1::7, 3:] = 0                                                    # t = 0 exactly: the viewpoint decides
    P[2::7, 3:] = -P[2::7, 3:]
    view = (5.0, 4.0, 1.5)
    n0, i0 = sctx.scale_features(P, s8k.radii, viewpoint=view, orient=0, min_neighbours=MIN_NB)
    n1, i1 = sctx.scale_features(P, s8k.radii, viewpoint=view, orient=1, min_neighbours=MIN_NB)
    assert all(same_bits(i0[k], i1[k]) for k in ("chosen", "features", "count", "fitted_mask", "eigenvalues"))
    f = i0["fitted_mask"]
    N0, N1 = i0["normals"], i1["normals"]
    w = np.asarray(view)[None, None, :] - np.repeat(P[:, None, :3].astype(np.float64), 4, axis=1)
    assert ((w[f] * N0[f].astype(np.float64)).sum(-1) >= -1e-6 * np.linalg.norm(w[f], axis=-1)).all()
    g = np.repeat(P[:, None, 3:].astype(np.float64), 4, axis=1)
    with np.errstate(invalid="ignore"):
        t = (g * N0.astype(np.float64)).sum(-1)
    keep = f & ((t > 1e-6) | ~np.isfinite(t) | (np.abs(g).sum(-1) == 0))
    turn = f & (t < -1e-6)
    assert keep.sum() > 1000 and turn.sum() > 1000 and (keep | turn).sum() >= 0.99 * f.sum()
    assert same_bits(N1[keep], N0[keep]) and same_bits(N1[turn], -N0[turn])
    assert same_bits(np.abs(N1[f]), np.abs(N0[f]))
    assert same_but_nan(n1, R.pick(N1, i1["chosen"])) and same_but_nan(n0, R.pick(N0, i0["chosen"]))


def test_an_orthogonal_row_normal_falls_back_to_the_viewpoint(sctx):
    X = plane()                                                        # z = 0.5 exactly: the fit's normal is (0, 0, +-1) exactly
    P = np.zeros((len(X), 6), np.float32)
    P[:, :3] = X
    P[:, 3] = 1.0                                                      # along x: t = 0 exactly
    for view, z in (((0.5, 0.5, 10.0), 1.0), ((0.5, 0.5, -10.0), -1.0)):
        nrm, info = sctx.scale_features(P, (0.1, 0.2), viewpoint=view, orient=1)
        f = info["fitted_mask"]
        assert f.all(axis=1).sum() > 0.9 * len(P)
        assert (info["normals"][f] == np.array([0.0, 0.0, z], np.float32)).all()


# ---- 3. a scale does not depend on the smaller scales asked for -------------------------------------------------------------------
@pytest.mark.parametrize("s", [0, 1, 2])
def test_a_scale_is_independent_of_the_smaller_ones(sctx, s8k, s):
    _, full = s8k.gpu[0]
    _, two = sctx.scale_features(s8k.P, (s8k.radii[s], s8k.radii[3]), min_neighbours=MIN_NB, moments=True)
    for k in PER_SCALE:
        assert same_bits(two[k][:, 0], full[k][:, s]), k
        assert same_bits(two[k][:, 1], full[k][:, 3]), k


# ---- 4. edge shapes ---------------------------------------------------------------------------------------------------------------
def test_a_pair_at_exactly_a_radius(sctx):
    r0, r1 = np.float32(0.25), np.float32(0.375)                       # both squares are exact in fp32
    P = np.array([[0, 0, 0], [r0, 0, 0]], np.float32)
    _, info = sctx.scale_features(P, (r0, r1), min_neighbours=3)
    assert info["count"].tolist() == [[1, 2], [1, 2]]                  # d = r2 of scale 0: neighbours at scale 1, not at scale 0
    P[1, 0] = np.nextafter(r0, np.float32(0))
    _, info = sctx.scale_features(P, (r0, r1), min_neighbours=3)
    assert info["count"].tolist() == [[2, 2], [2, 2]]                  # one ulp closer: neighbours at both
    P[1, 0] = r1
    _, info = sctx.scale_features(P, (r0, r1), min_neighbours=3)
    assert info["count"].tolist() == [[1, 1], [1, 1]]                  # d = r2 of the largest scale: at neither
    P[1, 0] = np.nextafter(r1, np.float32(0))
    nrm, info = sctx.scale_features(P, (r0, r1), min_neighbours=3, moments=True)
    assert info["count"].tolist() == [[1, 2], [1, 2]] and not info["fitted_mask"].any() and (info["chosen"] == -1).all()
    assert np.isnan(nrm).all() and np.isnan(info["features"]).all()
    assert same_bits(info["moments"], R.moments(P, (r0, r1))[1])       # two terms: no order to differ in


def test_one_point_and_coincident_points(sctx):
    one = np.array([[1.0, -2.0, 3.0]], np.float32)
    nrm, info = sctx.scale_features(one, (0.5, 1.0), min_neighbours=3)
    assert info["count"].tolist() == [[1, 1]] and not info["fitted_mask"].any() and info["chosen"].tolist() == [-1]
    assert np.isnan(nrm).all() and (info["eigenvalues"] == 0).all()
    assert (info["queries"], info["fitted"], info["chosen_hist"], info["max_count"]) == (1, 0, (0, 0), 1)
    same = np.tile(np.array([[0.25, 4.0, -1.5]], np.float32), (50, 1))
    nrm, info = sctx.scale_features(same, (0.5, 1.0), min_neighbours=3, moments=True)
    assert (info["count"] == 50).all() and not info["fitted_mask"].any() and (info["chosen"] == -1).all()      # C = 0: unfitted
    assert (info["moments"] == 0).all() and (info["eigenvalues"] == 0).all() and np.isnan(nrm).all() and np.isnan(info["normals"]).all()
    assert (info["queries"], info["fitted"], info["max_count"]) == (50, 0, 50)


@pytest.mark.parametrize("n,S", [(65, 1), (257, 8), (65, 3), (257, 2)])
def test_small_clouds_and_the_extreme_numbers_of_scales(sctx, n, S):
    P = np.ascontiguousarray(sample_scene(n, scene_seed=5, sample_seed=6))
    radii = [np.float32((0.1 + 0.05 * s) * diag(P)) for s in range(S)]
    for mode in (0, 1):
        ref = R.scales(P, radii, mode=mode, min_neighbours=4)
        got = sctx.scale_features(P, radii, mode=mode, min_neighbours=4, moments=True)
        assert got[1]["count"].shape == (n, S) and got[1]["moments"].shape == (n, S, 9) and len(got[1]["chosen_hist"]) == S
        assert ref["fitted"].any()
        # 1 % of 65 queries is less than one: a cloud this sparse has stray points whose neighbourhoods coincide at two scales (an
        # exact tie); three of them are allowed.  The choice from the GPU's own outputs is pinned for every query all the same
        check(got, ref, mode, S, max_unsure=max(0.01, 3.0 / n))


@pytest.mark.parametrize("name", ["row0", "sheet2"])
def test_a_single_row_and_a_one_cell_thick_sheet(sctx, name):
    P = G.cloud(name)
    radii = (1.5, G.R)
    ref = R.scales(P, radii, min_neighbours=3)
    got = sctx.scale_features(P, radii, min_neighbours=3, moments=True)
    st = sctx.stats()
    assert [st["scales_grid_d" + "xyz"[a]] for a in G.unit_axes(name)] == [1.0] * len(G.unit_axes(name))
    # a row's points are collinear exactly: planarity is 0 at both scales, a tie at most of its queries, so there the choice is pinned
    # by the GPU's own outputs and against the restatement only where that is sure; a sheet keeps the scene's 1 %
    check(got, ref, 0, 2, max_unsure=1.0 if name == "row0" else 0.01)
    assert ref["fitted"].any() and got[1]["max_count"] == ref["count"].max()
    if name == "sheet2":
        f = got[1]["fitted_mask"]
        assert np.abs(np.abs(got[1]["normals"][f][:, 2]) - 1.0).max() <= 1e-6


def test_the_scene_far_from_the_origin(sctx, s8k):
    """100 D away the shift is not exact in fp32: the restatement is that of the shifted floats."""
    P = s8k.P.copy()
    P[:, :3] = (P[:, :3].astype(np.float64) + 100.0 * s8k.D).astype(np.float32)
    ref = R.scales(P, s8k.radii, min_neighbours=MIN_NB)
    got = sctx.scale_features(P, s8k.radii, min_neighbours=MIN_NB, moments=True)
    check(got, ref, 0, 4)
    assert ref["fitted"].mean() > 0.5


def test_query_lists(sctx, s8k):
    n = len(s8k.P)
    full = s8k.gpu[0]
    assert same_result(sctx.scale_features(s8k.P, s8k.radii, min_neighbours=MIN_NB, moments=True,
                                           query_index=np.arange(n, dtype=np.uint32)), full)
    for q in (np.array([0]), np.array([n - 1]), np.arange(0, n, 3)):
        nrm, info = sctx.scale_features(s8k.P, s8k.radii, min_neighbours=MIN_NB, moments=True, query_index=q)
        assert same_bits(nrm, full[0][q]) and all(same_bits(info[k], full[1][k][q]) for k in ARRAYS)
        want = R.summary(full[1]["chosen"][q], full[1]["count"][q], 4)
        assert {k: info[k] for k in want} == want


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_leave_the_context_usable(sctx, s8k):
    P, r = s8k.P[:500], s8k.radii
    before = sctx.scale_features(P, r, moments=True)
    bad_xyz = P.copy()
    bad_xyz[17, 1] = np.inf
    cases = [
        ("empty", dict(points=np.zeros((0, 3), np.float32))),
        ("stride6", dict(points=np.ascontiguousarray(P[:, :3]), orient=1)),
        ("scales", dict(radii=())), ("scales", dict(radii=[0.1 * (s + 1) for s in range(9)])),
        ("radius", dict(radii=(r[0], 0.0))), ("radius", dict(radii=(-1.0,))), ("radius", dict(radii=(r[0], np.inf))),
        ("radius", dict(radii=(r[0], np.nan))), ("radius", dict(radii=(1e-30,))), ("radius", dict(radii=(1e30,))),
        ("ascending", dict(radii=(r[1], r[0]))), ("ascending", dict(radii=(r[0], r[0]))),
        ("ascending", dict(radii=(float(r[0]), float(r[0]) * (1 + 1e-12)))),          # ascending in fp64, equal in fp32
        ("min_nb", dict(min_neighbours=2)), ("mode", dict(mode=2)), ("mode", dict(mode=-1)), ("orient", dict(orient=2)),
        ("viewpoint", dict(viewpoint=(0.0, np.nan, 0.0))), ("coordinate", dict(points=bad_xyz)),
        ("k0", dict(query_index=np.zeros(0, np.uint32))), ("index", dict(query_index=[0, 500])),
        ("order", dict(query_index=[3, 3])), ("order", dict(query_index=[4, 2])),
    ]
    for why, kw in cases:
        args = dict(points=P, radii=r)
        args.update(kw)
        with pytest.raises(plade_amd.PladeError) as e:
            sctx.scale_features(**args)
        assert e.value.code == plade_amd.PLADE_EINVAL and MESSAGES[why] in str(e.value), (why, kw, str(e.value))
    # stride < 3 cannot be said through the numpy wrapper
    prm = plade_amd.ScaleParams()
    sctx.L.plade_scale_default_params(ctypes.byref(prm))
    prm.scales, prm.radii[0] = 1, 0.1
    rc = sctx.L.plade_cloud_scale_features(sctx.h, P.ctypes.data, 10, 2, None, 0, ctypes.byref(prm), *([None] * 9))
    assert rc == plade_amd.PLADE_EINVAL and MESSAGES["stride"].encode() in sctx.L.plade_last_error(sctx.h)
    assert same_result(sctx.scale_features(P, r, moments=True), before)


# ---- 6. repeatability and the resident form ---------------------------------------------------------------------------------------
def test_two_runs_and_a_second_context_give_the_same_bytes(sctx, s8k):
    for mode in (0, 1):
        assert same_result(sctx.scale_features(s8k.P, s8k.radii, mode=mode, min_neighbours=MIN_NB, moments=True), s8k.gpu[mode])
    other = plade_amd.Context(0, **ORIENTED)
    try:
        assert same_result(other.scale_features(s8k.P, s8k.radii, min_neighbours=MIN_NB, moments=True), s8k.gpu[0])
    finally:
        other.close()


def test_the_resident_form_gives_the_host_forms_rows(sctx, s8k):
    cloud = sctx.upload(s8k.P)
    try:
        for orient, q in ((0, None), (1, None), (1, np.arange(1, len(s8k.P), 5)), (0, np.array([len(s8k.P) - 1]))):
            nrm, info = sctx.scale_features(s8k.P, s8k.radii, orient=orient, min_neighbours=MIN_NB, query_index=q)
            out, summ = sctx.scale_normals_dev(cloud, s8k.radii, orient=orient, min_neighbours=MIN_NB, query_index=q, info=True)
            try:
                rows = out.download()
            finally:
                out.free()
            pts = s8k.P if q is None else s8k.P[q]
            assert rows.shape == (len(pts), 6) and same_bits(rows[:, :3], pts[:, :3]) and same_but_nan(rows[:, 3:], nrm)
            assert summ == {k: info[k] for k in summ}
        # a refusal leaves *out NULL
        prm = plade_amd.ScaleParams()
        sctx.L.plade_scale_default_params(ctypes.byref(prm))
        prm.scales, prm.radii[0], prm.radii[1] = 2, 0.2, 0.1
        h = ctypes.c_void_p(1)
        rc = sctx.L.plade_cloud_scale_normals_dev(sctx.h, cloud.h, None, 0, ctypes.byref(prm), ctypes.byref(h), None)
        assert rc == plade_amd.PLADE_EINVAL and h.value is None and MESSAGES["ascending"].encode() in sctx.L.plade_last_error(sctx.h)
        h = ctypes.c_void_p(1)                                          # a NULL cloud: refused before anything else, *out NULL too
        rc = sctx.L.plade_cloud_scale_normals_dev(sctx.h, None, None, 0, ctypes.byref(prm), ctypes.byref(h), None)
        assert rc == plade_amd.PLADE_EINVAL and h.value is None
    finally:
        cloud.free()


def test_m3c2_takes_the_resident_result_as_its_core_points(sctx, s8k):
    A = s8k.P
    B = np.ascontiguousarray(sample_scene(8000, scene_seed=3, sample_seed=9))
    q = np.arange(0, len(A), 8, dtype=np.uint32)
    nrm, info = sctx.scale_features(A, s8k.radii, orient=1, min_neighbours=MIN_NB, query_index=q)
    core = np.ascontiguousarray(np.concatenate([A[q, :3], nrm], axis=1))
    R_, L_ = 0.03 * s8k.D, 0.1 * s8k.D
    host = sctx.m3c2(core, A, B, R_, L_, moments=True)
    ca, cb = sctx.upload(A), sctx.upload(B)
    try:
        cc = sctx.scale_normals_dev(ca, s8k.radii, orient=1, min_neighbours=MIN_NB, query_index=q)
        try:
            dev = sctx.m3c2_dev(cc, ca, cb, R_, L_, moments=True)
        finally:
            cc.free()
    finally:
        ca.free(); cb.free()
    assert same_bits(host[0], dev[0]) and all(same_bits(host[1][k], dev[1][k]) for k in ("lod", "significant_mask", "count", "sigma", "moments"))
    assert all(host[1][k] == dev[1][k] or (host[1][k] != host[1][k] and dev[1][k] != dev[1][k]) for k in ("m", "valid", "significant", "max_count"))
    assert info["fitted"] < len(q) or host[1]["valid"] > 0
    assert np.isnan(host[0][info["chosen"] < 0]).all()                 # no fitted scale: no axis
