"""DBSCAN on the GPU (plade_cluster_dbscan / plade_cloud_cluster_dbscan_dev, plade_amd/csrc/k_dbscan.hip) against the restatement
of its semantics (tests/dbscan_restate.py: the exact float32 edge set, the counts, scipy's components of the core-core edges
renumbered by smallest core index, the border rule by a lexsort, the selection in numpy).  label, kind, size, keep, kept_index, the
kept rows and the summary are compared bit for bit: the result is an exact function of the point set and the parameters, so there
is no tolerance anywhere in this file.
"""
import ctypes

import numpy as np
import pytest

import plade_amd
import components_restate as CR
import dbscan_restate as DR
import grid_shapes as GS
import icp_restate as IR
from outlier_restate import flann_d2
from plade_amd.synth import make_pair, sample_scene
from conftest import GT_TOL, ORIENTED

pytestmark = pytest.mark.gpu

F32 = np.float32
SUMMARY = ("n", "clusters", "core", "border", "noise", "kept_clusters", "kept", "largest")


@pytest.fixture(scope="module")
def dctx():
    c = plade_amd.Context(0, **ORIENTED)
    yield c
    c.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same(got, ref, P):
    """got = (rows, kept_index, info) of Context.dbscan, ref = DR.dbscan of the same cloud."""
    rows, kept, info = got
    for k in SUMMARY:
        assert info[k] == ref[k], (k, info[k], ref[k])
    assert info["label"].dtype == np.int32 and same_bits(info["label"], ref["label"])
    assert info["kind"].dtype == np.uint8 and same_bits(info["kind"], ref["kind"])
    assert info["size"].dtype == np.uint32 and same_bits(info["size"], ref["size"])
    assert np.array_equal(info["keep"], ref["keep"])
    assert kept.dtype == np.uint32 and same_bits(kept, ref["kept_index"])
    assert rows.shape == (len(kept), P.shape[1]) and same_bits(rows.view(np.uint32), P[kept].view(np.uint32))


def check(ctx, P, r, min_points, edge_list=None, **sel):
    P = np.ascontiguousarray(P, F32)
    ref = DR.dbscan(P, r, min_points, edge_list=edge_list, **sel)
    got = ctx.dbscan(P, r, min_points, **sel)
    i = got[2]
    print(f"n {len(P)} r {float(r):.6g} min_points {min_points} {sel}: clusters {i['clusters']} (restated {ref['clusters']}), core "
          f"{i['core']}, border {i['border']} ({ref['contested']} contested), noise {i['noise']}, largest {i['largest']}, kept "
          f"{i['kept']} in {i['kept_clusters']}")
    assert_same(got, ref, P)
    return got, ref


def tilted(t, origin=(0.3, -0.2, 0.1), direction=(0.48, 0.6, 0.64)):
    """points origin + t * direction (|direction| = 1), float32"""
    return (np.asarray(origin)[None, :] + np.asarray(t, np.float64)[:, None] * np.asarray(direction)[None, :]).astype(F32)


def shuffled(P, seed):
    return np.ascontiguousarray(P[np.random.default_rng(seed).permutation(len(P))])


# ---- the smallest clouds, the wavefront tails, the predicate ---------------------------------------------------------------------
def test_one_point(dctx):
    P = np.array([[1.0, -2.0, 3.0, 0.0, 0.0, 1.0]], F32)
    (rows, kept, info), _ = check(dctx, P, 0.5, 1)
    assert (info["clusters"], info["kept"], info["largest"], list(info["label"]), list(info["kind"])) == (1, 1, 1, [0], [2])
    s = dctx.stats()
    assert s["dbscan_clusters"] == 1 and s["dbscan_kept"] == 1
    (rows, kept, info), _ = check(dctx, P, 0.5, 2)                  # alone it is noise: PLADE_OK with nothing kept
    assert (info["clusters"], info["kept"], info["noise"], list(info["label"]), list(info["kind"])) == (0, 0, 1, [-1], [0])
    assert len(rows) == 0 and len(kept) == 0 and len(info["size"]) == 0


@pytest.mark.parametrize("n", [63, 64, 65])
def test_the_last_wavefront(dctx, n):
    """the ballot word of a wavefront that n ends inside, ends exactly, or begins"""
    P = np.random.default_rng(n).random((n, 3)).astype(F32)
    (_, _, info), _ = check(dctx, P, 0.25, 4)
    assert min(info["core"], info["border"], info["noise"]) > 0


def test_pair_just_below_and_exactly_at_the_radius(dctx):
    r = F32(0.625)
    a = np.array([1.0, 2.0, 3.0], F32)
    at = a + np.array([0.375, 0.5, 0.0], F32)                      # 0.140625 + 0.25 = 0.390625 = 0.625^2, every step exact in fp32
    below = at.copy()
    below[0] = np.nextafter(at[0], F32(0.0))
    assert flann_d2(a[None], at[None])[0, 0] == r * r
    assert flann_d2(a[None], below[None])[0, 0] < r * r
    (_, _, i_at), _ = check(dctx, np.stack([a, at]), r, 2)
    (_, _, i_below), _ = check(dctx, np.stack([a, below]), r, 2)
    assert (i_at["clusters"], i_at["noise"], list(i_at["label"])) == (0, 2, [-1, -1])
    assert (i_below["clusters"], i_below["core"], list(i_below["label"]), list(i_below["size"])) == (1, 2, [0, 0], [2])


# ---- the border rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a_first", [True, False])
def test_border_tie_goes_to_the_smaller_index(dctx, a_first):
    """q is 0.5 from a1 and from b1, the inner points of two clusters of six cores; it counts 3 and is the only non-core point"""
    q, a, b = [[0, 0, 0]], [[-0.5, 0, 0]] + [[-1, 0, 0]] * 5, [[0.5, 0, 0]] + [[1, 0, 0]] * 5
    P = np.array(q + a + b if a_first else q + b + a, F32)
    (_, _, info), ref = check(dctx, P, 0.625, 5)
    assert ref["contested"] == 1
    assert info["label"].tolist() == [0] * 7 + [1] * 6 and info["kind"].tolist() == [1] + [2] * 12 and info["size"].tolist() == [7, 6]


def test_a_bridge_joins_components_not_clusters(dctx):
    r = 0.02
    rng = np.random.default_rng(17)
    A = rng.random((400, 3)) * 0.05
    B = rng.random((400, 3)) * 0.05 + np.array([1.0, 0.0, 0.0])
    t = np.arange(0.05, 1.0, 0.9 * r)
    chain = np.stack([t, np.full(len(t), 0.025), np.full(len(t), 0.025)], 1)
    P = shuffled(np.concatenate([A, B, chain]).astype(F32), 3)
    e = CR.edges(P, r)
    assert dctx.connected_components(P, r)[2]["components"] == 1
    (_, _, info), _ = check(dctx, P, r, 4, edge_list=e)
    assert info["clusters"] == 2 and info["noise"] > 0 and min(info["size"]) >= 400


# ---- long paths, counting to the end ----------------------------------------------------------------------------------------------
def test_chain_of_5000(dctx):
    r = 0.01
    P = shuffled(tilted(np.arange(5000) * 0.9 * r), 1)
    e = CR.edges(P, r)
    (_, _, three), _ = check(dctx, P, r, 3, edge_list=e)
    assert (three["clusters"], three["core"], three["border"], three["noise"], three["largest"]) == (1, 4998, 2, 0, 5000)
    (_, _, four), _ = check(dctx, P, r, 4, edge_list=e)
    assert (four["clusters"], four["noise"], four["kept"]) == (0, 5000, 0)


def test_6200_points_in_one_cell(dctx):
    """The count at, and far past, any early exit.  The cube's diagonal is sqrt(3) r / 2 = 0.87 r: every one of the 19 million
    pairs is an edge (the float32 expression is off by parts in 10^7, the margin is 25 % of r^2), so every count is 6200 and the
    expected result is written down here, not restated from an edge list of that length."""
    r = 0.05
    P = (np.random.default_rng(8).random((6200, 3)) * (r / 2)).astype(F32) + F32(2.0)
    ext = (P.max(0) - P.min(0)).astype(np.float64)
    assert (ext ** 2).sum() < 0.8 * r * r
    one = {"label": np.zeros(6200, np.int32), "kind": np.full(6200, 2, np.uint8), "size": np.array([6200], np.uint32),
           "keep": np.ones(6200, bool), "kept_index": np.arange(6200, dtype=np.uint32), "n": 6200, "clusters": 1, "core": 6200,
           "border": 0, "noise": 0, "kept_clusters": 1, "kept": 6200, "largest": 6200}
    none = {"label": np.full(6200, -1, np.int32), "kind": np.zeros(6200, np.uint8), "size": np.zeros(0, np.uint32),
            "keep": np.zeros(6200, bool), "kept_index": np.zeros(0, np.uint32), "n": 6200, "clusters": 0, "core": 0, "border": 0,
            "noise": 6200, "kept_clusters": 0, "kept": 0, "largest": 0}
    for mp, ref in ((5, one), (6200, one), (6201, none)):
        assert_same(dctx.dbscan(P, r, mp), ref, P)


# ---- a scene: contested borders, the selection rules ----------------------------------------------------------------------------
R_SCENE, MP_SCENE = F32(0.35), 8


class Scene:
    def __init__(self):
        self.P = np.ascontiguousarray(sample_scene(8000, scene_seed=3, sample_seed=4, outliers=0.03))
        self.r, self.mp = R_SCENE, MP_SCENE
        self.edges = CR.edges(self.P, self.r)
        self.ref = DR.dbscan(self.P, self.r, self.mp, edge_list=self.edges)


@pytest.fixture(scope="module")
def scene():
    return Scene()


def test_scene_full(dctx, scene):
    assert scene.ref["clusters"] >= 20 and scene.ref["contested"] >= 50     # the border rule decides real cases
    assert min(scene.ref["core"], scene.ref["border"], scene.ref["noise"]) > 100
    (_, _, info), _ = check(dctx, scene.P, scene.r, scene.mp, edge_list=scene.edges)
    assert info["clusters"] < CR.components(scene.P, scene.r, edge_list=scene.edges)["components"]
    s = dctx.stats()
    assert s["dbscan_clusters"] == info["clusters"] and s["dbscan_kept"] == info["kept"] == len(scene.P) - info["noise"]
    assert min(s[f"dbscan_{k}_s"] for k in ("grid", "core", "link", "label", "compact")) > 0


@pytest.mark.parametrize("sel", [dict(min_size=50), dict(min_size=2, max_size=150), dict(max_size=8), dict(keep_largest=1),
                                 dict(keep_largest=3), dict(min_size=2, max_size=150, keep_largest=1),
                                 dict(min_size=100000), dict(keep_largest=100000)])
def test_scene_selection(dctx, scene, sel):
    (_, _, info), ref = check(dctx, scene.P, scene.r, scene.mp, edge_list=scene.edges, **sel)
    if sel == dict(min_size=100000):
        assert info["kept"] == 0 and info["kept_clusters"] == 0


def test_size_tie_goes_to_the_smaller_id(dctx):
    blob = (np.random.default_rng(21).random((150, 3)) * 0.05).astype(F32)
    big = (np.random.default_rng(22).random((400, 3)) * 0.05).astype(F32)
    P = np.concatenate([blob + F32(1.0), big + F32(3.0), blob + F32(2.0)])    # two equal blobs (a shift by 1: the same bits apart)
    (_, _, info), ref = check(dctx, P, 0.05, 4, keep_largest=2)
    assert info["size"].tolist() == [150, 400, 150] and np.unique(info["label"][info["keep"]]).tolist() == [0, 1]
    (_, _, info), _ = check(dctx, P, 0.05, 4, min_size=150, max_size=150, keep_largest=1)
    assert np.unique(info["label"][info["keep"]]).tolist() == [0]


# ---- what the result must not depend on -----------------------------------------------------------------------------------------
def test_negative_coordinates_and_a_far_frame(dctx, scene):
    check(dctx, scene.P - F32(50.0), scene.r, scene.mp)
    check(dctx, IR.move(scene.P, IR.frame(1000.0)), scene.r, scene.mp, min_size=3)


def test_a_far_point_changes_the_grid_not_the_partition(dctx, scene):
    far = np.zeros((1, scene.P.shape[1]), F32)
    far[0, :3] = scene.P[:, :3].max(0) + F32(700.0)
    (_, _, info), _ = check(dctx, np.concatenate([scene.P, far]), scene.r, scene.mp)
    n = len(scene.P)
    assert info["clusters"] == scene.ref["clusters"] and info["label"][n] == -1 and info["kind"][n] == 0
    assert same_bits(info["label"][:n], scene.ref["label"]) and same_bits(info["size"], scene.ref["size"])
    assert same_bits(info["kind"][:n], scene.ref["kind"])


def test_a_permuted_input_gives_the_permuted_partition(dctx, scene):
    perm = np.random.default_rng(13).permutation(len(scene.P))
    (_, _, info), _ = check(dctx, scene.P[perm], scene.r, scene.mp)     # (the restatement of the permuted input decides the ties)
    assert same_bits(info["kind"], scene.ref["kind"][perm])
    core = info["kind"] == 2
    pairs = np.unique(np.stack([scene.ref["label"][perm][core], info["label"][core]], 1), axis=0)
    assert len(pairs) == scene.ref["clusters"] == info["clusters"]      # on the core points: a bijection between the two sets of ids


def test_repeated_calls_two_contexts_host_and_resident(dctx, scene):
    sel = dict(min_size=20, keep_largest=5)
    ref = DR.dbscan(scene.P, scene.r, scene.mp, edge_list=scene.edges, **sel)
    assert_same(dctx.dbscan(scene.P, scene.r, scene.mp, **sel), ref, scene.P)
    assert_same(dctx.dbscan(scene.P, scene.r, scene.mp, **sel), ref, scene.P)
    other = plade_amd.Context(0, **ORIENTED)
    try:
        assert_same(other.dbscan(scene.P, scene.r, scene.mp, **sel), ref, scene.P)
    finally:
        other.close()
    c = dctx.upload(scene.P)
    try:
        f, kept, info = dctx.dbscan_dev(c, scene.r, scene.mp, info=True, **sel)
        try:
            assert f.n == ref["kept"] and same_bits(kept, ref["kept_index"])
            assert same_bits(info["label"], ref["label"]) and same_bits(info["kind"], ref["kind"])
            assert all(info[k] == ref[k] for k in SUMMARY)
            assert same_bits(f.download().view(np.uint32), scene.P[kept].view(np.uint32))
        finally:
            f.free()
    finally:
        c.free()


def test_min_points_1_is_the_components_tool(dctx, scene):
    for sel in (dict(), dict(min_size=3, keep_largest=4)):
        rows_c, kept_c, ic = dctx.connected_components(scene.P, scene.r, **sel)
        rows_d, kept_d, idb = dctx.dbscan(scene.P, scene.r, 1, **sel)
        assert (idb["kind"] == 2).all() and idb["clusters"] == ic["components"] and idb["kept_clusters"] == ic["kept_components"]
        assert same_bits(idb["label"], ic["label"]) and same_bits(idb["size"], ic["size"]) and np.array_equal(idb["keep"], ic["keep"])
        assert same_bits(kept_d, kept_c) and same_bits(rows_d.view(np.uint32), rows_c.view(np.uint32))
        assert (idb["kept"], idb["largest"]) == (ic["kept"], ic["largest"])


# ---- odd grids ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1.25, GS.R])
@pytest.mark.parametrize("name", GS.SHAPES)
def test_grid_shapes(dctx, name, r):
    from test_gpu_grid_shapes import met
    P = GS.cloud(name)
    ref = DR.dbscan(P, r, 3)
    got = dctx.dbscan(P, r, 3)
    met(dctx, "dbscan", name, GS.radius_cell(P, r))
    print(f"dbscan on {name}, r = {r}: clusters {got[2]['clusters']} (restated {ref['clusters']}), core {got[2]['core']}, border "
          f"{got[2]['border']}, noise {got[2]['noise']}")
    assert_same(got, ref, P)


# ---- the resident result is a cloud like any other -----------------------------------------------------------------------------
def test_resident_result_goes_through_the_chain(dctx):
    tg, sr, T = make_pair(80000, seed=0)
    r = F32(2.5) * dctx.average_spacing(tg)
    ct, cs = dctx.upload(tg), dctx.upload(sr)
    try:
        ft, kt, it = dctx.dbscan_dev(ct, r, 6, min_size=50, info=True)
        fs = dctx.dbscan_dev(cs, r, 6, min_size=50)
        try:
            assert 0.8 * len(tg) < ft.n < len(tg) and 0.8 * len(sr) < fs.n < len(sr)
            rows = ft.download()
            assert same_bits(rows.view(np.uint32), tg[kt].view(np.uint32))
            idx, d2, plane, s = dctx.cloud_distances_dev(ft, ft, 0.01)
            assert s["fitness"] == 1.0 and s["count"] == ft.n and (d2 == 0).all()
            ok, Tr = dctx.registration_dev(ft, fs)
        finally:
            ft.free()
            fs.free()
        with pytest.raises(plade_amd.PladeError) as e:             # nothing kept: a resident cloud has no empty form
            dctx.dbscan_dev(ct, r, 6, min_size=len(tg) + 1)
        assert e.value.code == plade_amd.PLADE_EFAIL and "no point" in str(e.value)
        again = dctx.dbscan_dev(ct, r, 6, min_size=50)
        assert again.n == it["kept"]
        again.free()
    finally:
        ct.free()
        cs.free()
    assert ok
    assert np.linalg.norm(Tr.astype(np.float64) - T) < GT_TOL


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_the_context_usable(dctx, scene):
    P = np.ascontiguousarray(scene.P[:3000, :3])
    r = float(scene.r)
    ref = DR.dbscan(P, r, 5, min_size=2)
    nan = P.copy()
    nan[17, 1] = np.nan
    inf = P.copy()
    inf[5, 2] = -np.inf
    cases = [(P, dict(radius=0.0)), (P, dict(radius=-1.0)), (P, dict(radius=np.nan)), (P, dict(radius=np.inf)), (P, dict(radius=1e30)),
             (P, dict(radius=1e-30)), (P, dict(radius=r, min_points=0)), (P, dict(radius=r, min_points=-3)),
             (P, dict(radius=r, min_size=0)), (P, dict(radius=r, min_size=-4)), (P, dict(radius=r, min_size=5, max_size=3)),
             (P, dict(radius=r, max_size=-1)), (P, dict(radius=r, keep_largest=-1)), (np.zeros((0, 3), F32), dict(radius=r)),
             (nan, dict(radius=r)), (inf, dict(radius=r))]
    for arr, kw in cases:
        with pytest.raises(plade_amd.PladeError) as e:
            dctx.dbscan(arr, **kw)
        assert e.value.code == plade_amd.PLADE_EINVAL and str(e.value), kw
        assert_same(dctx.dbscan(P, r, 5, min_size=2), ref, P)       # the next call on the same context succeeds
    # stride < 3, a NULL cloud and NULL params through the C ABI itself; the outputs stay untouched
    prm = plade_amd.DbscanParams(radius=r, min_points=5, min_size=1)
    summ = plade_amd.DbscanSummary()
    two = np.zeros((10, 2), F32)
    label = np.full(len(P), 77, np.int32)
    rc = dctx.L.plade_cluster_dbscan(dctx.h, two.ctypes.data, 10, 2, ctypes.byref(prm), label.ctypes.data, None, None, None, None, None,
                                     ctypes.byref(summ))
    assert rc == plade_amd.PLADE_EINVAL and b"stride" in dctx.L.plade_last_error(dctx.h)
    rc = dctx.L.plade_cluster_dbscan(dctx.h, None, 10, 3, ctypes.byref(prm), label.ctypes.data, None, None, None, None, None,
                                     ctypes.byref(summ))
    assert rc == plade_amd.PLADE_EINVAL and b"NULL" in dctx.L.plade_last_error(dctx.h)
    rc = dctx.L.plade_cluster_dbscan(dctx.h, P.ctypes.data, len(P), 3, None, label.ctypes.data, None, None, None, None, None,
                                     ctypes.byref(summ))
    assert rc == plade_amd.PLADE_EINVAL and b"radius" in dctx.L.plade_last_error(dctx.h)      # the defaults carry no radius
    assert (label == 77).all() and summ.n == 0
    h = ctypes.c_void_p(123)
    rc = dctx.L.plade_cloud_cluster_dbscan_dev(dctx.h, None, ctypes.byref(prm), ctypes.byref(h), None, None, None, ctypes.byref(summ))
    assert rc == plade_amd.PLADE_EINVAL and b"NULL" in dctx.L.plade_last_error(dctx.h)
    assert_same(dctx.dbscan(P, r, 5, min_size=2), ref, P)
