"""Connected components on the GPU (plade_label_components / plade_cloud_filter_components_dev, plade_amd/csrc/k_components.hip)
against the restatement of their semantics (tests/components_restate.py: the exact float32 edge set, scipy's components renumbered
by smallest index, the selection in numpy).  label, size, keep, kept_index, the kept rows and the summary are compared bit for bit:
the components are an exact set, so there is no tolerance anywhere in this file.
"""
import ctypes

import numpy as np
import pytest

import plade_amd
import components_restate as CR
import icp_restate as IR
from outlier_restate import flann_d2
from plade_amd.synth import make_pair, sample_scene
from conftest import GT_TOL, ORIENTED

pytestmark = pytest.mark.gpu

F32 = np.float32
SUMMARY = ("n", "components", "kept_components", "kept", "largest")


@pytest.fixture(scope="module")
def cctx():
    c = plade_amd.Context(0, **ORIENTED)
    yield c
    c.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same(got, ref, P):
    """got = (rows, kept_index, info) of Context.connected_components, ref = CR.components of the same cloud."""
    rows, kept, info = got
    for k in SUMMARY:
        assert info[k] == ref[k], (k, info[k], ref[k])
    assert info["label"].dtype == np.int32 and same_bits(info["label"], ref["label"])
    assert info["size"].dtype == np.uint32 and same_bits(info["size"], ref["size"])
    assert np.array_equal(info["keep"], ref["keep"])
    assert kept.dtype == np.uint32 and same_bits(kept, ref["kept_index"])
    assert rows.shape == (len(kept), P.shape[1]) and same_bits(rows.view(np.uint32), P[kept].view(np.uint32))


def check(ctx, P, r, edge_list=None, **sel):
    P = np.ascontiguousarray(P, F32)
    ref = CR.components(P, r, edge_list=edge_list, **sel)
    got = ctx.connected_components(P, r, **sel)
    print(f"n {len(P)} r {float(r):.6g} {sel}: components {got[2]['components']} (restated {ref['components']}), largest "
          f"{got[2]['largest']}, kept {got[2]['kept']} in {got[2]['kept_components']}")
    assert_same(got, ref, P)
    return got, ref


def tilted(t, origin=(0.3, -0.2, 0.1), direction=(0.48, 0.6, 0.64)):
    """points origin + t * direction (|direction| = 1), float32"""
    return (np.asarray(origin)[None, :] + np.asarray(t, np.float64)[:, None] * np.asarray(direction)[None, :]).astype(F32)


def shuffled(P, seed):
    return np.ascontiguousarray(P[np.random.default_rng(seed).permutation(len(P))])


# ---- the smallest clouds and the edge predicate ----------------------------------------------------------------------------------
def test_one_point(cctx):
    P = np.array([[1.0, -2.0, 3.0, 0.0, 0.0, 1.0]], F32)
    (rows, kept, info), _ = check(cctx, P, 0.5)
    assert (info["components"], info["kept"], info["largest"], list(info["label"])) == (1, 1, 1, [0])
    s = cctx.stats()
    assert s["components_count"] == 1 and s["components_kept"] == 1


def test_pair_just_below_and_exactly_at_the_radius(cctx):
    r = F32(0.625)
    a = np.array([1.0, 2.0, 3.0], F32)
    at = a + np.array([0.375, 0.5, 0.0], F32)                      # 0.140625 + 0.25 = 0.390625 = 0.625^2, every step exact in fp32
    below = at.copy()
    below[0] = np.nextafter(at[0], F32(0.0))
    assert flann_d2(a[None], at[None])[0, 0] == r * r
    assert flann_d2(a[None], below[None])[0, 0] < r * r
    (_, _, i_at), _ = check(cctx, np.stack([a, at]), r)
    (_, _, i_below), _ = check(cctx, np.stack([a, below]), r)
    assert i_at["components"] == 2 and i_below["components"] == 1
    assert list(i_at["label"]) == [0, 1] and list(i_below["label"]) == [0, 0]


def test_exact_duplicates(cctx):
    rng = np.random.default_rng(3)
    base = rng.random((700, 3)).astype(F32)
    P = shuffled(np.concatenate([base, base, base[:300]]), 4)
    (_, _, info), _ = check(cctx, P, 0.02)
    assert info["components"] <= 700 and info["largest"] >= 3
    (_, _, tiny), _ = check(cctx, P, 1e-6)                         # only the duplicates themselves are connected
    assert tiny["components"] == 700 and tiny["largest"] == 3


# ---- long paths, many workgroups, re-rooting ----------------------------------------------------------------------------------
def test_chain_of_5000(cctx):
    r = 0.01
    t = np.arange(5000) * 0.9 * r
    (_, _, one), _ = check(cctx, shuffled(tilted(t), 1), r)
    assert one["components"] == 1 and one["largest"] == 5000
    t[2600:] += 0.2 * r                                            # one gap of 1.1 r
    (_, _, two), _ = check(cctx, shuffled(tilted(t), 1), r)
    assert two["components"] == 2 and sorted(two["size"]) == [2400, 2600]


def test_two_chains_that_meet_at_their_highest_indices(cctx):
    r = 0.01
    t = (2500 - np.arange(2500)) * 0.9 * r                         # index 2499 of each chain is the one next to the junction
    A = tilted(t, origin=(0.0, 0.0, 0.0), direction=(1.0, 0.0, 0.0))
    B = tilted(t, origin=(0.0, 0.0, 0.0), direction=(0.5, np.sqrt(0.75), 0.0))   # 60 degrees: the ends are 0.9 r apart
    P = np.concatenate([A, B])
    e = CR.edges(P, r)
    cross = e[(e[:, 0] < 2500) & (e[:, 1] >= 2500)]
    assert cross.tolist() == [[2499, 4999]]
    (_, _, info), _ = check(cctx, P, r, edge_list=e)
    assert info["components"] == 1
    (_, _, apart), _ = check(cctx, P[:-1], r)                      # without the junction's point of B: two components
    assert apart["components"] == 2


@pytest.mark.parametrize("gap, components", [(1.05, 2), (0.95, 1)])
def test_parallel_sheets(cctx, gap, components):
    r = 0.1
    u = np.arange(40) * 0.8 * r
    x, y = np.meshgrid(u, u, indexing="ij")
    sheet = np.stack([x.ravel(), y.ravel(), np.zeros(1600)], 1)
    other = sheet + np.array([0.0, 0.0, gap * r])
    P = shuffled(np.concatenate([sheet, other]).astype(F32) - F32(1.7), 2)
    (_, _, info), _ = check(cctx, P, r)
    assert info["components"] == components


def test_6200_points_in_one_cell(cctx):
    r = 0.05
    P = (np.random.default_rng(8).random((6200, 3)) * r).astype(F32) + F32(2.0)
    (_, _, info), _ = check(cctx, P, r)
    assert info["components"] == 1


def test_lattice_every_point_its_own_component(cctx):
    r = 0.02
    g = np.stack(np.meshgrid(np.arange(20), np.arange(25), np.arange(40), indexing="ij"), -1).reshape(-1, 3)
    P = (g * 1.5 * r).astype(F32)
    (_, _, info), _ = check(cctx, P, r)
    assert info["components"] == 20000 and np.array_equal(info["label"], np.arange(20000)) and (info["size"] == 1).all()


def test_blob_of_20k_in_one_component(cctx):
    P = np.random.default_rng(9).random((20000, 3)).astype(F32)
    (_, _, info), _ = check(cctx, P, 0.1)
    assert info["components"] == 1 and info["size"].tolist() == [20000]


# ---- a scene: the selection rules ---------------------------------------------------------------------------------------------
class Scene:
    def __init__(self, ctx):
        S = sample_scene(20000, scene_seed=3, sample_seed=4, outliers=0.03)
        rng = np.random.default_rng(21)
        blob = (rng.random((150, 3)) * 0.05).astype(F32)           # two equal blobs outside the room: a tie of sizes
        hi = S[:, :3].max(0)
        extra = np.zeros((300, S.shape[1]), F32)
        extra[:150, :3] = blob + hi + F32(1.0)
        extra[150:, :3] = blob + hi + F32(2.0)
        self.P = np.ascontiguousarray(np.concatenate([S, extra]))
        self.r = F32(2.5) * ctx.average_spacing(S)
        self.edges = CR.edges(self.P, self.r)
        self.ref = CR.components(self.P, self.r, edge_list=self.edges)


@pytest.fixture(scope="module")
def scene(cctx):
    return Scene(cctx)


def test_scene_full(cctx, scene):
    (_, _, info), ref = check(cctx, scene.P, scene.r, edge_list=scene.edges)
    assert 10 < info["components"] < len(scene.P) // 4 and info["kept"] == len(scene.P)
    assert (info["size"] == 150).sum() == 2
    s = cctx.stats()
    assert s["components_count"] == info["components"] and s["components_kept"] == info["kept"]
    assert min(s[f"components_{k}_s"] for k in ("grid", "link", "label", "compact")) > 0


@pytest.mark.parametrize("sel", [dict(min_size=50), dict(min_size=2, max_size=150), dict(max_size=1), dict(keep_largest=1),
                                 dict(keep_largest=3), dict(min_size=2, max_size=150, keep_largest=1),
                                 dict(min_size=100000), dict(keep_largest=100000)])
def test_scene_selection(cctx, scene, sel):
    (_, _, info), ref = check(cctx, scene.P, scene.r, edge_list=scene.edges, **sel)
    if sel == dict(min_size=100000):
        assert info["kept"] == 0 and info["kept_components"] == 0


def test_scene_size_tie_goes_to_the_smaller_id(cctx, scene):
    tie = np.flatnonzero(scene.ref["size"] == 150)
    assert len(tie) == 2
    m = int((scene.ref["size"] > 150).sum()) + 1                   # everything larger, then one of the two equal blobs
    (_, _, info), _ = check(cctx, scene.P, scene.r, edge_list=scene.edges, keep_largest=m)
    ids = np.unique(info["label"][info["keep"]])
    assert len(ids) == m and tie[0] in ids and tie[1] not in ids
    (_, _, info), _ = check(cctx, scene.P, scene.r, edge_list=scene.edges, min_size=150, max_size=150, keep_largest=1)
    assert np.unique(info["label"][info["keep"]]).tolist() == [tie[0]]


def test_scene_200k(cctx):
    P = sample_scene(200000, scene_seed=5, sample_seed=6, outliers=0.03)
    r = F32(2.5) * cctx.average_spacing(P)
    (_, _, info), _ = check(cctx, P, r, min_size=50)
    assert info["components"] > 100 and info["largest"] > 100000


# ---- what the result must not depend on -----------------------------------------------------------------------------------------
def test_negative_coordinates_and_a_far_frame(cctx, scene):
    P = scene.P[:8000]
    check(cctx, P - F32(50.0), scene.r)
    check(cctx, IR.move(P, IR.frame(1000.0)), scene.r, min_size=3)


def test_a_far_point_changes_the_grid_not_the_partition(cctx, scene):
    far = np.zeros((1, scene.P.shape[1]), F32)
    far[0, :3] = scene.P[:, :3].max(0) + F32(700.0)
    (_, _, info), _ = check(cctx, np.concatenate([scene.P, far]), scene.r)
    n, C = len(scene.P), scene.ref["components"]
    assert info["components"] == C + 1 and info["label"][n] == C and info["size"][C] == 1
    assert same_bits(info["label"][:n], scene.ref["label"]) and same_bits(info["size"][:C], scene.ref["size"])


def test_a_permuted_input_gives_the_permuted_partition(cctx, scene):
    perm = np.random.default_rng(13).permutation(len(scene.P))
    (_, _, info), _ = check(cctx, scene.P[perm], scene.r)
    pairs = np.unique(np.stack([scene.ref["label"][perm], info["label"]], 1), axis=0)
    assert len(pairs) == scene.ref["components"] == info["components"]          # a bijection between the two sets of ids
    assert np.array_equal(np.sort(info["size"]), np.sort(scene.ref["size"]))


def test_repeated_calls_two_contexts_host_and_resident(cctx, scene):
    sel = dict(min_size=20, keep_largest=5)
    ref = CR.components(scene.P, scene.r, edge_list=scene.edges, **sel)
    first = cctx.connected_components(scene.P, scene.r, **sel)
    assert_same(first, ref, scene.P)
    assert_same(cctx.connected_components(scene.P, scene.r, **sel), ref, scene.P)
    other = plade_amd.Context(0, **ORIENTED)
    try:
        assert_same(other.connected_components(scene.P, scene.r, **sel), ref, scene.P)
    finally:
        other.close()
    c = cctx.upload(scene.P)
    try:
        f, kept, info = cctx.filter_components_dev(c, scene.r, info=True, **sel)
        try:
            assert f.n == ref["kept"] and same_bits(kept, ref["kept_index"]) and same_bits(info["label"], ref["label"])
            assert all(info[k] == ref[k] for k in SUMMARY)
            assert same_bits(f.download().view(np.uint32), ref["rows"].view(np.uint32))
        finally:
            f.free()
    finally:
        c.free()


# ---- the resident result is a cloud like any other -----------------------------------------------------------------------------
def test_resident_result_goes_through_the_chain(cctx):
    tg, sr, T = make_pair(80000, seed=0)
    r = F32(2.5) * cctx.average_spacing(tg)
    ct, cs = cctx.upload(tg), cctx.upload(sr)
    try:
        ft, kt, it = cctx.filter_components_dev(ct, r, min_size=50, info=True)
        fs = cctx.filter_components_dev(cs, r, min_size=50)
        try:
            assert 0.9 * len(tg) < ft.n < len(tg) and 0.9 * len(sr) < fs.n < len(sr)
            rows = ft.download()
            assert same_bits(rows.view(np.uint32), tg[kt].view(np.uint32))
            idx, d2, plane, s = cctx.cloud_distances_dev(ft, ft, 0.01)
            assert s["fitness"] == 1.0 and s["count"] == ft.n and (d2 == 0).all()
            fo = cctx.remove_outliers_dev(ft, k=16)
            try:
                assert fo.n == cctx.remove_outliers(rows, k=16, per_point=False)[2]["kept"]
            finally:
                fo.free()
            ok, Tr = cctx.registration_dev(ft, fs)
        finally:
            ft.free()
            fs.free()
        with pytest.raises(plade_amd.PladeError) as e:             # nothing kept: a resident cloud has no empty form
            cctx.filter_components_dev(ct, r, min_size=len(tg) + 1)
        assert e.value.code == plade_amd.PLADE_EFAIL and "no point" in str(e.value)
        again = cctx.filter_components_dev(ct, r, min_size=50)
        assert again.n == it["kept"]
        again.free()
    finally:
        ct.free()
        cs.free()
    assert ok
    assert np.linalg.norm(Tr.astype(np.float64) - T) < GT_TOL


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_the_context_usable(cctx, scene):
    P = np.ascontiguousarray(scene.P[:3000, :3])
    ref = CR.components(P, scene.r, min_size=2)
    nan = P.copy()
    nan[17, 1] = np.nan
    inf = P.copy()
    inf[5, 2] = -np.inf
    r = float(scene.r)
    cases = [(P, dict(radius=0.0)), (P, dict(radius=-1.0)), (P, dict(radius=np.nan)), (P, dict(radius=np.inf)), (P, dict(radius=1e30)),
             (P, dict(radius=r, min_size=0)), (P, dict(radius=r, min_size=-4)), (P, dict(radius=r, min_size=5, max_size=3)),
             (P, dict(radius=r, max_size=-1)), (P, dict(radius=r, keep_largest=-1)), (np.zeros((0, 3), F32), dict(radius=r)),
             (nan, dict(radius=r)), (inf, dict(radius=r))]
    for arr, kw in cases:
        with pytest.raises(plade_amd.PladeError) as e:
            cctx.connected_components(arr, **kw)
        assert e.value.code == plade_amd.PLADE_EINVAL and str(e.value), kw
        assert_same(cctx.connected_components(P, scene.r, min_size=2), ref, P)      # the next call on the same context succeeds
    # stride < 3 and a NULL cloud through the C ABI itself
    prm = plade_amd.ComponentParams(radius=r, min_size=1)
    summ = plade_amd.ComponentSummary()
    two = np.zeros((10, 2), F32)
    rc = cctx.L.plade_label_components(cctx.h, two.ctypes.data, 10, 2, ctypes.byref(prm), None, None, None, None, None, ctypes.byref(summ))
    assert rc == plade_amd.PLADE_EINVAL and b"stride" in cctx.L.plade_last_error(cctx.h)
    rc = cctx.L.plade_label_components(cctx.h, None, 10, 3, ctypes.byref(prm), None, None, None, None, None, ctypes.byref(summ))
    assert rc == plade_amd.PLADE_EINVAL and b"NULL" in cctx.L.plade_last_error(cctx.h)
    rc = cctx.L.plade_label_components(cctx.h, P.ctypes.data, len(P), 3, None, None, None, None, None, None, ctypes.byref(summ))
    assert rc == plade_amd.PLADE_EINVAL and b"radius" in cctx.L.plade_last_error(cctx.h)      # the defaults carry no radius
    assert_same(cctx.connected_components(P, scene.r, min_size=2), ref, P)
