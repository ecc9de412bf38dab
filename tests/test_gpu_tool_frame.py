"""The host frame the cloud tools share (plade_amd/csrc/work_slot.h, cloud_tool.h): a context's work slots, the keep tail and the
resident result, on seeded sheets of 65 and 257 points (one wavefront and one 256-lane workgroup, each plus one).  Everything here
is compared bit for bit: nothing in this file has a tolerance.

  lifetime      a context on which no tool ran closes; a context on which every one of the 14 slots was used once closes, and a
                context made afterwards gives the same bits.  TOOLS below names one call per slot (and the linearisation of each
                refinement): normals_work, icp_work, gicp_work (whose sample also goes through merge_work), dist_work, outlier_work,
                merge_work, component_work, smooth_work, m3c2_work, fpfh_work, corr_pose_work, iss_work, subsample_work, orient_work.
  independence  two live contexts, the same tool in the order A(257), B(65), A(257): A's two results are the same bits.
  failure       the five filter / transform _dev entry points through the C ABI with *out set beforehand: NULL after a refused
                parameter (PLADE_EINVAL) and after the two empty-result refusals (PLADE_EFAIL), and the next valid call on the
                context gives the bits it gave before.
  agreement     keep (components: label), kept_index and the downloaded rows of the resident form against the host form, for the
                radius filter and the components, with everything kept and with exactly one point kept.

Asserted elsewhere and not repeated here: the subsample's host and resident forms, also with everything and with one point kept
(test_gpu_subsample.py: check() with stride 6, test_spacing_below_the_smallest_gap_keeps_everything,
test_spacing_above_the_diameter_keeps_the_first_key); the statistical filter's resident form (test_gpu_outliers.py:
test_resident_cloud_gives_the_host_bits); a second context after repeated calls for single tools (test_gpu_components.py:
test_repeated_calls_two_contexts_host_and_resident, test_gpu_smooth.py: test_repetition_second_context_and_resident_path); a NULL
*out after a NULL cloud (test_gpu_subsample.py, test_gpu_orient.py: test_errors).
"""
import ctypes
import hashlib

import numpy as np
import pytest

import plade_amd

pytestmark = pytest.mark.gpu

F32 = np.float32
R = 2.0                                # at a mean spacing of 1 a point has a dozen neighbours
SHIFT = np.array([0.03, -0.02, 0.01], F32)


def sheet(n, seed):
    """(n, 6) float32: a doubly curved sheet over a sqrt(n) x sqrt(n) square, mean spacing 1, with its analytic unit normals"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, np.sqrt(n), size=(n, 2))
    z = 0.6 * np.sin(0.7 * xy[:, 0]) + 0.5 * np.cos(0.9 * xy[:, 1])
    nr = np.stack([-0.42 * np.cos(0.7 * xy[:, 0]), 0.45 * np.sin(0.9 * xy[:, 1]), np.ones(n)], 1)
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    return np.ascontiguousarray(np.concatenate([xy, z[:, None], nr], 1), dtype=F32)


P257, P65 = sheet(257, 1), sheet(65, 2)


def source_of(P):
    """every fourth point, moved a little: a source cloud for the tools that take two"""
    S = P[::4].copy()
    S[:, :3] += SHIFT
    return S


def bits(v):
    """arrays as a digest of their bytes, floats in hex, containers in order (dicts by key)"""
    if isinstance(v, np.ndarray):
        return f"{v.dtype}{list(v.shape)}:" + hashlib.sha1(np.ascontiguousarray(v).tobytes()).hexdigest()
    if isinstance(v, dict):
        return "{" + " ".join(f"{k}={bits(v[k])}" for k in sorted(v)) + "}"
    if isinstance(v, (tuple, list)):
        return "(" + " ".join(bits(x) for x in v) + ")"
    if isinstance(v, (float, np.floating)):
        return float(v).hex()
    return repr(v)


def moved(P):
    """the whole cloud, moved a little: the source of the two refinements (65 correspondences are fewer than their default minimum)"""
    S = P.copy()
    S[:, :3] += SHIFT
    return S


def pose(c, P):
    S = source_of(P)
    corr = np.stack([np.arange(len(S)), 4 * np.arange(len(S))], 1).astype(np.int32)
    return c.estimate_pose(S, P, corr, 0.5, hypotheses=64, seed=3)


def match(c, P):
    dt, ds = c.fpfh(P, 1.5 * R)[0], c.fpfh(source_of(P), 3.0 * R)[0]
    return c.match_features(ds, dt, mutual=True)


# one call per work slot of a context (and the seam of each refinement)
TOOLS = {
    "normals": lambda c, P: c.estimate_normals(np.ascontiguousarray(P[:, :3]), k=16, curvature=True),
    "icp": lambda c, P: c.refine_icp(P, moved(P), np.eye(4, dtype=F32), min_correspondences=32),
    "icp_linearize": lambda c, P: c.icp_linearize(P, np.ascontiguousarray(source_of(P)[:, :3]), np.eye(4), R),
    "gicp": lambda c, P: c.refine_gicp(P, moved(P), np.eye(4, dtype=F32), min_correspondences=32),
    "gicp_linearize": lambda c, P: c.gicp_linearize(P, source_of(P), np.eye(4), R),
    "distances": lambda c, P: c.cloud_distances(P, source_of(P), R),
    "outliers_stat": lambda c, P: c.remove_outliers(P, mode="statistical", k=8, alpha=1.0),
    "outliers_radius": lambda c, P: c.remove_outliers(P, mode="radius", radius=R, min_neighbours=10),
    "merge": lambda c, P: c.merge_clouds([P, source_of(P)], None, leaf=R),
    "components": lambda c, P: c.connected_components(P, 0.6 * R, min_size=2),
    "smooth": lambda c, P: c.smooth_cloud(P, R),
    "m3c2": lambda c, P: c.m3c2(P[::3], P, source_of(P), R, 2.0 * R),
    "fpfh": lambda c, P: c.fpfh(P, 1.5 * R),
    "match": match,
    "pose": pose,
    "iss": lambda c, P: c.iss_keypoints(P, 1.5 * R),
    "subsample": lambda c, P: c.subsample(P, R, seed=5),
    "orient": lambda c, P: c.orient_consistent(P, R, mode=plade_amd.ORIENT_EXTREME),
}


def use_all(c, P):
    return {name: bits(tool(c, P)) for name, tool in TOOLS.items()}


# ---- lifetime ----------------------------------------------------------------------------------------------------------------------
def test_contexts_close_unused_and_used_and_a_later_one_gives_the_same_bits():
    plade_amd.Context(0).close()                                   # no tool ran: 14 empty slots
    first = plade_amd.Context(0)
    a = use_all(first, P257)
    first.close()                                                  # every slot is released, before the context's stream
    second = plade_amd.Context(0)
    try:
        b = use_all(second, P257)
    finally:
        second.close()
    assert a == b, [k for k in a if a[k] != b[k]]


# ---- independence ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair():
    a, b = plade_amd.Context(0), plade_amd.Context(0)
    yield a, b
    a.close()
    b.close()


@pytest.mark.parametrize("name", sorted(TOOLS))
def test_two_live_contexts_do_not_share_a_slot(pair, name):
    a, b = pair
    first = bits(TOOLS[name](a, P257))
    other = bits(TOOLS[name](b, P65))
    again = bits(TOOLS[name](a, P257))
    assert first == again and other != first


# ---- failure leaves nothing behind ---------------------------------------------------------------------------------------------------
SET = 0xDEAD0                          # what *out holds before the call: never read, never freed


def raw_outliers(c, cloud, prm):
    out, summ = ctypes.c_void_p(SET), plade_amd.OutlierSummary()
    return c.L.plade_cloud_filter_outliers_dev(c.h, cloud.h, ctypes.byref(prm), ctypes.byref(out), None, None, ctypes.byref(summ)), out


def raw_components(c, cloud, prm):
    out, summ = ctypes.c_void_p(SET), plade_amd.ComponentSummary()
    return c.L.plade_cloud_filter_components_dev(c.h, cloud.h, ctypes.byref(prm), ctypes.byref(out), None, None, ctypes.byref(summ)), out


def raw_subsample(c, cloud, prm):
    out, summ = ctypes.c_void_p(SET), plade_amd.SubsampleSummary()
    return c.L.plade_cloud_subsample_dev(c.h, cloud.h, ctypes.byref(prm), ctypes.byref(out), None, None, ctypes.byref(summ)), out


def raw_orient(c, cloud, prm):
    out, summ = ctypes.c_void_p(SET), plade_amd.OrientSummary()
    return c.L.plade_cloud_orient_normals_dev(c.h, cloud.h, ctypes.byref(prm), ctypes.byref(out), None, None, ctypes.byref(summ)), out


def raw_smooth(c, cloud, prm):
    out, summ = ctypes.c_void_p(SET), plade_amd.SmoothSummary()
    return c.L.plade_cloud_smooth_dev(c.h, cloud.h, ctypes.byref(prm), 1, ctypes.byref(out), ctypes.byref(summ)), out


def downloaded(res):
    """a resident call's (cloud, ...) with the cloud's rows in its place"""
    cloud, rest = (res[0], res[1:]) if isinstance(res, tuple) else (res, ())
    try:
        return bits((cloud.download(), rest))
    finally:
        cloud.free()


V0, Z1 = (0.0, 0.0, 0.0), (0.0, 0.0, 1.0)


def refused(name):
    """(raw call, refused parameters, their message, the valid call); made inside the test: the structs' defaults come from the library"""
    return {
      "outliers": (raw_outliers, plade_amd._outlier_params("radius", None, None, -1.0, 1), "filter_outliers: radius must be finite and > 0",
                   lambda c, cl: c.remove_outliers_dev(cl, mode="radius", radius=R, min_neighbours=10, info=True)),
      "components": (raw_components, plade_amd._component_params(float("nan"), 1, 0, 0), "label_components: radius must be finite and > 0",
                     lambda c, cl: c.filter_components_dev(cl, 0.6 * R, min_size=2, info=True)),
      "subsample": (raw_subsample, plade_amd._subsample_params(1e-30, 0),
                    "subsample_spacing: spacing must be finite and > 0, its fp32 square finite and not below FLT_MIN",
                    lambda c, cl: c.subsample_dev(cl, R, seed=5, info=True)),
      "orient": (raw_orient, plade_amd._orient_params(0.0, plade_amd.ORIENT_VOTE, 0, V0, Z1),
                 "orient_normals: radius must be finite and > 0, its fp32 square finite and not below FLT_MIN",
                 lambda c, cl: c.orient_consistent_dev(cl, R, info=True)),
      "smooth": (raw_smooth, plade_amd._smooth_params(float("inf"), None, V0),
                 "smooth_cloud: radius must be finite and > 0, and its fp32 square finite and not below FLT_MIN",
                 lambda c, cl: c.smooth_cloud_dev(cl, R, info=True)),
    }[name]


@pytest.mark.parametrize("n", (65, 257))
@pytest.mark.parametrize("name", ("components", "orient", "outliers", "smooth", "subsample"))
def test_a_refused_parameter_leaves_out_null_and_the_context_as_it_was(pair, name, n):
    c = pair[0]
    raw, bad, message, valid = refused(name)
    cloud = c.upload(P65 if n == 65 else P257)
    try:
        before = downloaded(valid(c, cloud))
        rc, out = raw(c, cloud, bad)
        assert rc == plade_amd.PLADE_EINVAL and c.L.plade_last_error(c.h).decode() == message
        assert out.value is None                                   # NULL, not what it held before the call
        assert downloaded(valid(c, cloud)) == before
    finally:
        cloud.free()


FIVE = np.zeros((5, 6), F32)
FIVE[:, 0] = np.arange(5)              # five points in a row, 1 apart
FIVE[:, 5] = 1.0


def empty(name):
    """(raw call, parameters under which nothing is kept, the refusal, a valid call)"""
    return {
      "outliers": (raw_outliers, plade_amd._outlier_params("radius", None, None, 1.5, 10),
                   "plade_cloud_filter_outliers_dev: the filter keeps no point (a resident cloud cannot be empty)",
                   lambda c, cl: c.remove_outliers_dev(cl, mode="radius", radius=1.5, min_neighbours=2, info=True)),
      "components": (raw_components, plade_amd._component_params(1.5, 6, 0, 0),
                     "plade_cloud_filter_components_dev: the selection keeps no point (a resident cloud cannot be empty)",
                     lambda c, cl: c.filter_components_dev(cl, 1.5, min_size=5, info=True)),
    }[name]


@pytest.mark.parametrize("name", ("components", "outliers"))
def test_an_empty_result_leaves_out_null_and_the_context_as_it_was(pair, name):
    c = pair[0]
    raw, nothing, message, valid = empty(name)
    cloud = c.upload(FIVE)
    try:
        before = downloaded(valid(c, cloud))
        rc, out = raw(c, cloud, nothing)
        assert rc == plade_amd.PLADE_EFAIL and c.L.plade_last_error(c.h).decode() == message
        assert out.value is None
        assert downloaded(valid(c, cloud)) == before
    finally:
        cloud.free()


# ---- the host form and the resident form agree ---------------------------------------------------------------------------------------
def lattice_with_a_cross(n):
    """n points: a centre with four arms 0.9 away (the arms 1.27 and 1.8 from each other), the rest on a lattice of pitch 5 far off"""
    P = np.zeros((n, 6), F32)
    P[:, 5] = 1.0
    P[1:5, :3] = 0.9 * np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], F32)
    i = np.arange(n - 5)
    P[5:, 0], P[5:, 1], P[5:, 2] = 100.0 + 5.0 * (i % 8), 5.0 * (i // 8), 0.0
    return P


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def agree(c, P, host, dev, mask, kept_count=None):
    """host(c, P) -> (rows, kept_index, info), dev(c, cloud) -> (cloud, kept_index, info); mask: the per-point array both give"""
    rows, kept, info = host(c, P)
    cloud = c.upload(P)
    try:
        f, dkept, dinfo = dev(c, cloud)
        try:
            print(f"n {len(P)}: kept {len(kept)}")
            assert f.n == len(kept) == info["kept"] == dinfo["kept"] and same_bits(dkept, kept)
            assert same_bits(dinfo[mask], info[mask])
            assert same_bits(f.download().view(np.uint32), rows.view(np.uint32))
            assert same_bits(rows.view(np.uint32), P[kept].view(np.uint32))
        finally:
            f.free()
    finally:
        cloud.free()
    if kept_count is not None:
        assert len(kept) == kept_count
    return kept


def radius_filter(radius, min_neighbours):
    return (lambda c, P: c.remove_outliers(P, mode="radius", radius=radius, min_neighbours=min_neighbours),
            lambda c, cl: c.remove_outliers_dev(cl, mode="radius", radius=radius, min_neighbours=min_neighbours, info=True), "keep")


def components(radius, **sel):
    return (lambda c, P: c.connected_components(P, radius, **sel),
            lambda c, cl: c.filter_components_dev(cl, radius, info=True, **sel), "label")


@pytest.mark.parametrize("n", (65, 257))
def test_radius_filter_host_and_resident(pair, n):
    c, P = pair[0], P65 if n == 65 else P257
    kept = agree(c, P, *radius_filter(R, 10))
    assert 0 < len(kept) < n                                       # a real selection
    agree(c, P, *radius_filter(1000.0, 1), kept_count=n)           # everything is kept
    X = lattice_with_a_cross(n)
    assert agree(c, X, *radius_filter(1.0, 4), kept_count=1).tolist() == [0]   # the centre alone has four neighbours


@pytest.mark.parametrize("n", (65, 257))
def test_components_host_and_resident(pair, n):
    c, P = pair[0], P65 if n == 65 else P257
    kept = agree(c, P, *components(0.6 * R, min_size=3))
    assert 0 < len(kept) < n
    agree(c, P, *components(0.6 * R, min_size=1), kept_count=n)    # everything is kept
    X = lattice_with_a_cross(n)[5:]                                # isolated points: n - 5 components of one point
    assert agree(c, X, *components(1.0, keep_largest=1), kept_count=1).tolist() == [0]   # the tie goes to the smaller id
