"""Point-to-plane ICP refinement, host side (no GPU): the entry points are exported and bound, the defaults come through the
ctypes struct, and the numpy restatement of the semantics (tests/icp_restate.py) refines the golden real-data cases to well
within 1e-3 of their ground truth."""
import ctypes
import os

import numpy as np
import pytest

import plade_amd
import icp_restate as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
NEW = ("plade_icp_default_params", "plade_refine_icp", "plade_refine_icp_dev", "plade_icp_linearize")


def test_new_symbols_are_exported_and_bound():
    L = plade_amd.load_library()
    for s in NEW:
        assert hasattr(L, s), s
        assert s in plade_amd.ABI_SYMBOLS
    for m in ("refine_icp", "refine_icp_dev", "icp_linearize"):
        assert callable(getattr(plade_amd.Context, m))
    assert callable(plade_amd.icp_default_params)


def test_default_params_through_the_struct():
    p = plade_amd.IcpParams()
    p.max_iterations = -7
    plade_amd.load_library().plade_icp_default_params(ctypes.byref(p))
    assert (p.source_leaf, p.max_dist, p.min_dist, p.eps_translation) == (0.0, 0.0, 0.0, 0.0)   # scale-free automatic values
    assert (p.eps_rotation, p.max_iterations, p.min_correspondences) == (1e-6, 60, 100)
    d = plade_amd.icp_default_params()
    assert d == {"source_leaf": 0.0, "max_dist": 0.0, "min_dist": 0.0, "eps_rotation": 1e-6, "eps_translation": 0.0,
                 "max_iterations": 60, "min_correspondences": 100}
    assert ctypes.sizeof(plade_amd.IcpParams) == 48 and ctypes.sizeof(plade_amd.IcpResult) == 48


def test_stage_schedule():
    c = R.resolve(10.0)
    assert c["dists"] == [0.25, 0.125, 0.0625, 0.03125, 0.025]
    assert c["leaf"] == pytest.approx(0.05, rel=1e-15) and c["eps_trans"] == pytest.approx(1e-5, rel=1e-15) and (c["max_iter"], c["min_corr"]) == (60, 100)
    assert R.resolve(10.0, max_dist=0.01)["dists"] == [0.01]     # an automatic min_dist is capped at max_dist


def test_tolerances_never_fall_below_the_fp32_resolution():
    ulp = 2.0 ** -23
    c = R.resolve(10.0, amax=6.0)                                 # near the origin the floor (2.9e-6) is inactive
    assert (c["eps_trans"], c["eps_rot"]) == (1e-6 * 10.0, 1e-6)
    c = R.resolve(10.0, amax=5000.0)                              # 500 D away: 4 ulp(5000) = 2.4e-3 > 1e-5
    assert c["eps_trans"] == 4 * ulp * 5000.0 and c["eps_rot"] == 4 * ulp * 5000.0 / 10.0
    c = R.resolve(10.0, eps_translation=1e-9, eps_rotation=1e-12, amax=5000.0)   # given values are floored too
    assert c["eps_trans"] == 4 * ulp * 5000.0 and c["eps_rot"] == 4 * ulp * 5000.0 / 10.0
    c = R.resolve(10.0, eps_translation=1.0, eps_rotation=0.5, amax=5000.0)      # and a looser value stays
    assert (c["eps_trans"], c["eps_rot"]) == (1.0, 0.5)


def test_exact_match_breaks_ties_by_index_and_skips_nan_normals():
    tgt = np.zeros((4, 6), np.float32)
    tgt[:, :3] = [[1, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, 5]]
    tgt[:, 5] = 1
    tgt[0, 3:] = np.nan                                        # the nearest (and smallest index) point has no normal
    t = R.Target(tgt)
    P = np.array([[0.5, 0, 0], [0, 0.5, 0], [0, 0, 4.9], [0, 0, 9]], np.float32)
    assert t.match(P, 1.0).tolist() == [-1, 1, 3, -1]          # 0 wins the tie with 2 but is not matched; the last is too far
    # the boundary: flann_d2 == d * d is not a correspondence
    assert t.match(np.array([[0, 0, 4.5]], np.float32), 0.5).tolist() == [-1]
    assert t.match(np.array([[0, 0, 4.5]], np.float32), 0.5000001).tolist() == [3]


def _fixture(name):
    return np.load(os.path.join(GOLDEN, name))


def test_restatement_refines_the_polyhedron_from_its_recorded_result():
    z = _fixture("g8_polyhedron.npz")
    T, info = R.refine(z["target"], z["source"], z["recorded"])
    assert info["converged"] and info["failure"] == 0
    assert np.linalg.norm(T - z["groundtruth"]) <= 1e-3


def test_restatement_refines_the_room_from_a_perturbation():
    z = _fixture("g9_room.npz")
    T0 = R.perturb(z["groundtruth"], 0.05, 0.05, seed=1)
    assert 0.08 < np.linalg.norm(T0 - z["groundtruth"]) < 0.2
    T, info = R.refine(z["target"], z["source"], T0)
    assert info["converged"] and info["failure"] == 0 and info["stages"] == len(R.resolve(R.Target(z["target"]).diag)["dists"])
    assert np.linalg.norm(T - z["groundtruth"]) <= 1e-3


def test_restatement_failure_reasons():
    rng = np.random.default_rng(0)
    plane = np.zeros((5000, 6), np.float32)
    plane[:, :2] = rng.uniform(-1, 1, size=(5000, 2))
    plane[:, 5] = 1
    T, info = R.refine(plane, plane, np.eye(4))
    assert info["failure"] == R.DEGENERATE and np.array_equal(T, np.eye(4))
    far = plane.copy()
    far[:, 2] += 100
    T, info = R.refine(plane, far, np.eye(4))
    assert info["failure"] == R.TOO_FEW and info["correspondences"] == 0


# ---- changes of frame and units -------------------------------------------------------------------------------------------------
def planes(normals, n=6000, seed=0):
    """Points on the unit squares through the origin with the given exact axis normals (the other two coordinates in [0, 1])."""
    rng = np.random.default_rng(seed)
    parts = []
    for ax in normals:
        p = np.zeros((n // len(normals), 6), np.float32)
        free = [k for k in range(3) if k != ax]
        p[:, free] = rng.uniform(0, 1, size=(len(p), 2))
        p[:, 3 + ax] = 1
        parts.append(p)
    return np.ascontiguousarray(np.concatenate(parts))


@pytest.mark.parametrize("offset", [0.0, 1000.0])
def test_restatement_single_plane_and_crease_are_degenerate_in_any_frame(offset):
    for normals in ((2,), (0, 1)):            # a crease of two planes: translation along their common line is unconstrained
        cloud = planes(normals)
        F = R.frame(offset * R.Target(cloud).diag)
        moved = R.move(cloud, F)
        T, info = R.refine(moved, moved, np.eye(4), S=moved[:, :3])
        assert info["failure"] == R.DEGENERATE and info["iterations"] == 0, (normals, info)


def test_restatement_three_planes_are_not_degenerate_far_away():
    cloud = planes((0, 1, 2))
    for offset in (0.0, 1000.0):
        F = R.frame(offset * R.Target(cloud).diag)
        moved = R.move(cloud, F)
        T0 = R.conjugate(R.perturb(np.eye(4), 0.01, 0.01, seed=2), F)
        T, info = R.refine(moved, moved, T0, S=moved[:, :3])
        assert info["failure"] == 0 and info["converged"], info
        assert np.linalg.norm(R.back(T, F) - np.eye(4)) <= 1e-3


def _g9_subsample(n=4000):
    z = _fixture("g9_room.npz")
    target = R.Target(z["target"])
    S = R.voxel_downsample(z["source"][:, :3], 0.005 * target.diag)
    S = S[np.random.default_rng(1).choice(len(S), n, replace=False)]
    return z, target.diag, np.ascontiguousarray(S)


def test_restatement_is_equivariant_under_changes_of_frame():
    """g9 on a subsample of S, moved up to 500 D from the origin (and rotated): the far frames converge like the near one, to
    the same T.  About the origin, the linearisation spins to the cap from ~16 D and fails from ~160 D."""
    z, D, S = _g9_subsample()
    T0, gt = R.perturb(z["groundtruth"], 0.05, 0.05, seed=1), z["groundtruth"]
    base, info0 = R.refine(z["target"], None, T0, S=S)
    assert info0["converged"] and np.linalg.norm(base - gt) <= 1e-3
    for offset, rot in ((100.0, 0.0), (500.0, 0.0), (100.0, 0.4)):
        F = R.frame(offset * D, rot)
        T, info = R.refine(R.move(z["target"], F), None, R.conjugate(T0, F), S=R.move(S, F))
        assert info["converged"] and info["failure"] == 0 and info["iterations"] < 60, (offset, rot, info)
        assert np.linalg.norm(R.back(T, F) - gt) <= 1e-3
        assert np.linalg.norm(R.back(T, F) - base) <= 1e-4, (offset, rot, np.linalg.norm(R.back(T, F) - base))


def test_restatement_does_not_depend_on_the_units():
    z, D, S = _g9_subsample()
    T0, gt = R.perturb(z["groundtruth"], 0.05, 0.05, seed=1), z["groundtruth"]
    _, info0 = R.refine(z["target"], None, T0, S=S)
    F = np.eye(4)
    for scale in (1000.0, 0.001):
        T, info = R.refine(R.move(z["target"], F, scale), None, R.conjugate(T0, F, scale), S=R.move(S, F, scale))
        assert info["converged"] and abs(info["iterations"] - info0["iterations"]) <= 2, (scale, info, info0)
        assert np.linalg.norm(R.back(T, F, scale) - gt) <= 1e-3

