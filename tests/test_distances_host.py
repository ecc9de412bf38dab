"""Cloud-to-cloud distances, host side (no GPU): the entry points are exported, bound and listed, the summary struct matches the
header, and the numpy restatement of the semantics (tests/distance_restate.py) agrees with a k-d tree and separates right from
wrong registrations on the synthetic rooms."""
import ctypes

import numpy as np
import pytest

import plade_amd
from plade_amd.synth import make_pair
import distance_restate as R

NEW = ("plade_cloud_distances", "plade_cloud_distances_dev")


def test_new_symbols_are_exported_bound_and_listed():
    L = plade_amd.load_library()
    for s in NEW:
        assert hasattr(L, s), s
        assert s in plade_amd.ABI_SYMBOLS
        assert getattr(L, s).argtypes is not None
    for m in ("cloud_distances", "cloud_distances_dev", "evaluate_registration"):
        assert callable(getattr(plade_amd.Context, m))


def test_summary_struct_matches_the_header():
    S = plade_amd.DistanceSummary
    assert ctypes.sizeof(S) == 3 * 8 + 5 * 8
    assert [f for f, _ in S._fields_] == ["n", "count", "plane_count", "fitness", "rmse", "mean", "max", "plane_rmse"]
    assert S.fitness.offset == 24 and S.plane_rmse.offset == 56


def test_restatement_agrees_with_a_kd_tree():
    spatial = pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(7)
    tgt = np.zeros((20_000, 6), np.float32)
    tgt[:, :3] = rng.uniform(-1, 1, size=(20_000, 3))
    tgt[:, 3:] = rng.normal(size=(20_000, 3))
    src = rng.uniform(-1.2, 1.2, size=(5_000, 3)).astype(np.float32)
    T = np.eye(4)
    T[:3, 3] = [0.01, -0.02, 0.03]
    P = R.transform_f32(T, src)
    tree = spatial.cKDTree(tgt[:, :3].astype(np.float64))
    dist, nn = tree.query(P.astype(np.float64), k=2)
    clear = (dist[:, 1] - dist[:, 0]) > 1e-5                  # no near-ties: fp32 and fp64 must agree on the nearest point
    for d in (0.02, 0.1, 5.0):
        idx, d2, plane, s = R.cloud_distances(tgt, src, d, T=T)
        inside = dist[:, 0] < d * (1 - 1e-5)
        outside = dist[:, 0] > d * (1 + 1e-5)
        assert np.array_equal(idx[clear & inside], nn[clear & inside, 0])
        assert (idx[outside] == -1).all() and np.isinf(d2[outside]).all() and np.isnan(plane[outside]).all()
        assert np.allclose(np.sqrt(d2[clear & inside]), dist[clear & inside, 0], rtol=1e-5, atol=1e-6)
        sel = idx >= 0
        assert s["count"] == sel.sum() and s["fitness"] == sel.sum() / len(src)
        assert np.isclose(s["rmse"], np.sqrt(np.mean(dist[sel, 0] ** 2)), rtol=1e-5)
    assert s["count"] == len(src)                            # d = 5: every point corresponds


def test_restatement_separates_right_from_wrong():
    # fitness at d = 0.01 D of a 4 000-point sample of make_pair(1M, seed 0): the issue's table, measured on all source points,
    # is 0.993 (T_gt and after a 0.01 rad yaw), 0.462 (the rooms' 180 degree symmetry), 0.000 (180 degrees about x), 0.188 (I)
    tg, sr, Tgt = make_pair(1_000_000, seed=0)
    D = R.diag(tg)
    assert abs(D - 13.22) < 0.01
    sub = sr[np.random.default_rng(0).choice(len(sr), 4000, replace=False), :3]
    fit = {}
    for name, T in (("gt", Tgt), ("yaw", R.rot_z(0.01) @ Tgt), ("z180", Tgt @ R.rot_z(np.pi)), ("x180", Tgt @ R.rot_x(np.pi)),
                    ("identity", np.eye(4))):
        idx, _ = R.nearest(tg[:, :3], R.transform_f32(T, sub), 0.01 * D)
        fit[name] = (idx >= 0).mean()
    assert fit["gt"] >= 0.97 and fit["yaw"] >= 0.97, fit
    assert 0.40 <= fit["z180"] <= 0.53, fit
    assert fit["x180"] <= 0.01, fit
    assert 0.14 <= fit["identity"] <= 0.24, fit
