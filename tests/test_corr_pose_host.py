"""The pose estimator over correspondences without a GPU: the ABI (declared, exported, bound, listed; defaults; struct layouts; a C99
header) and the numpy restatement of its semantics (tests/corr_pose_restate.py) on inputs whose answers are known by hand."""
import ctypes
import os
import re
import subprocess

import numpy as np

import plade_amd
import corr_cases
import corr_pose_restate as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("plade_corr_pose_default_params", "plade_estimate_pose_corr", "plade_estimate_pose_corr_dev", "plade_corr_pose_moments",
           "plade_register_features", "plade_register_features_dev")


def test_symbols_declared_exported_bound_listed():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "plade_hip.h")).read(), flags=re.S)
    L = plade_amd.load_library()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert hasattr(L, s), s
        assert s in plade_amd.ABI_SYMBOLS, s
        assert getattr(L, s).argtypes is not None, s
    for m in ("estimate_pose", "estimate_pose_dev", "corr_pose_moments", "register_features", "register_features_dev"):
        assert callable(getattr(plade_amd.Context, m)), m


def test_defaults():
    assert plade_amd.corr_pose_default_params() == dict(inlier_dist=0.0, edge_similarity=0.9, seed=0, hypotheses=65536, min_inliers=3,
                                                        refine_iterations=5)
    p = plade_amd.CorrPoseParams()
    ctypes.memset(ctypes.byref(p), 0xff, ctypes.sizeof(p))
    plade_amd.load_library().plade_corr_pose_default_params(ctypes.byref(p))
    assert p.reserved == 0


def test_struct_layouts_and_c99(tmp_path):
    """sizeof / offsetof of the two structs as a C99 compiler lays them out against the ctypes mirrors"""
    fields = {"plade_corr_pose_params": plade_amd.CorrPoseParams, "plade_corr_pose_result": plade_amd.CorrPoseResult}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "plade_hip.h"', 'int main(void) {']
    for name, cls in fields.items():
        lines.append('printf("%%zu", sizeof(%s));' % name)
        for f, _ in cls._fields_:
            lines.append('printf(" %%zu", offsetof(%s, %s));' % (name, f))
        lines.append('printf("\\n");')
    lines += ["return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                        str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    for line, cls in zip(out, fields.values()):
        got = [int(x) for x in line.split()]
        assert got == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_], cls


def test_mix64_and_draws():
    # the first three outputs of splitmix64 from state 0 (Steele, Lea, Flood 2014; the published test vector)
    assert P.mix64(0) == 0xE220A8397B1DCDAF
    assert P.mix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert P.mix64(2 * 0x9E3779B97F4A7C15 & ((1 << 64) - 1)) == 0x06C45D188009454F
    # hypothesis 0, draw 0 of seed 0 by hand: z = mix64(mix64(0) ^ 0), index = ((z >> 32) * M) >> 32
    for M in (3, 1000, 5000, (1 << 31) - 1):
        d = P.draws(0, 300, M)
        assert d.min() >= 0 and d.max() < M
        base = P.mix64(0)
        for h in (0, 1, 299):
            for k in range(3):
                z = P.mix64(base ^ (4 * h + k))
                assert d[h, k] == ((z >> 32) * M) >> 32
    assert (P.draws(1, 50, 1000) != P.draws(2, 50, 1000)).any()
    assert len(np.unique(P.draws(0, 4096, 1000))) > 900          # (spread over the range)


def test_dyadic_triangle_maps_exactly():
    """a 3-3 right triangle, turned by 90 degrees about z and moved by a dyadic vector: every intermediate is exact in fp64"""
    S = np.array([[0.0, 0, 0], [3, 0, 0], [0, 3, 0], [1, 1, 1]])
    t0 = np.array([1.0, 2.0, -0.5])
    Rz = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    Q = S @ Rz.T + t0
    tri, status, T = P.hypotheses(S, Q, triples=[[0, 1, 2]])
    assert status[0] == 0
    assert np.array_equal(T[0, :, :3], Rz) and np.array_equal(T[0, :, 3], t0)
    assert np.array_equal(P.d2_under(T[0], S, Q), np.zeros(4))
    assert P.flags_under(T[0], S, Q, 0.5).all()


def test_status_codes_on_constructed_triples():
    S = np.array([[0.0, 0, 0], [3, 0, 0], [0, 3, 0], [6, 0, 0], [0, 0, 0]])
    Q = S.copy()
    Q[2] = (0, 1, 0)                    # the edge (0, 2): 3 against 1
    _, status, T = P.hypotheses(S, Q, sim=0.9, triples=[[0, 0, 1], [1, 2, 1], [0, 1, 2], [0, 1, 3], [0, 4, 1]])
    # repeated index; repeated index; an edge-length mismatch; collinear on both sides; two coincident points (u = 0)
    assert status.tolist() == [1, 1, 2, 3, 3]
    assert not T.any()
    _, status, _ = P.hypotheses(S, Q, sim=0.0, triples=[[0, 1, 2]])      # nothing is rejected at 0
    assert status[0] == 0


def test_restatement_recovers_the_pose_without_noise():
    for seed, M, share in ((11, 200, 0.3), (12, 1500, 0.1)):
        S, Q, corr, T, inl = corr_cases.synthetic(M, share, seed)
        Sc, Qc = P.packed(S, Q, corr)
        r = P.estimate(Sc, Qc, 0.01, H=4096)
        assert r["ok"] and np.array_equal(r["flags"], inl)
        assert np.abs(r["T"] - T[:3]).max() < 1e-9
        assert r["inliers"] == inl.sum() and r["rmse"] < 1e-9
    S, Q, corr, T, inl = corr_cases.synthetic(300, 0.5, 13, shuffle=True)
    Sc, Qc = P.packed(S, Q, corr)
    assert np.abs(P.estimate(Sc, Qc, 0.01, H=1024)["T"] - T[:3]).max() < 1e-9


def test_failures_of_the_restatement():
    S, Q, corr, T, inl = corr_cases.synthetic(50, 0.5, 3)
    assert P.estimate(S[:2], Q[:2], 0.1)["failure"] == 1
    line = np.outer(np.arange(40.0), (1.0, 2.0, 0.5))
    assert P.estimate(line, line + 1.0, 0.1, H=256)["failure"] == 2
    assert P.estimate(S, Q, 0.01, H=256, min_inliers=40)["failure"] == 3


def test_horn_is_the_least_squares_rotation():
    rng = np.random.default_rng(5)
    for case in range(40):
        n = int(rng.integers(3, 60))
        S = rng.normal(size=(n, 3)) * rng.uniform(0.1, 10.0, 3)
        if case % 4 == 1:
            S[:, 2] = 0.5                                       # planar
        R0 = corr_cases.random_se3(case)[:3, :3]
        Q = S @ R0.T + 0.01 * rng.normal(size=(n, 3))
        if case % 4 == 2:
            Q[:, 0] = -Q[:, 0]                                  # mirrored: the best PROPER rotation is wanted
        C = (Q - Q.mean(0)).T @ (S - S.mean(0))
        Rh, Rk = P.horn(C), P.kabsch(C)
        assert np.abs(Rh.T @ Rh - np.eye(3)).max() < 1e-12 and np.linalg.det(Rh) > 0.999
        sv = np.linalg.svd(C, compute_uv=False)
        if sv[1] > 1e-3 * sv[0] and (case % 4 != 2 or sv[2] < 0.9 * sv[1]):      # (a unique maximiser)
            assert np.abs(Rh - Rk).max() < 1e-9, case
        assert np.trace(Rh.T @ C) >= np.trace(Rk.T @ C) - 1e-9 * sv[0]


def test_terrain_pair_shape():
    tg, sr, T = corr_cases.terrain_pair(500)
    assert tg.shape == (500, 6) and tg.dtype == np.float32 and sr.shape[1] == 6 and abs(len(sr) - 500) <= 2
    assert np.allclose(np.linalg.norm(tg[:, 3:], axis=1), 1.0, atol=1e-5)
    back = sr[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    assert back[:, 0].min() > -0.1 and back[:, 0].max() < 7.5 and np.abs(back[:, 2]).max() < 5.0
