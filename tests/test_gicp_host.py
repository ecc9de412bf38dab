"""Plane-to-plane ICP, host side (no GPU): the entry points are declared, exported, bound and listed; the default parameters need
no GPU; the structs match the header, which stays plain C; and the numpy restatement of the metric (tests/gicp_restate.py) has the
properties the semantics claim -- M = I / 2 at epsilon = 1, the point-to-plane limit for parallel normals, and its spectrum."""
import ctypes
import os
import re
import subprocess

import numpy as np

import plade_amd
import gicp_restate as G
import icp_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("plade_gicp_default_params", "plade_refine_gicp", "plade_refine_gicp_dev", "plade_gicp_linearize")
# Resolved when the module is imported: without the feature every test of this file fails here, the restatement's own included
# (those run no library code, but they pin the restatement of a library that must exist).
PARAMS, RESULT = plade_amd.GicpParams, plade_amd.GicpResult
ENTRY = {s: getattr(plade_amd.load_library(), s) for s in NEW}


def test_new_symbols_are_declared_exported_bound_and_listed():
    hdr = open(os.path.join(ROOT, "include", "plade_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(plade_[a-z_0-9]+)\s*\(", hdr))
    L = plade_amd.load_library()
    for s in NEW:
        assert s in declared, s
        assert hasattr(L, s), s
        assert s in plade_amd.ABI_SYMBOLS
        assert getattr(L, s).argtypes is not None
    for m in ("refine_gicp", "refine_gicp_dev", "gicp_linearize"):
        assert callable(getattr(plade_amd.Context, m))
    for t in ("plade_gicp_params", "plade_gicp_result"):
        assert re.search(r"\}\s*" + t + r"\s*;", hdr), t
    assert re.search(r"bool\s+refine_registration_gicp\s*\(", open(os.path.join(ROOT, "plade_amd", "csrc", "plade.h")).read())


def test_default_params_need_no_gpu():
    p = plade_amd.GicpParams()
    for k, _ in plade_amd.GicpParams._fields_:
        setattr(p, k, 7)
    plade_amd.load_library().plade_gicp_default_params(ctypes.byref(p))
    want = dict(plade_amd.icp_default_params(), epsilon=1e-3)
    assert {k: getattr(p, k) for k, _ in plade_amd.GicpParams._fields_} == want
    assert plade_amd.gicp_default_params() == want
    plade_amd.load_library().plade_gicp_default_params(None)          # NULL: nothing happens


def test_structs_match_the_header():
    P, Q = plade_amd.GicpParams, plade_amd.GicpResult
    assert [f for f, _ in P._fields_] == [f for f, _ in plade_amd.IcpParams._fields_] + ["epsilon"]
    assert ctypes.sizeof(P) == 56 and P.max_iterations.offset == 40 and P.min_correspondences.offset == 44 and P.epsilon.offset == 48
    assert [f for f, _ in Q._fields_] == [f for f, _ in plade_amd.IcpResult._fields_] + ["cost"]
    assert ctypes.sizeof(Q) == 56 and Q.rmse.offset == 24 and Q.final_dist.offset == 40 and Q.cost.offset == 48
    for f, _ in plade_amd.IcpParams._fields_:                          # the common fields sit where plade_icp_params has them
        assert getattr(P, f).offset == getattr(plade_amd.IcpParams, f).offset
    for f, _ in plade_amd.IcpResult._fields_:
        assert getattr(Q, f).offset == getattr(plade_amd.IcpResult, f).offset


def test_the_header_with_the_new_structs_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "plade_hip.h"\n#include <stddef.h>\n'
                   'int main(void) { plade_gicp_params p; plade_gicp_result r; plade_gicp_default_params(&p); r.cost = p.epsilon;\n'
                   '  return (int)(sizeof(p) + sizeof(r) + offsetof(plade_gicp_params, epsilon) + (size_t)r.cost) & 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _units(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    return [np.ascontiguousarray(v[:, k]) for k in range(3)]


def _full(M6):
    M00, M01, M02, M11, M12, M22 = M6
    return np.stack([np.stack([M00, M01, M02], -1), np.stack([M01, M11, M12], -1), np.stack([M02, M12, M22], -1)], -2)


# The tests below pin the restatement alone (its own sanity, before the GPU tests lean on it): they run no library code.
def test_epsilon_one_is_half_the_identity_bit_for_bit():
    M = _full(G.metric(_units(1000, 1), _units(1000, 2), 1.0))
    assert np.array_equal(M, np.broadcast_to(0.5 * np.eye(3), M.shape))


def test_epsilon_one_moments_are_half_the_point_to_point_moments():
    """27 moments at epsilon = 1 against point-to-point moments formed without any matrix inverse: J = [-[u]x | I], H = J^T J / 2,
    g = J^T e / 2 (a product by 1/2 is exact, so every term agrees bit for bit and the fsums are equal)."""
    import math
    z = np.load(os.path.join(ROOT, "tests", "golden", "g8_polyhedron.npz"))
    tgt, src, gt = z["target"], z["source"][:4000], z["groundtruth"]
    target = R.Target(tgt)
    T = R.perturb(gt, 0.02, 0.02, seed=3)
    c = np.array([0.3, -0.2, 0.1])
    d = 0.02 * target.diag
    corr, mom, _ = G.linearize(target, src, T, d, 1.0, center=c)
    sel = corr >= 0
    assert sel.sum() > 500
    X = src[sel, :3].astype(np.float64)
    q = tgt[corr[sel], :3].astype(np.float64)
    p = [((T[r, 0] * X[:, 0] + T[r, 1] * X[:, 1]) + T[r, 2] * X[:, 2]) + T[r, 3] for r in range(3)]
    e = [p[r] - q[:, r] for r in range(3)]
    u = [p[r] - c[r] for r in range(3)]
    zero, one = np.zeros(len(X)), np.ones(len(X))
    J = [[zero, u[2], -u[1], one, zero, zero], [-u[2], zero, u[0], zero, one, zero], [u[1], -u[0], zero, zero, zero, one]]
    H = [math.fsum(0.5 * ((J[0][a] * J[0][b] + J[1][a] * J[1][b]) + J[2][a] * J[2][b])) for a in range(6) for b in range(a, 6)]
    g = [math.fsum(0.5 * ((J[0][a] * e[0] + J[1][a] * e[1]) + J[2][a] * e[2])) for a in range(6)]
    assert np.array_equal(mom[:27], np.array(H + g)), mom[:27] - np.array(H + g)
    ee = math.fsum((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    assert mom[28] == ee and mom[27] == math.fsum(0.5 * ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])) and mom[29] == sel.sum()


def test_parallel_normals_give_the_point_to_plane_limit():
    """nh = ah = n: M = (I + ((1 - eps) / eps) n n^T) / 2 to 1e-12 relative (the condition number is 1 / eps: three orders of
    margin at eps = 1e-3)."""
    n = _units(2000, 4)
    N = np.stack(n, -1)
    for eps in (1e-3, 1e-2, 0.5):
        M = _full(G.metric(n, n, eps))
        want = 0.5 * (np.eye(3) + ((1.0 - eps) / eps) * N[:, :, None] * N[:, None, :])
        assert np.abs(M - want).max() <= 1e-12 * np.abs(want).max(), (eps, np.abs(M - want).max() / np.abs(want).max())


def test_the_metric_is_symmetric_with_its_spectrum_in_bounds():
    for eps in (1e-3, 0.1, 1.0):
        M = _full(G.metric(_units(10_000, 5), _units(10_000, 6), eps))
        assert np.array_equal(M, np.swapaxes(M, 1, 2))
        ev = np.linalg.eigvalsh(M)
        assert ev.min() >= 0.5 * (1 - 1e-9) and ev.max() <= (1 + 1e-9) / (2 * eps), (eps, ev.min(), ev.max())


def test_restated_sample_on_a_cloud_worked_by_hand():
    """Five points, leaf 1: three in the voxel [0, 1)^3 (one of them with a NaN normal), two in [1, 2) x [0, 1)^2 whose normals cancel.
    Every value is exact in fp32 and fp64, so the fused rows are known without running anything."""
    nan = np.nan
    src = np.array([[1.25, 0.5, 0.5, 0, 0, 1],        # voxel (1, 0, 0)
                    [0.25, 0.25, 0.5, 0, 0, 2],       # voxel (0, 0, 0): finite normals (0, 0, 2) and (0, 3, 2) -> (0, 3, 4) / 5
                    [0.75, 0.25, 0.5, nan, 0, 0],     #   a NaN normal counts for the position only
                    [1.75, 0.5, 0.5, 0, 0, -1],       # voxel (1, 0, 0): opposite normals cancel -> three NaNs
                    [0.5, 0.25, 0.5, 0, 3, 2]], np.float32)
    S = G.sample(src, 1.0)
    assert S.shape == (2, 6)
    assert np.array_equal(S[0], np.array([0.5, 0.25, 0.5, 0.0, 0.6, 0.8], np.float32))       # ascending voxel order
    assert np.array_equal(S[1, :3], np.array([1.5, 0.5, 0.5], np.float32)) and np.isnan(S[1, 3:]).all()
    corr = G.match(R.Target(np.array([[0.5, 0.25, 0.5, 0, 0, 1], [1.5, 0.5, 0.5, 0, 0, 1]], np.float32)), S, np.eye(4), 0.1)
    assert list(corr) == [0, -1]                                        # the sample point without a normal has no correspondence
