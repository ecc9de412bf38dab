"""Plane-to-plane (generalized) ICP refinement on the GPU (plade_refine_gicp, plade_gicp_linearize, plade_amd/csrc/k_gicp.hip)
against the numpy restatement of its semantics (tests/gicp_restate.py): exact correspondences, moments, the sample, one step and
the whole loop, accuracy, down-weighting, symmetry, determinism, failure paths and the CLI switch."""
import os
import subprocess
import threading

import numpy as np
import pytest

import plade_amd
from plade_amd.plyio import write_ply
from plade_amd.synth import make_pair
from conftest import ORIENTED
import gicp_restate as G
import icp_restate as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "plade_amd", "PLADE")
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def gctx():
    c = plade_amd.Context(0, **ORIENTED)
    yield c
    c.close()


def _g(name):
    return np.load(os.path.join(GOLDEN, name))


def _same_moments(m_gpu, m_ref, absm):
    """The tolerance of tests/test_gpu_icp.py: the count equal, every other moment within 1e-12 of the sum of |terms| (the terms
    are bit-equal by construction; only the order of a few thousand fp64 additions differs)."""
    assert m_gpu[29] == m_ref[29]
    assert np.all(np.abs(m_gpu - m_ref) <= 1e-12 * absm + 1e-300), np.abs(m_gpu - m_ref) / np.maximum(absm, 1e-300)


def _check_seam(ctx, target, tgt, src, T, d, eps, center=None):
    corr, mom = ctx.gicp_linearize(tgt, src, T, d, epsilon=eps, center=center)
    c_ref, m_ref, absm = G.linearize(target, src, T, d, eps, center=center)
    assert np.array_equal(corr, c_ref), (int((corr != c_ref).sum()), d)
    _same_moments(mom, m_ref, absm)
    return corr, mom


def _boundary_dist(target, S, T):
    """A stage distance d with (float)d * (float)d equal to some probe's nearest flann_d2: that probe sits on the boundary."""
    P = R.transform_f32(T, S[:64, :3])
    for p in P:
        dd = ((p[0] - target.xyz[:, 0]) ** 2 + (p[1] - target.xyz[:, 1]) ** 2) + (p[2] - target.xyz[:, 2]) ** 2
        v = np.float32(dd.min())
        if not v > 0:
            continue
        d = np.float32(np.sqrt(np.float64(v)))
        for cand in (d, np.nextafter(d, np.float32(1)), np.nextafter(d, np.float32(0))):
            if np.float32(cand) * np.float32(cand) == v:
                return float(cand)
    return None


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _fro(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)))


# ---- 1. the seam on the golden scenes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g8_polyhedron.npz", "g9_room.npz"])
def test_seam_is_exact_on_the_golden_scenes(gctx, name):
    z = _g(name)
    tgt, src, gt = z["target"], np.ascontiguousarray(z["source"]), z["groundtruth"]
    target = R.Target(tgt)
    D = target.diag
    for T in (gt, R.perturb(gt, 0.03, 0.03, seed=5)):
        for d in (0.025 * D, 0.0025 * D):
            for eps in (1e-3, 1.0):
                corr, mom = _check_seam(gctx, target, tgt, src, T, d, eps)
                assert (corr >= 0).sum() > 1000
                corr2, mom2 = gctx.gicp_linearize(tgt, src, T, d, epsilon=eps)        # repeat: bitwise
                assert np.array_equal(corr, corr2) and np.array_equal(_bits(mom), _bits(mom2))
    corr0, mom0 = gctx.gicp_linearize(tgt, src, gt, 0.025 * D)                         # epsilon 0: the default 1e-3
    corr1, mom1 = gctx.gicp_linearize(tgt, src, gt, 0.025 * D, epsilon=1e-3)
    assert np.array_equal(corr0, corr1) and np.array_equal(_bits(mom0), _bits(mom1))


# ---- 2. the seam's edge cases (a few thousand points each) ------------------------------------------------------------------------
def _small(seed=0, n_t=4000, n_s=2000):
    z = _g("g9_room.npz")
    rng = np.random.default_rng(seed)
    tgt = np.ascontiguousarray(z["target"][rng.choice(len(z["target"]), n_t, replace=False)])
    src = np.ascontiguousarray(z["source"][rng.choice(len(z["source"]), n_s, replace=False)])
    return tgt, src, z["groundtruth"]


def test_seam_boundary_probe(gctx):
    tgt, src, gt = _small()
    target = R.Target(tgt)
    d = _boundary_dist(target, src, gt)
    assert d is not None
    corr, _ = _check_seam(gctx, target, tgt, src, gt, d, 1e-3)
    dd = np.float32(d) * np.float32(d)
    P = R.transform_f32(gt, src[:64, :3])
    near = np.array([np.float32((((p[0] - target.xyz[:, 0]) ** 2 + (p[1] - target.xyz[:, 1]) ** 2) + (p[2] - target.xyz[:, 2]) ** 2).min())
                     for p in P])
    on = np.flatnonzero(near == dd)
    assert len(on) >= 1 and (corr[on] == -1).all()                     # on the boundary: strict <, no correspondence


@pytest.mark.parametrize("side", ["target", "source"])
def test_seam_nan_zero_and_long_normals(gctx, side):
    tgt, src, gt = _small(1)
    d = 0.05 * R.Target(tgt).diag
    base, _ = gctx.gicp_linearize(tgt, src, gt, d)
    assert (base >= 0).sum() > 500
    rows = np.unique(base[base >= 0]) if side == "target" else np.flatnonzero(base >= 0)
    nan_rows, zero_rows, long_rows = rows[0::3], rows[1::3], rows[2::3]
    mod = (tgt if side == "target" else src).copy()
    mod[nan_rows, 3 + (nan_rows % 3)] = np.nan                            # one component NaN
    mod[zero_rows, 3:] = 0.0
    generic, long_rows = long_rows[0::2], long_rows[1::2]
    mod[generic, 3:] *= np.float32(3.0)                                   # the scene's own normals, length 3: the product rounds in fp32,
    #                                                                       so these rows are checked against the restatement on the same rows
    mod[long_rows, 3:] = 0.0                                              # exact axis normals: 3 / sqrt(9) = 1 with no rounding
    mod[long_rows, 3 + (long_rows % 3)] = 1.0
    unit_form = mod.copy()
    mod[long_rows, 3:] *= np.float32(3.0)
    ln = np.linalg.norm(mod[generic, 3:].astype(np.float64), axis=1)
    assert len(generic) > 20 and np.all(np.abs(ln - 3) < 1e-3) and np.any(ln != 3.0)
    t2, s2 = (mod, src) if side == "target" else (tgt, mod)
    corr, mom = _check_seam(gctx, R.Target(t2), t2, s2, gt, d, 1e-3)
    dead = np.r_[nan_rows, zero_rows]
    if side == "target":
        assert not np.isin(corr, dead).any() and (corr[np.isin(base, dead)] == -1).all()      # no second choice
        assert np.isin(corr, long_rows).any() and np.isin(corr, generic).any()
    else:
        assert (corr[dead] == -1).all() and (corr[long_rows] >= 0).all() and (corr[generic] >= 0).all()
    keep = np.ones(len(base), bool)
    keep[np.isin(base, dead) if side == "target" else dead] = False
    assert np.array_equal(corr[keep], base[keep])
    # an axis normal of length 3 gives the moments of its unit normal (the generic rows are the same in both forms)
    t1, s1 = (unit_form, src) if side == "target" else (tgt, unit_form)
    c_ref, m_ref, absm = G.linearize(R.Target(t1), s1, gt, d, 1e-3)
    assert np.array_equal(corr, c_ref)
    _same_moments(mom, m_ref, absm)


def test_seam_ties_go_to_the_lower_index(gctx):
    tgt, src, gt = _small(2)
    rng = np.random.default_rng(3)
    dup = tgt[rng.choice(len(tgt), 1500, replace=False)].copy()
    dup[:, 3:] = dup[:, [4, 5, 3]]                                       # the same positions, other normals
    both = np.ascontiguousarray(np.concatenate([dup, tgt]))
    target = R.Target(both)
    corr, _ = _check_seam(gctx, target, both, src, gt, 0.05 * R.Target(tgt).diag, 1e-3)
    assert (corr[corr >= 0] < len(dup)).any()
    hit = corr[corr >= len(dup)]
    twins = {p.tobytes() for p in dup[:, :3]}
    assert not any(both[j, :3].tobytes() in twins for j in hit)          # a duplicated position is never matched at its higher index


@pytest.mark.parametrize("offset_in_diagonals", [False, True])
def test_seam_far_from_the_origin_and_a_given_centre(gctx, offset_in_diagonals):
    tgt0, src0, gt0 = _small(4)
    D = R.Target(tgt0).diag
    F = R.frame(500.0 * (D if offset_in_diagonals else 1.0), 0.3)
    tgt, src = R.move(tgt0, F), R.move(src0, F)
    target = R.Target(tgt)
    T = R.conjugate(R.perturb(gt0, 0.02, 0.02, seed=6), F)
    for c in (None, (3.0, -2.0, 0.5), R.apply(T, R.sample_mean(src))):
        corr, _ = _check_seam(gctx, target, tgt, src, T, 0.05 * D, 1e-3, center=c)
        assert (corr >= 0).sum() > 300
    c0, m0 = gctx.gicp_linearize(tgt, src, T, 0.05 * D)                 # no centre: the origin
    c1, m1 = gctx.gicp_linearize(tgt, src, T, 0.05 * D, center=(0.0, 0.0, 0.0))
    assert np.array_equal(c0, c1) and np.array_equal(_bits(m0), _bits(m1))


def test_seam_one_source_point(gctx):
    tgt, src, gt = _small(5)
    target = R.Target(tgt)
    d = 0.05 * target.diag
    base, _ = gctx.gicp_linearize(tgt, src, gt, d)
    i = int(np.flatnonzero(base >= 0)[0])
    corr, mom = _check_seam(gctx, target, tgt, src[i:i + 1], gt, d, 1e-3, center=(0.1, 0.2, 0.3))
    assert corr[0] == base[i] and mom[29] == 1.0
    k = int(np.flatnonzero(base < 0)[0]) if (base < 0).any() else None
    if k is not None:
        corr, mom = gctx.gicp_linearize(tgt, src[k:k + 1], gt, d)
        assert corr[0] == -1 and not mom.any()


# ---- 3. the sample ---------------------------------------------------------------------------------------------------------------
def _sample(ctx, src, leaf):
    rows, _ = ctx.merge_clouds([np.ascontiguousarray(src)], leaf=np.float32(leaf), per_voxel=False)
    return rows


def test_the_sample_is_the_merge_of_the_source_alone(gctx):
    z = _g("g9_room.npz")
    tgt, src, gt = z["target"], z["source"], z["groundtruth"]
    leaf = 0.005 * R.Target(tgt).diag
    _, info = gctx.refine_gicp(tgt, src, gt)
    S = _sample(gctx, src, leaf)
    assert info["samples"] == len(S)
    assert G.MR.same_bits(S, G.sample(src, leaf))                         # and the merge is what the restatement samples
    _, info2 = gctx.refine_gicp(tgt, src, gt, source_leaf=2 * leaf)
    assert info2["samples"] == len(_sample(gctx, src, 2 * leaf)) < len(S)


# ---- 4. one step and the whole loop against the restatement --------------------------------------------------------------------
def _one_step_cases():
    """The cases of tests/test_gpu_icp.py's test_one_step_equals_the_restatement."""
    z = _g("g9_room.npz")
    gt = z["groundtruth"]
    D = R.Target(z["target"]).diag
    cases = []
    for k, rot in enumerate((0.02, 0.05, 0.1, 0.15, 0.2)):
        cases.append((1.0, np.eye(4), R.perturb(gt, rot, 0.0, seed=20 + k), dict(max_dist=0.3 * D, min_dist=0.3 * D)))
    for k, tr in enumerate((0.01, 0.05, 0.1)):
        cases.append((1.0, np.eye(4), R.perturb(gt, 0.0, tr * D, seed=30 + k), dict(max_dist=0.2 * D, min_dist=0.2 * D)))
    for k in range(4):
        cases.append((1.0, np.eye(4), R.perturb(gt, 0.01 * (k + 1), 0.01 * (k + 1), seed=40 + k), {}))
    cases.append((1.0, np.eye(4), gt, {}))
    for k, (offset, rot) in enumerate(((100.0, 0.0), (500.0, 0.0), (100.0, 0.4))):
        F = R.frame(offset * D, rot)
        cases.append((1.0, F, R.perturb(gt, 0.1, 0.02, seed=50 + k), dict(max_dist=0.2 * D, min_dist=0.2 * D)))
        cases.append((1.0, F, R.perturb(gt, 0.02, 0.02, seed=60 + k), {}))
    for scale in (1000.0, 0.001):
        cases.append((scale, np.eye(4), R.perturb(gt, 0.1, 0.02, seed=70), dict(max_dist=0.2 * D * scale, min_dist=0.2 * D * scale)))
    return z, cases


_P2P_STARTS = (0, 8, 13, 19)                                           # point-to-point: a rotation, a default stage, a far frame, other units


@pytest.mark.parametrize("k,eps", [(k, 1e-3) for k in range(21)] + [(k, 1.0) for k in _P2P_STARTS])
def test_one_step_equals_the_restatement(gctx, k, eps):
    """max_iterations = 1 from 21 starts: the fp32 T_1 equals the restatement's one step to 2e-7 max(1, |T|) per entry, the
    tolerance of the point-to-plane test: the same solver on the same scenes, and the metric's 1 / epsilon conditioning enters x
    only through H and g, which agree to 1e-12.  (The restatement run against itself with its sums permuted moves T_1 by less
    than 7e-15: DESIGN.md section 16.)"""
    z, cases = _one_step_cases()
    assert len(cases) == 21
    scale, F, T0, prm = cases[k]
    tgt, src = R.move(z["target"], F, scale), R.move(z["source"], F, scale)
    target = R.Target(tgt)
    Ts = R.conjugate(T0, F, scale)
    T1, info = gctx.refine_gicp(tgt, src, Ts, max_iterations=1, epsilon=eps, **prm)
    assert info["failure"] == 0 and info["iterations"] == 1, (scale, prm, info)
    c = R.resolve(target.diag, amax=target.amax, **prm)
    S = _sample(gctx, src, c["leaf"])
    assert len(S) == info["samples"]
    T = np.asarray(Ts, np.float32).astype(np.float64)
    c0 = R.apply(T, R.sample_mean(S))
    _, m, _ = G.linearize(target, S, T, c["dists"][0], eps, center=c0)
    assert int(m[29]) == info["correspondences"]
    assert info["rmse"] == pytest.approx(np.sqrt(m[28] / m[29]), rel=1e-9) and info["cost"] == pytest.approx(m[27] / m[29], rel=1e-9)
    x, T1_ref = R.step(m, T, c0)
    assert x is not None
    tol = 2e-7 * max(1.0, float(np.abs(T1_ref).max()))
    assert np.all(np.abs(T1.astype(np.float64) - T1_ref) <= tol), (scale, prm, np.abs(T1 - T1_ref).max(), tol)
    if eps != 1.0 and k in (2, 3, 4):
        assert np.linalg.norm(x[:3]) > 0.05                              # a step that rotates far from Rodrigues' small-angle form


@pytest.mark.timeout(900)
def test_golden_scenes_agree_with_the_restatement(gctx):
    """The whole loop at the default epsilon, with the point-to-plane test's tolerances.  (The restatement run against itself with
    its sums permuted ends within 8e-16 of itself on g9, far inside 1e-5: DESIGN.md section 16.)"""
    eps = 1e-3
    for name in ("g8_polyhedron.npz", "g9_room.npz"):
        z = _g(name)
        tgt, src, gt = z["target"], z["source"], z["groundtruth"]
        T0 = z["recorded"] if "recorded" in z.files else R.perturb(gt, 0.05, 0.05, seed=1)
        T, info = gctx.refine_gicp(tgt, src, T0, epsilon=eps)
        assert info["converged"] and _fro(T, gt) <= 1e-3, (name, _fro(T, gt), info)
        st = gctx.stats()
        assert st["gicp_iterations"] == info["iterations"] and st["gicp_loop_s"] > 0 and st["gicp_grid_s"] > 0 and st["gicp_sample_s"] > 0
        assert st["gicp_stages"] == 5
        target = R.Target(tgt)
        S = _sample(gctx, src, 0.005 * target.diag)
        assert len(S) == info["samples"]
        T_ref, info_ref = G.refine(target, src, T0, S=S, epsilon=eps)
        assert _fro(T, T_ref) <= 1e-5, (name, _fro(T, T_ref))
        assert info_ref["converged"]
        same = ("iterations", "stages", "converged", "failure", "correspondences", "samples")
        assert {k: info[k] for k in same} == {k: info_ref[k] for k in same}
        assert info["cost"] == pytest.approx(info_ref["cost"], rel=1e-6) and info["rmse"] == pytest.approx(info_ref["rmse"], rel=1e-6)


# ---- 5. accuracy ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def room300k():
    return make_pair(300_000, seed=2)


def test_ground_truth_is_a_fixed_point(gctx, room300k):
    tg, sr, Tgt = room300k
    T, info = gctx.refine_gicp(tg, sr, Tgt)
    assert info["converged"] and _fro(T, Tgt) <= 1e-3, (_fro(T, Tgt), info)
    assert info["rmse"] < 0.02 and info["fitness"] > 0.5


def test_basin(gctx, room300k):
    tg, sr, Tgt = room300k
    T, info = gctx.refine_gicp(tg, sr, R.perturb(Tgt, 0.05, 0.05, seed=7))
    assert _fro(T, Tgt) <= 1e-3, (_fro(T, Tgt), info)


# ---- 6. down-weighting --------------------------------------------------------------------------------------------------------------
def test_clutter_in_front_of_a_wall_counts_less(gctx, capsys):
    rng = np.random.default_rng(8)
    plane = np.zeros((3000, 6), np.float32)
    plane[:, :2] = rng.uniform(0, 1, size=(3000, 2))
    plane[:, 5] = 1
    slab = np.zeros((300, 6), np.float32)
    slab[:, :2] = rng.uniform(0.3, 0.7, size=(300, 2))
    slab[:, 2] = 0.02
    slab[:, 3] = 1
    tgt = np.ascontiguousarray(np.concatenate([plane, slab]))
    src = np.zeros((3000, 6), np.float32)
    src[:, :2] = rng.uniform(0, 1, size=(3000, 2))
    src[:, 5] = 1
    T = np.eye(4)
    T[:3, 3] = (0.003, -0.002, 0.012)                                    # above the wall, below the clutter
    target = R.Target(tgt)
    c = (0.5, 0.5, 0.0)
    corr, mom = _check_seam(gctx, target, tgt, src, T, 0.05, 1e-3, center=c)           # J^T M e among the 30 moments
    on_slab = corr >= len(plane)
    assert 50 < on_slab.sum() < 1500
    sub = np.ascontiguousarray(src[on_slab])
    corr_s, mom_s = _check_seam(gctx, target, tgt, sub, T, 0.05, 1e-3, center=c)
    assert np.array_equal(corr_s, corr[on_slab])
    _, ref, _ = G.linearize(target, src, T, 0.05, 1e-3, center=c)
    _, ref_s, _ = G.linearize(target, sub, T, 0.05, 1e-3, center=c)
    share_cost, share_ee = mom_s[27] / mom[27], mom_s[28] / mom[28]
    want_cost, want_ee = ref_s[27] / ref[27], ref_s[28] / ref[28]
    with capsys.disabled():
        print(f"\nclutter: {int(on_slab.sum())} of {int((corr >= 0).sum())} correspondences, share of e.e {share_ee:.4f}, of e^T M e "
              f"{share_cost:.6f}: down-weighted by {share_ee / share_cost:.1f} (restated {want_ee / want_cost:.1f})")
    assert share_cost == pytest.approx(want_cost, rel=1e-9) and share_ee == pytest.approx(want_ee, rel=1e-9)
    assert share_cost < share_ee


# ---- 7. symmetry -------------------------------------------------------------------------------------------------------------------
def test_cost_is_symmetric_on_mutual_nearest_pairs(gctx):
    """gicp_linearize(A, B, T) and gicp_linearize(B, A, T^-1) on g9 at ground truth: sum e^T M e over the pairs that are each
    other's nearest point agrees to 1e-6 relative (the restatement's own gap is 4.6e-11: the fp32 probes of the two directions
    round differently, the fp64 terms do not care)."""
    z = _g("g9_room.npz")
    A, B, T = np.ascontiguousarray(z["target"]), np.ascontiguousarray(z["source"]), z["groundtruth"]
    Ti = np.linalg.inv(T)
    d = 0.0025 * R.Target(A).diag
    cab, _ = gctx.gicp_linearize(A, B, T, d)
    cba, _ = gctx.gicp_linearize(B, A, Ti, d)
    i = np.flatnonzero(cab >= 0)
    j = cab[i]
    mutual = cba[j] == i
    i, j = i[mutual], j[mutual]
    assert len(i) > 10_000
    c1, m1 = gctx.gicp_linearize(A, np.ascontiguousarray(B[i]), T, d)
    c2, m2 = gctx.gicp_linearize(B, np.ascontiguousarray(A[j]), Ti, d)
    assert np.array_equal(c1, j) and np.array_equal(c2, i)
    assert m1[29] == m2[29] == len(i)
    assert abs(m1[27] - m2[27]) <= 1e-6 * max(m1[27], m2[27]), (m1[27], m2[27])


# ---- 8. determinism ---------------------------------------------------------------------------------------------------------------
def test_determinism_host_dev_contexts_and_load(gctx):
    tg, sr, Tgt = make_pair(200_000, seed=4)
    T0 = R.perturb(Tgt, 0.05, 0.05, seed=3).astype(np.float32)
    T1, i1 = gctx.refine_gicp(tg, sr, T0)
    assert i1["failure"] == 0 and i1["iterations"] >= 2
    Tb, ib = gctx.refine_gicp(tg, sr, T0)
    assert np.array_equal(_bits(T1), _bits(Tb)) and i1 == ib
    ct, cs = gctx.upload(tg), gctx.upload(sr)
    T2, i2 = gctx.refine_gicp_dev(ct, cs, T0)
    ct.free(); cs.free()
    assert np.array_equal(_bits(T1), _bits(T2)) and i1 == i2
    other = plade_amd.Context(0, **ORIENTED)
    try:
        T3, i3 = other.refine_gicp(tg, sr, T0)
        assert np.array_equal(_bits(T1), _bits(T3)) and i1 == i3
        tg2, sr2, _ = make_pair(300_000, seed=5)
        errors = []

        def busy():
            try:
                for _ in range(3):
                    other.registration(tg2, sr2)
            except Exception as e:   # noqa: BLE001
                errors.append(e)
        th = threading.Thread(target=busy)
        th.start()
        outs = [gctx.refine_gicp(tg, sr, T0) for _ in range(3)]
        th.join()
        assert not errors
        for T4, i4 in outs:
            assert np.array_equal(_bits(T1), _bits(T4)) and i1 == i4
    finally:
        other.close()


# ---- 9. failures and errors --------------------------------------------------------------------------------------------------------
def test_failures(gctx):
    tg, sr, Tgt = make_pair(100_000, seed=0)
    T0 = Tgt.astype(np.float32)
    far = sr.copy()
    far[:, :3] += 1000.0
    with pytest.raises(plade_amd.PladeError) as e:
        gctx.refine_gicp(tg, far, T0)
    assert e.value.code == plade_amd.PLADE_EFAIL and e.value.info["reason"] == "too few correspondences"
    assert np.array_equal(e.value.T, T0) and "too few" in str(e.value)
    # points exactly on the x axis, normals (0, 0, 1): the rotation about the line is an exactly zero column
    line = np.zeros((20_000, 6), np.float32)
    line[:, 0] = np.random.default_rng(0).uniform(-2, 2, size=20_000)
    line[:, 5] = 1
    Ti = np.eye(4, dtype=np.float32)
    with pytest.raises(plade_amd.PladeError) as e:
        gctx.refine_gicp(line, line, Ti)
    assert e.value.code == plade_amd.PLADE_EFAIL and e.value.info["reason"] == "degenerate"
    assert np.array_equal(e.value.T, Ti)
    # a single plane is NOT degenerate here: the isotropic part of M holds the in-plane motions
    rng = np.random.default_rng(0)
    plane = np.zeros((60_000, 6), np.float32)
    plane[:, :2] = rng.uniform(0, 2, size=(60_000, 2))
    plane[:, 5] = 1
    T, info = gctx.refine_gicp(plane, plane, Ti)
    assert info["failure"] == 0 and info["reason"] is None
    # across the plane e is exactly 0 and the weight is 1 / (2 epsilon): nothing moves there.  Inside the plane only the sample's
    # offsets to its nearest points pull, at relative weight epsilon (inherent to GICP): no bound is claimed for that drift
    assert np.abs(T[2] - np.array([0, 0, 1, 0])).max() <= 1e-6 and np.abs(T[:3, 2] - np.array([0, 0, 1])).max() <= 1e-6, T
    T, _ = gctx.refine_gicp(tg, sr, T0)                                  # the context is still usable
    assert _fro(T, Tgt) <= 1e-3


def test_invalid_arguments_leave_the_context_usable(gctx):
    z = _g("g9_room.npz")
    tg, sr, gt = z["target"], z["source"], z["groundtruth"]
    before, info0 = gctx.refine_gicp(tg, sr, gt)
    L, h = gctx.L, gctx.h
    T = np.eye(4, dtype=np.float32)
    out = np.zeros((4, 4), np.float32)
    p = lambda a: a.ctypes.data_as(plade_amd.C.c_void_p)   # noqa: E731
    assert L.plade_refine_gicp(h, None, len(tg), p(sr), len(sr), p(T), None, p(out), None) == plade_amd.PLADE_EINVAL
    assert L.plade_refine_gicp(h, p(tg), 0, p(sr), len(sr), p(T), None, p(out), None) == plade_amd.PLADE_EINVAL
    assert L.plade_refine_gicp(h, p(tg), len(tg), p(sr), len(sr), p(T), None, None, None) == plade_amd.PLADE_EINVAL
    bad = T.copy()
    bad[0, 3] = np.nan
    for kw in ({}, {"epsilon": -1.0}, {"epsilon": 1.5}, {"epsilon": np.nan}, {"min_dist": 0.5, "max_dist": 0.1}, {"max_dist": -1.0},
               {"max_iterations": -1}, {"source_leaf": np.inf}, {"max_dist": 1.0, "min_dist": 1e-6}):
        with pytest.raises(plade_amd.PladeError) as e:
            gctx.refine_gicp(tg, sr, bad if not kw else gt, **kw)
        assert e.value.code == plade_amd.PLADE_EINVAL, kw
        assert "refine_gicp: " in str(e.value) and ("epsilon" in str(e.value)) == ("epsilon" in kw), (kw, str(e.value))
    nan_pt = sr.copy()
    nan_pt[7, 1] = np.nan
    with pytest.raises(plade_amd.PladeError) as e:
        gctx.refine_gicp(tg, nan_pt, gt)
    assert e.value.code == plade_amd.PLADE_EINVAL
    with pytest.raises(plade_amd.PladeError) as e:                        # what the merge refuses for the sample, under this name
        gctx.refine_gicp(tg, sr, gt, source_leaf=1e-7)
    assert e.value.code == plade_amd.PLADE_ELIMIT and "refine_gicp: the sample: " in str(e.value) and "merge_clouds" not in str(e.value)
    for kw in ({"dist": 0.0}, {"epsilon": 2.0}, {"epsilon": -0.5}):
        with pytest.raises(plade_amd.PladeError) as e:
            gctx.gicp_linearize(tg, sr, np.eye(4), kw.get("dist", 0.1), epsilon=kw.get("epsilon", 0.0))
        assert e.value.code == plade_amd.PLADE_EINVAL
    after, info1 = gctx.refine_gicp(tg, sr, gt)                          # the same context, the earlier bits
    assert np.array_equal(_bits(before), _bits(after)) and info0 == info1


# ---- 10. the CLI switch ------------------------------------------------------------------------------------------------------------
def _results(path):
    rows = []
    for line in open(path).read().split("\n"):
        try:
            vals = [float(x) for x in line.split()]
        except ValueError:
            continue
        if len(vals) == 4:
            rows.append(vals)
    return [np.array(rows[i:i + 4], np.float64) for i in range(0, len(rows), 4)]


def _line(info):
    return "GICP refinement: %d iterations, %s, rmse %.6g, cost %.6g, fitness %.4f" % (
        info["iterations"], "converged" if info["converged"] else "not converged", info["rmse"], info["cost"], info["fitness"])


@pytest.mark.timeout(900)
def test_cli_switch(tmp_path, gctx):
    tg, sr, Tgt = make_pair(200_000, seed=1)
    pt, ps = str(tmp_path / "t.ply"), str(tmp_path / "s.ply")
    write_ply(pt, tg)
    write_ply(ps, sr)
    tg, sr = plade_amd.read_ply(pt), plade_amd.read_ply(ps)                # the rows the CLI reads
    base = {k: v for k, v in os.environ.items() if k not in ("PLADE_REFINE_ICP", "PLADE_REFINE_GICP")}
    base.update(PLADE_ORIENT_NORMALS="1", PLADE_GPUS="1")
    runs = {}
    for tag, extra in (("unset", {}), ("zero", {"PLADE_REFINE_GICP": "0"}), ("abc", {"PLADE_REFINE_GICP": "abc"}),
                       ("seven", {"PLADE_REFINE_GICP": "1,7"}), ("on", {"PLADE_REFINE_GICP": "1"}), ("p2p", {"PLADE_REFINE_GICP": "1,1"}),
                       ("both", {"PLADE_REFINE_GICP": "1", "PLADE_REFINE_ICP": "1"})):
        res = str(tmp_path / f"r_{tag}.txt")
        r = subprocess.run([CLI, pt, ps, res], capture_output=True, text=True, timeout=600, env=dict(base, **extra))
        assert r.returncode == 0, r.stdout + r.stderr
        runs[tag] = (r.stdout, r.stderr, open(res).read(), res)

    def strip(out, res):   # the timings and the result file's name differ from run to run
        return "\n".join(x for x in out.replace(res, "RESULT").split("\n") if not x.startswith("done. time:"))
    for tag in ("zero", "abc", "seven"):
        assert runs[tag][2] == runs["unset"][2], tag
        assert strip(runs[tag][0], runs[tag][3]) == strip(runs["unset"][0], runs["unset"][3]), tag
        assert "GICP refinement" not in runs[tag][0]
        assert runs[tag][1].count("warning: PLADE_REFINE_GICP=") == (0 if tag == "zero" else 1), runs[tag][1]
    assert "GICP" not in runs["unset"][0] + runs["unset"][1]
    ok, T0 = gctx.registration(tg, sr)
    assert ok
    for tag, eps in (("on", 1e-3), ("p2p", 1.0), ("both", 1e-3)):
        T1, info = gctx.refine_gicp(tg, sr, T0, epsilon=eps)
        out = runs[tag][0]
        assert out.count("GICP refinement: ") == 1 and "ICP refinement: " not in out.replace("GICP refinement: ", "")
        assert _line(info) in out, (tag, _line(info), [x for x in out.split("\n") if "GICP" in x])
        M = _results(runs[tag][3])[0]
        assert np.abs(M - T1.astype(np.float64)).max() <= 1e-5, (tag, M, T1)           # the file prints six digits
        assert tag == "p2p" or _fro(M, Tgt) <= 1e-3, (tag, _fro(M, Tgt))                # (no accuracy is claimed for point-to-point)
        assert runs[tag][1].count("PLADE_REFINE_ICP and PLADE_REFINE_GICP are both set") == (1 if tag == "both" else 0)
    assert runs["on"][2] != runs["unset"][2] and runs["on"][2] == runs["both"][2] and runs["on"][2] != runs["p2p"][2]
