"""Point-to-plane ICP refinement on the GPU (plade_refine_icp, plade_icp_linearize) against the numpy restatement of its
semantics (tests/icp_restate.py): exact correspondences, moments, accuracy, determinism, failure paths and the CLI switch."""
import os
import subprocess
import threading

import numpy as np
import pytest

import plade_amd
from plade_amd.plyio import write_ply
from plade_amd.synth import make_pair
from conftest import ORIENTED
import icp_restate as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "plade_amd", "PLADE")
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def ictx():
    c = plade_amd.Context(0, **ORIENTED)
    yield c
    c.close()


def _g(name):
    return np.load(os.path.join(GOLDEN, name))


def _same_moments(m_gpu, m_ref, absm):
    assert m_gpu[28] == m_ref[28]
    assert np.all(np.abs(m_gpu - m_ref) <= 1e-12 * absm + 1e-300), np.abs(m_gpu - m_ref) / np.maximum(absm, 1e-300)


def _check_seam(ctx, target, tgt, S, T, d, center=None):
    corr, mom = ctx.icp_linearize(tgt, S, T, d, center=center)
    c_ref, m_ref, absm = target.linearize(S, T, d, center=center)
    assert np.array_equal(corr, c_ref), (int((corr != c_ref).sum()), d)
    _same_moments(mom, m_ref, absm)
    return corr, mom


def _boundary_dist(target, S, T):
    """A stage distance d with (float)d * (float)d equal to some probe's nearest flann_d2: that probe sits on the boundary."""
    P = R.transform_f32(T, S[:64])
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


@pytest.mark.parametrize("name", ["g8_polyhedron.npz", "g9_room.npz"])
def test_seam_is_exact_on_the_golden_scenes(ictx, name):
    z = _g(name)
    tgt, src = z["target"], z["source"]
    target = R.Target(tgt)
    D = target.diag
    S = np.ascontiguousarray(src[:, :3])
    gt = z["groundtruth"]
    for T in (gt, R.perturb(gt, 0.03, 0.03, seed=5)):
        for d in (0.025 * D, 0.0025 * D):
            corr, mom = _check_seam(ictx, target, tgt, S, T, d)
            assert (corr >= 0).sum() > 1000
            corr2, mom2 = ictx.icp_linearize(tgt, S, T, d)            # repeat: bitwise
            assert np.array_equal(corr, corr2) and np.array_equal(mom.view(np.uint64), mom2.view(np.uint64))
    d = _boundary_dist(target, S, gt)
    assert d is not None
    corr, _ = _check_seam(ictx, target, tgt, S, gt, d)


@pytest.mark.parametrize("offset", [100.0, 500.0])
@pytest.mark.parametrize("name", ["g8_polyhedron.npz", "g9_room.npz"])
def test_seam_is_exact_far_from_the_origin(ictx, name, offset):
    """The golden-scene seam check with both clouds moved offset x D away, about the origin and about the refinement's centre
    T s-bar: the grid's cell carries 4e-6 max|coordinate| of slack for the fp32 cell assignment, which only matters at large
    coordinates."""
    z = _g(name)
    F = R.frame(offset * R.Target(z["target"]).diag)
    tgt, src = R.move(z["target"], F), R.move(z["source"], F)
    target = R.Target(tgt)
    D = target.diag
    S = np.ascontiguousarray(src[:, :3])
    gt = R.conjugate(z["groundtruth"], F)
    for T in (gt, R.conjugate(R.perturb(z["groundtruth"], 0.03, 0.03, seed=5), F)):
        for d in (0.025 * D, 0.0025 * D):
            for c in (None, R.apply(T, R.sample_mean(S))):
                corr, mom = _check_seam(ictx, target, tgt, S, T, d, center=c)
                assert (corr >= 0).sum() > 1000
    d = _boundary_dist(target, S, gt)
    assert d is not None
    _check_seam(ictx, target, tgt, S, gt, d, center=R.apply(gt, R.sample_mean(S)))


def test_seam_takes_the_centre_it_is_given(ictx):
    z = _g("g9_room.npz")
    tgt = z["target"]
    target = R.Target(tgt)
    S = np.ascontiguousarray(z["source"][:, :3])
    T = z["groundtruth"]
    d = 0.01 * target.diag
    for c in ((0.0, 0.0, 0.0), (3.0, -2.0, 0.5), R.apply(T, R.sample_mean(S))):
        corr, mom = ictx.icp_linearize(tgt, S, T, d, center=c)
        c_ref, m_ref, absm = target.linearize(S, T, d, center=np.array(c))
        assert np.array_equal(corr, c_ref)
        _same_moments(mom, m_ref, absm)
    corr0, mom0 = ictx.icp_linearize(tgt, S, T, d)                      # no centre: the origin
    corr1, mom1 = ictx.icp_linearize(tgt, S, T, d, center=(0.0, 0.0, 0.0))
    assert np.array_equal(corr0, corr1) and np.array_equal(mom0.view(np.uint64), mom1.view(np.uint64))


def test_seam_ties_nan_normals_and_cell_size(ictx):
    z = _g("g9_room.npz")
    tgt = z["target"].copy()
    rng = np.random.default_rng(2)
    tgt[rng.choice(len(tgt), len(tgt) // 4, replace=False), 3:] = np.nan     # never matched
    dup = tgt[rng.choice(len(tgt), 5000, replace=False)].copy()
    dup[:, 3:] = -dup[:, 3:]
    tgt = np.ascontiguousarray(np.concatenate([dup, tgt]))                 # exact duplicates: the smaller index wins
    target = R.Target(tgt)
    S = np.ascontiguousarray(z["source"][:, :3])
    T = z["groundtruth"]
    d = 0.01 * target.diag
    corr, mom = _check_seam(ictx, target, tgt, S, T, d)
    assert np.isfinite(tgt[corr[corr >= 0], 3:]).all()
    assert (corr[corr >= 0] < len(dup)).any()
    # a different grid -- one far point moves the origin and makes the cell budget enlarge the cell --, the same answer
    far = tgt[:1].copy()
    far[0, :3] += 1000.0 * target.diag
    tgt2 = np.ascontiguousarray(np.concatenate([tgt, far]))
    corr2, mom2 = ictx.icp_linearize(tgt2, S, T, d)
    assert np.array_equal(corr, corr2) and np.array_equal(mom.view(np.uint64), mom2.view(np.uint64))


def test_seam_on_a_1m_target_sample(ictx):
    tg, sr, Tgt = make_pair(1_000_000, seed=3)
    target = R.Target(tg)
    rng = np.random.default_rng(0)
    S = np.ascontiguousarray(sr[rng.choice(len(sr), 3000, replace=False), :3])
    for T, d in ((Tgt, 0.025 * target.diag), (R.perturb(Tgt, 0.02, 0.02, seed=1), 0.005 * target.diag)):
        _check_seam(ictx, target, tg, S, T, d)


def _fro(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)))


@pytest.mark.timeout(900)
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_default_arithmetic_registration_is_refined_to_1e_3(ictx, seed):
    tg, sr, Tgt = make_pair(1_000_000, seed=seed)
    assert ictx.params.closest_point_mode == 1
    ok, T0 = ictx.registration(tg, sr)
    assert ok
    T, info = ictx.refine_icp(tg, sr, T0)
    assert info["failure"] == 0 and info["iterations"] >= 1
    assert _fro(T, Tgt) <= 1e-3, (_fro(T0, Tgt), _fro(T, Tgt), info)
    assert _fro(T, Tgt) < _fro(T0, Tgt)


@pytest.mark.timeout(900)
def test_golden_scenes_agree_with_the_restatement(ictx):
    for name in ("g8_polyhedron.npz", "g9_room.npz"):
        z = _g(name)
        tgt, src, gt = z["target"], z["source"], z["groundtruth"]
        T0 = z["recorded"] if "recorded" in z.files else R.perturb(gt, 0.05, 0.05, seed=1)
        T, info = ictx.refine_icp(tgt, src, T0)
        assert info["converged"] and _fro(T, gt) <= 1e-3
        target = R.Target(tgt)
        leaf = 0.005 * target.diag
        S = ictx.voxel_downsample(np.ascontiguousarray(src[:, :3]), np.float32(leaf))
        assert len(S) == info["samples"]
        T_ref, info_ref = R.refine(target, src, T0, S=S)
        assert _fro(T, T_ref) <= 1e-5
        assert info_ref["converged"]


@pytest.mark.parametrize("rot,trans", [(0.05, 0.05), (0.1, 0.1), (0.15, 0.15)])
def test_basin(ictx, rot, trans):
    tg, sr, Tgt = make_pair(300_000, seed=1)
    T, info = ictx.refine_icp(tg, sr, R.perturb(Tgt, rot, trans, seed=7))
    assert _fro(T, Tgt) <= 1e-3, info


def test_ground_truth_is_a_fixed_point(ictx):
    tg, sr, Tgt = make_pair(300_000, seed=2)
    T, info = ictx.refine_icp(tg, sr, Tgt)
    assert info["converged"] and _fro(T, Tgt) <= 1e-3
    assert info["rmse"] < 0.02 and info["fitness"] > 0.5
    st = ictx.stats()
    assert st["icp_iterations"] == info["iterations"] and st["icp_loop_s"] > 0 and st["icp_grid_s"] > 0


def test_determinism_host_dev_contexts_and_load(ictx):
    tg, sr, Tgt = make_pair(200_000, seed=4)
    T0 = R.perturb(Tgt, 0.05, 0.05, seed=3).astype(np.float32)
    T1, i1 = ictx.refine_icp(tg, sr, T0)
    ct, cs = ictx.upload(tg), ictx.upload(sr)
    T2, i2 = ictx.refine_icp_dev(ct, cs, T0)
    ct.free(); cs.free()
    assert np.array_equal(T1.view(np.uint32), T2.view(np.uint32)) and i1 == i2
    other = plade_amd.Context(0, **ORIENTED)
    try:
        T3, i3 = other.refine_icp(tg, sr, T0)
        assert np.array_equal(T1.view(np.uint32), T3.view(np.uint32)) and i1 == i3
        # a registration in flight on the other context
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
        outs = [ictx.refine_icp(tg, sr, T0) for _ in range(3)]
        th.join()
        assert not errors
        for T4, i4 in outs:
            assert np.array_equal(T1.view(np.uint32), T4.view(np.uint32)) and i1 == i4
    finally:
        other.close()


def test_failures(ictx):
    tg, sr, Tgt = make_pair(100_000, seed=0)
    T0 = Tgt.astype(np.float32)
    far = sr.copy()
    far[:, :3] += 1000.0
    with pytest.raises(plade_amd.PladeError) as e:
        ictx.refine_icp(tg, far, T0)
    assert e.value.code == plade_amd.PLADE_EFAIL and e.value.info["reason"] == "too few correspondences"
    assert np.array_equal(e.value.T, T0)
    rng = np.random.default_rng(0)
    plane = np.zeros((50_000, 6), np.float32)
    plane[:, :2] = rng.uniform(-2, 2, size=(50_000, 2))
    plane[:, 5] = 1
    with pytest.raises(plade_amd.PladeError) as e:
        ictx.refine_icp(plane, plane, np.eye(4, dtype=np.float32))
    assert e.value.code == plade_amd.PLADE_EFAIL and e.value.info["reason"] == "degenerate"
    T, _ = ictx.refine_icp(tg, sr, T0)                                       # the context is still usable
    assert _fro(T, Tgt) <= 1e-3


def test_invalid_arguments_leave_the_context_usable(ictx):
    tg, sr, Tgt = make_pair(50_000, seed=1)
    L, h = ictx.L, ictx.h
    T = np.eye(4, dtype=np.float32)
    out = np.zeros((4, 4), np.float32)
    p = lambda a: a.ctypes.data_as(plade_amd.C.c_void_p)   # noqa: E731
    assert L.plade_refine_icp(h, None, len(tg), p(sr), len(sr), p(T), None, p(out), None) == plade_amd.PLADE_EINVAL
    assert L.plade_refine_icp(h, p(tg), 0, p(sr), len(sr), p(T), None, p(out), None) == plade_amd.PLADE_EINVAL
    bad = T.copy()
    bad[0, 3] = np.nan
    for kw in ({}, {"min_dist": 0.5, "max_dist": 0.1}, {"max_dist": -1.0}, {"max_iterations": -1}, {"source_leaf": np.inf},
               {"max_dist": 1.0, "min_dist": 1e-6}):
        with pytest.raises(plade_amd.PladeError) as e:
            ictx.refine_icp(tg, sr, bad if not kw else T, **kw)
        assert e.value.code == plade_amd.PLADE_EINVAL
    with pytest.raises(plade_amd.PladeError) as e:
        ictx.icp_linearize(tg, sr[:, :3], np.eye(4), 0.0)
    assert e.value.code == plade_amd.PLADE_EINVAL
    T1, info = ictx.refine_icp(tg, sr, Tgt)
    assert info["failure"] == 0 and _fro(T1, Tgt) <= 1e-3


def _results(path):
    """The 4 x 4 matrices of a result file, in order."""
    rows = []
    for line in open(path).read().split("\n"):
        try:
            vals = [float(x) for x in line.split()]
        except ValueError:
            continue
        if len(vals) == 4:
            rows.append(vals)
    return [np.array(rows[i:i + 4], np.float64) for i in range(0, len(rows), 4)]


@pytest.mark.timeout(900)
def test_cli_switch(tmp_path):
    pairs, gts = [], []
    for seed in range(3):
        tg, sr, T = make_pair(200_000, seed=seed)
        pt, ps = str(tmp_path / f"t{seed}.ply"), str(tmp_path / f"s{seed}.ply")
        write_ply(pt, tg)
        write_ply(ps, sr)
        pairs += [pt, ps]
        gts.append(T)
    lst = tmp_path / "pairs.txt"
    lst.write_text("\n".join(pairs) + "\n")
    base = dict(os.environ, PLADE_ORIENT_NORMALS="1", PLADE_GPUS="1")
    base.pop("PLADE_REFINE_ICP", None)
    runs = {}
    for tag, extra in (("unset", {}), ("zero", {"PLADE_REFINE_ICP": "0"}), ("on", {"PLADE_REFINE_ICP": "1"})):
        res = str(tmp_path / f"r_{tag}.txt")
        r = subprocess.run([CLI, str(lst), res], capture_output=True, text=True, timeout=600, env=dict(base, **extra))
        assert r.returncode == 0, r.stdout + r.stderr
        runs[tag] = (r.stdout, open(res).read(), res)
    assert runs["zero"][1] == runs["unset"][1]
    def strip(out, res):   # the timings and the result file's name differ from run to run
        return "\n".join(x for x in out.replace(res, "RESULT").split("\n") if not x.startswith("done. time:"))
    assert strip(runs["zero"][0], runs["zero"][2]) == strip(runs["unset"][0], runs["unset"][2])
    assert "ICP refinement" not in runs["unset"][0] and runs["on"][0].count("ICP refinement: ") == 3
    mats = _results(runs["on"][2])
    assert len(mats) == 3
    for M, T in zip(mats, gts):
        assert _fro(M, T) <= 1e-3
    # the single-pair path
    res = str(tmp_path / "single.txt")
    r = subprocess.run([CLI, pairs[0], pairs[1], res], capture_output=True, text=True, timeout=600,
                       env=dict(base, PLADE_REFINE_ICP="1"))
    assert r.returncode == 0 and r.stdout.count("ICP refinement: ") == 1, r.stdout + r.stderr
    assert _fro(_results(res)[0], gts[0]) <= 1e-3


# ---- changes of frame and units ------------------------------------------------------------------------------------------------
def _near(T, T_ref):
    """T (fp32, the library's output) equals the fp64 T_ref to 1e-5 plus two fp32 ulps of each entry: far from the origin the
    output's own rounding (an ulp of a translation of 500 D) is larger than 1e-5."""
    T, T_ref = np.asarray(T, np.float64), np.asarray(T_ref, np.float64)
    slack = 1e-5 + 2 * np.spacing(np.abs(T_ref).astype(np.float32)).astype(np.float64)
    return bool(np.all(np.abs(T - T_ref) <= slack)), float(np.max(np.abs(T - T_ref) - slack))


def _scene(name):
    """(target, source, ground truth, start) of g9 (from a 0.1 perturbation) or a 300k make_pair room."""
    if name == "g9":
        z = _g("g9_room.npz")
        return z["target"], z["source"], z["groundtruth"], R.perturb(z["groundtruth"], 0.05, 0.05, seed=1)
    tg, sr, Tgt = make_pair(300_000, seed=1)
    return tg, sr, Tgt, R.perturb(Tgt, 0.05, 0.05, seed=7)


FRAMES = [(0.0, 0.0), (10.0, 0.0), (100.0, 0.4), (500.0, 0.0)]     # (distance from the origin in D, rotation of the frame)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("name", ["g9", "room300k"])
def test_refinement_is_equivariant_under_changes_of_frame(ictx, name):
    """refine_icp(F tgt, F src, F T0 F^-1) for rigid F up to 500 D from the origin: converged before the cap, F^-1 T F within
    1e-3 of the generator's T and equal to the restatement in the same frame.  (About the origin, the linearisation hit the
    cap from ~16 D and failed from ~160 D.)  The 300k room is compared with the restatement in its farthest frame only."""
    tgt0, src0, gt, T0 = _scene(name)
    D = R.Target(tgt0).diag
    for offset, rot in FRAMES:
        F = R.frame(offset * D, rot)
        tgt, src = R.move(tgt0, F), R.move(src0, F)
        target = R.Target(tgt)
        assert np.spacing(np.float32(target.amax)) <= 0.0025 * target.diag / 10     # fp32 still resolves min_dist
        Ts = R.conjugate(T0, F)
        T, info = ictx.refine_icp(tgt, src, Ts)
        assert info["converged"] and info["failure"] == 0 and info["iterations"] < 60, (offset, rot, info)
        assert _fro(R.back(T, F), gt) <= 1e-3, (offset, rot, _fro(R.back(T, F), gt))
        if name == "g9" or offset == FRAMES[-1][0]:
            S = ictx.voxel_downsample(np.ascontiguousarray(src[:, :3]), np.float32(0.005 * target.diag))
            T_ref, info_ref = R.refine(target, src, Ts, S=S)
            ok, excess = _near(T, T_ref)
            assert ok and info_ref["converged"], (offset, rot, excess, info, info_ref)


@pytest.mark.timeout(900)
def test_refinement_does_not_depend_on_the_units(ictx):
    """Coordinates x 1024 and x 2^-10 are the same problem exactly (every fp32 input and fp64 step scales by a power of two): the
    same iterations and stages, the rotation bit for bit.  x 1000 and x 0.001 round the inputs differently (the sample moves by a
    point or two), which shifts the iteration count by up to three here; they converge to the same T."""
    tgt0, src0, gt, T0 = _scene("g9")
    T_1, info0 = ictx.refine_icp(tgt0, src0, T0)
    F = np.eye(4)
    for scale in (1024.0, 2.0 ** -10):
        T, info = ictx.refine_icp(R.move(tgt0, F, scale), R.move(src0, F, scale), R.conjugate(T0, F, scale))
        same = ("iterations", "stages", "converged", "failure", "correspondences", "samples", "fitness")
        assert {k: info[k] for k in same} == {k: info0[k] for k in same}, (scale, info, info0)
        assert np.array_equal(T[:3, :3], T_1[:3, :3]) and np.array_equal(T[:3, 3], T_1[:3, 3] * np.float32(scale))
    for scale in (1000.0, 0.001):
        T, info = ictx.refine_icp(R.move(tgt0, F, scale), R.move(src0, F, scale), R.conjugate(T0, F, scale))
        assert info["converged"] and abs(info["iterations"] - info0["iterations"]) <= 4, (scale, info, info0)
        assert _fro(R.back(T, F, scale), gt) <= 1e-3
        assert _fro(R.back(T, F, scale), T_1) <= 1e-4


# ---- one step of the solve: k_icp_mean + k_icp_solve against the restatement -----------------------------------------------------
def _one_step_cases():
    z = _g("g9_room.npz")
    gt = z["groundtruth"]
    D = R.Target(z["target"]).diag
    cases = []
    for k, rot in enumerate((0.02, 0.05, 0.1, 0.15, 0.2)):             # large steps: Rodrigues far from its small-angle form
        cases.append((1.0, np.eye(4), R.perturb(gt, rot, 0.0, seed=20 + k), dict(max_dist=0.3 * D, min_dist=0.3 * D)))
    for k, tr in enumerate((0.01, 0.05, 0.1)):                        # pure translations
        cases.append((1.0, np.eye(4), R.perturb(gt, 0.0, tr * D, seed=30 + k), dict(max_dist=0.2 * D, min_dist=0.2 * D)))
    for k in range(4):                                                # the default first stage
        cases.append((1.0, np.eye(4), R.perturb(gt, 0.01 * (k + 1), 0.01 * (k + 1), seed=40 + k), {}))
    cases.append((1.0, np.eye(4), gt, {}))                            # the ground truth: a near-zero step
    for k, (offset, rot) in enumerate(((100.0, 0.0), (500.0, 0.0), (100.0, 0.4))):       # far frames
        F = R.frame(offset * D, rot)
        cases.append((1.0, F, R.perturb(gt, 0.1, 0.02, seed=50 + k), dict(max_dist=0.2 * D, min_dist=0.2 * D)))
        cases.append((1.0, F, R.perturb(gt, 0.02, 0.02, seed=60 + k), {}))
    for scale in (1000.0, 0.001):                                     # other units
        cases.append((scale, np.eye(4), R.perturb(gt, 0.1, 0.02, seed=70), dict(max_dist=0.2 * D * scale, min_dist=0.2 * D * scale)))
    return z, cases


def test_one_step_equals_the_restatement(ictx):
    """max_iterations = 1 from 21 starts: the fp32 T_1 equals the restatement's one step -- the moments of Target.linearize about
    c_0 = T_0 s-bar, cholesky_solve, rodrigues and the update -- to 2e-7 max(1, |T|) per entry.  The end-to-end checks cannot
    see a wrong solve: the fixed point depends only on the gradient."""
    z, cases = _one_step_cases()
    big = 0
    for scale, F, T0, prm in cases:
        tgt, src = R.move(z["target"], F, scale), R.move(z["source"], F, scale)
        target = R.Target(tgt)
        Ts = R.conjugate(T0, F, scale)
        T1, info = ictx.refine_icp(tgt, src, Ts, max_iterations=1, **prm)
        assert info["failure"] == 0 and info["iterations"] == 1, (scale, prm, info)
        c = R.resolve(target.diag, amax=target.amax, **prm)
        S = ictx.voxel_downsample(np.ascontiguousarray(src[:, :3]), np.float32(c["leaf"]))
        T = np.asarray(Ts, np.float32).astype(np.float64)
        c0 = R.apply(T, R.sample_mean(S))
        _, m, _ = target.linearize(S, T, c["dists"][0], center=c0)
        assert int(m[28]) == info["correspondences"]
        x, T1_ref = R.step(m, T, c0)
        assert x is not None
        tol = 2e-7 * max(1.0, float(np.abs(T1_ref).max()))
        assert np.all(np.abs(T1.astype(np.float64) - T1_ref) <= tol), (scale, prm, np.abs(T1 - T1_ref).max(), tol)
        big += np.linalg.norm(x[:3]) > 0.05
    assert big >= 3                                                   # some steps rotate by more than 0.05 rad


# ---- the schedule ----------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
@pytest.mark.parametrize("name", ["g8_polyhedron.npz", "g9_room.npz"])
def test_schedule_equals_the_restatement_at_every_cap(ictx, name):
    """max_iterations = 1 ... 12: iterations, stages, converged and the last stage distance as the restatement's run with the
    same cap (a run with cap k is the first k iterations of the uncapped one)."""
    z = _g(name)
    tgt, src, gt = z["target"], z["source"], z["groundtruth"]
    T0 = z["recorded"] if "recorded" in z.files else R.perturb(gt, 0.05, 0.05, seed=1)
    target = R.Target(tgt)
    S = ictx.voxel_downsample(np.ascontiguousarray(src[:, :3]), np.float32(0.005 * target.diag))
    trace = []
    R.refine(target, src, T0, S=S, max_iterations=12, trace=trace)
    for cap in range(1, 13):
        _, info = ictx.refine_icp(tgt, src, T0, max_iterations=cap)
        want = trace[min(cap, len(trace)) - 1]
        got = {k: info[k] for k in ("iterations", "stages", "converged", "failure")}
        assert got == {k: want[k] for k in got}, (cap, got, want)
        assert info["final_dist"] == pytest.approx(want["final_dist"], rel=1e-12)


# ---- degeneracy ------------------------------------------------------------------------------------------------------------------
def _planes(normals, n=60_000, seed=0):
    rng = np.random.default_rng(seed)
    parts = []
    for ax in normals:
        p = np.zeros((n // len(normals), 6), np.float32)
        free = [k for k in range(3) if k != ax]
        p[:, free] = rng.uniform(0, 2, size=(len(p), 2))
        p[:, 3 + ax] = 1
        parts.append(p)
    return np.ascontiguousarray(np.concatenate(parts))


@pytest.mark.parametrize("offset", [0.0, 1000.0])
def test_single_plane_and_crease_are_degenerate_in_any_frame(ictx, offset):
    """Exact normals: a plane leaves three motions free, a crease of two perpendicular planes the translation along its line
    (an exactly zero Jacobian column).  The relative pivot test sees both at the origin and 1000 D away."""
    for normals in ((2,), (0, 1)):
        cloud = _planes(normals)
        moved = R.move(cloud, R.frame(offset * R.Target(cloud).diag))
        T0 = np.eye(4, dtype=np.float32)
        with pytest.raises(plade_amd.PladeError) as e:
            ictx.refine_icp(moved, moved, T0)
        assert e.value.code == plade_amd.PLADE_EFAIL and e.value.info["reason"] == "degenerate", (normals, offset)
        assert np.array_equal(e.value.T, T0)


def test_three_planes_are_not_degenerate_far_away(ictx):
    cloud = _planes((0, 1, 2))
    for offset in (0.0, 1000.0):
        F = R.frame(offset * R.Target(cloud).diag)
        moved = R.move(cloud, F)
        T, info = ictx.refine_icp(moved, moved, R.conjugate(R.perturb(np.eye(4), 0.01, 0.01, seed=2), F))
        assert info["failure"] == 0 and info["converged"], (offset, info)
        assert _fro(R.back(T, F), np.eye(4)) <= 1e-3
