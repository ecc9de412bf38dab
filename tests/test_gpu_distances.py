"""Cloud-to-cloud distances and registration fitness on the GPU (plade_cloud_distances, plade_cloud_distances_dev) against the
numpy restatement of their semantics (tests/distance_restate.py): idx and d2 bit for bit, the plane term to 1 ulp, the summary,
invariances, agreement with the ICP's matcher, errors and the CLI switch."""
import os
import subprocess

import numpy as np
import pytest

import plade_amd
from plade_amd.plyio import write_ply
from plade_amd.synth import make_pair
import distance_restate as R
import icp_restate as IR
import ring_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "plade_amd", "PLADE")
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
COUNTS = ("n", "count", "plane_count")
SUMS = ("fitness", "rmse", "mean", "max", "plane_rmse")


@pytest.fixture(scope="module")
def dctx():
    c = plade_amd.Context(0)
    yield c
    c.close()


def _g(name):
    return np.load(os.path.join(GOLDEN, name))


def _perturb(T, rot, trans, seed):
    rng = np.random.default_rng(seed)
    w = rng.normal(size=3)
    w *= rot / np.linalg.norm(w)
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    P = np.eye(4)
    P[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    t = rng.normal(size=3)
    P[:3, 3] = trans * t / np.linalg.norm(t)
    return P @ np.asarray(T, np.float64)


def _same_summary(s, ref):
    for k in COUNTS:
        assert s[k] == ref[k], (k, s[k], ref[k])
    for k in SUMS:
        a, b = s[k], ref[k]
        if np.isnan(b):
            assert np.isnan(a), k
        else:
            assert abs(a - b) <= 1e-12 * abs(b), (k, a, b)


def _check(ctx, tgt, src, d, T=None):
    """GPU against the restatement: idx and d2 bitwise, plane within 1 ulp (NaN at the same places), the summary."""
    idx, d2, plane, s = ctx.cloud_distances(tgt, src, d, T=T)
    r_idx, r_d2, r_plane, r_s = R.cloud_distances(tgt, src, d, T=T)
    bad = np.flatnonzero(idx != r_idx)
    assert len(bad) == 0, (len(bad), d, bad[:5], idx[bad[:5]], r_idx[bad[:5]])
    assert np.array_equal(d2.view(np.uint32), r_d2.view(np.uint32))
    nan = np.isnan(r_plane)
    assert np.array_equal(np.isnan(plane), nan)
    ulps = np.abs(plane[~nan].view(np.int32).astype(np.int64) - r_plane[~nan].view(np.int32).astype(np.int64))
    assert ulps.max(initial=0) <= 1
    _same_summary(s, r_s)
    return idx, d2, plane, s


@pytest.mark.parametrize("name", ["g8_polyhedron.npz", "g9_room.npz"])
def test_golden_scenes_are_exact(dctx, name):
    z = _g(name)
    tgt, src, gt = z["target"], z["source"], z["groundtruth"]
    D = R.diag(tgt)
    for T in (gt, _perturb(gt, 0.03, 0.03, seed=5)):
        idx, _, _, s = _check(dctx, tgt, src, 0.01 * D, T=T)
        assert s["count"] > 1000


@pytest.mark.parametrize("frac", [0.002, 0.01, 0.05, 2.0])
def test_20k_scene_at_every_scale(dctx, frac):
    tg, sr, T = make_pair(20_000, seed=0)
    D = R.diag(tg)
    idx, _, _, s = _check(dctx, tg, sr, frac * D, T=T)
    if frac == 2.0:
        assert s["count"] == len(sr)           # every point corresponds


@pytest.mark.parametrize("offset", [100.0, 500.0])
@pytest.mark.parametrize("frac", [0.002, 0.01, 0.05, 2.0])
def test_20k_scene_at_every_scale_far_from_the_origin(dctx, frac, offset):
    tg, sr, T = make_pair(20_000, seed=0)
    D = R.diag(tg)
    F = IR.frame(offset * D)
    tg, sr = IR.move(tg, F), IR.move(sr, F)
    idx, _, _, s = _check(dctx, tg, sr, frac * D, T=IR.conjugate(T, F).astype(np.float32))
    if frac == 2.0:
        assert s["count"] == len(sr)


def test_1m_pair_sample(dctx):
    tg, sr, T = make_pair(1_000_000, seed=3)
    rng = np.random.default_rng(0)
    S = np.ascontiguousarray(sr[rng.choice(len(sr), 3000, replace=False), :3])
    D = R.diag(tg)
    for TT, d in ((T, 0.01 * D), (_perturb(T, 0.02, 0.02, seed=1), 0.05 * D)):
        _check(dctx, tg, S, d, T=TT)


def test_duplicates_tie_to_the_smaller_index(dctx):
    g = np.arange(12, dtype=np.float32) * np.float32(0.1)
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    lat = np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1)
    pts = np.concatenate([lat, lat[::-1], lat])                       # every point three times
    tgt = np.zeros((len(pts), 6), np.float32)
    tgt[:, :3] = pts
    tgt[:, 5] = 1
    rng = np.random.default_rng(1)
    src = np.concatenate([lat[rng.choice(len(lat), 500)],              # exactly on a lattice point: a three-way tie
                          rng.uniform(-0.1, 1.2, size=(2000, 3)).astype(np.float32)])
    for d in (0.05, 0.3):
        idx, d2, _, _ = _check(dctx, tgt, src, d)
        assert (idx[:500] < len(lat)).all() and (d2[:500] == 0).all()


def test_the_bound_is_strict(dctx):
    tgt = np.zeros((1, 6), np.float32)
    tgt[0, 5] = 1
    for x in (np.float32(0.3), np.float32(1.7), np.float32(0.013)):
        v = x * x
        d = np.float32(np.sqrt(np.float64(v)))
        for c in (d, np.nextafter(d, np.float32(1)), np.nextafter(d, np.float32(0))):
            if c * c == v:
                d = c
                break
        assert d * d == v
        src = np.array([[x, 0, 0]], np.float32)
        idx, d2, _, s = dctx.cloud_distances(tgt, src, float(d))
        assert idx[0] == -1 and d2[0] == np.inf and s["count"] == 0     # d2 == (float)d * (float)d: outside
        up = np.nextafter(d, np.float32(np.inf))
        while not up * up > v:
            up = np.nextafter(up, np.float32(np.inf))
        idx, d2, _, s = dctx.cloud_distances(tgt, src, float(up))
        assert idx[0] == 0 and d2[0] == v and s["count"] == 1           # the next representable bound: inside


def test_far_outliers_and_a_far_source(dctx):
    tg, sr, T = make_pair(20_000, seed=2)
    D = R.diag(tg)
    far = sr.copy()
    far[:, :3] += np.float32(1e3 * D)
    idx, d2, plane, s = dctx.cloud_distances(tg, far, 0.01 * D, T=T)
    assert (idx == -1).all() and np.isinf(d2).all() and np.isnan(plane).all()
    assert s["count"] == 0 and s["fitness"] == 0 and np.isnan(s["rmse"]) and np.isnan(s["plane_rmse"])
    rng = np.random.default_rng(3)
    mixed = np.concatenate([sr[:, :3], rng.uniform(-3 * D, 3 * D, size=(500, 3)).astype(np.float32),
                            np.float32(1e3 * D) * np.ones((10, 3), np.float32)])
    for d in (0.01 * D, 0.5 * D, 2 * D):
        _check(dctx, tg, mixed, d, T=T)


def test_ring_pass_is_exercised_and_exact(dctx):
    tg, sr, T = make_pair(20_000, seed=1)
    D = R.diag(tg)
    rng = np.random.default_rng(4)
    empty = rng.uniform(-0.6 * D, 0.6 * D, size=(3000, 3)).astype(np.float32)   # probes in and around the room's empty space
    src = np.concatenate([sr[:, :3], empty])
    for d in (0.1 * D, 2 * D):
        _check(dctx, tg, src, d, T=T)
        assert dctx.stats()["distances_ring_queries"] > 0


@pytest.mark.parametrize("d", ring_scene.RADII)
def test_the_ring_walk_does_everything(dctx, d):
    """ring_scene.py: the isolated probes' blocks span more than 64 rows, grow at least three times, have whole-row and side runs
    and are clipped by the grid's edge (test_ring_scene_host.py).  The bounds lie below and above the probes' distance."""
    idx = _check(dctx, ring_scene.target(), ring_scene.probes(), d)[0]
    assert dctx.stats()["distances_ring_queries"] >= len(ring_scene.PROBES)
    assert (idx[256:] >= 0).all() == (d > ring_scene.GAP) and (idx[:256] >= 0).all()


def test_plane_term_with_nan_normals(dctx):
    z = _g("g9_room.npz")
    tgt = z["target"].copy()
    rng = np.random.default_rng(2)
    tgt[rng.choice(len(tgt), len(tgt) // 4, replace=False), 3:] = np.nan
    idx, _, plane, s = _check(dctx, tgt, z["source"], 0.01 * R.diag(tgt), T=z["groundtruth"])
    hit = idx >= 0
    assert np.isnan(plane[hit][~np.isfinite(tgt[idx[hit], 3])]).all()
    assert 0 < s["plane_count"] < s["count"]


def test_invariances(dctx):
    tg, sr, T = make_pair(50_000, seed=4)
    D = R.diag(tg)
    d = 0.02 * D
    idx, d2, plane, s = dctx.cloud_distances(tg, sr, d, T=T)
    perm = np.random.default_rng(0).permutation(len(sr))
    i2, d22, p2, s2 = dctx.cloud_distances(tg, sr[perm], d, T=T)
    assert np.array_equal(i2, idx[perm]) and np.array_equal(d22.view(np.uint32), d2[perm].view(np.uint32))
    assert np.array_equal(p2.view(np.uint32), plane[perm].view(np.uint32))
    assert all(s2[k] == s[k] for k in COUNTS)
    far = tg[:1].copy()
    far[0, :3] += np.float32(100 * D)
    i3, d23, p3, s3 = dctx.cloud_distances(np.ascontiguousarray(np.concatenate([tg, far])), sr, d, T=T)
    assert np.array_equal(i3, idx) and np.array_equal(d23.view(np.uint32), d2.view(np.uint32))
    assert np.array_equal(p3.view(np.uint32), plane.view(np.uint32)) and s3 == s
    # repeated calls, another context, resident clouds, no per-point outputs: the same summary bits
    other = plade_amd.Context(0)
    ct, cs = dctx.upload(tg), dctx.upload(sr)
    try:
        outs = [dctx.cloud_distances(tg, sr, d, T=T) for _ in range(3)] + [other.cloud_distances(tg, sr, d, T=T),
                                                                          dctx.cloud_distances_dev(ct, cs, d, T=T)]
        for i4, d24, p4, s4 in outs:
            assert s4 == s and np.array_equal(i4, idx) and np.array_equal(d24.view(np.uint32), d2.view(np.uint32))
            assert np.array_equal(p4.view(np.uint32), plane.view(np.uint32))
        for q in (dctx.cloud_distances(tg, sr, d, T=T, per_point=False), dctx.cloud_distances_dev(ct, cs, d, T=T, per_point=False)):
            assert q[:3] == (None, None, None) and q[3] == s
        assert dctx.evaluate_registration(tg, sr, T, d) == s
    finally:
        ct.free(); cs.free()
        other.close()


def test_agrees_with_the_icp_matcher(dctx):
    z = _g("g9_room.npz")
    tgt = z["target"].copy()
    rng = np.random.default_rng(5)
    tgt[rng.choice(len(tgt), len(tgt) // 5, replace=False), 3:] = np.nan
    S = np.ascontiguousarray(z["source"][:, :3])
    D = R.diag(tgt)
    for T in (z["groundtruth"], _perturb(z["groundtruth"], 0.02, 0.02, seed=2)):
        Tf = np.asarray(T).astype(np.float32)
        for d in (0.0025 * D, 0.025 * D):
            idx, _, _, _ = dctx.cloud_distances(tgt, S, d, T=Tf)
            corr, _ = dctx.icp_linearize(tgt, S, Tf.astype(np.float64), d)
            fin = np.isfinite(tgt[:, 3])
            expect = np.where((idx >= 0) & fin[np.maximum(idx, 0)], idx, -1)
            assert np.array_equal(corr, expect)


@pytest.mark.timeout(900)
def test_fitness_separates_right_from_wrong(dctx):
    # restatement on a 20k sample (tools: tests/distance_restate.py): 0.993 at T_gt, 0.466 after the rooms' 180 degree symmetry
    tg, sr, Tgt = make_pair(1_000_000, seed=0)
    D = R.diag(tg)
    s_gt = dctx.evaluate_registration(tg, sr, Tgt, 0.01 * D)
    s_sym = dctx.evaluate_registration(tg, sr, Tgt @ R.rot_z(np.pi), 0.01 * D)
    s_x = dctx.evaluate_registration(tg, sr, Tgt @ R.rot_x(np.pi), 0.01 * D)
    assert s_gt["fitness"] >= 0.95 and s_sym["fitness"] < 0.6 and s_x["fitness"] < 0.05, (s_gt, s_sym, s_x)
    assert s_gt["n"] == len(sr) and s_gt["rmse"] < 0.01 * D


def test_invalid_arguments_leave_the_context_usable(dctx):
    tg, sr, T = make_pair(20_000, seed=1)
    L, h = dctx.L, dctx.h
    p = lambda a: a.ctypes.data_as(plade_amd.C.c_void_p)   # noqa: E731
    S = np.ascontiguousarray(sr[:, :3])
    summ = plade_amd.DistanceSummary()
    ref = plade_amd.C.byref(summ)
    E = plade_amd.PLADE_EINVAL
    Tf = np.eye(4, dtype=np.float32)
    assert L.plade_cloud_distances(h, None, len(tg), p(S), len(S), 3, None, 0.1, None, None, None, ref) == E
    assert L.plade_cloud_distances(h, p(tg), len(tg), None, len(S), 3, None, 0.1, None, None, None, ref) == E
    assert L.plade_cloud_distances(h, p(tg), len(tg), p(S), len(S), 3, None, 0.1, None, None, None, None) == E
    assert L.plade_cloud_distances(h, p(tg), 0, p(S), len(S), 3, None, 0.1, None, None, None, ref) == E
    assert L.plade_cloud_distances(h, p(tg), len(tg), p(S), 0, 3, None, 0.1, None, None, None, ref) == E
    assert L.plade_cloud_distances(h, p(tg), len(tg), p(S), len(S), 2, None, 0.1, None, None, None, ref) == E
    for d in (0.0, -1.0, float("inf"), float("nan")):
        assert L.plade_cloud_distances(h, p(tg), len(tg), p(S), len(S), 3, None, d, None, None, None, ref) == E
    for v in (np.nan, np.inf):
        bad = Tf.copy()
        bad[1, 3] = v
        assert L.plade_cloud_distances(h, p(tg), len(tg), p(S), len(S), 3, p(bad), 0.1, None, None, None, ref) == E
        badS = S.copy()
        badS[7, 1] = v
        assert L.plade_cloud_distances(h, p(tg), len(tg), p(badS), len(S), 3, None, 0.1, None, None, None, ref) == E
        badT = tg.copy()
        badT[3, 2] = v
        assert L.plade_cloud_distances(h, p(badT), len(tg), p(S), len(S), 3, None, 0.1, None, None, None, ref) == E
    ct, cs = dctx.upload(tg), dctx.upload(sr)
    try:
        assert L.plade_cloud_distances_dev(h, None, cs.h, None, 0.1, None, None, None, ref) == E
        assert L.plade_cloud_distances_dev(h, ct.h, cs.h, None, 0.0, None, None, None, ref) == E
        assert L.plade_cloud_distances_dev(h, ct.h, cs.h, None, 0.1, None, None, None, None) == E
    finally:
        ct.free(); cs.free()
    with pytest.raises(plade_amd.PladeError) as e:
        dctx.cloud_distances(tg, S, -0.5)
    assert e.value.code == E and "max_dist" in str(e.value)
    _check(dctx, tg, S, 0.01 * R.diag(tg), T=T)                             # the context still works


@pytest.mark.timeout(900)
def test_cli_switch(tmp_path):
    pairs = []
    for seed in range(3):
        tg, sr, T = make_pair(200_000, seed=seed)
        pt, ps = str(tmp_path / f"t{seed}.ply"), str(tmp_path / f"s{seed}.ply")
        write_ply(pt, tg)
        write_ply(ps, sr)
        pairs += [pt, ps]
    lst = tmp_path / "pairs.txt"
    lst.write_text("\n".join(pairs) + "\n")
    base = dict(os.environ, PLADE_ORIENT_NORMALS="1", PLADE_GPUS="1")
    base.pop("PLADE_EVALUATE", None)
    base.pop("PLADE_REFINE_ICP", None)
    runs = {}
    for tag, extra in (("unset", {}), ("on", {"PLADE_EVALUATE": "0.1"}), ("bad", {"PLADE_EVALUATE": "-1"}),
                       ("icp", {"PLADE_EVALUATE": "0.1", "PLADE_REFINE_ICP": "1"})):
        res = str(tmp_path / f"r_{tag}.txt")
        r = subprocess.run([CLI, str(lst), res], capture_output=True, text=True, timeout=600, env=dict(base, **extra))
        assert r.returncode == 0, r.stdout + r.stderr
        runs[tag] = (r.stdout, open(res).read(), res, r.stderr)

    def strip(out, res):   # the timings and the result file's name differ from run to run
        return [x for x in out.replace(res, "RESULT").split("\n") if not x.startswith("done. time:")]
    assert runs["on"][1] == runs["unset"][1] and runs["bad"][1] == runs["unset"][1]
    assert "evaluation:" not in runs["unset"][0] + runs["bad"][0]
    assert runs["on"][0].count("evaluation: fitness ") == 3 and runs["icp"][0].count("evaluation: fitness ") == 3
    assert runs["on"][0].count(" source points within 0.1\n") == 3
    assert [x for x in strip(runs["on"][0], runs["on"][2]) if not x.startswith("evaluation: ")] == strip(runs["unset"][0], runs["unset"][2])
    assert strip(runs["bad"][0], runs["bad"][2]) == strip(runs["unset"][0], runs["unset"][2])
    assert (runs["bad"][0] + runs["bad"][3]).count("warning: PLADE_EVALUATE=-1") == 1
    for line in runs["on"][0].split("\n"):
        if line.startswith("evaluation: "):
            fit = float(line.split("fitness ")[1].split(",")[0])
            assert 0.5 < fit <= 1.0, line
    # the single-pair path
    single = {}
    for tag, extra in (("unset", {}), ("on", {"PLADE_EVALUATE": "0.1"})):
        res = str(tmp_path / f"single_{tag}.txt")
        r = subprocess.run([CLI, pairs[0], pairs[1], res], capture_output=True, text=True, timeout=600, env=dict(base, **extra))
        assert r.returncode == 0, r.stdout + r.stderr
        single[tag] = (r.stdout, open(res).read())
    assert single["on"][0].count("evaluation: fitness ") == 1 and "evaluation:" not in single["unset"][0]
    assert single["on"][1] == single["unset"][1]
