"""Smoothing on the GPU (plade_smooth_cloud / plade_cloud_smooth_dev, plade_amd/csrc/k_smooth.hip) against the numpy restatement
of its semantics (tests/smooth_restate.py: fp32 brute force for the distances, fp64 sums in ascending (d, j) order, numpy's eigh).

Counts and the fitted flag bit for bit; every moment within 1e-12 of the sum of the absolute values of its terms (a few hundred
fp64 terms at 2^-53 each: four orders of margin); normals within 1e-4 rad and curvatures within 1e-5 where the restated gap
(l1 - l0) / trace exceeds 1e-3 (the numbers of test_gpu_normals.py for the same solver; the test asserts on the restatement alone
that this excludes at most 1 % of the fitted points -- here none); the projection from the GPU's own outputs to an fp32 ulp.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import plade_amd
import smooth_restate as S
from plade_amd.synth import make_pair, sample_scene
from conftest import GT_TOL, ORIENTED
from test_smooth_host import plane

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "plade_amd", "PLADE")
FRACTIONS = (0.01, 0.02, 0.05)         # of the diagonal D
MIN_NB = 6
LINE = "smoothing: fitted %d of %d points (rms displacement %.6g, max %.6g)"


@pytest.fixture(scope="module")
def sctx():
    c = plade_amd.Context(0, **ORIENTED)
    yield c
    c.close()


def diag(P):
    return float(np.linalg.norm(P[:, :3].max(0).astype(np.float64) - P[:, :3].min(0).astype(np.float64)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def restate(P, radii, min_nb=MIN_NB, viewpoint=(0.0, 0.0, 0.0)):
    out = []
    for count, mom, mag in S.moments(P, radii):
        ref = S.fit(P, count, mom, min_nb, viewpoint)
        ref.update(count=count, moments=mom, mag=mag)
        out.append(ref)
    return out


class Scene20k:
    """The 20k scene, its restatement at the three radii and the GPU's answer at each (computed once, never changed)."""
    def __init__(self, ctx):
        self.P = np.ascontiguousarray(sample_scene(20000, scene_seed=3, sample_seed=4))
        self.D = diag(self.P)
        self.radii = [np.float32(f * self.D) for f in FRACTIONS]
        self.ref = restate(self.P, self.radii)
        self.gpu = [ctx.smooth_cloud(self.P, r, min_neighbours=MIN_NB, moments=True) for r in self.radii]


@pytest.fixture(scope="module")
def s20k(sctx):
    return Scene20k(sctx)


def check_counts(ctx, P, r, ref, min_nb=MIN_NB):
    rows, info = ctx.smooth_cloud(P, r, min_neighbours=min_nb)
    assert info["count"].dtype == np.uint32 and np.array_equal(info["count"], ref["count"])
    assert np.array_equal(info["fitted_mask"], ref["fitted"]) and info["fitted"] == int(ref["fitted"].sum())
    return rows, info


# ---- 1. counts and the fitted flag --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [0, 1, 2])
def test_counts_and_fitted_of_a_20k_scene(s20k, t):
    (rows, info), ref = s20k.gpu[t], s20k.ref[t]
    print(f"r = {FRACTIONS[t]} D: median count {np.median(ref['count']):.0f}, max {ref['count'].max()}, fitted {ref['fitted'].sum()}")
    assert np.array_equal(info["count"], ref["count"])
    assert np.array_equal(info["fitted_mask"], ref["fitted"]) and info["fitted"] == int(ref["fitted"].sum())
    assert (info["n"], info["max_count"]) == (len(s20k.P), int(ref["count"].max()))
    assert 0 < ref["fitted"].sum() < len(s20k.P)                    # both branches are exercised


def test_a_pair_at_exactly_the_radius(sctx):
    r = np.float32(0.375)                                           # r * r is exact in fp32
    P = np.array([[0, 0, 0], [r, 0, 0]], np.float32)
    rows, info = sctx.smooth_cloud(P, r, min_neighbours=3)
    assert list(info["count"]) == [1, 1] and not info["fitted_mask"].any()       # d = r2: not neighbours
    P[1, 0] = np.nextafter(r, np.float32(0))
    rows, info = sctx.smooth_cloud(P, r, min_neighbours=3)
    assert list(info["count"]) == [2, 2] and not info["fitted_mask"].any()       # one ulp closer: neighbours, too few to fit
    assert same_bits(rows[:, :3], P) and np.isnan(rows[:, 3:]).all() and (info["displacement"] == 0).all()


def test_one_point_and_coincident_points(sctx):
    one = np.array([[1.0, -2.0, 3.0]], np.float32)
    rows, info = sctx.smooth_cloud(one, 0.5, min_neighbours=3)
    assert list(info["count"]) == [1] and not info["fitted_mask"].any() and same_bits(rows[:, :3], one)
    assert (info["n"], info["fitted"], info["rms"], info["max"], info["max_count"]) == (1, 0, 0.0, 0.0, 1)
    same = np.tile(np.array([[0.25, 4.0, -1.5]], np.float32), (50, 1))
    rows, info = sctx.smooth_cloud(same, 0.5, min_neighbours=3)
    assert (info["count"] == 50).all() and not info["fitted_mask"].any()     # C = 0: unfitted
    assert same_bits(rows[:, :3], same) and np.isnan(rows[:, 3:]).all() and np.isnan(info["curvature"]).all()
    assert (info["displacement"] == 0).all() and info["max_count"] == 50


def test_duplicates_mixed_into_the_20k_scene(sctx, s20k):
    rng = np.random.default_rng(11)
    P = np.ascontiguousarray(np.concatenate([s20k.P, s20k.P[rng.choice(len(s20k.P), 700, replace=False)]])[rng.permutation(20700)])
    ref = restate(P, [s20k.radii[1]])[0]
    check_counts(sctx, P, s20k.radii[1], ref)


def test_20k_scene_far_from_the_origin(sctx, s20k):
    """100 D away the shift is not exact in fp32: the restatement is that of the shifted floats."""
    shift = (100.0 * s20k.D / np.sqrt(3.0)) * np.ones(3)
    P = s20k.P.copy()
    P[:, :3] = (s20k.P[:, :3].astype(np.float64) + shift).astype(np.float32)
    ref = restate(P, [s20k.radii[1]], viewpoint=shift)[0]
    rows, info = sctx.smooth_cloud(P, s20k.radii[1], min_neighbours=MIN_NB, viewpoint=shift, moments=True)
    assert np.array_equal(info["count"], ref["count"]) and np.array_equal(info["fitted_mask"], ref["fitted"])
    err = np.abs(info["moments"] - ref["moments"])
    assert (err <= 1e-12 * ref["mag"]).all()


# ---- 2. moments ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [0, 1, 2])
def test_moments_of_every_point(s20k, t):
    (rows, info), ref = s20k.gpu[t], s20k.ref[t]
    err = np.abs(info["moments"] - ref["moments"])
    worst = float(np.max(err / np.maximum(ref["mag"], 1e-300)))
    print(f"r = {FRACTIONS[t]} D: worst |moment - restated| / sum |terms| = {worst:.3e}")
    assert (err <= 1e-12 * ref["mag"]).all()
    assert (info["moments"][:, 0] >= 1.0).all()                     # the point itself: w = 1


# ---- 3. fit -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [0, 1, 2])
def test_normals_curvature_and_orientation(s20k, t):
    (rows, info), ref = s20k.gpu[t], s20k.ref[t]
    f = ref["fitted"]
    clear = f & (np.nan_to_num(ref["gap"], nan=0.0) > 1e-3)
    assert (f & ~clear).sum() <= 0.01 * f.sum()                     # on the restatement alone (here: none excluded)
    n_gpu = rows[:, 3:].astype(np.float64)
    assert np.abs(np.linalg.norm(n_gpu[f], axis=1) - 1.0).max() <= 1e-6
    c = np.abs((n_gpu[clear] * ref["normal"][clear]).sum(1))
    s = np.linalg.norm(np.cross(n_gpu[clear], ref["normal"][clear]), axis=1)
    ang = np.arctan2(s, c)
    dc = np.abs(info["curvature"][f].astype(np.float64) - ref["curvature"][f])
    print(f"r = {FRACTIONS[t]} D: excluded {(f & ~clear).sum()}, max angle {ang.max():.3e}, max curvature error {dc.max():.3e}")
    assert ang.max() <= 1e-4
    assert dc.max() <= 1e-5
    to_view = -s20k.P[f, :3].astype(np.float64)                     # viewpoint 0 0 0
    assert ((to_view * n_gpu[f]).sum(1) >= -1e-6 * np.linalg.norm(to_view, axis=1)).all()


# ---- 4. projection ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [0, 1, 2])
def test_projection(s20k, t):
    (rows, info), ref = s20k.gpu[t], s20k.ref[t]
    f, r = ref["fitted"], float(s20k.radii[t])
    d = info["displacement"]
    want = s20k.P[f, :3].astype(np.float64) + d[f, None] * rows[f, 3:].astype(np.float64)
    tol = np.spacing(np.abs(rows[f, :3])).astype(np.float64) + 2.0 ** -23 * np.abs(d[f, None])
    assert (np.abs(rows[f, :3].astype(np.float64) - want) <= tol).all()
    bound = np.linalg.norm(ref["mu"][f], axis=1) * 1e-4 + 1e-12 * r
    e = np.abs(d[f] - ref["delta"][f])
    print(f"r = {FRACTIONS[t]} D: max |delta - restated| {e.max():.3e}, max |delta| {np.abs(d).max():.3e}, bound used {float((e / bound).max()):.3e}")
    assert (e <= bound).all()
    u = ~f
    assert same_bits(rows[u, :3], s20k.P[u, :3]) and np.isnan(rows[u, 3:]).all() and np.isnan(info["curvature"][u]).all()
    assert (d[u] == 0).all() and not info["fitted_mask"][u].any()


# ---- 5. an exact plane stays put ------------------------------------------------------------------------------------------------
def test_an_exact_plane_stays_put(sctx):
    P = plane()
    rows, info = sctx.smooth_cloud(P, 0.1, min_neighbours=MIN_NB, viewpoint=(0.5, 0.5, 10.0))
    f = info["fitted_mask"]
    assert f.sum() > 0.9 * len(P)
    assert same_bits(rows[:, :3], P)
    assert np.abs(np.abs(rows[f, 3:].astype(np.float64)) - np.array([0.0, 0.0, 1.0])).max() <= 1e-12
    assert (rows[f, 5] == 1.0).all()                                # toward the viewpoint above the plane


# ---- 6. it smooths ------------------------------------------------------------------------------------------------------------
def test_a_noisy_plane_gets_flatter(sctx):
    rng = np.random.default_rng(21)
    r = 0.06
    nrm = np.array([0.3, -0.2, 1.0]) / np.linalg.norm([0.3, -0.2, 1.0])
    e1 = np.cross(nrm, [1.0, 0.0, 0.0]); e1 /= np.linalg.norm(e1)
    e2 = np.cross(nrm, e1)
    o = np.array([0.1, 0.2, 0.3])
    uv = rng.random((4000, 2))
    P = (o + uv[:, :1] * e1 + uv[:, 1:] * e2 + rng.normal(0.0, r / 8.0, 4000)[:, None] * nrm).astype(np.float32)
    rms = lambda X: float(np.sqrt(np.mean(((X.astype(np.float64) - o) @ nrm) ** 2)))
    view = o + 10.0 * nrm
    ref = S.smooth(P, r, MIN_NB, view)
    rows, info = sctx.smooth_cloud(P, r, min_neighbours=MIN_NB, viewpoint=view)
    before, after_ref, after_gpu = rms(P), rms(ref["xyz"]), rms(rows[:, :3])
    print(f"rms distance to the true plane: before {before:.6e}, restated after {after_ref:.6e}, GPU after {after_gpu:.6e}, "
          f"ratio {after_ref / before:.4f}")
    assert after_ref < before
    assert abs(after_gpu - after_ref) <= 1e-6 * after_ref
    assert np.array_equal(info["fitted_mask"], ref["fitted"])


# ---- 7. determinism and paths ---------------------------------------------------------------------------------------------------
def test_repetition_second_context_and_resident_path(sctx, s20k):
    r = s20k.radii[1]
    rows, info = s20k.gpu[1]
    rows2, info2 = sctx.smooth_cloud(s20k.P, r, min_neighbours=MIN_NB)
    assert same_bits(rows2, rows) and same_bits(info2["displacement"], info["displacement"])
    other = plade_amd.Context(0)
    try:
        other.smooth_cloud(s20k.P[:5000], 2 * r)
        rows3, info3 = other.smooth_cloud(s20k.P, r, min_neighbours=MIN_NB)
    finally:
        other.close()
    assert same_bits(rows3, rows) and same_bits(info3["displacement"], info["displacement"])
    for k in ("n", "fitted", "rms", "max", "max_count"):
        assert info2[k] == info[k] == info3[k], k
    c = sctx.upload(s20k.P)
    try:
        f, summ = sctx.smooth_cloud_dev(c, r, min_neighbours=MIN_NB, info=True)
        try:
            assert f.n == len(s20k.P) and same_bits(f.download(), rows)
            assert all(summ[k] == info[k] for k in ("n", "fitted", "rms", "max", "max_count"))
        finally:
            f.free()
        g = sctx.smooth_cloud_dev(c, r, min_neighbours=MIN_NB, fit_normals=False)
        try:
            got = g.download()
            assert same_bits(got[:, :3], rows[:, :3]) and same_bits(got[:, 3:], s20k.P[:, 3:])
        finally:
            g.free()
    finally:
        c.free()


@pytest.mark.parametrize("t", [0, 1, 2])
def test_summary_is_that_of_the_per_point_outputs(s20k, t):
    rows, info = s20k.gpu[t]
    want = S.summary(info["displacement"], info["fitted_mask"], info["count"])
    assert (info["n"], info["fitted"], info["max"], info["max_count"]) == (want["n"], want["fitted"], want["max"], want["max_count"])
    assert abs(info["rms"] - want["rms"]) <= 1e-12 * want["rms"]


def test_xyz_rows_and_wider_rows_give_the_same_bits(sctx, s20k):
    rows, info = s20k.gpu[1]
    rows3, info3 = sctx.smooth_cloud(np.ascontiguousarray(s20k.P[:, :3]), s20k.radii[1], min_neighbours=MIN_NB, per_point=False, normals=False)
    assert same_bits(rows3[:, :3], rows[:, :3]) and np.isnan(rows3[:, 3:]).all() and "count" not in info3
    assert info3["rms"] == info["rms"]


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_the_context_usable(sctx, s20k):
    P = np.ascontiguousarray(s20k.P[:3000, :3])
    good = sctx.smooth_cloud(P, 0.3)[0]
    bad = P.copy()
    bad[17, 1] = np.nan
    inf = P.copy()
    inf[5, 2] = np.inf
    cases = [(np.zeros((0, 3), np.float32), dict(radius=0.3)), (bad, dict(radius=0.3)), (inf, dict(radius=0.3)),
             (P, dict(radius=0.3, viewpoint=(0.0, np.inf, 0.0))), (P, dict(radius=0.3, viewpoint=(np.nan, 0.0, 0.0))),
             (P, dict(radius=0.0)), (P, dict(radius=-1.0)), (P, dict(radius=np.nan)), (P, dict(radius=np.inf)),
             (P, dict(radius=1e-30)), (P, dict(radius=1e-20)), (P, dict(radius=1e20)),   # r2 = 0, subnormal, inf in fp32
             (P, dict(radius=0.3, min_neighbours=2)), (P, dict(radius=0.3, min_neighbours=0))]
    for arr, kw in cases:
        with pytest.raises(plade_amd.PladeError) as e:
            sctx.smooth_cloud(arr, **kw)
        assert e.value.code == plade_amd.PLADE_EINVAL and str(e.value).split(": ", 1)[1], kw
        assert same_bits(sctx.smooth_cloud(P, 0.3)[0], good)       # the next call on the same context succeeds
    # stride < 3 through the C ABI itself
    two = np.zeros((10, 2), np.float32)
    out = np.zeros((10, 3), np.float32)
    prm = plade_amd.SmoothParams()
    sctx.L.plade_smooth_default_params(ctypes.byref(prm))
    prm.radius = 0.3
    rc = sctx.L.plade_smooth_cloud(sctx.h, two.ctypes.data, 10, 2, ctypes.byref(prm), out.ctypes.data, None, None, None, None, None, None, None)
    assert rc == plade_amd.PLADE_EINVAL and b"stride" in sctx.L.plade_last_error(sctx.h)
    # the defaults carry no radius
    rc = sctx.L.plade_smooth_cloud(sctx.h, P.ctypes.data, len(P), 3, None, out.ctypes.data, None, None, None, None, None, None, None)
    assert rc == plade_amd.PLADE_EINVAL and b"radius" in sctx.L.plade_last_error(sctx.h)
    assert same_bits(sctx.smooth_cloud(P, 0.3)[0], good)


# ---- 9. the chain ---------------------------------------------------------------------------------------------------------------
def test_noisy_resident_pair_registers_after_smoothing(sctx):
    """remove_outliers_dev -> smooth_cloud_dev (fit normals) -> registration_dev on a 300k pair with 5 mm of extra range noise
    along its normals; radius 8 cm.  A did-it-survive check, not an accuracy claim."""
    tg, sr, T = make_pair(300000, seed=0)
    rng = np.random.default_rng(31)
    for c in (tg, sr):
        c[:, :3] += (rng.normal(0.0, 0.005, len(c))[:, None] * c[:, 3:].astype(np.float64)).astype(np.float32)
    vs = np.linalg.inv(T)[:3, 3]                          # the target's sensor origin, in the source's frame
    made = []
    try:
        for cloud, view in ((tg, (0.0, 0.0, 0.0)), (sr, vs)):
            c = sctx.upload(cloud); made.append(c)
            f = sctx.remove_outliers_dev(c, k=16); made.append(f)
            s, summ = sctx.smooth_cloud_dev(f, 0.08, viewpoint=view, info=True); made.append(s)
            print(f"kept {f.n} of {len(cloud)}, fitted {summ['fitted']}, rms displacement {summ['rms']:.4e}, max count {summ['max_count']}")
            assert s.n == f.n and summ["fitted"] > 0.9 * f.n
        ok, Tr = sctx.registration_dev(made[2], made[5])
    finally:
        for c in made:
            c.free()
    assert ok
    print(f"|T - T_gt| = {np.linalg.norm(Tr.astype(np.float64) - T):.4f}")
    assert np.linalg.norm(Tr.astype(np.float64) - T) < GT_TOL


# ---- 10. the CLI switch ---------------------------------------------------------------------------------------------------------
def _write_ply(path, cloud):
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "property float nx\nproperty float ny\nproperty float nz\nend_header\n" % len(cloud))
    with open(path, "wb") as f:
        f.write(head.encode())
        f.write(np.ascontiguousarray(cloud, "<f4").tobytes())


def _matrix(text):
    rows = [[float(x) for x in line.split()] for line in text.split("\n")
            if line.strip() and not line.startswith(("target:", "source:", "transformation:", "registration failed"))]
    return np.array(rows, np.float64)


@pytest.mark.timeout(900)
def test_cli_switch(tmp_path, sctx):
    tg, sr, T = make_pair(80000, seed=0)
    pt, ps = str(tmp_path / "t.ply"), str(tmp_path / "s.ply")
    _write_ply(pt, tg)
    _write_ply(ps, sr)
    base = {k: v for k, v in os.environ.items() if not k.startswith("PLADE_")}
    base["PLADE_ORIENT_NORMALS"] = "1"

    def run(**extra):
        res = str(tmp_path / "r.txt")
        if os.path.exists(res):
            os.remove(res)
        r = subprocess.run([CLI, pt, ps, res], capture_output=True, text=True, timeout=300, env=dict(base, **extra))
        return r, (open(res).read() if os.path.exists(res) else None)

    def strip_time(s):
        return "\n".join(l for l in s.split("\n") if not l.startswith("done. time:"))

    r0, res0 = run()
    assert r0.returncode == 0, r0.stdout + r0.stderr
    assert "smoothing" not in r0.stdout + r0.stderr
    rz, resz = run(PLADE_SMOOTH="0")                                # 0 = off: the output without the variable
    assert (rz.returncode, strip_time(rz.stdout), rz.stderr, resz) == (0, strip_time(r0.stdout), r0.stderr, res0)
    # on: one line per cloud with the library's own numbers, the file's normals kept, and the pair registers
    r1, res1 = run(PLADE_SMOOTH="0.1,8")
    assert r1.returncode == 0, r1.stdout + r1.stderr
    lines = [l for l in r1.stdout.split("\n") if l.startswith("smoothing: fitted ")]
    expected = []
    for cloud in (tg, sr):
        info = sctx.smooth_cloud(cloud, 0.1, min_neighbours=8, per_point=False, normals=False)[1]
        expected.append(LINE % (info["fitted"], info["n"], info["rms"], info["max"]))
    assert lines == expected, r1.stdout
    assert np.linalg.norm(_matrix(res1) - T) < GT_TOL
    # after the outlier filter
    r2, _ = run(PLADE_REMOVE_OUTLIERS="16", PLADE_SMOOTH="0.1")
    assert r2.returncode == 0, r2.stdout + r2.stderr
    assert r2.stdout.count("outlier removal: kept ") == 2 and r2.stdout.count("smoothing: fitted ") == 2
    assert r2.stdout.index("outlier removal: kept ") < r2.stdout.index("smoothing: fitted ")
    # a value that does not parse: one warning, nothing smoothed, the output without the variable otherwise
    for badv in ("wide", "0.1,2", "-1", "0.1,8x"):
        rb, resb = run(PLADE_SMOOTH=badv)
        assert rb.stderr.count("warning: PLADE_SMOOTH=") == 1 and "no smoothing" in rb.stderr, badv
        assert "smoothing: fitted" not in rb.stdout
        assert (rb.returncode, strip_time(rb.stdout), resb) == (0, strip_time(r0.stdout), res0)
