"""Outlier removal on the GPU (plade_filter_outliers / plade_cloud_filter_outliers_dev, plade_amd/csrc/k_outliers.hip) against the
numpy restatement of its semantics (tests/outlier_restate.py: fp32 brute force for the keys, fp64 for the rest).

Statistical mode: every m_i, mu, sigma and t within 1e-12 relative; keep equal to m <= t from the GPU's own numbers bit for bit,
and equal to the restatement's keep for every point -- under a condition the test asserts on the restatement alone: no m_i within
1e-9 relative of t.  Radius mode: counts and keep bit for bit.  At 1M points the brute force covers 3 000 sampled points: their
m_i and counts are compared; mu, sigma and t are functions of all the m_i and are recomputed from the GPU's own m array.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import plade_amd
import icp_restate as IR
import outlier_restate as R
import ring_scene
from plade_amd.synth import make_pair, sample_scene
from conftest import GT_TOL, ORIENTED
from test_normals_host import PARENT_RESULT, PARENT_STDERR, PARENT_STDOUT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "plade_amd", "PLADE")
RADII = (0.002, 0.01, 0.05)          # of the diagonal D
REL = 1e-12
GAP = 1e-9


@pytest.fixture(scope="module")
def octx():
    c = plade_amd.Context(0, **ORIENTED)
    yield c
    c.close()


def diag(P):
    return float(np.linalg.norm(P[:, :3].max(0).astype(np.float64) - P[:, :3].min(0).astype(np.float64)))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class Scene:
    """A cloud with its brute-force restatement: the 64 smallest keys of every point and the counts at RADII x D."""
    def __init__(self, P):
        self.P = np.ascontiguousarray(P, np.float32)
        self.D = diag(self.P)
        self.radii = [np.float32(f * self.D) for f in RADII]
        self.keys, self.counts = R.neighbours(self.P, kmax=64, radii=self.radii)


def scene20k():
    return sample_scene(20000, scene_seed=3, sample_seed=4)


@pytest.fixture(scope="module")
def s20k():
    return Scene(scene20k())


def check_statistical(ctx, P, k, alpha, keys, label=""):
    """All of the statistical contract on the whole cloud P (keys: its restated neighbour keys)."""
    ref = R.statistical(P, k, alpha, keys=keys)
    out, kept, info = ctx.remove_outliers(P, k=k, alpha=alpha)
    m = info["mean_dist"]
    e_m = rel(m, ref["m"])
    e_s = [rel(info[a], ref[a]) for a in ("mu", "sigma", "threshold")]
    gap = R.nearest_gap(ref["m"], ref["threshold"])
    print(f"{label} k={k} alpha={alpha}: max rel m {e_m:.3e} (bit-equal: {same_bits(m, ref['m'])}), mu/sigma/t {e_s}, "
          f"nearest gap {gap:.3e}, kept {info['kept']} of {info['n']}, ring {ctx.stats()['outliers_ring_queries']:.0f}")
    assert e_m <= REL
    assert max(e_s) <= REL
    assert np.array_equal(info["keep"], m <= info["threshold"])
    assert gap > GAP, "a point sits on the threshold: choose another seed"
    assert np.array_equal(info["keep"], ref["keep"])
    check_outputs(P, out, kept, info)
    return info, ref


def check_outputs(P, out, kept, info):
    keep = info["keep"]
    assert info["n"] == len(P) and info["kept"] == int(keep.sum()) == len(kept)
    assert kept.dtype == np.uint32 and np.array_equal(kept, np.flatnonzero(keep))
    assert out.shape == (len(kept), P.shape[1]) and same_bits(out.view(np.uint32), P[kept].view(np.uint32))


# ---- statistical mode ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 8, 16, 17, 64])
def test_every_point_of_a_20k_scene(octx, s20k, k):
    info, _ = check_statistical(octx, s20k.P, k, 1.0, s20k.keys, "20k")
    s = octx.stats()
    assert s["outliers_kept"] == info["kept"] and s["outliers_grid_s"] > 0 and s["outliers_search_s"] > 0


def test_alpha_zero(octx, s20k):
    info, ref = check_statistical(octx, s20k.P, 16, 0.0, s20k.keys, "20k")
    assert info["threshold"] == info["mu"]
    assert 0.2 < info["kept"] / info["n"] < 0.8          # the mean itself: a good part of the cloud goes


@pytest.mark.parametrize("offset", [100.0, 500.0])
def test_20k_scene_far_from_the_origin(octx, offset):
    P = scene20k()
    P = IR.move(P, IR.frame(offset * diag(P)))
    sc = Scene(P)
    check_statistical(octx, sc.P, 16, 1.0, sc.keys, f"{offset:.0f} D")
    check_radius(octx, sc, 1, 3)


@pytest.fixture(scope="module")
def s1m():
    P = np.ascontiguousarray(sample_scene(1_000_000, scene_seed=3, sample_seed=6))
    q = np.sort(np.random.default_rng(1).choice(len(P), 3000, replace=False))
    D = diag(P)
    radii = [np.float32(f * D) for f in RADII]
    keys, counts = R.neighbours(P, q, kmax=16, radii=radii)
    return P, q, radii, keys, counts


@pytest.mark.timeout(900)
def test_sampled_points_of_a_1m_scene(octx, s1m):
    P, q, radii, keys, counts = s1m
    out, kept, info = octx.remove_outliers(P, k=16, alpha=1.0)
    m = info["mean_dist"]
    want = R.mean_dist(keys, 16)
    e_m = rel(m[q], want)
    mu, sigma, t = R.threshold(m, 1.0)                  # all 1M m_i are the GPU's: the sample vouches for them
    e_s = [rel(info["mu"], mu), rel(info["sigma"], sigma), rel(info["threshold"], t)]
    gap = R.nearest_gap(want, t)
    print(f"1M: max rel m {e_m:.3e} (bit-equal: {same_bits(m[q], want)}), mu/sigma/t {e_s}, nearest gap of the sample {gap:.3e}, "
          f"kept {info['kept']}, ring {octx.stats()['outliers_ring_queries']:.0f}")
    assert e_m <= REL and max(e_s) <= REL
    assert np.array_equal(info["keep"], m <= info["threshold"])
    assert gap > GAP
    assert np.array_equal(info["keep"][q], want <= t)
    check_outputs(P, out, kept, info)
    for r, c_want in zip(radii, counts):
        out, kept, info = octx.remove_outliers(P, mode="radius", radius=r, min_neighbours=4)
        assert np.array_equal(info["count"][q].astype(np.int64), c_want)
        assert np.array_equal(info["keep"], info["count"] >= 4)
        check_outputs(P, out, kept, info)


def lattice():
    g = np.stack(np.meshgrid(np.arange(14), np.arange(12), np.arange(9), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([g, g, g]))    # every lattice point three times


def test_integer_lattice_with_triplicated_points(octx):
    """Duplicates are neighbours at distance 0 (the point itself is left out by its index), ties go to the smaller index.  Every
    point has the same six-neighbourhood up to the faces, so m takes a few exact values; alpha keeps t away from all of them."""
    P = lattice()
    keys = R.neighbours(P, kmax=33)[0]
    out, kept, info = octx.remove_outliers(P, k=2)          # the two twins, at distance 0: m = mu = sigma = t = 0, all kept
    assert (info["mean_dist"] == 0).all() and (info["mu"], info["sigma"], info["threshold"]) == (0.0, 0.0, 0.0)
    check_outputs(P, out, kept, info)
    assert info["kept"] == len(P)
    for k, alpha in ((16, 0.37), (27, 0.37), (33, 1.23)):
        check_statistical(octx, P, k, alpha, keys, "lattice")


def test_far_outliers_take_the_ring_pass(octx):
    P = scene20k()[:, :3]
    far = np.array([[100.0, 3.0, 1.0], [-2.0, 104.0, 0.5], [1.0, 1.0, -100.0], [100.2, 3.1, 1.0], [100.1, 2.9, 1.2]], np.float32)
    P = np.ascontiguousarray(np.concatenate([P[:7000], far, P[7000:]]))
    keys = R.neighbours(P, kmax=16)[0]
    info, _ = check_statistical(octx, P, 16, 1.0, keys, "far")
    assert octx.stats()["outliers_ring_queries"] >= len(far)
    assert not info["keep"][7000:7005].any()


@pytest.fixture(scope="module")
def ring_keys():
    return R.neighbours(ring_scene.scene(), kmax=64)[0]


@pytest.mark.parametrize("k", [1, 16, 64])
def test_the_ring_walk_does_everything(octx, ring_keys, k):
    """ring_scene.py: the isolated points' blocks span more than 64 rows, grow at least three times, have whole-row and side runs
    and are clipped by the grid's edge (test_ring_scene_host.py)."""
    P = ring_scene.scene()
    ref = R.statistical(P, k, 1.0, keys=ring_keys)
    assert R.nearest_gap(ref["m"], ref["threshold"]) > GAP
    check_statistical(octx, P, k, 1.0, ring_keys, "ring scene")
    assert octx.stats()["outliers_ring_queries"] >= ring_scene.N_FAR


def test_tiny_clouds(octx):
    one = np.array([[1.0, 2.0, 3.0]], np.float32)
    out, kept, info = octx.remove_outliers(one, k=16)
    assert (info["mean_dist"] == 0).all() and (info["mu"], info["sigma"], info["threshold"]) == (0.0, 0.0, 0.0)
    assert info["kept"] == 1 and same_bits(out, one)
    two = np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0]], np.float32)
    out, kept, info = octx.remove_outliers(two, k=16)
    assert (info["mean_dist"] == 5.0).all() and info["mu"] == 5.0 and info["sigma"] == 0.0 and info["kept"] == 2
    rng = np.random.default_rng(3)
    for n, k in ((5, 16), (17, 16), (17, 64), (40, 64)):          # n <= k: k_eff = n - 1, every other point is a neighbour
        P = rng.normal(size=(n, 3)).astype(np.float32)
        check_statistical(octx, P, k, 1.0, R.neighbours(P, kmax=k)[0], f"n={n}")
    # a radius that reaches nothing keeps nothing: PLADE_OK with an empty result
    out, kept, info = octx.remove_outliers(two, mode="radius", radius=1.0)
    assert info["kept"] == 0 and len(out) == 0 and len(kept) == 0 and not info["keep"].any() and np.isnan(info["threshold"])


# ---- radius mode --------------------------------------------------------------------------------------------------------------
def check_radius(ctx, sc, t, min_nb):
    r, want = sc.radii[t], sc.counts[t]
    out, kept, info = ctx.remove_outliers(sc.P, mode="radius", radius=r, min_neighbours=min_nb)
    assert info["count"].dtype == np.uint32 and np.array_equal(info["count"].astype(np.int64), want)
    assert np.array_equal(info["keep"], want >= min_nb)
    assert np.isnan(info["mu"]) and np.isnan(info["sigma"]) and np.isnan(info["threshold"])
    check_outputs(sc.P, out, kept, info)
    # the early stop (no per-point counts) gives the same keep
    out2, kept2, info2 = ctx.remove_outliers(sc.P, mode="radius", radius=r, min_neighbours=min_nb, per_point=False)
    assert "count" not in info2 and np.array_equal(info2["keep"], info["keep"]) and same_bits(kept, kept2) and same_bits(out, out2)
    print(f"radius {float(r):.5f}, min {min_nb}: kept {info['kept']} of {info['n']}, max count {int(want.max())}")
    return info


@pytest.mark.parametrize("t,min_nb", [(0, 1), (1, 4), (2, 60)])
def test_radius_counts_of_a_20k_scene(octx, s20k, t, min_nb):
    info = check_radius(octx, s20k, t, min_nb)
    assert 0 < info["kept"] < info["n"]


def test_radius_on_the_lattice_boundary(octx):
    """r exactly on a lattice distance: points at that distance are NOT counted (`<`); one ulp above they are."""
    P = lattice()
    for r0 in (1.0, 2.0, 3.0):
        r_lo = np.float32(r0)
        r_hi = np.nextafter(r_lo, np.float32(np.inf))
        (c_lo, c_hi) = R.neighbours(P, kmax=0, radii=(r_lo, r_hi))[1]
        assert (c_hi > c_lo).all()
        for r, want in ((r_lo, c_lo), (r_hi, c_hi)):
            mn = int(np.median(want))
            out, kept, info = octx.remove_outliers(P, mode="radius", radius=r, min_neighbours=mn)
            assert np.array_equal(info["count"].astype(np.int64), want)
            assert np.array_equal(info["keep"], want >= mn)
            check_outputs(P, out, kept, info)


# ---- outputs and invariance ---------------------------------------------------------------------------------------------------
def test_rows_are_copied_bit_for_bit(octx):
    cloud = sample_scene(30000, scene_seed=3, sample_seed=7)
    cloud[::7, 3:] = np.nan                               # NaN normal columns, as plade_ply_read_points gives
    cloud[3::11, 4] = np.float32(-0.0)
    xyz = np.ascontiguousarray(cloud[:, :3])
    o3, k3, i3 = octx.remove_outliers(xyz, k=16)
    o6, k6, i6 = octx.remove_outliers(cloud, k=16)
    check_outputs(xyz, o3, k3, i3)
    check_outputs(cloud, o6, k6, i6)
    assert same_bits(k3, k6) and same_bits(i3["mean_dist"], i6["mean_dist"]) and i3["threshold"] == i6["threshold"]
    assert 0 < i3["kept"] < len(cloud) and np.isnan(o6[:, 3:]).any()


def test_permutation_far_point_and_repetition(octx):
    rng = np.random.default_rng(7)
    P = np.ascontiguousarray(sample_scene(30000, scene_seed=3, sample_seed=8)[:, :3])
    assert len(np.unique(P, axis=0)) == len(P)
    oa, ka, ia = octx.remove_outliers(P, k=16)
    # a permuted input keeps the same set of points (m_i bit for bit; mu and sigma are summed in another order)
    perm = rng.permutation(len(P))
    ob, kb, ib = octx.remove_outliers(P[perm], k=16)
    assert same_bits(ia["mean_dist"][perm], ib["mean_dist"])
    assert rel(ib["threshold"], ia["threshold"]) <= REL and R.nearest_gap(ia["mean_dist"], ia["threshold"]) > GAP
    assert np.array_equal(ia["keep"][perm], ib["keep"])
    assert np.array_equal(np.sort(perm[kb]), ka)
    # an extra far point changes no other point's m
    far = np.concatenate([P, np.array([[500.0, -300.0, 80.0]], np.float32)])
    of, kf, inf_ = octx.remove_outliers(far, k=16)
    assert same_bits(inf_["mean_dist"][:-1], ia["mean_dist"]) and not inf_["keep"][-1]
    # repeated calls, another context, other work in between: the same bits
    o2, k2, i2 = octx.remove_outliers(P, k=16)
    other = plade_amd.Context(0)
    try:
        other.remove_outliers(P[:5000], k=32)
        o3, k3, i3 = other.remove_outliers(P, k=16)
    finally:
        other.close()
    for o, k, i in ((o2, k2, i2), (o3, k3, i3)):
        assert same_bits(o, oa) and same_bits(k, ka) and same_bits(i["mean_dist"], ia["mean_dist"])
        assert (i["mu"], i["sigma"], i["threshold"]) == (ia["mu"], ia["sigma"], ia["threshold"])


def test_resident_cloud_gives_the_host_bits(octx):
    cloud = sample_scene(50000, scene_seed=3, sample_seed=9)
    oh, kh, ih = octx.remove_outliers(cloud, k=16)
    c = octx.upload(cloud)
    try:
        f, kd, idv = octx.remove_outliers_dev(c, k=16, info=True)
        try:
            assert f.n == ih["kept"] and same_bits(kd, kh) and np.array_equal(idv["keep"], ih["keep"])
            assert (idv["mu"], idv["sigma"], idv["threshold"]) == (ih["mu"], ih["sigma"], ih["threshold"])
            # the resident rows are the host's: every filtered host point finds itself in the resident cloud at distance 0
            ch = octx.upload(oh)
            try:
                idx, d2, plane, s = octx.cloud_distances_dev(f, ch, 0.01)
            finally:
                ch.free()
            assert np.array_equal(idx, np.arange(len(oh))) and (d2 == 0).all() and s["count"] == len(oh)
        finally:
            f.free()
        fr = octx.remove_outliers_dev(c, mode="radius", radius=0.01 * diag(cloud), min_neighbours=4)
        try:
            assert fr.n == octx.remove_outliers(cloud, mode="radius", radius=0.01 * diag(cloud), min_neighbours=4)[2]["kept"]
        finally:
            fr.free()
        with pytest.raises(plade_amd.PladeError) as e:      # nothing kept: a resident cloud has no empty form
            octx.remove_outliers_dev(c, mode="radius", radius=1e-7, min_neighbours=5)
        assert e.value.code == plade_amd.PLADE_EFAIL and "no point" in str(e.value)
        f = octx.remove_outliers_dev(c, k=16)
        assert f.n == ih["kept"]
        f.free()
    finally:
        c.free()


# ---- the registration path ----------------------------------------------------------------------------------------------------
def test_filtered_resident_pair_registers(octx):
    tg, sr, T = make_pair(200000, seed=0)
    ct, cs = octx.upload(tg), octx.upload(sr)
    try:
        ft, fs = octx.remove_outliers_dev(ct, k=16), octx.remove_outliers_dev(cs, k=16)
        try:
            assert 0.9 * len(tg) < ft.n < len(tg) and 0.9 * len(sr) < fs.n < len(sr)
            ok, Tr = octx.registration_dev(ft, fs)
        finally:
            ft.free()
            fs.free()
    finally:
        ct.free()
        cs.free()
    assert ok
    assert np.linalg.norm(Tr.astype(np.float64) - T) < GT_TOL


@pytest.mark.parametrize("seed", [0, 2])
def test_chain_on_raw_coordinates(octx, seed):
    """filter -> upload_xyz (normals) -> registration_dev on a pair stripped of its normals."""
    tg, sr, T = make_pair(80000, seed=seed)
    vs = np.linalg.inv(T)[:3, 3]                          # the target's sensor origin, in the source's frame
    tx, _, it = octx.remove_outliers(np.ascontiguousarray(tg[:, :3]), k=16)
    sx, _, is_ = octx.remove_outliers(np.ascontiguousarray(sr[:, :3]), k=16)
    assert it["kept"] < len(tg) and is_["kept"] < len(sr)
    ct, cs = octx.upload_xyz(tx, k=16), octx.upload_xyz(sx, k=16, viewpoint=vs)
    try:
        ok, Tr = octx.registration_dev(ct, cs)
    finally:
        ct.free()
        cs.free()
    assert ok
    assert np.linalg.norm(Tr.astype(np.float64) - T) < GT_TOL


# ---- errors -------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_the_context_usable(octx, s20k):
    P = np.ascontiguousarray(s20k.P[:3000, :3])
    keys = R.neighbours(P, kmax=16)[0]
    bad = P.copy()
    bad[17, 1] = np.nan
    inf = P.copy()
    inf[5, 2] = np.inf
    cases = [(P, dict(k=0)), (P, dict(k=65)), (P, dict(k=-3)), (P, dict(alpha=-0.5)), (P, dict(alpha=np.nan)), (P, dict(alpha=np.inf)),
             (np.zeros((0, 3), np.float32), {}), (bad, {}), (inf, {}), (bad, dict(mode="radius", radius=0.1)),
             (P, dict(mode="radius", radius=0.0)), (P, dict(mode="radius", radius=-1.0)), (P, dict(mode="radius", radius=np.nan)),
             (P, dict(mode="radius", radius=np.inf)), (P, dict(mode="radius")), (P, dict(mode="radius", radius=0.1, min_neighbours=0))]
    for arr, kw in cases:
        with pytest.raises(plade_amd.PladeError) as e:
            octx.remove_outliers(arr, **kw)
        assert e.value.code == plade_amd.PLADE_EINVAL and str(e.value), kw
        check_statistical(octx, P, 16, 1.0, keys, "after an error")          # the next call on the same context succeeds
    # stride < 3 through the C ABI itself
    two = np.zeros((10, 2), np.float32)
    summ = plade_amd.OutlierSummary()
    rc = octx.L.plade_filter_outliers(octx.h, two.ctypes.data, 10, 2, None, None, None, None, None, None, ctypes.byref(summ))
    assert rc == plade_amd.PLADE_EINVAL and b"stride" in octx.L.plade_last_error(octx.h)
    check_statistical(octx, P, 16, 1.0, keys, "after stride 2")


# ---- the CLI switch -----------------------------------------------------------------------------------------------------------
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
def test_cli_switch(tmp_path, octx):
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
    assert "outlier removal" not in r0.stdout + r0.stderr
    rz, resz = run(PLADE_REMOVE_OUTLIERS="0")
    assert (rz.returncode, strip_time(rz.stdout), rz.stderr) == (0, strip_time(r0.stdout), r0.stderr)
    assert resz == res0
    # on: one line per cloud, the library's own numbers, and the pair still registers
    r1, res1 = run(PLADE_REMOVE_OUTLIERS="16,1.5")
    assert r1.returncode == 0, r1.stdout + r1.stderr
    lines = [l for l in r1.stdout.split("\n") if l.startswith("outlier removal: kept ")]
    assert len(lines) == 2, r1.stdout
    for line, cloud in zip(lines, (tg, sr)):
        info = octx.remove_outliers(cloud, k=16, alpha=1.5, per_point=False)[2]
        assert line == "outlier removal: kept %d of %d points (threshold %.6g)" % (info["kept"], info["n"], info["threshold"])
    assert np.linalg.norm(_matrix(res1) - T) < GT_TOL
    # a value that does not parse: one warning, nothing filtered, the parent's output otherwise
    for badv in ("sixteen", "16,", "16,-1", "65", "16,1.0x", "-2"):
        rb, resb = run(PLADE_REMOVE_OUTLIERS=badv)
        assert rb.returncode == 0
        assert rb.stderr.count("warning: PLADE_REMOVE_OUTLIERS=") == 1 and "no outlier removal" in rb.stderr, badv
        assert "outlier removal: kept" not in rb.stdout and strip_time(rb.stdout) == strip_time(r0.stdout)
        assert resb == res0


def test_cli_switch_precedes_normal_estimation(tmp_path):
    tg, sr, T = make_pair(80000, seed=0)
    vs = np.linalg.inv(T)[:3, 3]
    src = (sr[:, :3].astype(np.float64) - vs).astype(np.float32)      # the source with its own sensor at its origin
    T_shift = np.eye(4)
    T_shift[:3, 3] = -vs
    pt, ps, res = str(tmp_path / "t.ply"), str(tmp_path / "s.ply"), str(tmp_path / "r.txt")
    for path, xyz in ((pt, tg[:, :3]), (ps, src)):
        head = f"ply\nformat binary_little_endian 1.0\nelement vertex {len(xyz)}\nproperty float x\nproperty float y\nproperty float z\nend_header\n"
        with open(path, "wb") as f:
            f.write(head.encode())
            f.write(np.ascontiguousarray(xyz, "<f4").tobytes())
    env = {k: v for k, v in os.environ.items() if not k.startswith("PLADE_")}
    env.update(PLADE_ORIENT_NORMALS="1", PLADE_ESTIMATE_NORMALS="16", PLADE_REMOVE_OUTLIERS="16")
    r = subprocess.run([CLI, pt, ps, res], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert out.count("outlier removal: kept ") == 2 and out.count("estimated from 16 nearest neighbours") == 2
    assert out.index("outlier removal: kept ") < out.index("estimated from 16 nearest neighbours")
    assert np.linalg.norm(_matrix(open(res).read()) @ T_shift - T) < GT_TOL
    # without either switch the xyz-only files fail as the parent revision's CLI does
    env0 = {k: v for k, v in env.items() if k not in ("PLADE_ESTIMATE_NORMALS", "PLADE_REMOVE_OUTLIERS")}
    r0 = subprocess.run([CLI, pt, ps, str(tmp_path / "r0.txt")], capture_output=True, text=True, timeout=300, env=env0)
    assert (r0.returncode, r0.stdout, r0.stderr) == (1, PARENT_STDOUT.format(t=pt, s=ps), PARENT_STDERR)
    assert open(str(tmp_path / "r0.txt")).read() == PARENT_RESULT
