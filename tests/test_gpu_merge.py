"""Cloud merge on the GPU (plade_merge_clouds*, plade_cloud_download): rows, count, mask and summary against
the numpy restatement of the semantics (tests/merge_restate.py) BIT FOR BIT -- NaNs by position --, the invariances the semantics
promise, resident clouds, the error codes and the CLI switch.  Every case holds at most ~20k points (the CLI pair apart)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import plade_amd
import merge_restate as R
from plade_amd import plyio
from plade_amd.synth import make_pair, sample_scene
from conftest import GT_TOL, ORIENTED

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "plade_amd", "PLADE")
KEYS = ("n_in", "n_out", "n_shared", "max_count")


@pytest.fixture(scope="module")
def mctx():
    c = plade_amd.Context(0, **ORIENTED)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pair():
    tg, sr, T = make_pair(8000, seed=0)
    return tg, sr, T.astype(np.float32)


def cloud(rng, n, lo=-1.0, hi=1.0):
    c = rng.uniform(lo, hi, (n, 6)).astype(np.float32)
    c[:, 3:] = rng.normal(size=(n, 3)).astype(np.float32)
    c[:, 3:] /= np.linalg.norm(c[:, 3:], axis=1, keepdims=True)
    return c


def same_result(a, b):
    (ra, ia), (rb, ib) = a, b
    return (R.same_bits(ra, rb) and np.array_equal(ia["count"], ib["count"]) and np.array_equal(ia["mask"], ib["mask"])
            and all(ia[k] == ib[k] for k in KEYS))


def check(ctx, clouds, Ts, leaf):
    """The library's merge of the host clouds against the restatement, bit for bit; returns (rows, info)."""
    rows, info = ctx.merge_clouds(clouds, Ts, leaf)
    want_rows, want_count, want_mask, want = R.merge(clouds, Ts, leaf)
    assert {k: info[k] for k in KEYS} == want
    assert np.array_equal(info["count"], want_count) and np.array_equal(info["mask"], want_mask)
    assert rows.shape == want_rows.shape
    nan_g, nan_w = np.isnan(rows), np.isnan(want_rows)
    assert np.array_equal(nan_g, nan_w), "NaNs at other positions"
    diff = np.flatnonzero((rows.view(np.uint32) != want_rows.view(np.uint32))[~nan_g])
    assert diff.size == 0, f"{diff.size} floats differ in bits, first {rows[~nan_g][diff[0]]!r} vs {want_rows[~nan_g][diff[0]]!r}"
    return rows, info


def test_two_overlapping_rotated_room_scans(mctx, pair):
    tg, sr, T = pair
    src_frame = sr.copy()            # the source as scanned: in its own frame, T takes it onto the target
    rows, info = check(mctx, [tg, src_frame], [None, T], 0.25)
    m = info["mask"]
    assert set(np.unique(m)) == {1, 2, 3}
    assert info["n_shared"] == int((m == 3).sum()) > 0.1 * info["n_out"]      # the overlap is one row per voxel, not two
    assert info["count"].sum() == len(tg) + len(sr) and info["n_out"] < info["n_in"]


def test_sixteen_clouds_with_one_point_clouds(mctx):
    rng = np.random.default_rng(1)
    sizes = [1, 700, 1, 33, 4097, 1, 256, 257, 64, 2, 1000, 1, 511, 129, 3000, 1]
    clouds = [cloud(rng, n) for n in sizes]
    Ts = []
    for c in range(16):
        T = np.eye(4, dtype=np.float32)
        a = 0.05 * c
        T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        T[:3, 3] = rng.uniform(-0.2, 0.2, 3)
        Ts.append(None if c == 5 else T)
    rows, info = check(mctx, clouds, Ts, 0.25)
    assert np.bitwise_or.reduce(info["mask"]) == 0xffff and info["n_shared"] > 0


def test_every_point_in_its_own_voxel(mctx):
    g = np.stack(np.meshgrid(np.arange(21), np.arange(19), np.arange(17), indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(2)
    c = cloud(rng, len(g))
    c[:, :3] = (g + 0.5).astype(np.float32)[rng.permutation(len(g))]
    rows, info = check(mctx, [c[:3000], c[3000:]], None, 1.0)
    assert info["n_out"] == info["n_in"] == len(g) and info["max_count"] == 1 and info["n_shared"] == 0


def test_all_points_in_one_voxel_across_tiles_and_chunks(mctx):
    rng = np.random.default_rng(3)
    a, b = cloud(rng, 5000, 0.05, 0.95), cloud(rng, 1200, 0.05, 0.95)
    rows, info = check(mctx, [a, b], None, 1.0)
    assert info["n_out"] == 1 and info["max_count"] == 6200 and info["n_shared"] == 1 and info["mask"][0] == 3


def test_a_run_that_straddles_a_tile_boundary(mctx):
    rng = np.random.default_rng(4)
    parts = []
    for v, n in enumerate((4000, 300, 900, 3100, 1, 50)):   # sorted positions 4000..4299 hold one voxel: across position 4096
        p = cloud(rng, n, 0.05, 0.95)
        p[:, 0] += v
        parts.append(p)
    c = np.concatenate(parts)[rng.permutation(8351)]
    rows, info = check(mctx, [c[:5000], c[5000:]], None, 1.0)
    assert list(info["count"]) == [4000, 300, 900, 3100, 1, 50]


@pytest.mark.parametrize("leaf, wide", [(0.004, True), (0.1, False)])
def test_key_widths(mctx, leaf, wide):
    rng = np.random.default_rng(5)
    a, b = cloud(rng, 6000, -5.0, 5.0), cloud(rng, 5000, -5.0, 5.0)
    b[:2000, :3] = a[:2000, :3] + np.float32(0.0005)      # neighbours that share voxels at either leaf
    ijk = R.voxel_ijk(np.concatenate([a, b])[:, :3], leaf)
    bits = sum(max(1, int(v).bit_length()) for v in ijk.max(0))
    assert (bits > 31) == wide
    rows, info = check(mctx, [a, b], None, leaf)
    assert info["n_shared"] > 0
    assert (rows[:, :3].min(0) < 0).all()                 # negative coordinates


def test_a_frame_1000_units_from_the_origin(mctx, pair):
    tg, sr, T = pair
    off = np.array([1000.0, -1000.0, 1000.0])
    far_t = tg.copy()
    far_t[:, :3] = (tg[:, :3].astype(np.float64) + off).astype(np.float32)
    Tf = T.astype(np.float64).copy()
    Tf[:3, 3] += off
    rows, info = check(mctx, [far_t, sr], [None, Tf.astype(np.float32)], 0.1)
    assert info["n_shared"] > 0 and np.abs(rows[:, :3]).min() > 900


def test_nan_normals_mixed_and_all_nan_in_a_voxel(mctx):
    rng = np.random.default_rng(6)
    a, b = cloud(rng, 4000), cloud(rng, 3000)
    a[::3, 3:] = np.nan
    b[::5, 4] = np.nan                                    # one non-finite component: the normal does not count
    b[7, 3] = np.inf
    for c in (a, b):
        c[(c[:, 0] < -0.5) & (c[:, 1] < 0.0), 3:] = np.nan   # whole voxels without a finite normal
    rows, info = check(mctx, [a, b], None, 0.5)
    all_nan = np.isnan(rows[:, 3:]).all(1)
    assert all_nan.any() and (~all_nan).any() and np.isfinite(rows[:, :3]).all()
    assert np.allclose(np.linalg.norm(rows[~all_nan, 3:], axis=1), 1.0, atol=1e-6)


def test_exactly_cancelling_normals(mctx):
    rng = np.random.default_rng(7)
    a = cloud(rng, 3000)
    b = a.copy()
    b[:, 3:] = -a[:, 3:]
    rows, info = check(mctx, [a, b], None, 1e-3)           # (nearly) every point alone with its mirror twin
    twins = info["count"] == 2
    assert twins.sum() > 2900 and np.isnan(rows[twins, 3:]).all() and (info["mask"][twins] == 3).all()


def test_leaf_zero_and_null_transforms(mctx):
    rng = np.random.default_rng(8)
    a, b = cloud(rng, 3001), cloud(rng, 1999)
    a[::4, 3:] = np.nan
    rows, info = check(mctx, [a, b], None, 0.0)
    assert np.array_equal(rows[:, :3], np.concatenate([a, b])[:, :3])     # the identity keeps the coordinates' values
    assert (info["count"] == 1).all() and np.array_equal(info["mask"], np.r_[np.full(3001, 1), np.full(1999, 2)])
    eye = np.eye(4, dtype=np.float32)
    for leaf in (0.0, 0.3):
        assert same_result(mctx.merge_clouds([a, b], None, leaf), mctx.merge_clouds([a, b], [eye, eye], leaf))
        assert same_result(mctx.merge_clouds([a, b], None, leaf), mctx.merge_clouds([a, b], [None, eye], leaf))
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    T[:3, 3] = [1, 2, 3]
    check(mctx, [a, b], [None, T], 0.0)


def test_invariances(mctx, pair):
    tg, sr, T = pair
    base = mctx.merge_clouds([tg, sr], [None, T], 0.1)
    # repeated calls, per_voxel off, a second context: the same bits
    assert same_result(base, mctx.merge_clouds([tg, sr], [None, T], 0.1))
    rows_only, info_only = mctx.merge_clouds([tg, sr], [None, T], 0.1, per_voxel=False)
    assert R.same_bits(rows_only, base[0]) and "count" not in info_only and all(info_only[k] == base[1][k] for k in KEYS)
    other = plade_amd.Context(0, **ORIENTED)
    try:
        check(other, [sr[:100]], None, 0.5)                # (its work areas have seen another shape first)
        assert same_result(base, other.merge_clouds([tg, sr], [None, T], 0.1))
    finally:
        other.close()
    # a permutation inside a cloud changes the order of the sums and nothing else: voxels, counts and masks stay, the rows are
    # the restatement's for the permuted order and agree with the unpermuted ones to fp64 rounding
    rng = np.random.default_rng(9)
    perm = check(mctx, [tg[rng.permutation(len(tg))], sr[rng.permutation(len(sr))]], [None, T], 0.1)
    assert np.array_equal(perm[1]["count"], base[1]["count"]) and np.array_equal(perm[1]["mask"], base[1]["mask"])
    assert np.allclose(perm[0], base[0], rtol=0, atol=1e-5, equal_nan=True)


def test_host_and_resident_clouds_agree(mctx, pair):
    tg, sr, T = pair
    ct, cs = mctx.upload(tg), mctx.upload(sr)
    try:
        for leaf in (0.1, 0.004, 0.0):
            host = mctx.merge_clouds([tg, sr], [None, T], leaf)
            merged, info = mctx.merge_clouds_dev([ct, cs], [None, T], leaf, info=True)
            try:
                assert merged.n == host[1]["n_out"]
                assert same_result(host, (merged.download(), info))
            finally:
                merged.free()
    finally:
        ct.free(); cs.free()


def test_one_cloud_identity_against_voxel_downsample(mctx, pair):
    tg = pair[0]
    leaf = 0.15
    rows, info = check(mctx, [tg], None, leaf)
    ref = mctx.voxel_downsample(tg[:, :3], leaf)
    assert len(ref) == len(rows)
    # row by row (the same voxels in the same order) within the fp32 sequential-sum bound of the fp32 centroid
    bound = (int(info["count"].max()) + 1) * 2.0 ** -24 * float(np.abs(tg[:, :3]).max())
    assert np.abs(rows[:, :3].astype(np.float64) - ref.astype(np.float64)).max() <= bound
    # and voxel_downsample keeps its bits whatever ran before it on the context
    assert R.same_bits(ref, mctx.voxel_downsample(tg[:, :3], leaf))


def test_download_of_every_kind_of_resident_cloud(mctx, pair):
    tg = pair[0]
    up = mctx.upload(tg)
    xyz = mctx.upload_xyz(tg[:, :3], k=12)
    flt = mctx.remove_outliers_dev(up, k=8, alpha=1.0)
    mrg = mctx.merge_clouds_dev([up, flt], None, 0.2)
    try:
        assert R.same_bits(up.download(), tg)
        got = xyz.download()
        assert got.shape == tg.shape and R.same_bits(got[:, :3], tg[:, :3])
        assert R.same_bits(got, mctx.estimate_normals(tg[:, :3], k=12))
        host_rows = mctx.remove_outliers(tg, k=8, alpha=1.0, per_point=False)[0]
        assert R.same_bits(flt.download(), host_rows) and flt.n == len(host_rows)
        assert R.same_bits(mrg.download(), mctx.merge_clouds([tg, host_rows], None, 0.2)[0])
        # capacity too small: PLADE_ECAP; rows NULL: n only
        n = ctypes.c_uint32(0)
        small = np.empty((10, 6), np.float32)
        assert mctx.L.plade_cloud_download(mctx.h, up.h, small.ctypes.data_as(ctypes.c_void_p), 10, ctypes.byref(n)) == plade_amd.PLADE_ECAP
        assert mctx.L.plade_cloud_download(mctx.h, up.h, None, 0, ctypes.byref(n)) == 0 and n.value == len(tg)
    finally:
        for c in (up, xyz, flt, mrg):
            c.free()


def test_a_merged_resident_cloud_is_a_cloud_like_any_other(mctx, pair):
    tg = pair[0]
    leaf = 0.1
    ct = mctx.upload(tg)
    merged = mctx.merge_clouds_dev([ct], None, leaf)
    try:
        # a fused point lies in its voxel, which holds a target point: never farther than the voxel's diagonal
        summ = mctx.cloud_distances_dev(ct, merged, 1.01 * leaf * 3 ** 0.5, per_point=False)[3]
        assert summ["n"] == merged.n and summ["fitness"] == 1.0
        kept = mctx.remove_outliers_dev(merged, k=8, alpha=3.0)
        assert 0 < kept.n <= merged.n
        kept.free()
        T, info = mctx.refine_icp_dev(ct, merged, np.eye(4, dtype=np.float32))
        assert np.linalg.norm(T - np.eye(4)) < 0.05
    finally:
        ct.free(); merged.free()


def test_a_merged_resident_pair_registers(mctx):
    tg, sr, T = make_pair(30000, seed=0)
    ct, cs = mctx.upload(tg), mctx.upload(sr)
    mt, ms = mctx.merge_clouds_dev([ct], None, 0.0), mctx.merge_clouds_dev([cs], None, 0.0)
    try:
        ok, Tr = mctx.registration_dev(mt, ms)
        assert ok and np.linalg.norm(Tr.astype(np.float64) - T) < GT_TOL
    finally:
        for c in (ct, cs, mt, ms):
            c.free()


def test_errors_leave_the_context_usable(mctx):
    rng = np.random.default_rng(10)
    a, b = cloud(rng, 500), cloud(rng, 300)
    good = lambda: check(mctx, [a, b], None, 0.3)
    good()

    def fails(code, clouds, Ts=None, leaf=0.3):
        with pytest.raises(plade_amd.PladeError) as e:
            mctx.merge_clouds(clouds, Ts, leaf)
        assert e.value.code == code, e.value
        good()

    E, Lm = plade_amd.PLADE_EINVAL, plade_amd.PLADE_ELIMIT
    fails(E, [])
    fails(E, [a] * 17)
    fails(E, [a, np.zeros((0, 6), np.float32)])
    for bad in (np.nan, np.inf, -np.inf):
        c = a.copy()
        c[123, 1] = bad
        fails(E, [b, c])
        T = np.eye(4, dtype=np.float32)
        T[1, 3] = bad
        fails(E, [a, b], [None, T])
    fails(E, [a, b], None, -0.1)
    fails(E, [a, b], None, np.nan)
    fails(E, [a, b], None, np.inf)
    far = a.copy()
    far[0, 0] = 300.0
    fails(Lm, [far, b], None, 0.001)                       # 3e5 leaves along x
    check(mctx, [far, b], None, 0.002)                     # 1.5e5: allowed
    # sum n_c >= 2^31 is refused before anything is touched
    ptrs = (ctypes.c_void_p * 2)(a.ctypes.data, b.ctypes.data)
    ns = (ctypes.c_uint32 * 2)(1 << 30, 1 << 30)
    out = np.empty((4, 6), np.float32)
    summ = plade_amd.MergeSummary()
    assert mctx.L.plade_merge_clouds(mctx.h, 2, ptrs, ns, None, 0.3, out.ctypes.data_as(ctypes.c_void_p), None, None, ctypes.byref(summ)) == Lm
    good()
    # a NULL cloud (host table and resident)
    ptrs = (ctypes.c_void_p * 2)(a.ctypes.data, None)
    ns = (ctypes.c_uint32 * 2)(500, 300)
    assert mctx.L.plade_merge_clouds(mctx.h, 2, ptrs, ns, None, 0.3, out.ctypes.data_as(ctypes.c_void_p), None, None, ctypes.byref(summ)) == E
    ca = mctx.upload(a)
    freed = mctx.upload(b)
    freed.free()
    with pytest.raises(plade_amd.PladeError) as e:
        mctx.merge_clouds_dev([ca, freed], None, 0.3)
    assert e.value.code == E
    with pytest.raises(plade_amd.PladeError) as e:
        mctx.merge_clouds_dev([ca], None, -1.0)
    assert e.value.code == E
    ca.free()
    good()


# ---- the CLI switch -----------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
def test_cli_switch(tmp_path):
    tg, sr, T = make_pair(80000, seed=0)
    pt, ps = str(tmp_path / "t.ply"), str(tmp_path / "s.ply")
    plyio.write_ply(pt, tg)
    plyio.write_ply(ps, sr)
    base = {k: v for k, v in os.environ.items() if not k.startswith("PLADE_")}
    base["PLADE_ORIENT_NORMALS"] = "1"
    res = str(tmp_path / "r.txt")
    merged = res + ".merged.ply"

    def run(args=None, **extra):
        for f in (res, merged):
            if os.path.exists(f):
                os.remove(f)
        return subprocess.run([CLI] + (args or [pt, ps, res]), capture_output=True, text=True, timeout=300, env=dict(base, **extra))

    def strip_time(s):
        return "\n".join(l for l in s.split("\n") if not l.startswith("done. time:"))

    def merge_line(r):
        lines = [l for l in r.stdout.split("\n") if l.startswith("merge: ")]
        assert len(lines) == 1, r.stdout + r.stderr
        w = lines[0].split()
        assert lines[0] == "merge: %s of %s points kept, %s voxels seen by both clouds" % (w[1], w[3], w[6])
        return int(w[1]), int(w[3]), int(w[6])

    r0 = run()
    assert r0.returncode == 0, r0.stdout + r0.stderr
    assert "merge" not in r0.stdout + r0.stderr and not os.path.exists(merged)
    res0 = open(res).read()
    lo, hi = tg[:, :3].min(0), tg[:, :3].max(0)
    for leaf in (0.05, 0.0):
        r1 = run(PLADE_MERGE=str(leaf))
        assert r1.returncode == 0, r1.stdout + r1.stderr
        assert open(res).read() == res0 and r1.stderr == r0.stderr
        assert strip_time("\n".join(l for l in r1.stdout.split("\n") if not l.startswith("merge: "))) == strip_time(r0.stdout)
        n_out, n_in, n_shared = merge_line(r1)
        rows = plyio.read_ply(merged)
        assert len(rows) == n_out and n_in == len(tg) + len(sr)
        # in the target file's frame: the merged cloud's box contains the target's -- exactly when the points are kept (leaf
        # 0), and to within one leaf when they are fused (a voxel's mean lies in the voxel that holds the extreme point)
        assert (rows[:, :3].min(0) <= lo + leaf).all() and (rows[:, :3].max(0) >= hi - leaf).all()
        if leaf == 0.0:
            assert n_out == n_in and n_shared == 0 and np.array_equal(rows[:len(tg)], tg)
        else:
            assert n_out < n_in and n_shared > 0.1 * n_out    # the registered source falls into the target's voxels
    # a value that does not parse: one warning, nothing merged, the parent's output otherwise
    for badv in ("fine", "-0.1", "0.05x", "nan", "inf", ""):
        rb = run(PLADE_MERGE=badv)
        assert rb.returncode == 0
        assert rb.stderr.count("warning: PLADE_MERGE=") == 1 and "no merge" in rb.stderr, badv
        assert "merge: " not in rb.stdout and strip_time(rb.stdout) == strip_time(r0.stdout)
        assert open(res).read() == res0 and not os.path.exists(merged)
    # a list: <result file>.<pair index>.merged.ply
    lst = str(tmp_path / "pairs.txt")
    with open(lst, "w") as f:
        f.write("\n".join([pt, ps, pt, ps]) + "\n")
    rl = run([lst, res], PLADE_MERGE="0.05")
    assert rl.returncode == 0, rl.stdout + rl.stderr
    assert rl.stdout.count("merge: ") == 2 and not os.path.exists(merged)
    for i in (0, 1):
        rows = plyio.read_ply(res + ".%d.merged.ply" % i)
        assert len(rows) == int([l for l in rl.stdout.split("\n") if l.startswith("merge: ")][i].split()[1])
