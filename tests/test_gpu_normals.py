"""Normal estimation on the GPU (plade_estimate_normals / plade_cloud_upload_xyz, plade_amd/csrc/k_normals.hip) against a CPU
restatement of its semantics (include/plade_hip.h): brute-force fp32 distances in the library's operation order,
a stable sort on (d, j), fp64 PCA with numpy's eigh.  Neighbour lists must be equal; normals and curvature within tolerances."""
import os
import subprocess

import numpy as np
import pytest

import plade_amd
import icp_restate as IR
import ring_scene
from plade_amd.synth import make_pair, sample_scene
from conftest import GT_TOL, ORIENTED
from test_normals_host import PARENT_RESULT, PARENT_STDERR, PARENT_STDOUT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "plade_amd", "PLADE")


@pytest.fixture(scope="module")
def nctx():
    c = plade_amd.Context(0, **ORIENTED)
    yield c
    c.close()


# ---- the CPU restatement ------------------------------------------------------------------------------------------------------
def d2_fp32(q, P):
    """flann_d2(q, p) for every p: ((qx - px)^2 + (qy - py)^2) + (qz - pz)^2, each step rounded to fp32"""
    q = q.astype(np.float32)
    ax, ay, az = q[0] - P[:, 0], q[1] - P[:, 1], q[2] - P[:, 2]
    r = ax * ax
    r = r + ay * ay
    r = r + az * az
    return r


def knn_ref(P, queries, k):
    """neighbour lists (len(queries) x min(k, n)) in ascending (d, j) order"""
    P = np.ascontiguousarray(P[:, :3], np.float32)
    m = min(k, len(P))
    out = np.empty((len(queries), m), np.int64)
    for r, i in enumerate(queries):
        d = d2_fp32(P[i], P)
        t = np.partition(d, m - 1)[m - 1]
        cand = np.nonzero(d <= t)[0]
        order = np.lexsort((cand, d[cand]))
        out[r] = cand[order[:m]]
    return out


def pca_ref(P, i, nbr):
    q = P[nbr, :3].astype(np.float64) - P[i, :3].astype(np.float64)
    c = q - q.mean(0)
    C = c.T @ c / len(nbr)
    w, v = np.linalg.eigh(C)
    return w, v[:, 0]


def angle(u, v):
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    c = abs(u @ v) / (np.linalg.norm(u) * np.linalg.norm(v))
    return float(np.arccos(min(1.0, c)))


def check_against_ref(P, out, curv, nbr, queries, k, view=(0.0, 0.0, 0.0)):
    want = knn_ref(P, queries, k)
    m = want.shape[1]
    got = nbr[queries, :m]
    bad = np.nonzero((got != want).any(1))[0]
    assert len(bad) == 0, f"{len(bad)} of {len(queries)} neighbour lists differ, e.g. query {queries[bad[0]]}: {got[bad[0]]} vs {want[bad[0]]}"
    if m < k:
        assert (nbr[queries, m:] == -1).all()
    checked = 0
    for r, i in enumerate(queries):
        w, v = pca_ref(P, i, want[r])
        s = w.sum()
        if m < 3 or s == 0:
            assert np.isnan(out[i, 3:]).all() and np.isnan(curv[i])
            continue
        assert np.isfinite(out[i, 3:]).all()
        assert abs(curv[i] - max(w[0], 0.0) / s) <= 1e-5
        if (w[1] - w[0]) / s > 1e-3:
            assert angle(out[i, 3:], v) <= 1e-4, (i, out[i, 3:], v)
            checked += 1
    return checked


def scene_xyz(n, seed=1, **kw):
    return np.ascontiguousarray(sample_scene(n, sample_seed=seed, **kw)[:, :3])


def gen_queries(n, count, seed=0):
    return np.sort(np.random.default_rng(seed).choice(n, size=min(count, n), replace=False))


# ---- exact neighbours ---------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
def test_every_query_of_a_20k_scene(nctx):
    P = scene_xyz(20000)
    out, curv, nbr = nctx.estimate_normals(P, k=16, curvature=True, neighbours=True)
    assert np.array_equal(out[:, :3].view(np.uint32), P.view(np.uint32))
    checked = check_against_ref(P, out, curv, nbr, np.arange(len(P)), 16)
    assert checked > 0.8 * len(P)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("offset", [100.0, 500.0])
def test_20k_scene_far_from_the_origin(nctx, offset):
    """The 20k scene moved offset x D away (fp32 coordinates of ~10^4 with a 13 m room): the grid's cell keeps its slack of
    4e-6 max|coordinate|, so the neighbour lists stay exact."""
    P = scene_xyz(20000)
    D = float(np.linalg.norm(P.max(0).astype(np.float64) - P.min(0)))
    P = IR.move(P, IR.frame(offset * D))
    out, curv, nbr = nctx.estimate_normals(P, k=16, curvature=True, neighbours=True)
    assert np.array_equal(out[:, :3].view(np.uint32), P.view(np.uint32))
    checked = check_against_ref(P, out, curv, nbr, gen_queries(len(P), 4000, seed=int(offset)), 16)
    assert checked > 0.8 * 4000


@pytest.mark.parametrize("k", [3, 8, 24, 40, 64])
def test_every_k_path(nctx, k):
    P = scene_xyz(6000, seed=4)
    out, curv, nbr = nctx.estimate_normals(P, k=k, curvature=True, neighbours=True)
    assert nbr.shape == (len(P), k)
    check_against_ref(P, out, curv, nbr, gen_queries(len(P), 1500, seed=k), k)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("n,count", [(1_000_000, 1024), (10_000_000, 256)])
def test_sampled_queries_of_large_scenes(nctx, n, count):
    P = scene_xyz(n, seed=2)
    out, curv, nbr = nctx.estimate_normals(P, k=16, curvature=True, neighbours=True)
    check_against_ref(P, out, curv, nbr, gen_queries(n, count, seed=n), 16)


def test_integer_lattice_with_duplicates(nctx):
    g = np.stack(np.meshgrid(np.arange(14), np.arange(12), np.arange(9), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    dup = g[np.random.default_rng(0).choice(len(g), 300, replace=False)]
    P = np.ascontiguousarray(np.concatenate([g, dup, dup[:50]]))
    for k in (16, 27, 33):
        out, curv, nbr = nctx.estimate_normals(P, k=k, curvature=True, neighbours=True)
        check_against_ref(P, out, curv, nbr, np.arange(len(P)), k)


def test_far_outliers_take_the_ring_path(nctx):
    P = scene_xyz(20000, seed=5)
    far = np.array([[100.0, 3.0, 1.0], [-2.0, 104.0, 0.5], [1.0, 1.0, -100.0], [100.2, 3.1, 1.0], [100.1, 2.9, 1.2]], np.float32)
    P = np.ascontiguousarray(np.concatenate([P[:7000], far, P[7000:]]))
    out, curv, nbr = nctx.estimate_normals(P, k=16, curvature=True, neighbours=True)
    assert nctx.stats()["normals_ring_queries"] >= len(far)
    q = np.concatenate([np.arange(7000, 7005), gen_queries(len(P), 2000, seed=9)])
    check_against_ref(P, out, curv, nbr, np.unique(q), 16)


@pytest.mark.parametrize("k", [8, 64])
def test_the_ring_walk_does_everything(nctx, k):
    """ring_scene.py: the isolated points' blocks span more than 64 rows, grow at least three times, have whole-row and side runs
    and are clipped by the grid's edge (test_ring_scene_host.py)."""
    P = ring_scene.scene()
    out, curv, nbr = nctx.estimate_normals(P, k=k, curvature=True, neighbours=True)
    assert nctx.stats()["normals_ring_queries"] >= ring_scene.N_FAR
    check_against_ref(P, out, curv, nbr, np.arange(len(P)), k)


# ---- normals, orientation, invariance -----------------------------------------------------------------------------------------
def test_orientation_toward_the_viewpoint(nctx):
    P = scene_xyz(30000, seed=6)
    for view in ((0.0, 0.0, 0.0), (3.0, -2.0, 1.0)):
        out = nctx.estimate_normals(P, k=16, viewpoint=view)
        ok = np.isfinite(out[:, 3]).all()
        assert ok
        d = ((np.asarray(view, np.float64) - P.astype(np.float64)) * out[:, 3:].astype(np.float64)).sum(1)
        assert (d >= -1e-6 * np.linalg.norm(np.asarray(view) - P, axis=1)).all()


def test_permutation_and_repetition_are_bitwise(nctx):
    rng = np.random.default_rng(7)
    P = scene_xyz(30000, seed=7, outliers=0.0)
    assert len(np.unique(P, axis=0)) == len(P)
    perm = rng.permutation(len(P))
    a, ca, na = nctx.estimate_normals(P, k=16, curvature=True, neighbours=True)
    b, cb, nb = nctx.estimate_normals(P[perm], k=16, curvature=True, neighbours=True)
    assert np.array_equal(a[perm].view(np.uint32), b.view(np.uint32))
    assert np.array_equal(ca[perm].view(np.uint32), cb.view(np.uint32))
    assert np.array_equal(perm[nb], na[perm])        # row r of the permuted call is point perm[r], its indices name P[perm[.]]
    # a second call, another context, other work in between
    a2 = nctx.estimate_normals(P, k=16)
    assert np.array_equal(a.view(np.uint32), a2.view(np.uint32))
    other = plade_amd.Context(0)
    try:
        other.estimate_normals(scene_xyz(5000, seed=8), k=32)
        a3 = other.estimate_normals(P, k=16)
    finally:
        other.close()
    assert np.array_equal(a.view(np.uint32), a3.view(np.uint32))
    # an N x 6 input (stride 6) is the same cloud
    a4 = nctx.estimate_normals(np.concatenate([P, np.ones_like(P)], 1), k=16)
    assert np.array_equal(a.view(np.uint32), a4.view(np.uint32))


def test_accuracy_against_the_generator(nctx):
    cloud, labels = sample_scene(1_000_000, sample_seed=3, return_labels=True)
    out = nctx.estimate_normals(np.ascontiguousarray(cloud[:, :3]), k=16)
    inl = labels >= 0
    cos = np.abs((out[inl, 3:].astype(np.float64) * cloud[inl, 3:]).sum(1))
    frac = float(np.mean(cos >= 0.95))
    assert frac >= 0.92, frac
    s = nctx.stats()
    assert s["normals_grid_s"] > 0 and s["normals_search_s"] > 0


# ---- degenerate input and errors ----------------------------------------------------------------------------------------------
def test_degenerate_clouds(nctx):
    for n in (1, 2):
        P = np.arange(3 * n, dtype=np.float32).reshape(n, 3)
        out, curv, nbr = nctx.estimate_normals(P, k=16, curvature=True, neighbours=True)
        assert np.isnan(out[:, 3:]).all() and np.isnan(curv).all()
        assert np.array_equal(out[:, :3], P)
        assert (nbr[:, n:] == -1).all() and sorted(nbr[0, :n]) == list(range(n))
    # 40 coincident points far from a plane of others: their 16 neighbours coincide -> NaN
    rng = np.random.default_rng(1)
    plane = np.concatenate([rng.uniform(-1, 1, (2000, 2)), np.zeros((2000, 1))], 1)
    P = np.ascontiguousarray(np.concatenate([plane, np.tile([[5.0, 5.0, 5.0]], (40, 1))]).astype(np.float32))
    out, curv = nctx.estimate_normals(P, k=16, curvature=True)
    assert np.isnan(out[2000:, 3:]).all() and np.isnan(curv[2000:]).all()
    assert np.isfinite(out[:2000, 3:]).all()
    # collinear points: a finite unit normal orthogonal to the line
    t = np.linspace(-3.0, 3.0, 500)
    u = np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    L = np.ascontiguousarray((t[:, None] * u + np.array([0.3, 0.1, 0.2])).astype(np.float32))
    out = nctx.estimate_normals(L, k=16)
    assert np.isfinite(out[:, 3:]).all()
    assert np.allclose(np.linalg.norm(out[:, 3:], axis=1), 1.0, atol=1e-5)
    assert np.abs(out[:, 3:].astype(np.float64) @ u).max() < 1e-3


def test_invalid_arguments_leave_the_context_usable(nctx):
    P = scene_xyz(3000, seed=11)
    bad = P.copy()
    bad[17, 1] = np.nan
    inf = P.copy()
    inf[5, 2] = np.inf
    cases = [(P, 2), (P, 65), (P, 0), (np.zeros((0, 3), np.float32), 16), (bad, 16), (inf, 16)]
    for arr, k in cases:
        with pytest.raises(plade_amd.PladeError) as e:
            nctx.estimate_normals(arr, k=k)
        assert e.value.code == plade_amd.PLADE_EINVAL and str(e.value)
    for view in ((np.nan, 0.0, 0.0), (0.0, np.inf, 0.0)):
        with pytest.raises(plade_amd.PladeError) as e:
            nctx.estimate_normals(P, k=16, viewpoint=view)
        assert e.value.code == plade_amd.PLADE_EINVAL and "viewpoint" in str(e.value)
    for arr, view in ((bad, (0.0, 0.0, 0.0)), (P, (0.0, 0.0, -np.inf))):
        with pytest.raises(plade_amd.PladeError) as e:
            nctx.upload_xyz(arr, k=16, viewpoint=view)
        assert e.value.code == plade_amd.PLADE_EINVAL
    out, curv, nbr = nctx.estimate_normals(P, k=16, curvature=True, neighbours=True)
    check_against_ref(P, out, curv, nbr, gen_queries(len(P), 300), 16)


# ---- the registration path ----------------------------------------------------------------------------------------------------
def _stripped_pair(n, seed):
    tg, sr, T = make_pair(n, seed=seed)
    view_src = np.linalg.inv(T)[:3, 3]           # the target's sensor origin, in the source's frame
    return np.ascontiguousarray(tg[:, :3]), np.ascontiguousarray(sr[:, :3]), T, view_src


def test_device_cloud_registers_like_the_host_array(nctx):
    tx, sx, T, vs = _stripped_pair(60000, seed=1)
    tg = nctx.estimate_normals(tx, k=16)
    sr = nctx.estimate_normals(sx, k=16, viewpoint=vs)
    ok_h, T_h = nctx.registration(tg, sr)
    ct, cs = nctx.upload_xyz(tx, k=16), nctx.upload_xyz(sx, k=16, viewpoint=vs)
    try:
        ok_d, T_d = nctx.registration_dev(ct, cs)
    finally:
        ct.free()
        cs.free()
    assert ok_h == ok_d
    assert np.array_equal(T_h.view(np.uint32), T_d.view(np.uint32))


@pytest.mark.parametrize("seed", [0, 2])
def test_pair_without_normals_registers(nctx, seed):
    tx, sx, T, vs = _stripped_pair(80000, seed)
    tg = nctx.estimate_normals(tx, k=16)
    sr = nctx.estimate_normals(sx, k=16, viewpoint=vs)
    ok, Tr = nctx.registration(tg, sr)
    assert ok
    assert np.linalg.norm(Tr.astype(np.float64) - T) < GT_TOL


def _write_xyz_ply(path, xyz):
    head = f"ply\nformat binary_little_endian 1.0\nelement vertex {len(xyz)}\nproperty float x\nproperty float y\nproperty float z\nend_header\n"
    with open(path, "wb") as f:
        f.write(head.encode())
        f.write(np.ascontiguousarray(xyz, "<f4").tobytes())


@pytest.mark.timeout(600)
def test_cli_estimates_normals_on_request(tmp_path):
    tg, sr, T = make_pair(80000, seed=0)
    # the source in its own frame, with its own sensor at its origin: move it so that the target's origin lands at 0
    vs = np.linalg.inv(T)[:3, 3]
    T_shift = np.eye(4)
    T_shift[:3, 3] = -vs
    src = (sr[:, :3].astype(np.float64) - vs).astype(np.float32)
    pt, ps, res = str(tmp_path / "t.ply"), str(tmp_path / "s.ply"), str(tmp_path / "r.txt")
    _write_xyz_ply(pt, tg[:, :3])
    _write_xyz_ply(ps, src)
    env = dict(os.environ, PLADE_ORIENT_NORMALS="1", PLADE_ESTIMATE_NORMALS="16")
    r = subprocess.run([CLI, pt, ps, res], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "estimated from 16 nearest neighbours" in r.stdout
    rows = [[float(x) for x in line.split()] for line in open(res).read().split("\n")
            if line.strip() and not line.startswith(("target:", "source:", "transformation:", "registration failed"))]
    Tr = np.array(rows, np.float64)
    assert Tr.shape == (4, 4)
    # Tr maps the shifted source onto the target: Tr = T @ inv(T_shift)
    assert np.linalg.norm(Tr @ T_shift - T) < GT_TOL
    # without the variable the same files fail exactly as the parent revision's CLI does
    env0 = dict(os.environ, PLADE_ORIENT_NORMALS="1")
    env0.pop("PLADE_ESTIMATE_NORMALS", None)
    r0 = subprocess.run([CLI, pt, ps, str(tmp_path / "r0.txt")], capture_output=True, text=True, timeout=300, env=env0)
    assert (r0.returncode, r0.stdout, r0.stderr) == (1, PARENT_STDOUT.format(t=pt, s=ps), PARENT_STDERR)
    assert open(str(tmp_path / "r0.txt")).read() == PARENT_RESULT
