"""Cloud merge, host side (no GPU): the entry points are declared, exported, bound and listed; the summary struct matches the
header; the numpy restatement of the semantics (tests/merge_restate.py) agrees with an independent plain-Python loop, and for one
cloud under the identity with the oracle's voxel grid."""
import ctypes
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import plade_amd
import merge_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("plade_merge_clouds", "plade_merge_clouds_dev", "plade_cloud_download")


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
    for m in ("merge_clouds", "merge_clouds_dev"):
        assert callable(getattr(plade_amd.Context, m))
    assert callable(plade_amd.Cloud.download)
    assert re.search(r"\}\s*plade_merge_summary\s*;", hdr)


def test_struct_matches_the_header():
    S = plade_amd.MergeSummary
    assert [f for f, _ in S._fields_] == ["n_in", "n_out", "n_shared", "max_count", "reserved"]
    assert ctypes.sizeof(S) == 32 and S.n_out.offset == 8 and S.n_shared.offset == 16 and S.max_count.offset == 24 and S.reserved.offset == 28


def test_the_header_with_the_new_struct_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "plade_hip.h"\nint main(void) { plade_merge_summary s; s.n_out = 0; s.max_count = 0;\n'
                   '  return (int)(sizeof(s) + s.n_out + s.max_count) & 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def _loop_merge(clouds, transforms, leaf):
    """The semantics once more with Python floats (fp64) and explicit float32 roundings, no numpy arithmetic."""
    pts = []
    for c, (rows, T) in enumerate(zip(clouds, transforms)):
        T = [[float(v) for v in row] for row in T]
        for r in rows.tolist():
            x, y, z, nx, ny, nz = r
            p = [_f32(_f32(_f32(_f32(T[k][0] * x) + _f32(T[k][1] * y)) + _f32(T[k][2] * z)) + T[k][3]) for k in range(3)]
            n = [_f32(_f32(_f32(T[k][0] * nx) + _f32(T[k][1] * ny)) + _f32(T[k][2] * nz)) if all(map(math.isfinite, (nx, ny, nz)))
                 else float("nan") for k in range(3)]
            pts.append((c, p, n))
    inv = _f32(1.0 / _f32(leaf))
    lo = [math.floor(_f32(min(p[1][k] for p in pts) * inv)) for k in range(3)]
    vox = {}
    for c, p, n in pts:       # ascending (cloud, index)
        i, j, k = (math.floor(_f32(p[a] * inv)) - lo[a] for a in range(3))
        v = vox.setdefault((k, j, i), [0, [0.0] * 3, [0.0] * 3, 0, 0])
        v[0] += 1
        for a in range(3):
            v[1][a] += p[a]
        if all(map(math.isfinite, n)):
            for a in range(3):
                v[2][a] += n[a]
            v[3] += 1
        v[4] |= 1 << c
    rows, count, mask = [], [], []
    for key in sorted(vox):
        cnt, ps, ns, nf, m = vox[key]
        q = (ns[0] * ns[0] + ns[1] * ns[1]) + ns[2] * ns[2]
        nrm = [_f32(s / math.sqrt(q)) for s in ns] if nf and q != 0 else [float("nan")] * 3
        rows.append([_f32(s / cnt) for s in ps] + nrm)
        count.append(cnt)
        mask.append(m)
    return np.array(rows, np.float32), np.array(count, np.uint32), np.array(mask, np.uint32)


def _rot(axis, angle, t):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K
    T[:3, 3] = t
    return T.astype(np.float32)


def test_restatement_against_a_plain_python_loop():
    rng = np.random.default_rng(5)
    a = rng.uniform(-1, 1, (120, 6)).astype(np.float32)
    b = rng.uniform(-1, 1, (80, 6)).astype(np.float32)
    a[::7, 3:] = np.nan
    b[3, 4] = np.nan
    Ts = [_rot((1, 2, 3), 0.3, (0.1, -0.2, 0.05)), _rot((0, 1, 1), -0.2, (0.0, 0.1, 0.0))]
    rows, count, mask, summ = R.merge([a, b], Ts, 0.35)
    lrows, lcount, lmask = _loop_merge([a, b], Ts, 0.35)
    assert R.same_bits(rows, lrows)
    assert np.array_equal(count, lcount) and np.array_equal(mask, lmask)
    assert summ == {"n_in": 200, "n_out": len(lrows), "n_shared": int(((lmask & (lmask - 1)) != 0).sum()), "max_count": int(lcount.max())}
    assert summ["n_shared"] > 0 and summ["max_count"] > 1 and np.isnan(rows[:, 3:]).any() and np.isfinite(rows[:, 3:]).any()


def test_leaf_zero_is_the_transformed_concatenation():
    rng = np.random.default_rng(6)
    a, b = (rng.uniform(-2, 2, (n, 6)).astype(np.float32) for n in (9, 5))
    rows, count, mask, summ = R.merge([a, b], None, 0.0)
    assert np.array_equal(rows[:, :3], np.concatenate([a, b])[:, :3])
    assert (count == 1).all() and np.array_equal(mask, np.r_[np.full(9, 1), np.full(5, 2)].astype(np.uint32))
    assert summ == {"n_in": 14, "n_out": 14, "n_shared": 0, "max_count": 1}
    T = _rot((1, 0, 0), 0.5, (1, 2, 3))
    rows2 = R.merge([a], [T], 0.0)[0]
    assert np.allclose(rows2[:, :3], a[:, :3] @ T[:3, :3].T + T[:3, 3], atol=1e-5)
    assert np.allclose(rows2[:, 3:], a[:, 3:] @ T[:3, :3].T, atol=1e-5)


def test_one_cloud_identity_against_the_oracle_voxel_grid():
    from oracle.oracle import Oracle
    rng = np.random.default_rng(7)
    pts = rng.uniform(-3, 5, (5000, 6)).astype(np.float32)
    leaf = 0.9
    rows, count, mask, summ = R.merge([pts], None, leaf)
    ref = Oracle().voxel_downsample(pts[:, :3], leaf, sort_mode=1)
    # the same number of voxels, the counts of the voxel keys in ascending (k, j, i) ...
    assert len(ref) == len(rows) == summ["n_out"]
    ijk = R.voxel_ijk(pts[:, :3], leaf)
    key = ijk[:, 0] + (ijk[:, 1] << 18) + (ijk[:, 2] << 36)
    assert np.array_equal(count, np.unique(key, return_counts=True)[1])
    # ... and row by row (so: the same voxels in the same order) positions within the fp32 sequential-sum bound of the oracle's
    # fp32 centroid, (m + 1) 2^-24 max|coordinate|; the restatement's fp64 sum is the more exact of the two
    m = int(count.max())
    bound = (m + 1) * 2.0 ** -24 * float(np.abs(pts[:, :3]).max())
    assert np.abs(rows[:, :3].astype(np.float64) - ref.astype(np.float64)).max() <= bound
    assert (mask == 1).all() and summ["n_shared"] == 0 and summ["max_count"] == m


@pytest.mark.parametrize("kw, code", [
    (dict(clouds=[]), R.EINVAL), (dict(clouds=[np.zeros((1, 6), np.float32)] * 17), R.EINVAL),
    (dict(clouds=[np.zeros((0, 6), np.float32)]), R.EINVAL), (dict(clouds=[None]), R.EINVAL),
    (dict(clouds=[np.full((2, 6), np.inf, np.float32)]), R.EINVAL),
    (dict(clouds=[np.zeros((2, 6), np.float32)], transforms=[np.full((4, 4), np.nan)]), R.EINVAL),
    (dict(clouds=[np.zeros((2, 6), np.float32)], leaf=-1.0), R.EINVAL), (dict(clouds=[np.zeros((2, 6), np.float32)], leaf=np.nan), R.EINVAL),
    (dict(clouds=[np.array([[0, 0, 0, 0, 0, 1], [300, 0, 0, 0, 0, 1]], np.float32)], leaf=0.001), R.ELIMIT),
])
def test_restatement_errors(kw, code):
    with pytest.raises(R.MergeError) as e:
        R.merge(**kw)
    assert e.value.code == code
