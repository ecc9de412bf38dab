"""FPFH descriptors and their match, host side (no GPU): the entry points are declared, exported, bound and listed; the default
parameters need no GPU; and the numpy restatement of the semantics (tests/fpfh_restate.py) is exact on a lattice and on a hand-made
match table."""
import ctypes
import os
import re
import subprocess

import numpy as np

import plade_amd
import fpfh_restate as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("plade_fpfh_default_params", "plade_cloud_fpfh", "plade_cloud_fpfh_dev", "plade_features_free",
       "plade_feature_match_default_params", "plade_match_features", "plade_match_features_dev")


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
    for m in ("fpfh", "fpfh_dev", "match_features", "match_features_dev"):
        assert callable(getattr(plade_amd.Context, m))
    assert callable(plade_amd.Features.free)
    for t in ("plade_fpfh_params", "plade_fpfh_summary", "plade_feature_match_params"):
        assert re.search(r"\}\s*" + t + r"\s*;", hdr), t


def test_default_params_need_no_gpu():
    p = plade_amd.FpfhParams()
    p.radius, p.min_pairs, p.reserved = -1.0, -7, 9
    plade_amd.load_library().plade_fpfh_default_params(ctypes.byref(p))
    assert (p.radius, p.min_pairs, p.reserved) == (0.0, 5, 0)
    assert plade_amd.fpfh_default_params() == {"radius": 0.0, "min_pairs": 5}
    q = plade_amd.FeatureMatchParams()
    q.mutual, q.max_ratio = 7, -3.0
    plade_amd.load_library().plade_feature_match_default_params(ctypes.byref(q))
    assert (q.mutual, q.max_ratio) == (1, 0.0)
    assert plade_amd.feature_match_default_params() == {"mutual": 1, "max_ratio": 0.0}


def test_structs_match_the_header():
    P, S, M = plade_amd.FpfhParams, plade_amd.FpfhSummary, plade_amd.FeatureMatchParams
    assert [f for f, _ in P._fields_] == ["radius", "min_pairs", "reserved"]
    assert ctypes.sizeof(P) == 16 and P.min_pairs.offset == 8 and P.reserved.offset == 12
    assert [f for f, _ in S._fields_] == ["n", "described", "mean_pairs", "max_pairs", "reserved"]
    assert ctypes.sizeof(S) == 32 and S.described.offset == 8 and S.mean_pairs.offset == 16 and S.max_pairs.offset == 24
    assert [f for f, _ in M._fields_] == ["mutual", "max_ratio"]
    assert ctypes.sizeof(M) == 8 and M.max_ratio.offset == 4


def test_the_header_with_the_new_structs_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "plade_hip.h"\nint main(void) { plade_fpfh_params p; plade_fpfh_summary s; plade_feature_match_params m;\n'
                   '  plade_features *f = 0; plade_fpfh_default_params(&p); plade_feature_match_default_params(&m); plade_features_free(f);\n'
                   '  s.described = 0; return (int)(sizeof(p) + sizeof(s) + sizeof(m) + s.described) & 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


PITCH = 2.0 ** -5
LATTICE_R = 0.1


def lattice():
    """A 32 x 32 lattice of pitch 2^-5 at z = 0.5 with the normals (0, 0, 1)."""
    g = np.arange(32, dtype=np.float32) * np.float32(PITCH)
    x, y = np.meshgrid(g, g, indexing="ij")
    n = 32 * 32
    return np.ascontiguousarray(np.stack([x.ravel(), y.ravel(), np.full(n, 0.5, np.float32), np.zeros(n, np.float32),
                                          np.zeros(n, np.float32), np.ones(n, np.float32)], axis=1).astype(np.float32))


def check_lattice(out):
    """The exact answer on lattice(): `out` is a dict with spfh, pairs, described and desc."""
    H, c = np.asarray(out["spfh"]).astype(np.int64), np.asarray(out["pairs"]).astype(np.int64)
    m = np.asarray(out["described"], bool)
    assert m.all() and c.min() == 12 and c.max() == 36      # a corner, an interior point: the lattice points with 0 < d2 < 10.24 pitch^2
    on = np.zeros(33, bool)
    on[[5, 16, 27]] = True
    assert (H[:, on] == c[:, None]).all() and (H[:, ~on] == 0).all()
    d = np.asarray(out["desc"]).astype(np.float64)
    assert (d[:, ~on] == 0).all() and (np.abs(d[:, on] - 100.0) <= 100.0 * 1e-12).all()


# The tests below pin the restatement alone (its own sanity, before the GPU tests lean on it): they run no library code.
def test_restatement_is_exact_on_a_lattice():
    cloud = lattice()
    i, j, d, r2 = F.neighbour_pairs(cloud, LATTICE_R)
    counted, b1, b2, b3, near = F.pair_features(cloud, i, j)
    assert counted.all() and (b1 == 5).all() and (b2 == 5).all() and (b3 == 5).all() and not near.any()
    out = F.fpfh(cloud, LATTICE_R)
    check_lattice(out)
    assert not out["edge_near"].any() and out["counted_pairs"] == len(i)
    s = F.summary(out["pairs"], out["described"])
    assert (s["n"], s["described"], s["max_pairs"]) == (1024, 1024, 36) and s["mean_pairs"] == out["pairs"].sum() / 1024.0
    blocks = out["desc"].astype(np.float64).reshape(1024, 3, 11)
    assert (np.abs((blocks[:, :, 0] + blocks[:, :, 1:].sum(axis=2)) - 100.0) < 1e-4).all()


def test_restatement_skips_missing_axes_coincident_points_and_parallel_pairs():
    cloud = lattice()
    cloud[40, 3:] = 0.0
    cloud[41, 4] = np.nan
    cloud[42, 3:] = (0.0, 0.0, -3.5)                          # not unit, flipped: an axis all the same
    cloud[43, :3] = cloud[44, :3]                             # coincident with 44: no neighbours of each other
    cloud[100, :3] = (cloud[101, 0], cloud[101, 1], 0.5 + 2 * PITCH)   # straight above 101: dp is parallel to n1
    ref = F.fpfh(lattice(), LATTICE_R)
    out = F.fpfh(cloud, LATTICE_R)
    assert list(np.nonzero(~out["has_axis"])[0]) == [40, 41]
    assert not out["described"][[40, 41]].any() and (out["pairs"][[40, 41]] == 0).all() and np.isnan(out["desc"][[40, 41]]).all()
    assert (out["raw"][[40, 41]] == 0).all()
    # 39 is next to 40 and 41 in its row: both fall out of its count; 42 counts as before
    assert out["pairs"][39] == ref["pairs"][39] - 2 and out["pairs"][42] == ref["pairs"][42] - 2
    i, j, d, _ = F.neighbour_pairs(cloud, LATTICE_R)
    assert not ((i == 43) & (j == 44)).any() and not ((i == 44) & (j == 43)).any()
    assert ((i == 100) & (j == 101)).sum() == 1
    counted = F.pair_features(cloud, i, j)[0]
    assert not counted[(i == 100) & (j == 101)].any() and not counted[(i == 101) & (j == 100)].any()
    few = F.fpfh(lattice(), LATTICE_R, min_pairs=37)          # more than any point has: nothing is described
    assert not few["described"].any() and np.isnan(few["desc"]).all() and np.array_equal(few["spfh"], ref["spfh"])


def match_table():
    """Sources and targets with exact ties, duplicated rows and NaN rows."""
    T = np.zeros((7, 33), np.float32)
    T[0, 0] = 1.0
    T[1, 0] = 3.0                    # as far from S[0] as T[0] on the other side: the tie goes to index 0
    T[2] = np.nan
    T[3, 5] = 2.0
    T[4, 5] = 2.0                    # a duplicate of T[3]
    T[5, 0], T[5, 1] = 0.0, np.nan   # valid by its first value, NaN further in: passed over
    T[6, 32] = 8.0
    S = np.zeros((6, 33), np.float32)
    S[0, 0] = 2.0
    S[1] = np.nan
    S[2, 5] = 2.0
    S[3, 32] = 7.0
    S[4, 0] = 1.0
    S[5, 0] = 1.0                    # a duplicate of S[4]
    return S, T


def test_restated_match_on_a_hand_made_table():
    S, T = match_table()
    m = F.match(S, T, mutual=False)
    assert list(m["nn"]) == [0, -1, 3, 6, 0, 0]
    assert np.array_equal(m["d2"][0], [1.0, 1.0]) and np.isnan(m["d2"][1]).all()
    assert np.array_equal(m["d2"][2], [0.0, 0.0]) and np.array_equal(m["d2"][3], [1.0, 50.0]) and np.array_equal(m["d2"][4], [0.0, 4.0])
    assert list(m["back"]) == [4, 0, -1, 2, 2, -1, 3]         # T[5]: every delta is NaN
    assert m["corr"].tolist() == [[0, 0], [2, 3], [3, 6], [4, 0], [5, 0]]
    assert F.match(S, T, mutual=True)["corr"].tolist() == [[2, 3], [3, 6], [4, 0]]
    # the ratio test: 0 < r r 0 fails (S[2]), 1 < 0.25 * 50 holds, 0 < 0.25 * 4 holds; S[0]: 1 < 0.25 * 1 fails
    assert F.match(S, T, mutual=False, max_ratio=0.5)["corr"].tolist() == [[3, 6], [4, 0], [5, 0]]
    one = F.match(S[:1], T[:1], mutual=True, max_ratio=0.5)   # no second neighbour: kept
    assert one["corr"].tolist() == [[0, 0]] and one["d2"][0, 0] == 1.0 and np.isnan(one["d2"][0, 1])
    none = F.match(S, np.full((3, 33), np.nan, np.float32))
    assert (none["nn"] == -1).all() and (none["back"] == -1).all() and len(none["corr"]) == 0
