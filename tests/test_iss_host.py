"""ISS keypoints, host side (no GPU): the entry points are declared, exported, bound and listed; the default parameters need no GPU;
the structs are the header's; and the numpy restatement of the semantics (tests/iss_restate.py) is exact on lattices, flat
neighbourhoods and a hand-made tie, and its closed-form eigenvalues agree with numpy.linalg.eigvalsh on the clouds of the GPU tests."""
import ctypes
import os
import re
import subprocess

import numpy as np

import plade_amd
import iss_cases
import iss_restate as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("plade_iss_default_params", "plade_cloud_keypoints_iss", "plade_cloud_keypoints_iss_dev", "plade_features_select",
       "plade_register_keypoints", "plade_register_keypoints_dev")


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
    for m in ("iss_keypoints", "iss_keypoints_dev", "select_features", "register_keypoints", "register_keypoints_dev"):
        assert callable(getattr(plade_amd.Context, m))
    assert callable(plade_amd.Features.select)
    for t in ("plade_iss_params", "plade_iss_summary"):
        assert re.search(r"\}\s*" + t + r"\s*;", hdr), t


def test_default_params_need_no_gpu():
    p = plade_amd.IssParams()
    p.salient_radius, p.non_max_radius, p.gamma21, p.gamma32, p.min_neighbours, p.reserved = -1.0, 3.0, 7.0, -2.0, -7, 9
    plade_amd.load_library().plade_iss_default_params(ctypes.byref(p))
    assert (p.salient_radius, p.non_max_radius, p.gamma21, p.gamma32, p.min_neighbours, p.reserved) == (0.0, 0.0, 0.975, 0.975, 5, 0)
    assert plade_amd.iss_default_params() == {"salient_radius": 0.0, "non_max_radius": 0.0, "gamma21": 0.975, "gamma32": 0.975,
                                              "min_neighbours": 5}


C_PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "plade_hip.h"
int main(void) {
    plade_iss_params p; plade_iss_summary s; plade_features *f = 0; plade_features **o = &f;
    (void)o; s.keypoints = 0;
    printf("%d %d %d %d %d %d %d ", (int)sizeof(p), (int)offsetof(plade_iss_params, salient_radius),
           (int)offsetof(plade_iss_params, non_max_radius), (int)offsetof(plade_iss_params, gamma21),
           (int)offsetof(plade_iss_params, gamma32), (int)offsetof(plade_iss_params, min_neighbours),
           (int)offsetof(plade_iss_params, reserved));
    printf("%d %d %d %d %d %d\n", (int)sizeof(s), (int)offsetof(plade_iss_summary, n), (int)offsetof(plade_iss_summary, salient),
           (int)offsetof(plade_iss_summary, keypoints), (int)offsetof(plade_iss_summary, max_count),
           (int)offsetof(plade_iss_summary, reserved));
    return (int)s.keypoints;
}
"""


def test_structs_match_a_c99_compile_of_the_header(tmp_path):
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text(C_PROBE)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                        str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P, S = plade_amd.IssParams, plade_amd.IssSummary
    assert [f for f, _ in P._fields_] == ["salient_radius", "non_max_radius", "gamma21", "gamma32", "min_neighbours", "reserved"]
    assert [f for f, _ in S._fields_] == ["n", "salient", "keypoints", "max_count", "reserved"]
    mine = [ctypes.sizeof(P)] + [getattr(P, f).offset for f, _ in P._fields_] + [ctypes.sizeof(S)] + [getattr(S, f).offset
                                                                                                    for f, _ in S._fields_]
    assert got == mine == [40, 0, 8, 16, 24, 32, 36, 32, 0, 8, 16, 24, 28]


# The tests below pin the restatement alone (its own sanity, before the GPU tests lean on it): they run no library code.
def test_restatement_is_exact_on_a_cubic_lattice():
    """8 x 8 x 8, pitch 2^-3, rs = 0.3: the offsets with |k|^2 <= 5 pitches^2 (57 of them for an interior point)"""
    cloud = iss_cases.cubic_lattice()
    out = I.iss(cloud, 0.3)
    g = (cloud / 0.125).astype(np.int64)
    interior = ((g >= 2) & (g <= 5)).all(axis=1)
    assert interior.sum() == 64 and (out["count"][interior] == 57).all() and out["count"].min() == 17      # a corner
    M = out["scatter"][interior]
    # sum of k_x^2 over the 57 offsets = 66, times pitch^2: exact dyadic numbers, whatever the order of the sum
    assert (M[:, [0, 3, 5]] == 66 * 0.125 ** 2).all() and (M[:, [1, 2, 4]] == 0).all()
    L = out["eigenvalues"][interior]
    assert (L[:, 0] == L[:, 1]).all() and (L[:, 1] == L[:, 2]).all()
    # Nothing is salient where the neighbourhood is cut by at most one face of the cube: two of the three eigenvalues stay equal
    # there by symmetry, and gamma = 0.975 refuses a ratio of 1.  Along the cube's edges the neighbourhood is a quarter ball with
    # the eigenvalues a + e, a - e, b: those points are salient by geometry, not by rounding (none of them is borderline).
    depth = np.minimum(g, 7 - g)
    cut = (depth < 2).sum(axis=1)
    assert (cut <= 1).sum() == 256 and not out["salient"][cut <= 1].any() and (out["saliency"][cut <= 1] == 0).all()
    assert not out["edge_near"].any() and out["salient"].sum() == 192 and not out["keypoint"][cut <= 1].any()
    assert I.summary(out) == dict(n=512, salient=192, keypoints=8, max_count=57)


def test_flat_neighbourhoods_are_not_salient():
    """a 32 x 32 planar lattice and a row of 64 points: with both gammas at 1 only the 1e-9 rule stands between a boundary point and
    a salient verdict.  On the plane l3 is 0 to a few ulp of l1.  On the row l2 = l3 = 0 is a double root, where the closed form is
    good to sqrt(ulp) only (r = 1 - ulp gives phi = 1e-8): l3 comes out at -4e-9 l1 -- on the low side, where the cosine puts it."""
    for cloud, tol in ((iss_cases.planar_lattice(), 1e-14), (iss_cases.point_row(), 1e-7)):
        out = I.iss(cloud, 0.1, gamma21=1.0, gamma32=1.0)
        L = out["eigenvalues"]
        assert (L[:, 0] > 0).all() and (np.abs(L[:, 2]) <= tol * L[:, 0]).all() and (L[:, 2] <= I.FLAT * L[:, 0]).all()
        assert not out["salient"].any() and not out["keypoint"].any()


def test_a_coincident_pair_ties_and_the_smaller_index_wins():
    cloud = iss_cases.tie_cloud()
    out = I.iss(cloud, 1.0, 0.5, min_neighbours=1)
    a, b = iss_cases.TIE_PAIR
    assert a < b and out["salient"][[a, b]].all() and out["saliency"][a] == out["saliency"][b] > 0
    assert np.array_equal(out["scatter"][a], out["scatter"][b]) and out["count"][a] == out["count"][b]
    assert out["keypoint"][a] and not out["keypoint"][b]
    assert out["unsure"][[a, b]].all()                        # an exact tie is a near tie: the flag is for rounding, the rule holds
    # the far point has two neighbours, itself included: below three no eigenvalue makes it salient
    f = iss_cases.TIE_LONELY
    assert out["count"][f] == 2 and out["eigenvalues"][f, 0] > 0 and not out["salient"][f] and out["saliency"][f] == 0
    # min_neighbours goes through m - 1: the pair sees each other and nothing else within 0.5
    assert out["nms_count"][a] == 2 and not I.iss(cloud, 1.0, 0.5, min_neighbours=2)["keypoint"].any()


def test_closed_form_eigenvalues_against_eigvalsh():
    """Where the three eigenvalues are apart (by 1e-3 l1) the closed form loses some 50 ulp of l1; at a double root -- the 16 points
    of the scene with one neighbour, l2 = l3 = 0 -- it is good to sqrt(ulp): acos near 1 turns an ulp of r into 1e-8 of phi."""
    worst, worst_apart = 0.0, 0.0
    for name, cloud, rs, rn, gamma in iss_cases.gpu_cases():
        out = iss_cases.restated(name, rs, rn, gamma)
        M, c, L = out["scatter"], out["count"], out["eigenvalues"]
        C = np.stack([M[:, [0, 1, 2]], M[:, [1, 3, 4]], M[:, [2, 4, 5]]], axis=1) / c[:, None, None]
        ref = np.linalg.eigvalsh(C)[:, ::-1]
        ok = ref[:, 0] > 0
        assert ok.sum() >= 0.9 * len(cloud)                   # (l1 = 0: a point alone within rs)
        err = np.abs(L[ok] - ref[ok]).max(axis=1) / ref[ok, 0]
        apart = ((ref[ok, 0] - ref[ok, 1]) > 1e-3 * ref[ok, 0]) & ((ref[ok, 1] - ref[ok, 2]) > 1e-3 * ref[ok, 0])
        assert apart.sum() >= 0.9 * len(cloud)
        worst, worst_apart = max(worst, float(err.max())), max(worst_apart, float(err[apart].max()))
    print("closed form against eigvalsh, worst |dl| / l1: all points", worst, "eigenvalues apart", worst_apart)
    assert worst < 1e-7 and worst_apart < 1e-12               # (measured 5.7e-9 and 1.2e-14)
