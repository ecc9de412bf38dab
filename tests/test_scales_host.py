"""Multi-scale normals and dimensionality features, host side (no GPU): the entry points are declared, exported, bound and listed; the
header with the new structs is plain C99; the default parameters need no GPU; and the numpy restatement of the semantics
(tests/scales_restate.py) reacts to the mutations a wrong kernel would make: a radius one ulp off, two scales' criteria swapped, and the wrong sense of a criterion."""
import ctypes
import os
import re
import subprocess

import numpy as np

import plade_amd
import scales_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("plade_scale_default_params", "plade_cloud_scale_features", "plade_cloud_scale_normals_dev")


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
    for m in ("scale_features", "scale_normals_dev"):
        assert callable(getattr(plade_amd.Context, m))
    for t in ("plade_scale_params", "plade_scale_summary"):
        assert re.search(r"\}\s*" + t + r"\s*;", hdr), t


def test_default_params_need_no_gpu():
    p = plade_amd.ScaleParams()
    p.radii[:] = [9.0] * 8
    p.scales, p.min_neighbours, p.mode, p.orient, p.reserved = 5, -7, 3, 4, 9
    p.viewpoint[:] = [1.0, 2.0, 3.0]
    plade_amd.load_library().plade_scale_default_params(ctypes.byref(p))
    assert tuple(p.radii) == (0.0,) * 8 and tuple(p.viewpoint) == (0.0, 0.0, 0.0)
    assert (p.scales, p.min_neighbours, p.mode, p.orient, p.reserved) == (0, 6, 0, 0, 0)
    assert plade_amd.scale_default_params() == {"radii": (0.0,) * 8, "scales": 0, "min_neighbours": 6, "mode": 0, "orient": 0,
                                                "viewpoint": (0.0, 0.0, 0.0)}


def test_structs_match_the_header():
    P, Q = plade_amd.ScaleParams, plade_amd.ScaleSummary
    assert [f for f, _ in P._fields_] == ["radii", "scales", "min_neighbours", "mode", "orient", "viewpoint", "reserved"]
    assert ctypes.sizeof(P) == 96 and P.scales.offset == 64 and P.orient.offset == 76 and P.viewpoint.offset == 80 and P.reserved.offset == 92
    assert [f for f, _ in Q._fields_] == ["queries", "fitted", "chosen_hist", "max_count", "reserved"]
    assert ctypes.sizeof(Q) == 56 and Q.chosen_hist.offset == 16 and Q.max_count.offset == 48


def test_the_header_with_the_new_structs_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "plade_hip.h"\n'
                   'int main(void) { plade_scale_params p; plade_scale_summary s; plade_cloud *out = 0; int rc;\n'
                   '  plade_scale_default_params(&p); s.fitted = 0;\n'
                   '  rc = plade_cloud_scale_features(0, 0, 0, 3, 0, 0, &p, 0, 0, 0, 0, 0, 0, 0, 0, &s);\n'
                   '  rc += plade_cloud_scale_normals_dev(0, 0, 0, 0, &p, &out, &s);\n'
                   '  return (int)(sizeof(p) + sizeof(s) + s.fitted + (unsigned)rc) & 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# The tests below pin the restatement alone (its own sanity, before the GPU tests lean on it): they run no library code.
def test_restatement_counts_the_point_itself_and_each_scale_uses_its_own_strict_bound():
    r0, r1 = np.float32(0.25), np.float32(0.375)                                   # both squares are exact in fp32
    P = np.array([[0, 0, 0], [r1, 0, 0]], np.float32)
    assert R.moments(P, (r0, r1))[0].tolist() == [[1, 1], [1, 1]]                  # d = r2 of scale 1: not neighbours
    P[1, 0] = np.nextafter(r1, np.float32(0))
    count, mom, mag = R.moments(P, (r0, r1))
    assert count.tolist() == [[1, 2], [1, 2]]                                      # one ulp closer: neighbours at scale 1 alone
    assert mom[0, 0].tolist() == [0.0] * 9 and mom[0, 1, 0] == float(P[1, 0]) and mom[0, 1, 3] == float(P[1, 0]) ** 2


def test_restatement_mutation_a_radius_one_ulp_off_changes_a_count():
    r0, r1 = np.float32(0.25), np.float32(0.375)
    P = np.array([[0, 0, 0], [r1, 0, 0]], np.float32)
    exact = R.moments(P, (r0, r1))[0]
    wider = R.moments(P, (r0, np.nextafter(r1, np.float32(1))))[0]
    assert exact.tolist() == [[1, 1], [1, 1]] and wider.tolist() == [[1, 2], [1, 2]]
    P[1, 0] = np.nextafter(r0, np.float32(0))
    assert R.moments(P, (r0, r1))[0].tolist() == [[2, 2], [2, 2]]
    assert R.moments(P, (np.nextafter(r0, np.float32(0)), r1))[0].tolist() == [[1, 2], [1, 2]]


def test_restatement_x_window_changes_no_pair():
    rng = np.random.default_rng(9)
    P = (rng.random((3000, 3)) * np.array([4.0, 1.0, 0.5]) + 50.0).astype(np.float32)
    P[::50] = P[1::50]                                                             # duplicates
    for q in (None, np.arange(0, 3000, 7)):
        for r2 in R.radii2((0.05, 0.2)):
            a, b = R.pairs_within(P, r2, q, rows=200), R.pairs_within(P, r2, q, window=False)
            assert len(a[0]) > 3000 // (1 if q is None else 7) and all(np.array_equal(x, y) for x, y in zip(a, b))
            assert (np.diff(a[0]) >= 0).all() and (np.diff(a[1])[np.diff(a[0]) == 0] > 0).all()       # ascending in (t, j)


def rough_patch(seed=2):
    """a plane with fine relief: rough at the small radius, flat at the large ones"""
    rng = np.random.default_rng(seed)
    P = np.empty((1500, 3), np.float32)
    P[:, :2] = rng.random((1500, 2))
    P[:, 2] = 0.02 * rng.standard_normal(1500)
    return P


def test_restatement_chooses_the_flatter_scale_and_the_mutated_criterion_another():
    P = rough_patch()
    ref = R.scales(P, (0.05, 0.1, 0.2), mode=0, viewpoint=(0.5, 0.5, 10.0))
    inner = (np.abs(P[:, :2] - 0.5) < 0.25).all(axis=1) & ref["fitted"].all(axis=1)
    assert inner.sum() > 100
    assert (ref["chosen"][inner] == 2).mean() > 0.9                                # relief of 0.02: the plane shows at r = 0.2
    F = ref["features"]
    assert np.allclose(F[inner][..., :3].sum(-1), 1.0, atol=1e-12)                 # linearity + planarity + sphericity = 1
    n = ref["normal"][inner & (ref["chosen"] == 2)]
    assert (n[:, 2] > 0.95).all()                                                  # toward the viewpoint above the plane
    # mutation: the two modes' criteria swapped (the largest variation instead of the smallest) choose another scale
    swapped = R.choose(F[..., 3], ref["fitted"])
    honest = R.choose(R.criterion(F, 1), ref["fitted"])
    assert (swapped[inner] != honest[inner]).mean() > 0.9
    assert (honest[inner] == 2).mean() > 0.9
    # mutation: two scales' criteria swapped (columns 0 and 2 of the criterion) change chosen wherever either of them was chosen
    crit = R.criterion(F, 0)
    mixed = R.choose(crit[:, [2, 1, 0]], ref["fitted"])
    was = inner & (ref["chosen"] != 1)
    assert was.sum() > 100 and (mixed[was] != ref["chosen"][was]).mean() > 0.9 and np.array_equal(R.choose(crit, ref["fitted"]), ref["chosen"])
    # ties keep the smaller radius; no fitted scale: -1
    assert R.choose(np.array([[0.5, 0.5, 0.5]]), np.array([[False, True, True]])).tolist() == [1]
    assert R.choose(np.array([[0.5, 0.7, 0.6]]), np.array([[True, True, True]])).tolist() == [1]
    assert R.choose(np.array([[0.5, 0.7, 0.6]]), np.array([[False, False, False]])).tolist() == [-1]


def test_restatement_marks_ties_and_minimal_degenerate_neighbourhoods_unsure():
    crit = np.array([[0.3, 0.3 + 5e-10, 0.9], [0.3, 0.4, 0.9], [0.3, 0.3, 0.9]])
    fit = np.array([[True, True, True], [True, True, True], [True, False, True]])
    L = np.tile(np.array([1.0, 0.5, 0.1]), (3, 3, 1))
    count = np.full((3, 3), 50)
    assert R.unsure(crit, fit, count, L).tolist() == [True, False, False]
    count[1, 0], L[1, 0] = 6, (1.0, 0.0, 0.0)                                      # six collinear neighbours
    assert R.unsure(crit, fit, count, L).tolist() == [True, True, False]


def test_restatement_orientation_falls_back_to_the_viewpoint():
    P = np.zeros((4, 3), np.float32)
    N = np.tile(np.array([0.0, 0.0, 1.0]), (4, 1, 1))
    g = np.array([[0, 0, -1], [0, 0, 1], [1, 0, 0], [np.nan, 0, 1]], np.float32)   # against, along, orthogonal, not finite
    assert R.flips(P, N, (0, 0, -5.0), g)[:, 0].tolist() == [True, False, True, True]
    assert R.flips(P, N, (0, 0, 5.0), g)[:, 0].tolist() == [True, False, False, False]
    assert R.flips(P, N, (0, 0, -5.0))[:, 0].tolist() == [True] * 4


def test_restated_eigenvalues_agree_with_eigh_and_with_long_double():
    P = rough_patch(3)
    count, mom, mag = R.moments(P, (0.1, 0.2))
    C = R.covariance(mom, count)
    L, LL = R.sym3(C), R.sym3(C.astype(np.longdouble), np.longdouble)
    A = np.empty(C.shape[:-1] + (3, 3))
    for e, (a, b) in enumerate(R.UPPER):
        A[..., a, b] = A[..., b, a] = C[..., e]
    lam = np.linalg.eigvalsh(A)[..., ::-1]
    assert np.abs(L - lam).max() <= 1e-12 * np.abs(lam).max()
    assert np.abs(L - LL.astype(np.float64)).max() <= 1e-12 * np.abs(lam).max()
