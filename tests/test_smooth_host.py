"""Smoothing, host side (no GPU): the entry points are declared, exported, bound and listed; the default parameters need no GPU;
and the numpy restatement of the semantics (tests/smooth_restate.py) leaves an exact plane where it is and finds its normal."""
import ctypes
import os
import re
import subprocess

import numpy as np

import plade_amd
import smooth_restate as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("plade_smooth_default_params", "plade_smooth_cloud", "plade_cloud_smooth_dev")


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
    for m in ("smooth_cloud", "smooth_cloud_dev"):
        assert callable(getattr(plade_amd.Context, m))
    for t in ("plade_smooth_params", "plade_smooth_summary"):
        assert re.search(r"\}\s*" + t + r"\s*;", hdr), t


def test_default_params_need_no_gpu():
    p = plade_amd.SmoothParams()
    p.radius, p.min_neighbours, p.reserved = -1.0, -7, 9
    p.viewpoint[:] = [1.0, 2.0, 3.0]
    plade_amd.load_library().plade_smooth_default_params(ctypes.byref(p))
    assert (p.radius, p.min_neighbours, tuple(p.viewpoint), p.reserved) == (0.0, 6, (0.0, 0.0, 0.0), 0)
    assert plade_amd.smooth_default_params() == {"radius": 0.0, "min_neighbours": 6, "viewpoint": (0.0, 0.0, 0.0)}


def test_structs_match_the_header():
    P, Q = plade_amd.SmoothParams, plade_amd.SmoothSummary
    assert [f for f, _ in P._fields_] == ["radius", "min_neighbours", "viewpoint", "reserved"]
    assert ctypes.sizeof(P) == 32 and P.min_neighbours.offset == 8 and P.viewpoint.offset == 12 and P.reserved.offset == 24
    assert [f for f, _ in Q._fields_] == ["n", "fitted", "rms", "max", "max_count", "reserved"]
    assert ctypes.sizeof(Q) == 40 and Q.rms.offset == 16 and Q.max_count.offset == 32


def test_the_header_with_the_new_structs_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "plade_hip.h"\nint main(void) { plade_smooth_params p; plade_smooth_summary s; plade_smooth_default_params(&p);\n'
                   '  s.fitted = 0; return (int)(sizeof(p) + sizeof(s) + s.fitted) & 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def plane(n=2000, seed=5):
    """n points on z = 0.5 with x, y multiples of 2^-10 in [0, 1): every sum of the fit is exact in z"""
    rng = np.random.default_rng(seed)
    P = np.empty((n, 3), np.float32)
    P[:, :2] = rng.integers(0, 1024, (n, 2)).astype(np.float32) / np.float32(1024.0)
    P[:, 2] = 0.5
    return P


# The two tests below pin the restatement alone (its own sanity, before the GPU tests lean on it): they run no library code.
def test_restatement_leaves_an_exact_plane_where_it_is():
    P = plane()
    ref = S.smooth(P, 0.1, viewpoint=(0.5, 0.5, 10.0))
    f = ref["fitted"]
    assert f.sum() > 0.9 * len(P) and (ref["count"][f] >= 6).all()
    assert (ref["delta"][f] == 0).all() or np.abs(ref["delta"][f]).max() < 1e-15
    assert np.array_equal(ref["xyz"].view(np.uint32), P.view(np.uint32))
    assert np.abs(ref["normal"][f] - np.array([0.0, 0.0, 1.0])).max() <= 1e-12     # toward the viewpoint above the plane
    assert np.abs(ref["curvature"][f]).max() <= 1e-15
    assert np.isnan(ref["normal"][~f]).all() and (ref["delta"][~f] == 0).all()
    below = S.smooth(P, 0.1, viewpoint=(0.5, 0.5, -10.0))
    assert np.abs(below["normal"][f] - np.array([0.0, 0.0, -1.0])).max() <= 1e-12


def test_restatement_counts_the_point_itself_and_uses_a_strict_bound():
    r = np.float32(0.375)
    P = np.array([[0, 0, 0], [r, 0, 0]], np.float32)
    assert list(S.smooth(P, r)["count"]) == [1, 1]                                 # d = r2: not neighbours
    P[1, 0] = np.nextafter(r, np.float32(0))
    out = S.smooth(P, r, min_neighbours=3)
    assert list(out["count"]) == [2, 2] and not out["fitted"].any()
    assert np.array_equal(out["xyz"].view(np.uint32), P.view(np.uint32))
