"""M3C2 distances, host side (no GPU): the entry points are declared, exported, bound and listed; the default parameters need no
GPU; and the numpy restatement of the semantics (tests/m3c2_restate.py) is exact on two exact planes."""
import ctypes
import os
import re
import subprocess

import numpy as np

import plade_amd
import m3c2_restate as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("plade_m3c2_default_params", "plade_cloud_m3c2", "plade_cloud_m3c2_dev")


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
    for m in ("m3c2", "m3c2_dev"):
        assert callable(getattr(plade_amd.Context, m))
    for t in ("plade_m3c2_params", "plade_m3c2_summary"):
        assert re.search(r"\}\s*" + t + r"\s*;", hdr), t


def test_default_params_need_no_gpu():
    p = plade_amd.M3c2Params()
    p.radius, p.depth, p.reg_error, p.min_points, p.reserved = -1.0, -2.0, -3.0, -7, 9
    plade_amd.load_library().plade_m3c2_default_params(ctypes.byref(p))
    assert (p.radius, p.depth, p.reg_error, p.min_points, p.reserved) == (0.0, 0.0, 0.0, 4, 0)
    assert plade_amd.m3c2_default_params() == {"radius": 0.0, "depth": 0.0, "reg_error": 0.0, "min_points": 4}


def test_structs_match_the_header():
    P, Q = plade_amd.M3c2Params, plade_amd.M3c2Summary
    assert [f for f, _ in P._fields_] == ["radius", "depth", "reg_error", "min_points", "reserved"]
    assert ctypes.sizeof(P) == 32 and P.depth.offset == 8 and P.reg_error.offset == 16 and P.min_points.offset == 24 and P.reserved.offset == 28
    assert [f for f, _ in Q._fields_] == ["m", "valid", "significant", "mean", "rms", "max", "max_count", "reserved"]
    assert ctypes.sizeof(Q) == 56 and Q.significant.offset == 16 and Q.mean.offset == 24 and Q.max.offset == 40 and Q.max_count.offset == 48


def test_the_header_with_the_new_structs_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "plade_hip.h"\nint main(void) { plade_m3c2_params p; plade_m3c2_summary s; plade_m3c2_default_params(&p);\n'
                   '  s.valid = 0; return (int)(sizeof(p) + sizeof(s) + s.valid) & 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


PITCH = 2.0 ** -6
PLANE_R, PLANE_L, PLANE_REG = 0.1, 0.25, 2.0 ** -10


def planes(normal=(0.0, 0.0, 1.0)):
    """(core, A, B): A = a 64 x 64 lattice of pitch 2^-6 at z = 0.5, B the same at z = 0.5 + 2^-6, core = every 7th point of A with
    the given normal: every t is 0 or +-2^-6, every sum is exact."""
    g = np.arange(64, dtype=np.float32) * np.float32(PITCH)
    x, y = np.meshgrid(g, g, indexing="ij")
    A = np.stack([x.ravel(), y.ravel(), np.full(64 * 64, 0.5, np.float32)], axis=1).astype(np.float32)
    B = A.copy()
    B[:, 2] = np.float32(0.5 + PITCH)
    core = np.concatenate([A[::7], np.tile(np.asarray(normal, np.float32), (len(A[::7]), 1))], axis=1)
    return np.ascontiguousarray(core), A, B


def check_planes(out, sign):
    """The exact answer on planes(): `out` is a dict with distance, lod, significant and count."""
    assert (out["distance"] == sign * PITCH).all()
    assert (out["lod"] == 1.96 * PLANE_REG).all()
    assert np.asarray(out["significant"], bool).all()
    c = np.asarray(out["count"])
    assert (c[:, 0] == c[:, 1]).all() and c.min() == 39 and c.max() == 129


# The two tests below pin the restatement alone (its own sanity, before the GPU tests lean on it): they run no library code.
def test_restatement_is_exact_on_two_exact_planes():
    core, A, B = planes()
    ref = M.m3c2(core, A, B, [(PLANE_R, PLANE_L)], reg_error=PLANE_REG)[0]
    assert ref["valid"].all()
    check_planes(ref, 1.0)
    assert (ref["sigma"] == 0).all()
    assert (ref["moments"][:, 0] == 0).all() and (ref["moments"][:, 2] == ref["count"][:, 1] * PITCH).all()
    s = M.summary(ref["distance"], ref["significant"], ref["count"])
    assert (s["m"], s["valid"], s["significant"], s["mean"], s["rms"], s["max"], s["max_count"]) == (586, 586, 586, PITCH, PITCH, PITCH, 129)


def test_restatement_follows_the_sign_of_the_normal_and_skips_a_missing_axis():
    core, A, B = planes((0.0, 0.0, -1.0))
    ref = M.m3c2(core, A, B, [(PLANE_R, PLANE_L)], reg_error=PLANE_REG)[0]
    check_planes(ref, -1.0)
    core[3, 3:] = 0.0
    core[5, 4] = np.nan
    core[8, 3:] = (0.0, 0.0, -3.5)                                     # not unit: the same axis
    bad = M.m3c2(core, A, B, [(PLANE_R, PLANE_L)], reg_error=PLANE_REG)[0]
    assert list(np.nonzero(~bad["has_axis"])[0]) == [3, 5] and (bad["count"][[3, 5]] == 0).all()
    assert np.isnan(bad["distance"][[3, 5]]).all() and np.isnan(bad["lod"][[3, 5]]).all() and not bad["significant"][[3, 5]].any()
    keep = np.ones(len(core), bool)
    keep[[3, 5]] = False
    assert np.array_equal(bad["distance"][keep], ref["distance"][keep]) and np.array_equal(bad["count"][keep], ref["count"][keep])
    few = M.m3c2(core, A, B, [(PLANE_R, PLANE_L)], min_points=130)[0]  # more than any cylinder holds: nothing is valid
    assert not few["valid"].any() and np.isnan(few["distance"]).all() and np.array_equal(few["count"], bad["count"])
