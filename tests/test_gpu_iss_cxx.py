"""The C++ API's detect_keypoints() and register_by_keypoints() (plade_amd/csrc/plade.h, plade_host.cpp) through a small program of
its own (tests/cxx/iss_harness.cpp): the keypoints, the correspondences, the matrix and the summaries against Context.iss_keypoints /
register_keypoints on the same points, bit for bit, and refused calls that leave their outputs alone."""
import os
import subprocess

import numpy as np
import pytest

import iss_cases
from plade_amd.plyio import write_ply

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cxx_detect_and_register(tmp_path, ctx):
    tg, sr, T = iss_cases.terrain()
    K = iss_cases.TERRAIN
    ps, pt, exe = str(tmp_path / "s.ply"), str(tmp_path / "t.ply"), str(tmp_path / "iss_harness")
    ok, oc, oT = str(tmp_path / "key.bin"), str(tmp_path / "corr.bin"), str(tmp_path / "T.bin")
    write_ply(ps, sr)
    write_ply(pt, tg)
    csrc = os.path.join(ROOT, "plade_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                           os.path.join(ROOT, "tests", "cxx", "iss_harness.cpp"), os.path.join(csrc, "plade_host.cpp"),
                           os.path.join(csrc, "ply_reader.cpp"), "-o", exe, "-L", os.path.join(ROOT, "plade_amd"),
                           "-lplade_hip", "-Wl,-rpath," + os.path.join(ROOT, "plade_amd")])
    env = {k: v for k, v in os.environ.items() if not k.startswith("PLADE_")}
    r = subprocess.run([exe, ps, pt, repr(K["radius"]), repr(K["inlier_dist"]), repr(K["salient_radius"]), repr(K["non_max_radius"]), ok, oc,
                        oT], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    index, ki = ctx.iss_keypoints(sr, K["salient_radius"], K["non_max_radius"])
    Tr, info = ctx.register_keypoints(tg, sr, K["radius"], K["inlier_dist"], K["salient_radius"], K["non_max_radius"])
    assert info["ok"] and len(index) > 100
    assert np.fromfile(ok, np.int32).tobytes() == index.astype(np.int32).tobytes()
    assert np.fromfile(oT, np.float32).reshape(4, 4).tobytes() == Tr.tobytes()
    corr = np.fromfile(oc, np.int32).reshape(-1, 2)
    assert len(corr) > 100 and corr.tobytes() == info["corr"].tobytes()
    lines = r.stdout.split("\n")
    want = [str(ki[k]) for k in ("n", "salient", "keypoints", "max_count")]
    assert [l.split()[1:] for l in lines if l.startswith("@keypoints ")] == [want, want] and info["iss"]["keypoints"] == ki["keypoints"]
    w = [l.split()[1:] for l in lines if l.startswith("@pose ")]
    assert len(w) == 1
    assert [int(x) for x in w[0][:7]] == [len(corr), info["hypotheses"], info["scored"], info["best_hypothesis"], info["best_count"],
                                          info["inliers"], info["refinements"]]
    assert (float(w[0][7]), float(w[0][8])) == (info["rmse"], info["fitness"])
    assert "@refused_detect 1" in r.stdout and "@refused_register 1" in r.stdout
    assert "keypoint detection failed: " in r.stdout + r.stderr and "keypoint registration failed: " in r.stdout + r.stderr
