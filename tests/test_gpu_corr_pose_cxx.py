"""The C++ API's estimate_pose_from_correspondences() and register_by_features() (plade_amd/csrc/plade.h, plade_host.cpp) through a
small program of its own (tests/cxx/corr_pose_harness.cpp): the matrices, the correspondences and the summaries against
Context.register_features / estimate_pose on the same points, bit for bit, and two refused calls that leave their outputs alone."""
import os
import subprocess

import numpy as np
import pytest

import corr_cases
from plade_amd.plyio import write_ply

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADIUS, DIST = 0.6, 0.1


def test_cxx_pose_and_register(tmp_path, ctx):
    tg, sr, T = corr_cases.terrain_pair(6000)
    ps, pt, exe = str(tmp_path / "s.ply"), str(tmp_path / "t.ply"), str(tmp_path / "corr_pose_harness")
    oc, oT = str(tmp_path / "corr.bin"), str(tmp_path / "T.bin")
    write_ply(ps, sr)
    write_ply(pt, tg)
    csrc = os.path.join(ROOT, "plade_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                           os.path.join(ROOT, "tests", "cxx", "corr_pose_harness.cpp"), os.path.join(csrc, "plade_host.cpp"),
                           os.path.join(csrc, "ply_reader.cpp"), "-o", exe, "-L", os.path.join(ROOT, "plade_amd"),
                           "-lplade_hip", "-Wl,-rpath," + os.path.join(ROOT, "plade_amd")])
    env = {k: v for k, v in os.environ.items() if not k.startswith("PLADE_")}
    r = subprocess.run([exe, ps, pt, repr(RADIUS), repr(DIST), oc, oT], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    Tr, info = ctx.register_features(tg, sr, RADIUS, DIST)
    Te, ie = ctx.estimate_pose(sr, tg, info["corr"], DIST)
    assert info["ok"] and ie["ok"] and Tr.tobytes() == Te.tobytes()
    got = np.fromfile(oT, np.float32).reshape(2, 4, 4)
    assert got[0].tobytes() == Tr.tobytes() and got[1].tobytes() == Te.tobytes()
    corr = np.fromfile(oc, np.int32).reshape(-1, 2)
    assert len(corr) > 100 and corr.tobytes() == info["corr"].tobytes()
    w = [l.split()[1:] for l in r.stdout.split("\n") if l.startswith("@pose ")]
    assert len(w) == 2
    for words, i in zip(w, (info, ie)):
        assert [int(x) for x in words[:7]] == [len(corr), i["hypotheses"], i["scored"], i["best_hypothesis"], i["best_count"], i["inliers"],
                                               i["refinements"]]
        assert (float(words[7]), float(words[8])) == (i["rmse"], i["fitness"])
    assert "@refused_pose 1" in r.stdout and "@refused_register 1" in r.stdout
    assert "pose estimation failed: " in r.stdout + r.stderr and "feature registration failed: " in r.stdout + r.stderr
