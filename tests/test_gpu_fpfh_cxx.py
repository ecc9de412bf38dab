"""The C++ API's describe_cloud() and match_features() (plade_amd/csrc/plade.h, plade_host.cpp) through a small program of its own
(tests/cxx/fpfh_harness.cpp): the descriptors, the summaries and the correspondences against Context.fpfh / match_features on the
same points, bit for bit, and two refused calls."""
import os
import subprocess

import numpy as np
import pytest

from plade_amd.plyio import write_ply
from plade_amd.synth import sample_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADIUS, MIN_PAIRS, MUTUAL, RATIO = 0.5, 6, 1, 0.95


def test_cxx_describe_and_match(tmp_path, ctx):
    A = np.ascontiguousarray(sample_scene(6000, scene_seed=3, sample_seed=4))
    B = np.ascontiguousarray(sample_scene(6000, scene_seed=3, sample_seed=5))
    pa, pb, exe = str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), str(tmp_path / "fpfh_harness")
    oa, ob, oc = str(tmp_path / "fa.bin"), str(tmp_path / "fb.bin"), str(tmp_path / "corr.bin")
    write_ply(pa, A)
    write_ply(pb, B)
    csrc = os.path.join(ROOT, "plade_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                           os.path.join(ROOT, "tests", "cxx", "fpfh_harness.cpp"), os.path.join(csrc, "plade_host.cpp"),
                           os.path.join(csrc, "ply_reader.cpp"), "-o", exe, "-L", os.path.join(ROOT, "plade_amd"),
                           "-lplade_hip", "-Wl,-rpath," + os.path.join(ROOT, "plade_amd")])
    env = {k: v for k, v in os.environ.items() if not k.startswith("PLADE_")}
    r = subprocess.run([exe, pa, pb, repr(RADIUS), str(MIN_PAIRS), str(MUTUAL), repr(RATIO), oa, ob, oc],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    da, ia = ctx.fpfh(A, RADIUS, min_pairs=MIN_PAIRS)
    db, ib = ctx.fpfh(B, RADIUS, min_pairs=MIN_PAIRS)
    assert 0 < ia["described"] < len(A) and 0 < ib["described"] < len(B)
    ga, gb = np.fromfile(oa, np.float32).reshape(-1, 33), np.fromfile(ob, np.float32).reshape(-1, 33)
    assert ga.shape == da.shape and ga.tobytes() == da.tobytes() and gb.shape == db.shape and gb.tobytes() == db.tobytes()
    corr, info = ctx.match_features(da, db, mutual=bool(MUTUAL), max_ratio=np.float32(RATIO))
    got = np.fromfile(oc, np.int32).reshape(-1, 2)
    assert 0 < len(corr) < ia["described"] and got.shape == corr.shape and got.tobytes() == corr.tobytes()
    w = [l.split()[1:] for l in r.stdout.split("\n") if l.startswith("@info ")]
    assert len(w) == 2
    for words, i in zip(w, (ia, ib)):
        assert (int(words[0]), int(words[1]), float(words[2]), int(words[3])) == (i["n"], i["described"], i["mean_pairs"], i["max_pairs"])
    assert f"@refused 1 {33 * len(A)} {len(A)}" in r.stdout
    assert f"@refused_match 1 {len(corr)}" in r.stdout
    assert "cloud description failed: " in r.stdout + r.stderr and "radius" in r.stdout + r.stderr
