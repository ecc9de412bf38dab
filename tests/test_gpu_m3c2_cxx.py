"""The C++ API's compare_clouds() (plade_amd/csrc/plade.h, plade_host.cpp) through a small program of its own
(tests/cxx/m3c2_harness.cpp): the distances and the summary against Context.m3c2 on the same points, bit for bit, and a refused
radius."""
import os
import subprocess

import numpy as np
import pytest

from plade_amd.plyio import write_ply
from plade_amd.synth import sample_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADIUS, DEPTH, MIN_POINTS, REG = 0.25, 0.5, 5, 0.001
SHIFT = (0.0, 0.0, 0.03125)


def test_cxx_compare_clouds(tmp_path, ctx):
    A = np.ascontiguousarray(sample_scene(6000, scene_seed=3, sample_seed=4))
    B = np.ascontiguousarray(sample_scene(6000, scene_seed=3, sample_seed=5))
    pa, pb, out, exe = str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), str(tmp_path / "out.bin"), str(tmp_path / "m3c2_harness")
    write_ply(pa, A)
    write_ply(pb, B)
    csrc = os.path.join(ROOT, "plade_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                           os.path.join(ROOT, "tests", "cxx", "m3c2_harness.cpp"), os.path.join(csrc, "plade_host.cpp"),
                           os.path.join(csrc, "ply_reader.cpp"), "-o", exe, "-L", os.path.join(ROOT, "plade_amd"),
                           "-lplade_hip", "-Wl,-rpath," + os.path.join(ROOT, "plade_amd")])
    env = {k: v for k, v in os.environ.items() if not k.startswith("PLADE_")}
    r = subprocess.run([exe, pa, pb, repr(RADIUS), repr(DEPTH), str(MIN_POINTS), repr(REG)] + [repr(v) for v in SHIFT] + [out],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = SHIFT
    dist, info = ctx.m3c2(A, A, B, RADIUS, DEPTH, T=T, min_points=MIN_POINTS, reg_error=REG)
    assert 0 < info["valid"] < len(A) and 0 < info["significant"] < info["valid"]
    got = np.fromfile(out, np.float64)
    assert got.shape == dist.shape and got.tobytes() == dist.tobytes()
    w = [l.split()[1:] for l in r.stdout.split("\n") if l.startswith("@info ")]
    assert len(w) == 1
    w = w[0]
    assert (int(w[0]), int(w[1]), int(w[2]), float(w[3]), float(w[4]), float(w[5]), int(w[6])) == (
        info["m"], info["valid"], info["significant"], info["mean"], info["rms"], info["max"], info["max_count"])
    assert f"@refused 1 {len(A)} {len(A)}" in r.stdout
    assert "cloud comparison failed: " in r.stdout + r.stderr and "radius" in r.stdout + r.stderr
