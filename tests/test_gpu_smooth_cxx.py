"""The C++ API's smooth_cloud() (plade_amd/csrc/plade.h, plade_host.cpp) through a small program of its own
(tests/cxx/smooth_harness.cpp): the cloud's own normals kept, the fits' normals, in place, and a refused radius -- against
Context.smooth_cloud on the same points, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from plade_amd.plyio import write_ply
from plade_amd.synth import sample_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADIUS, MIN_NB = 0.25, 7


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_cxx_smooth_cloud(tmp_path, ctx):
    P = np.ascontiguousarray(sample_scene(6000, scene_seed=3, sample_seed=4))
    ply, out, exe = str(tmp_path / "c.ply"), str(tmp_path / "out.bin"), str(tmp_path / "smooth_harness")
    write_ply(ply, P)
    csrc = os.path.join(ROOT, "plade_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                           os.path.join(ROOT, "tests", "cxx", "smooth_harness.cpp"), os.path.join(csrc, "plade_host.cpp"),
                           os.path.join(csrc, "ply_reader.cpp"), "-o", exe, "-L", os.path.join(ROOT, "plade_amd"),
                           "-lplade_hip", "-Wl,-rpath," + os.path.join(ROOT, "plade_amd")])
    env = {k: v for k, v in os.environ.items() if not k.startswith("PLADE_")}
    r = subprocess.run([exe, ply, repr(RADIUS), str(MIN_NB), out], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    rows, info = ctx.smooth_cloud(P, RADIUS, min_neighbours=MIN_NB)
    assert 0 < info["fitted"] < len(P)                    # both branches: fitted points and NaN normals
    own, fit, inplace = np.fromfile(out, np.float32).reshape(3, len(P), 6)
    assert same_bits(own[:, :3], rows[:, :3]) and same_bits(own[:, 3:], P[:, 3:])
    assert same_bits(fit, rows)
    assert same_bits(inplace, own)
    infos = [l.split()[1:] for l in r.stdout.split("\n") if l.startswith("@info ")]
    assert len(infos) == 3
    for w in infos:
        assert (int(w[0]), int(w[1]), float(w[2]), float(w[3]), int(w[4])) == (info["n"], info["fitted"], info["rms"], info["max"],
                                                                               info["max_count"])
    assert f"@refused 1 {len(P)}" in r.stdout
    assert "smoothing failed: " in r.stdout + r.stderr and "radius" in r.stdout + r.stderr
