"""The C++ API's multiscale_normals() (plade_amd/csrc/plade.h, plade_host.cpp) through a small program of its own
(tests/cxx/scales_harness.cpp): normals toward the origin, along the cloud's own normals, in place, and refused descending radii --
against Context.scale_features on the same points, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from plade_amd.plyio import write_ply
from plade_amd.synth import sample_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADII, MODE, MIN_NB = (0.2, 0.35, 0.5), 1, 7


def same_but_nan(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(np.where(na, 0, a).view(np.uint32), np.where(nb, 0, b).view(np.uint32))


def test_cxx_multiscale_normals(tmp_path, ctx):
    P = np.ascontiguousarray(sample_scene(6000, scene_seed=3, sample_seed=4))
    ply, out, exe = str(tmp_path / "c.ply"), str(tmp_path / "out.bin"), str(tmp_path / "scales_harness")
    write_ply(ply, P)
    csrc = os.path.join(ROOT, "plade_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                           os.path.join(ROOT, "tests", "cxx", "scales_harness.cpp"), os.path.join(csrc, "plade_host.cpp"),
                           os.path.join(csrc, "ply_reader.cpp"), "-o", exe, "-L", os.path.join(ROOT, "plade_amd"),
                           "-lplade_hip", "-Wl,-rpath," + os.path.join(ROOT, "plade_amd")])
    env = {k: v for k, v in os.environ.items() if not k.startswith("PLADE_")}
    r = subprocess.run([exe, ply, str(MODE), str(MIN_NB), out] + [repr(x) for x in RADII], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    n0, i0 = ctx.scale_features(P, RADII, mode=MODE, min_neighbours=MIN_NB, orient=0, per_scale=False)
    n1, i1 = ctx.scale_features(P, RADII, mode=MODE, min_neighbours=MIN_NB, orient=1, per_scale=False)
    assert 0 < i0["fitted"] < len(P) and (n0 != n1).any()  # fitted points and NaN normals; the two rules differ somewhere
    view, own, inplace = np.fromfile(out, np.float32).reshape(3, len(P), 6)
    for rows, nrm in ((view, n0), (own, n1), (inplace, n0)):
        assert np.array_equal(rows[:, :3].view(np.uint32), P[:, :3].view(np.uint32)) and same_but_nan(rows[:, 3:], nrm)
    infos = [[int(x) for x in l.split()[1:]] for l in r.stdout.split("\n") if l.startswith("@info ")]
    assert len(infos) == 3
    for w, info in zip(infos, (i0, i1, i0)):
        assert w == [info["queries"], info["fitted"], info["max_count"]] + list(info["chosen_hist"]) + [0] * 5
    assert f"@refused 1 {len(P)}" in r.stdout
    assert "multi-scale normals failed: " in r.stdout + r.stderr and "strictly ascending" in r.stdout + r.stderr
