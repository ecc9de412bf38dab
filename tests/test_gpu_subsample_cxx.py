"""The C++ API's subsample_cloud() (plade_amd/csrc/plade.h, plade_host.cpp) through a small program of its own
(tests/cxx/subsample_harness.cpp): the kept points and the summary against Context.subsample -- the C entry -- on the same points,
bit for bit, the call in place, and refused calls that leave their outputs alone."""
import os
import subprocess

import numpy as np
import pytest

import subsample_restate as SR
from plade_amd.plyio import write_ply

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cxx_subsample_cloud(tmp_path, ctx):
    P = np.zeros((2000, 6), np.float32)
    P[:, :3] = SR.sheet(2000)
    P[:, 3:] = np.random.default_rng(1).normal(size=(2000, 3)).astype(np.float32)
    ply, exe, out = str(tmp_path / "c.ply"), str(tmp_path / "subsample_harness"), str(tmp_path / "rows.bin")
    write_ply(ply, P)
    csrc = os.path.join(ROOT, "plade_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                           os.path.join(ROOT, "tests", "cxx", "subsample_harness.cpp"), os.path.join(csrc, "plade_host.cpp"),
                           os.path.join(csrc, "ply_reader.cpp"), "-o", exe, "-L", os.path.join(ROOT, "plade_amd"),
                           "-lplade_hip", "-Wl,-rpath," + os.path.join(ROOT, "plade_amd")])
    env = {k: v for k, v in os.environ.items() if not k.startswith("PLADE_")}
    r = subprocess.run([exe, ply, "2.0", "7", out], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    rows, kept, info = ctx.subsample(P, 2.0, seed=7)
    ref = SR.subsample(P, 2.0, seed=7)
    assert info["kept"] == ref["kept"] and 100 < len(kept) < 2000
    assert np.fromfile(out, np.float32).tobytes() == rows.tobytes()
    assert f"@subsample 2000 {info['kept']} {info['rounds']}" in r.stdout.split("\n")
    assert "@in_place 1" in r.stdout and "@refused 1" in r.stdout
    assert (r.stdout + r.stderr).count("subsampling failed: ") == 2
