"""The C++ API's refine_registration_gicp() (plade_amd/csrc/plade.h, plade_host.cpp) through a small program of its own
(tests/cxx/gicp_harness.cpp): the bits of Context.refine_gicp on the same points, the console line, and false with the
transformation untouched when the refinement fails."""
import os
import subprocess

import numpy as np
import pytest

import plade_amd
from plade_amd.plyio import write_ply
import icp_restate as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("epsilon", [0.0, 1.0])
def test_cxx_refine_registration_gicp(tmp_path, ctx, epsilon):
    z = np.load(os.path.join(ROOT, "tests", "golden", "g9_room.npz"))
    pt, ps, exe = str(tmp_path / "t.ply"), str(tmp_path / "s.ply"), str(tmp_path / "gicp_harness")
    write_ply(pt, z["target"])
    write_ply(ps, z["source"])
    tgt, src = plade_amd.read_ply(pt), plade_amd.read_ply(ps)              # the rows the program reads
    T0 = R.perturb(z["groundtruth"], 0.03, 0.03, seed=9).astype(np.float32)
    (tmp_path / "T.txt").write_text(" ".join(float(v).hex() for v in T0.reshape(-1)))
    csrc = os.path.join(ROOT, "plade_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                           os.path.join(ROOT, "tests", "cxx", "gicp_harness.cpp"), os.path.join(csrc, "plade_host.cpp"),
                           os.path.join(csrc, "ply_reader.cpp"), "-o", exe, "-L", os.path.join(ROOT, "plade_amd"),
                           "-lplade_hip", "-Wl,-rpath," + os.path.join(ROOT, "plade_amd")])
    env = {k: v for k, v in os.environ.items() if not k.startswith("PLADE_")}
    r = subprocess.run([exe, pt, ps, str(tmp_path / "T.txt"), repr(epsilon)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    T, info = ctx.refine_gicp(tgt, src, T0, epsilon=epsilon)
    assert info["iterations"] >= 2
    lines = {l.split()[0]: l.split()[1:] for l in r.stdout.split("\n") if l.startswith("@")}
    assert lines["@ok"] == ["1"]
    got = np.array([float.fromhex(v) for v in lines["@T"]], np.float32).reshape(4, 4)
    assert np.array_equal(got.view(np.uint32), T.view(np.uint32))
    line = "GICP refinement: %d iterations, %s, rmse %.6g, cost %.6g, fitness %.4f" % (
        info["iterations"], "converged" if info["converged"] else "not converged", info["rmse"], info["cost"], info["fitness"])
    assert line in r.stdout
    assert lines["@far"] == ["0", "1"]
    assert "GICP refinement failed" in r.stdout + r.stderr and "too few correspondences" in r.stdout + r.stderr
