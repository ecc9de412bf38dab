"""The C++ API's orient_cloud_normals() (plade_amd/csrc/plade.h, plade_host.cpp) through a small program of its own
(tests/cxx/orient_harness.cpp): the oriented points and the summary against Context.orient_consistent -- the C entry -- and the
restatement on the same points, bit for bit, both modes, the default reference, the call in place, and refused calls that leave
their outputs alone."""
import os
import subprocess

import numpy as np
import pytest

import orient_restate as OR
from plade_amd.plyio import write_ply

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("orient_cxx") / "orient_harness")
    csrc = os.path.join(ROOT, "plade_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                           os.path.join(ROOT, "tests", "cxx", "orient_harness.cpp"), os.path.join(csrc, "plade_host.cpp"),
                           os.path.join(csrc, "ply_reader.cpp"), "-o", exe, "-L", os.path.join(ROOT, "plade_amd"),
                           "-lplade_hip", "-Wl,-rpath," + os.path.join(ROOT, "plade_amd")])
    return exe


@pytest.mark.parametrize("mode,inward,ref", [(0, 0, (1.0, -2.0, 0.5)), (1, 1, (0.3, -2.0, -0.5))])
def test_cxx_orient_cloud_normals(tmp_path, ctx, harness, mode, inward, ref):
    P, U = OR.sphere(2000)
    rows = OR.with_normals(P, OR.random_flips(U))
    ply, out = str(tmp_path / "c.ply"), str(tmp_path / "rows.bin")
    write_ply(ply, rows)
    env = {k: v for k, v in os.environ.items() if not k.startswith("PLADE_")}
    r = subprocess.run([harness, ply, "2.0", str(mode), str(inward)] + [repr(x) for x in ref] + [out], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    kw = dict(mode=mode, inward=inward, **({"viewpoint": ref} if mode == 0 else {"direction": ref}))
    got, info = ctx.orient_consistent(rows, 2.0, **kw)
    want = OR.orient(rows, 2.0, **kw)
    assert got.tobytes() == want["rows"].tobytes() and want["components"] == 1 and 800 < want["flipped"] < 1200
    assert np.fromfile(out, np.float32).tobytes() == got.tobytes()
    line = f"@orient 2000 0 1 {info['flipped']} 1999 {info['tree_key_sum']} {info['rounds']}"
    assert line in r.stdout.split("\n"), r.stdout
    assert f"@default {OR.orient(rows, 2.0, mode=mode, inward=inward)['flipped']}" in r.stdout.split("\n")
    assert "@in_place 1" in r.stdout and "@refused 1" in r.stdout
    assert (r.stdout + r.stderr).count("normal orientation failed: ") == 3
