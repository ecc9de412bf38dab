"""The C++ API's cluster_cloud() (plade_amd/csrc/plade.h, plade_host.cpp) through a small program of its own
(tests/cxx/dbscan_harness.cpp): the kept points, the labels and the summary against Context.dbscan -- the C entry -- and the
restatement on the same points, bit for bit; the defaults, the call in place, and refused calls that leave their outputs alone."""
import os
import subprocess

import numpy as np
import pytest

import dbscan_restate as DR
from plade_amd.plyio import write_ply
from plade_amd.synth import sample_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dbscan_cxx") / "dbscan_harness")
    csrc = os.path.join(ROOT, "plade_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                           os.path.join(ROOT, "tests", "cxx", "dbscan_harness.cpp"), os.path.join(csrc, "plade_host.cpp"),
                           os.path.join(csrc, "ply_reader.cpp"), "-o", exe, "-L", os.path.join(ROOT, "plade_amd"),
                           "-lplade_hip", "-Wl,-rpath," + os.path.join(ROOT, "plade_amd")])
    return exe


def test_cxx_cluster_cloud(tmp_path, ctx, harness):
    rows = np.ascontiguousarray(sample_scene(8000, scene_seed=3, sample_seed=4, outliers=0.03))
    ply, out, lab = str(tmp_path / "c.ply"), str(tmp_path / "rows.bin"), str(tmp_path / "labels.bin")
    write_ply(ply, rows)
    env = {k: v for k, v in os.environ.items() if not k.startswith("PLADE_")}
    r = subprocess.run([harness, ply, "0.35", "8", "20", "5", out, lab], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    got, kept, info = ctx.dbscan(rows, 0.35, 8, min_size=20, keep_largest=5)
    want = DR.dbscan(rows, 0.35, 8, min_size=20, keep_largest=5)
    assert got.tobytes() == want["rows"].tobytes() and info["label"].tobytes() == want["label"].tobytes()
    assert want["clusters"] >= 20 and want["kept_clusters"] == 5 and 0 < want["kept"] < len(rows) - want["noise"]
    assert np.fromfile(out, np.float32).tobytes() == got.tobytes()
    assert np.fromfile(lab, np.int32).tobytes() == info["label"].tobytes()
    line = "@dbscan " + " ".join(str(info[k]) for k in ("n", "clusters", "core", "border", "noise", "kept_clusters", "kept", "largest"))
    assert line in r.stdout.split("\n"), r.stdout
    d = DR.dbscan(rows, 0.35, 4)
    assert f"@default {d['clusters']} {d['kept']}" in r.stdout.split("\n"), r.stdout
    assert "@in_place 1" in r.stdout and "@refused 1" in r.stdout
    assert (r.stdout + r.stderr).count("clustering failed: ") == 2
