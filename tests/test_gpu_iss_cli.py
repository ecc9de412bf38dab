"""The CLI's PLADE_FEATURE_KEYPOINTS=<salient_radius>[,<non_max_radius>[,<min_neighbours>]] switch (plade_host.cpp): next to
PLADE_FEATURE_REGISTER a pair whose plane registration failed goes through plade_register_keypoints, gets its matrix and two lines
with the library's own numbers; alone, or on a pair that registers by its planes, it changes no byte of the output; a value that does
not parse prints one warning and is ignored."""
import os
import subprocess

import numpy as np
import pytest

import corr_pose_restate as P
import iss_cases
from plade_amd.plyio import write_ply
from plade_amd.synth import make_pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "plade_amd", "PLADE")
K = iss_cases.TERRAIN
REGISTER = "%r,%r" % (K["radius"], K["inlier_dist"])
KEYPOINTS = "%r,%r" % (K["salient_radius"], K["non_max_radius"])
KEY_LINE = "keypoints: %d of %d source points"
REG_LINE = "feature registration: %d of %d correspondences, rmse %.6g"


def _matrix(text):
    rows = [[float(x) for x in line.split()] for line in text.split("\n")
            if line.strip() and not line.startswith(("target:", "source:", "transformation:", "registration failed"))]
    return np.array(rows, np.float64)


def strip_time(s):
    return "\n".join(l for l in s.split("\n") if not l.startswith("done. time:"))


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    d = tmp_path_factory.mktemp("iss_cli")
    base = {k: v for k, v in os.environ.items() if not k.startswith("PLADE_")}
    base["PLADE_ORIENT_NORMALS"] = "1"

    def run(a, b, **extra):
        res = str(d / "r.txt")
        if os.path.exists(res):
            os.remove(res)
        r = subprocess.run([CLI, a, b, res], capture_output=True, text=True, timeout=300, env=dict(base, **extra))
        return r, (open(res).read() if os.path.exists(res) else None)

    run.dir = d
    return run


@pytest.fixture(scope="module")
def terrain(cli):
    tg, sr, T = iss_cases.terrain()
    pt, ps = str(cli.dir / "terrain_t.ply"), str(cli.dir / "terrain_s.ply")
    write_ply(pt, tg)
    write_ply(ps, sr)
    return tg, sr, T, pt, ps


def both_lines(stdout):
    return [l for l in stdout.split("\n") if l.startswith(("keypoints:", "feature registration"))]


def test_terrain_registers_from_its_keypoints(cli, terrain, ctx):
    tg, sr, T, pt, ps = terrain
    Tr, info = ctx.register_keypoints(tg, sr, K["radius"], K["inlier_dist"], K["salient_radius"], K["non_max_radius"])
    assert info["ok"]
    r1, res1 = cli(pt, ps, PLADE_FEATURE_REGISTER=REGISTER, PLADE_FEATURE_KEYPOINTS=KEYPOINTS)
    assert r1.returncode == 0, r1.stdout + r1.stderr
    assert both_lines(r1.stdout) == [KEY_LINE % (info["iss"]["keypoints"], len(sr)),
                                     REG_LINE % (info["inliers"], info["n_corr"], info["rmse"])]
    assert "registration failed" not in res1 and "transformation:" in res1 and "failed as well" not in r1.stderr
    M = _matrix(res1)
    assert np.allclose(M, Tr, rtol=2e-5, atol=2e-6)
    rot, tr = P.pose_error(M, T)
    assert rot < 2.0 and tr < 0.1
    # the non-max radius defaults to the salient radius, min_neighbours is read
    for value, kw in (("%r" % K["salient_radius"], dict(non_max_radius=0.0)),
                      (KEYPOINTS + ",3", dict(non_max_radius=K["non_max_radius"], min_neighbours=3))):
        T2, i2 = ctx.register_keypoints(tg, sr, K["radius"], K["inlier_dist"], K["salient_radius"], **kw)
        r2, _ = cli(pt, ps, PLADE_FEATURE_REGISTER=REGISTER, PLADE_FEATURE_KEYPOINTS=value)
        want = [KEY_LINE % (i2["iss"]["keypoints"], len(sr))]
        if i2["ok"]:
            want.append(REG_LINE % (i2["inliers"], i2["n_corr"], i2["rmse"]))
            assert both_lines(r2.stdout) == want, value
        else:
            assert both_lines(r2.stdout) == [] and r2.stderr.count("feature registration failed as well: ") == 1, value
        assert i2["iss"]["keypoints"] != info["iss"]["keypoints"]


def test_alone_or_on_a_registered_pair_nothing_changes(cli, terrain):
    tg, sr, T, pt, ps = terrain
    r0, res0 = cli(pt, ps)
    r1, res1 = cli(pt, ps, PLADE_FEATURE_KEYPOINTS=KEYPOINTS)
    assert "registration failed" in r0.stderr
    assert res1 == res0 and r1.stderr == r0.stderr and strip_time(r1.stdout) == strip_time(r0.stdout) and r1.returncode == r0.returncode
    tg, sr, T = make_pair(30000, seed=0, n_boxes=4)
    qt, qs = str(cli.dir / "room_t.ply"), str(cli.dir / "room_s.ply")
    write_ply(qt, tg)
    write_ply(qs, sr)
    q0, qres0 = cli(qt, qs)
    assert q0.returncode == 0 and "transformation:" in qres0
    q1, qres1 = cli(qt, qs, PLADE_FEATURE_REGISTER=REGISTER, PLADE_FEATURE_KEYPOINTS=KEYPOINTS)
    assert qres1 == qres0 and q1.stderr == q0.stderr and strip_time(q1.stdout) == strip_time(q0.stdout)


def test_bad_values_warn_once_and_are_ignored(cli, terrain):
    tg, sr, T, pt, ps = terrain
    f0, fres0 = cli(pt, ps, PLADE_FEATURE_REGISTER=REGISTER)
    assert f0.returncode == 0 and "keypoints:" not in f0.stdout
    for badv in ("wide", "-0.5", "0.5,0", "0.5,0.15,0", "0.5,0.15,3x", "1e30"):
        rb, resb = cli(pt, ps, PLADE_FEATURE_REGISTER=REGISTER, PLADE_FEATURE_KEYPOINTS=badv)
        assert rb.stderr.count("warning: PLADE_FEATURE_KEYPOINTS=") == 1 and "no keypoints" in rb.stderr, badv
        assert "keypoints:" not in rb.stdout and resb == fres0 and strip_time(rb.stdout) == strip_time(f0.stdout), badv
        assert "\n".join(l for l in rb.stderr.split("\n") if not l.startswith("warning: PLADE_FEATURE_KEYPOINTS=")) == f0.stderr, badv
