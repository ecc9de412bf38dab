"""The CLI's PLADE_FEATURE_REGISTER=<radius>,<inlier_dist>[,<min_inliers>[,<hypotheses>]] switch (plade_host.cpp): a pair whose plane
registration failed goes through plade_register_features, gets its matrix and one line with the library's own numbers, and is a
registered pair for the switches behind it; a pair the features cannot register either fails as before with one more line; a pair
that registers by its planes is untouched; a value that does not parse prints one warning and does nothing."""
import os
import subprocess

import numpy as np
import pytest

import corr_cases
import corr_pose_restate as P
from plade_amd.plyio import write_ply
from plade_amd.synth import make_pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "plade_amd", "PLADE")
RADIUS, DIST = 0.6, 0.1
SWITCH = "%r,%r" % (RADIUS, DIST)
LINE = "feature registration: %d of %d correspondences, rmse %.6g"
ALSO = "feature registration failed as well: "


def _matrix(text):
    rows = [[float(x) for x in line.split()] for line in text.split("\n")
            if line.strip() and not line.startswith(("target:", "source:", "transformation:", "registration failed"))]
    return np.array(rows, np.float64)


def strip_time(s):
    return "\n".join(l for l in s.split("\n") if not l.startswith("done. time:"))


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    d = tmp_path_factory.mktemp("corr_pose_cli")
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
    tg, sr, T = corr_cases.terrain_pair(6000)
    pt, ps = str(cli.dir / "terrain_t.ply"), str(cli.dir / "terrain_s.ply")
    write_ply(pt, tg)
    write_ply(ps, sr)
    return tg, sr, T, pt, ps


def test_terrain_registers_by_its_features(cli, terrain, ctx):
    tg, sr, T, pt, ps = terrain
    r0, res0 = cli(pt, ps)
    assert "registration failed" in r0.stderr and "feature registration" not in r0.stdout + r0.stderr
    assert np.array_equal(_matrix(res0), np.eye(4))
    Tr, info = ctx.register_features(tg, sr, RADIUS, DIST)
    assert info["ok"]
    r1, res1 = cli(pt, ps, PLADE_FEATURE_REGISTER=SWITCH)
    assert r1.returncode == 0, r1.stdout + r1.stderr
    assert [l for l in r1.stdout.split("\n") if l.startswith("feature registration")] == [LINE % (info["inliers"], info["n_corr"], info["rmse"])]
    assert "registration failed" not in res1 and "transformation:" in res1 and ALSO not in r1.stderr
    M = _matrix(res1)
    assert np.allclose(M, Tr, rtol=2e-5, atol=2e-6)
    rot, tr = P.pose_error(M, T)
    assert rot < 2.0 and tr < 0.1
    # min_inliers and hypotheses are read
    T2, i2 = ctx.register_features(tg, sr, RADIUS, DIST, min_inliers=10, hypotheses=4096)
    r2, _ = cli(pt, ps, PLADE_FEATURE_REGISTER=SWITCH + ",10,4096")
    assert LINE % (i2["inliers"], i2["n_corr"], i2["rmse"]) in r2.stdout.split("\n")
    # from there on a registered pair: the refinement runs, from the features' pose
    r3, res3 = cli(pt, ps, PLADE_FEATURE_REGISTER=SWITCH, PLADE_REFINE_ICP="1")
    assert r3.returncode == 0 and "ICP refinement: " in r3.stdout and "transformation:" in res3
    Ti, ii = ctx.refine_icp(tg, sr, Tr)
    assert np.allclose(_matrix(res3), Ti, rtol=2e-5, atol=2e-6)
    rot, tr = P.pose_error(_matrix(res3), T)
    assert rot < 2.0 and tr < 0.1


def test_one_wall_fails_both_ways(cli, terrain):
    """a flat wall of 4 000 points against itself: too few planes; and with min_inliers = 5 000 -- more than there are points, so more
    than any pose can have -- the features' pose is refused as well (a cloud matched against itself would otherwise register)"""
    tg, _, _ = make_pair(80000, seed=0)
    wall = np.ascontiguousarray(tg[np.abs(tg[:, 5]) > 0.99][:4000])
    pw = str(cli.dir / "w.ply")
    write_ply(pw, wall)
    r0, res0 = cli(pw, pw)
    r1, res1 = cli(pw, pw, PLADE_FEATURE_REGISTER="0.5,0.01,5000")
    assert "registration failed" in r0.stderr and ALSO not in r0.stderr
    assert r1.stderr.count(ALSO) == 1 and "registration failed" in r1.stderr and res1 == res0
    assert "\n".join(l for l in r1.stderr.split("\n") if not l.startswith(ALSO)) == r0.stderr
    assert "feature registration:" not in r1.stdout


def test_registered_pair_is_untouched_and_bad_values_warn(cli, terrain):
    tg, sr, T = make_pair(30000, seed=0, n_boxes=4)
    pt, ps = str(cli.dir / "room_t.ply"), str(cli.dir / "room_s.ply")
    write_ply(pt, tg)
    write_ply(ps, sr)
    r0, res0 = cli(pt, ps)
    assert r0.returncode == 0 and "transformation:" in res0
    r1, res1 = cli(pt, ps, PLADE_FEATURE_REGISTER=SWITCH)
    assert res1 == res0 and r1.stderr == r0.stderr and strip_time(r1.stdout) == strip_time(r0.stdout)
    _, _, _, tt, ts = terrain
    f0, fres0 = cli(tt, ts)
    for badv in ("wide", "0.6", "0.6,-1", "0.6,0.1,2", "0.6,0.1,3,0", "0.6,0.1,3,4096x", "0.6,0.1,"):
        rb, resb = cli(tt, ts, PLADE_FEATURE_REGISTER=badv)
        assert rb.stderr.count("warning: PLADE_FEATURE_REGISTER=") == 1 and "no feature registration" in rb.stderr, badv
        assert "feature registration:" not in rb.stdout and ALSO not in rb.stderr and resb == fres0, badv
