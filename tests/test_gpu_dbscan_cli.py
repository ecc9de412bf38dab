"""The CLI's two DBSCAN switches (plade_amd/csrc/plade_host.cpp).

PLADE_DBSCAN=<radius>,<min_points>[,<min_size>[,<keep_largest>]]: both clouds keep the points of their clusters, one line per cloud
with the library's own numbers; unset, stdout, stderr and the result file are those of a run without it; a value that does not
parse prints one warning and filters nothing.

PLADE_M3C2_CLUSTERS=<radius>[,<min_points>[,<min_size>]] next to PLADE_M3C2: one line after the m3c2 line, the library's DBSCAN of
the significant core points under the CLI's transformation; the m3c2 line itself is unchanged; without PLADE_M3C2 it does
nothing."""
import os
import subprocess

import numpy as np
import pytest

import plade_amd
from plade_amd.plyio import write_ply
from plade_amd.synth import make_pair
from conftest import GT_TOL, ORIENTED

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "plade_amd", "PLADE")
LINE = "dbscan: kept %d of %d points in %d of %d clusters (largest %d; %d core, %d border, %d noise)"
M3C2_LINE = "m3c2: %d of %d core points valid, %d significant (mean %.6g, rms %.6g, max %.6g)"
CLUSTER_LINE = "m3c2 clusters: %d clusters of %d significant core points (largest %d, noise %d)"


def _matrix(text):
    rows = [[float(x) for x in line.split()] for line in text.split("\n")
            if line.strip() and not line.startswith(("target:", "source:", "transformation:", "registration failed"))]
    return np.array(rows, np.float64)


def strip_time(s):
    return "\n".join(l for l in s.split("\n") if not l.startswith("done. time:"))


def without(s, *prefixes):
    return "\n".join(l for l in s.split("\n") if not l.startswith(prefixes))


def runner(tmp_path, tg, sr):
    pt, ps = str(tmp_path / "t.ply"), str(tmp_path / "s.ply")
    write_ply(pt, tg)
    write_ply(ps, sr)
    base = {k: v for k, v in os.environ.items() if not k.startswith("PLADE_")}
    base["PLADE_ORIENT_NORMALS"] = "1"

    def run(**extra):
        res = str(tmp_path / "r.txt")
        if os.path.exists(res):
            os.remove(res)
        r = subprocess.run([CLI, pt, ps, res], capture_output=True, text=True, timeout=300, env=dict(base, **extra))
        return r, (open(res).read() if os.path.exists(res) else None)
    return run


@pytest.mark.timeout(900)
def test_cli_dbscan_switch(tmp_path):
    tg, sr, T = make_pair(20000, seed=0)
    ctx = plade_amd.Context(0, **ORIENTED)
    try:
        r = float(np.float32(3.0) * ctx.average_spacing(tg))
        expected, filtered = [], []
        for cloud in (tg, sr):
            rows, kept, i = ctx.dbscan(cloud, r, 6, min_size=100)
            filtered.append(rows)
            assert i["noise"] > 0 and i["border"] > 0 and 0.8 * len(cloud) < i["kept"] < len(cloud)
            expected.append(LINE % (i["kept"], i["n"], i["kept_clusters"], i["clusters"], i["largest"], i["core"], i["border"], i["noise"]))
        ok_lib, T_lib = ctx.registration(filtered[0], filtered[1])
        assert ok_lib
    finally:
        ctx.close()
    run = runner(tmp_path, tg, sr)
    r0, res0 = run()
    assert r0.returncode == 0, r0.stdout + r0.stderr
    assert "dbscan: " not in r0.stdout + r0.stderr              # (the line; the temporary paths carry the test's name)
    # on: one line per cloud with the library's own numbers, and the pair registers as the library registers the filtered clouds
    r1, res1 = run(PLADE_DBSCAN="%.9g,6,100" % r)
    assert r1.returncode == 0, r1.stdout + r1.stderr
    assert [l for l in r1.stdout.split("\n") if l.startswith("dbscan: kept ")] == expected, r1.stdout
    assert "registration failed" not in res1 and np.allclose(_matrix(res1), T_lib, rtol=2e-5, atol=2e-6)
    # after the component filter, before anything else that follows it
    r2, _ = run(PLADE_KEEP_COMPONENTS="%.9g" % r, PLADE_DBSCAN="%.9g,6,1,1" % r)
    assert r2.returncode == 0, r2.stdout + r2.stderr
    assert r2.stdout.count("component filter: kept ") == 2 and r2.stdout.count("dbscan: kept ") == 2 and r2.stdout.count(" in 1 of ") == 2
    assert r2.stdout.index("component filter: kept ") < r2.stdout.index("dbscan: kept ")
    # a value that does not parse: one warning, nothing filtered
    for badv in ("wide", "%.9g" % r, "0.1,6,1,1x"):          # (the grammar itself: test_dbscan_host.py)
        rb, resb = run(PLADE_DBSCAN=badv)
        assert rb.stderr.count("warning: PLADE_DBSCAN=") == 1 and "no clustering" in rb.stderr, badv
        assert "dbscan: kept" not in rb.stdout
        assert (rb.returncode, strip_time(rb.stdout), resb) == (r0.returncode, strip_time(r0.stdout), res0)


@pytest.mark.timeout(900)
def test_cli_m3c2_clusters_switch(tmp_path, ctx):
    tg, sr, T = make_pair(80000, seed=0)
    run = runner(tmp_path, tg, sr)
    r0, res0 = run()
    assert r0.returncode == 0, r0.stdout + r0.stderr
    ok, Tr = ctx.registration(tg, sr)                               # the CLI's registration, with all its digits
    assert ok and np.allclose(_matrix(res0), Tr, rtol=2e-5, atol=2e-6) and np.linalg.norm(Tr.astype(np.float64) - T) < GT_TOL
    info = ctx.m3c2(tg, tg, sr, 0.25, 0.5, T=Tr)[1]
    m3c2_line = M3C2_LINE % (info["valid"], info["m"], info["significant"], info["mean"], info["rms"], info["max"])
    sig = info["significant_mask"]
    assert sig.sum() == info["significant"] > 0

    def clusters_line(radius, **kw):
        d = ctx.dbscan(np.ascontiguousarray(tg[sig, :3]), radius, **kw)[2]
        print(f"{d['n']} significant core points at {radius} {kw}: {d['clusters']} clusters, {d['kept_clusters']} kept, largest "
              f"{d['largest']}, noise {d['noise']}")
        return CLUSTER_LINE % (d["kept_clusters"], d["n"], d["largest"], d["noise"])

    # alone it does nothing
    ra, resa = run(PLADE_M3C2_CLUSTERS="0.3,3")
    assert (ra.returncode, strip_time(ra.stdout), ra.stderr, resa) == (0, strip_time(r0.stdout), r0.stderr, res0)
    # next to PLADE_M3C2: the m3c2 line as it was, then the clusters line; everything else as without the variables
    for value, kw in (("0.3,3", dict(min_points=3)), ("0.5,3,10", dict(min_points=3, min_size=10))):
        r1, res1 = run(PLADE_M3C2="0.25,0.5", PLADE_M3C2_CLUSTERS=value)
        assert r1.returncode == 0, r1.stdout + r1.stderr
        lines = [l for l in r1.stdout.split("\n") if l.startswith("m3c2")]
        assert lines == [m3c2_line, clusters_line(float(value.split(",")[0]), **kw)], r1.stdout
        assert res1 == res0 and r1.stderr == r0.stderr
        assert strip_time(without(r1.stdout, "m3c2")) == strip_time(r0.stdout)
    # a value that does not parse: one warning, the m3c2 line alone
    rb, resb = run(PLADE_M3C2="0.25,0.5", PLADE_M3C2_CLUSTERS="0.3,0")
    assert rb.returncode == 0 and rb.stderr.count("warning: PLADE_M3C2_CLUSTERS=") == 1 and "no clusters of change" in rb.stderr
    assert [l for l in rb.stdout.split("\n") if l.startswith("m3c2")] == [m3c2_line] and resb == res0
