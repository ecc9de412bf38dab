"""The CLI's PLADE_FPFH_MATCH=<radius>[,<min_pairs>[,<max_ratio>]] switch (plade_host.cpp): one line per pair with the library's own
numbers (both clouds described, the source matched against the target, the share of the correspondences that the final
transformation brings within the radius), also for a pair that does not register; unset, nothing changes; a value that does not
parse prints one warning and does nothing."""
import os
import subprocess

import numpy as np
import pytest

from plade_amd.plyio import write_ply
from plade_amd.synth import make_pair
from conftest import GT_TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "plade_amd", "PLADE")
LINE = "fpfh: %d of %d target and %d of %d source points described, %d mutual correspondences"
RADIUS = 0.5


def _matrix(text):
    rows = [[float(x) for x in line.split()] for line in text.split("\n")
            if line.strip() and not line.startswith(("target:", "source:", "transformation:", "registration failed"))]
    return np.array(rows, np.float64)


def _expected(ctx, tg, sr, Tr, **kw):
    ft, it = ctx.fpfh(tg, RADIUS, min_pairs=kw.get("min_pairs"), per_point=False)
    fs, i_s = ctx.fpfh(sr, RADIUS, min_pairs=kw.get("min_pairs"), per_point=False)
    corr = ctx.match_features(fs, ft, max_ratio=kw.get("max_ratio", 0.0))[0]
    line = LINE % (it["described"], it["n"], i_s["described"], i_s["n"], len(corr))
    if Tr is None:
        return line
    T = Tr.astype(np.float64)
    p, q = sr[corr[:, 0], :3].astype(np.float64), tg[corr[:, 1], :3].astype(np.float64)
    moved = np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], axis=1)
    v = moved - q
    close = int((np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]) < RADIUS).sum())
    return line + ", %.4f of them within the radius" % (close / len(corr) if len(corr) else 0.0)


@pytest.mark.timeout(900)
def test_cli_switch(tmp_path, ctx):
    tg, sr, T = make_pair(80000, seed=0)
    pt, ps = str(tmp_path / "t.ply"), str(tmp_path / "s.ply")
    write_ply(pt, tg)
    write_ply(ps, sr)
    base = {k: v for k, v in os.environ.items() if not k.startswith("PLADE_")}
    base["PLADE_ORIENT_NORMALS"] = "1"

    def run(a=pt, b=ps, **extra):
        res = str(tmp_path / "r.txt")
        if os.path.exists(res):
            os.remove(res)
        r = subprocess.run([CLI, a, b, res], capture_output=True, text=True, timeout=300, env=dict(base, **extra))
        return r, (open(res).read() if os.path.exists(res) else None)

    def strip_time(s):
        return "\n".join(l for l in s.split("\n") if not l.startswith("done. time:"))

    def fpfh_lines(r):
        return [l for l in r.stdout.split("\n") if l.startswith("fpfh: ")]

    r0, res0 = run()
    assert r0.returncode == 0, r0.stdout + r0.stderr
    assert "fpfh" not in r0.stdout + r0.stderr
    ok, Tr = ctx.registration(tg, sr)                               # the CLI's registration, with all its digits
    assert ok and np.allclose(_matrix(res0), Tr, rtol=2e-5, atol=2e-6) and np.linalg.norm(Tr.astype(np.float64) - T) < GT_TOL
    # on: one line with the library's own numbers; everything else as without the variable
    r1, res1 = run(PLADE_FPFH_MATCH=repr(RADIUS))
    assert r1.returncode == 0, r1.stdout + r1.stderr
    assert fpfh_lines(r1) == [_expected(ctx, tg, sr, Tr)], r1.stdout
    assert res1 == res0 and r1.stderr == r0.stderr
    assert strip_time("\n".join(l for l in r1.stdout.split("\n") if not l.startswith("fpfh: "))) == strip_time(r0.stdout)
    # min_pairs and max_ratio
    r2, _ = run(PLADE_FPFH_MATCH="%r,8,0.9" % RADIUS)
    assert fpfh_lines(r2) == [_expected(ctx, tg, sr, Tr, min_pairs=8, max_ratio=np.float32(0.9))], r2.stdout
    # a pair that does not register (one wall against itself: too few planes): the line without the share
    wall = np.ascontiguousarray(tg[np.abs(tg[:, 5]) > 0.99][:4000])
    pw = str(tmp_path / "w.ply")
    write_ply(pw, wall)
    r3, res3 = run(pw, pw, PLADE_FPFH_MATCH=repr(RADIUS))
    r3off, _ = run(pw, pw)
    assert "registration failed" in r3.stderr and r3.stderr == r3off.stderr and "fpfh" not in r3off.stdout
    assert fpfh_lines(r3) == [_expected(ctx, wall, wall, None)], r3.stdout
    # a value that does not parse: one warning, nothing described, the output without the variable otherwise
    for badv in ("wide", "-1", "0.5,0", "0.5,5,-1", "0.5,5,0.9x", "0.5,"):
        rb, resb = run(PLADE_FPFH_MATCH=badv)
        assert rb.returncode == 0
        assert rb.stderr.count("warning: PLADE_FPFH_MATCH=") == 1 and "no descriptors" in rb.stderr, badv
        assert "fpfh: " not in rb.stdout and resb == res0 and strip_time(rb.stdout) == strip_time(r0.stdout), badv
