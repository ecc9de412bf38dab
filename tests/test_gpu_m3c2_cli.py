"""The CLI's PLADE_M3C2=<radius>,<depth>[,<min_points>[,<reg_error>]] switch (plade_host.cpp): one line per registered pair with
the library's own numbers (core = reference = the target, compared = the source under the final transformation), also after
PLADE_REFINE_ICP=1; unset, nothing changes; a value that does not parse prints one warning and compares nothing."""
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
LINE = "m3c2: %d of %d core points valid, %d significant (mean %.6g, rms %.6g, max %.6g)"


def _matrix(text):
    rows = [[float(x) for x in line.split()] for line in text.split("\n")
            if line.strip() and not line.startswith(("target:", "source:", "transformation:", "registration failed"))]
    return np.array(rows, np.float64)


@pytest.mark.timeout(900)
def test_cli_switch(tmp_path, ctx):
    tg, sr, T = make_pair(80000, seed=0)
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

    def strip_time(s):
        return "\n".join(l for l in s.split("\n") if not l.startswith("done. time:"))

    def expected(Tr, **kw):
        info = ctx.m3c2(tg, tg, sr, 0.25, 0.5, T=Tr, per_point=False, **kw)[1]
        return LINE % (info["valid"], info["m"], info["significant"], info["mean"], info["rms"], info["max"])

    r0, res0 = run()
    assert r0.returncode == 0, r0.stdout + r0.stderr
    assert "m3c2" not in r0.stdout + r0.stderr
    ok, Tr = ctx.registration(tg, sr)                               # the CLI's registration, with all its digits
    assert ok and np.allclose(_matrix(res0), Tr, rtol=2e-5, atol=2e-6) and np.linalg.norm(Tr.astype(np.float64) - T) < GT_TOL
    # on: one line with the library's own numbers; everything else as without the variable
    r1, res1 = run(PLADE_M3C2="0.25,0.5")
    assert r1.returncode == 0, r1.stdout + r1.stderr
    lines = [l for l in r1.stdout.split("\n") if l.startswith("m3c2: ")]
    assert lines == [expected(Tr)], r1.stdout
    assert res1 == res0 and r1.stderr == r0.stderr
    assert strip_time("\n".join(l for l in r1.stdout.split("\n") if not l.startswith("m3c2: "))) == strip_time(r0.stdout)
    # min_points and reg_error
    r2, _ = run(PLADE_M3C2="0.25,0.5,8,0.01")
    assert [l for l in r2.stdout.split("\n") if l.startswith("m3c2: ")] == [expected(Tr, min_points=8, reg_error=0.01)], r2.stdout
    # after the ICP refinement
    r3, res3 = run(PLADE_M3C2="0.25,0.5", PLADE_REFINE_ICP="1")
    assert r3.returncode == 0, r3.stdout + r3.stderr
    Ti = ctx.refine_icp(tg, sr, Tr)[0]
    assert np.allclose(_matrix(res3), Ti, rtol=2e-5, atol=2e-6)
    assert [l for l in r3.stdout.split("\n") if l.startswith("m3c2: ")] == [expected(Ti)], r3.stdout
    assert r3.stdout.index("ICP refinement: ") < r3.stdout.index("m3c2: ")
    # a value that does not parse: one warning, nothing compared, the output without the variable otherwise
    for badv in ("wide", "0.25", "-1,0.5", "0.25,0.5,1", "0.25,0.5,4,0.01x"):
        rb, resb = run(PLADE_M3C2=badv)
        assert rb.returncode == 0
        assert rb.stderr.count("warning: PLADE_M3C2=") == 1 and "no comparison" in rb.stderr, badv
        assert "m3c2: " not in rb.stdout and resb == res0 and strip_time(rb.stdout) == strip_time(r0.stdout), badv
