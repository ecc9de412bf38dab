"""The CLI's PLADE_SUBSAMPLE=<spacing>[,<seed>] and PLADE_M3C2_CORE=<spacing>[,<seed>] switches (plade_host.cpp).  The first thins
both clouds of a pair as the last preparation step and prints one line per cloud with the restatement's counts and rounds; the
second makes the subsample of the target the core points of PLADE_M3C2.  Unset or 0, no byte of the output changes; a value that
does not parse prints one warning and is ignored."""
import os
import subprocess

import numpy as np
import pytest

import subsample_restate as SR
from plade_amd.plyio import write_ply
from plade_amd.synth import make_pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "plade_amd", "PLADE")
SUB_LINE = "subsample: kept %d of %d points (spacing %g, %d rounds)"
M3C2_LINE = "m3c2: %d of %d core points valid, %d significant (mean %.6g, rms %.6g, max %.6g)"


def strip_time(s):
    return "\n".join(l for l in s.split("\n") if not l.startswith("done. time:"))


def lines(stdout, prefix):
    return [l for l in stdout.split("\n") if l.startswith(prefix)]


def _matrix(text):
    rows = [[float(x) for x in line.split()] for line in text.split("\n")
            if line.strip() and not line.startswith(("target:", "source:", "transformation:", "registration failed"))]
    return np.array(rows, np.float64)


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    d = tmp_path_factory.mktemp("subsample_cli")
    tg, sr, T = make_pair(30000, seed=0, n_boxes=4)
    pt, ps = str(d / "t.ply"), str(d / "s.ply")
    write_ply(pt, tg)
    write_ply(ps, sr)
    base = {k: v for k, v in os.environ.items() if not k.startswith("PLADE_")}
    base["PLADE_ORIENT_NORMALS"] = "1"

    def run(**extra):
        res = str(d / "r.txt")
        if os.path.exists(res):
            os.remove(res)
        r = subprocess.run([CLI, pt, ps, res], capture_output=True, text=True, timeout=300, env=dict(base, **extra))
        return r, (open(res).read() if os.path.exists(res) else None)

    r0, res0 = run()
    assert r0.returncode == 0 and "transformation:" in res0, r0.stdout + r0.stderr
    return tg, sr, run, r0, res0


def test_subsample_lines_carry_the_restated_counts(pair):
    tg, sr, run, r0, res0 = pair
    for value, spacing, seed in (("0.3", 0.3, 0), ("0.5,7", 0.5, 7)):
        want = []
        for P in (tg, sr):
            ref = SR.subsample(P[:, :3], spacing, seed)
            want.append(SUB_LINE % (ref["kept"], len(P), spacing, ref["rounds"]))
        r, _ = run(PLADE_SUBSAMPLE=value)
        assert lines(r.stdout, "subsample: ") == want, r.stdout + r.stderr
        assert r.stdout.index("target file:") < r.stdout.index("subsample: ") and "subsampling failed" not in r.stderr
    assert lines(r0.stdout, "subsample: ") == []


def test_m3c2_core_points_are_the_subsample_of_the_target(pair, ctx):
    tg, sr, run, r0, res0 = pair
    ok, Tr = ctx.registration(tg, sr)                               # the CLI's registration, with all its digits
    assert ok and np.allclose(_matrix(res0), Tr, rtol=2e-5, atol=2e-6)
    whole = ctx.m3c2(tg, tg, sr, 0.25, 0.5, T=Tr, per_point=False)[1]
    r1, res1 = run(PLADE_M3C2="0.25,0.5")
    assert lines(r1.stdout, "m3c2: ") == [M3C2_LINE % (whole["valid"], len(tg), whole["significant"], whole["mean"], whole["rms"], whole["max"])]
    for value, spacing, seed in (("0.3", 0.3, 0), ("0.3,5", 0.3, 5)):
        ref = SR.subsample(tg[:, :3], spacing, seed)
        info = ctx.m3c2(np.ascontiguousarray(tg[ref["kept_index"]]), tg, sr, 0.25, 0.5, T=Tr, per_point=False)[1]
        assert info["m"] == ref["kept"] < len(tg)
        r2, res2 = run(PLADE_M3C2="0.25,0.5", PLADE_M3C2_CORE=value)
        assert lines(r2.stdout, "m3c2: ") == [M3C2_LINE % (info["valid"], ref["kept"], info["significant"], info["mean"], info["rms"], info["max"])]
        assert res2 == res0 and r2.stderr == r0.stderr and lines(r2.stdout, "subsample: ") == []
    # without PLADE_M3C2 the core switch does nothing
    r3, res3 = run(PLADE_M3C2_CORE="0.3")
    assert res3 == res0 and r3.stderr == r0.stderr and strip_time(r3.stdout) == strip_time(r0.stdout)


def test_unset_or_zero_changes_no_byte(pair):
    tg, sr, run, r0, res0 = pair
    for extra in (dict(PLADE_SUBSAMPLE="0"), dict(PLADE_M3C2_CORE="0"), dict(PLADE_SUBSAMPLE="0,3", PLADE_M3C2_CORE="0")):
        r, res = run(**extra)
        assert res == res0 and r.stderr == r0.stderr and strip_time(r.stdout) == strip_time(r0.stdout) and r.returncode == 0, extra
    m0, mres0 = run(PLADE_M3C2="0.25,0.5")
    m1, mres1 = run(PLADE_M3C2="0.25,0.5", PLADE_M3C2_CORE="0")
    assert mres1 == mres0 and m1.stderr == m0.stderr and strip_time(m1.stdout) == strip_time(m0.stdout)


def test_bad_values_warn_once_and_are_ignored(pair):
    tg, sr, run, r0, res0 = pair
    for var, tail in (("PLADE_SUBSAMPLE", "no subsampling"), ("PLADE_M3C2_CORE", "the whole target as core points")):
        with_m3c2 = {"PLADE_M3C2": "0.25,0.5"} if var == "PLADE_M3C2_CORE" else {}
        base, bres = run(**with_m3c2)
        for badv in ("wide", "0.3,5.0", "0.3,", "inf"):
            rb, resb = run(**dict(with_m3c2, **{var: badv}))
            assert rb.stderr.count(f"warning: {var}={badv} is not <spacing>[,<seed>]") == 1 and rb.stderr.count(tail) == 1, badv
            assert resb == bres and strip_time(rb.stdout) == strip_time(base.stdout), badv
            assert "".join(l + "\n" for l in rb.stderr.split("\n")[:-1] if not l.startswith(f"warning: {var}=")) == base.stderr, badv
