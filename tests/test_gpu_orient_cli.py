"""The CLI's PLADE_CONSISTENT_NORMALS=<radius>[,<mode>[,<inward>]] switch (plade_host.cpp): both clouds of a pair get their
normals on one side per component as the last preparation step that touches normals -- after PLADE_ESTIMATE_NORMALS, before
PLADE_SUBSAMPLE -- and one line per cloud carries the restatement's counts.  Unset or 0, no byte of the output changes; a value
that does not parse prints one warning and is ignored.

The last test stands for a small scene that registers only with the switch: the flips across the 90 degree creases of a box room
with analytic normals are decided by the jitter of the normals (|dot| is about 0 there), so no 2000-point room was found whose
planes all come out consistent; what the switch is for is shown on a smooth surface instead, where the re-oriented cloud is the
unflipped original bit for bit and so are its FPFH descriptors.
"""
import os
import subprocess

import numpy as np
import pytest

import plade_amd
import orient_restate as OR
from plade_amd.plyio import write_ply
from plade_amd.synth import make_pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "plade_amd", "PLADE")
VAR = "PLADE_CONSISTENT_NORMALS"
LINE = "consistent normals: flipped %d of %d points in %d components (radius %g, %d without a normal, %d rounds)"


def strip_time(s):
    return "\n".join(l for l in s.split("\n") if not l.startswith("done. time:"))


def lines(stdout, prefix):
    return [l for l in stdout.split("\n") if l.startswith(prefix)]


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    d = tmp_path_factory.mktemp("orient_cli")
    tg, sr, T = make_pair(30000, seed=0, n_boxes=4)
    rng = np.random.default_rng(31)
    for c in (tg, sr):                                             # half of the normals turned round
        c[rng.random(len(c)) < 0.5, 3:] *= -1
    pt, ps, px = str(d / "t.ply"), str(d / "s.ply"), str(d / "x.ply")
    write_ply(pt, tg)
    write_ply(ps, sr)
    with open(px, "wb") as f:                                      # the target without normals
        f.write(f"ply\nformat binary_little_endian 1.0\nelement vertex {len(tg)}\nproperty float x\nproperty float y\nproperty float z\n"
                "end_header\n".encode())
        f.write(np.ascontiguousarray(tg[:, :3], "<f4").tobytes())
    base = {k: v for k, v in os.environ.items() if not k.startswith("PLADE_")}
    base["PLADE_ORIENT_NORMALS"] = "1"

    def run(without_normals=False, **extra):
        res = str(d / "r.txt")
        if os.path.exists(res):
            os.remove(res)
        r = subprocess.run([CLI, px if without_normals else pt, ps, res], capture_output=True, text=True, timeout=300, env=dict(base, **extra))
        return r, (open(res).read() if os.path.exists(res) else None)

    r0, res0 = run()
    assert "target file:" in r0.stdout, r0.stdout + r0.stderr
    return tg, sr, run, r0, res0


def test_lines_carry_the_restated_counts(pair, ctx):
    tg, sr, run, r0, res0 = pair
    for value, radius, kw in (("0.15", 0.15, {}), ("0.2,1,1", 0.2, dict(mode=1, inward=1))):
        want = []
        for P in (tg, sr):
            ref = OR.orient(P, radius, **kw)
            rounds = ctx.orient_consistent(P, radius, per_point=False, **kw)[1]["rounds"]
            want.append(LINE % (ref["flipped"], len(P), ref["components"], radius, ref["unoriented"], rounds))
        r, _ = run(**{VAR: value})
        assert lines(r.stdout, "consistent normals: ") == want, r.stdout + r.stderr
        assert r.stdout.index("target file:") < r.stdout.index("consistent normals: ") and "normal orientation failed" not in r.stderr
    assert lines(r0.stdout, "consistent normals: ") == []


def test_it_runs_after_the_estimate_and_before_the_subsample(pair, ctx):
    tg, sr, run, r0, res0 = pair
    r, _ = run(without_normals=True, PLADE_ESTIMATE_NORMALS="12", PLADE_SUBSAMPLE="0.3", **{VAR: "0.15"})
    est = ctx.estimate_normals(tg[:, :3], k=12)                    # the estimate's normals face the origin point by point ...
    ref = OR.orient(est, 0.15)                                     # ... and the orientation sees exactly those, at full density
    got = lines(r.stdout, "consistent normals: ")
    assert len(got) == 2 and got[0].startswith("consistent normals: flipped %d of %d points in %d components (radius 0.15, %d without a normal, "
                                               % (ref["flipped"], len(tg), ref["components"], ref["unoriented"])), r.stdout + r.stderr
    sub = lines(r.stdout, "subsample: ")
    assert len(sub) == 2 and sub[0].split(" of ")[1].startswith(f"{len(tg)} points")
    assert r.stdout.index("consistent normals: ") < r.stdout.index("subsample: ")


def test_unset_or_zero_changes_no_byte(pair):
    tg, sr, run, r0, res0 = pair
    for value in ("0", "0,1", "0,1,1", "-0"):
        r, res = run(**{VAR: value})
        assert res == res0 and r.stderr == r0.stderr and strip_time(r.stdout) == strip_time(r0.stdout) and r.returncode == r0.returncode, value


def test_bad_values_warn_once_and_are_ignored(pair):
    tg, sr, run, r0, res0 = pair
    for badv in ("wide", "0.15,2", "0.15,", "0.15,1,1,1", "inf", "-1"):
        rb, resb = run(**{VAR: badv})
        assert rb.stderr.count(f"warning: {VAR}={badv} is not <radius>[,<mode>[,<inward>]]") == 1 and rb.stderr.count("no orientation") == 1, badv
        assert resb == res0 and strip_time(rb.stdout) == strip_time(r0.stdout), badv
        assert "".join(l + "\n" for l in rb.stderr.split("\n")[:-1] if not l.startswith(f"warning: {VAR}=")) == r0.stderr, badv


def test_fpfh_of_the_reoriented_cloud_is_that_of_the_original(ctx):
    """a smooth closed surface with outward normals, half of them turned round: EXTREME along +z puts the anchor, the top point,
    back on its original side, the forest carries that to every point, and the descriptors of the result equal the original's bit
    for bit -- which those of the flipped cloud do not"""
    P, U = OR.sphere(3000)
    P[:, 0] *= 1.5                                                 # (an ellipsoid: the descriptors differ from point to point)
    N = U.astype(np.float64) / np.asarray([1.5, 1.0, 1.0])
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    original = OR.with_normals(P, N)
    flipped = OR.with_normals(P, OR.random_flips(original[:, 3:]))
    assert 1200 < (flipped[:, 3:] != original[:, 3:]).any(1).sum() < 1800
    rows, info = ctx.orient_consistent(flipped, 2.0, mode=plade_amd.ORIENT_EXTREME)
    assert info["components"] == 1 and rows.tobytes() == original.tobytes()
    d0, i0 = ctx.fpfh(original, 3.0)
    d1, i1 = ctx.fpfh(rows, 3.0)
    d2, i2 = ctx.fpfh(flipped, 3.0)
    assert i0["described"] == 3000 and d1.tobytes() == d0.tobytes() and d2.tobytes() != d0.tobytes()
    assert np.nanmax(np.abs(d2 - d0)) > 5.0                            # (bins are percentages: the flipped normals move whole bins)

