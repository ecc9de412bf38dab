"""The CLI's PLADE_M3C2_NORMALS=<r_min>,<r_max>[,<scales>[,<mode>]] switch (plade_host.cpp): the core points of PLADE_M3C2 -- the
whole target, or the PLADE_M3C2_CORE subsample -- get multi-scale normals estimated on the target instead of the file's.  The pair
is a small synthetic room whose file normals are those of a single small neighbourhood (the generator's jittered ones): what the
switch is for.

With PLADE_M3C2 alone the output is the parent's, byte for byte.  With the switch the `m3c2 normals:` line carries the
restatement's numbers (tests/scales_restate.py: the fitted count and the largest neighbourhood as they stand, the histogram through
the library's chosen scales, which equal the restated ones outside the restatement's unsure set -- one query of 30000 here).

The m3c2 line is held against Context.m3c2 at core points that carry the RESTATED normals (numpy's eigh, rounded to fp32).  Those are
not the library's bits, so the bounds are derived, not exact:
  DELTA   the angle between a restated chosen normal and the library's where the restated (l2 - l3) / trace > 1e-3 and the query is
          sure: two unit vectors rounded to fp32 are each within sqrt(3) 2^-25 = 5.2e-8 of their fp64 originals, which two
          backward-stable fp64 solvers give to 1e-13 / gap <= 1e-10: 1.1e-7 in all; 2e-7 is asserted.  The other fitted core points
          (U of them, at most 1 %, asserted on the restatement alone) have no such bound and count as possible events below.
  SLACK   a point of a cylinder lies within REACH = sqrt(R^2 + L^2) of its core point, so turning the axis by DELTA moves its t and
          its distance from the axis by at most REACH DELTA = 1.1e-7.
  TOL_D   a core point whose cylinders hold the same points under both axes: each of its two means moves by at most SLACK, its
          distance by 2 SLACK; 3e-7 with the fp64 sums' own noise.
  EVENTS  a core point whose cylinders do NOT hold the same points: some point lies within SLACK of a wall (radius R) or an end
          (+-L).  A cylinder holds about 2 x 22 points here (110 points / m^2, pi R^2 = 0.2 m^2); the shell within SLACK of the
          walls is 2 SLACK / R + SLACK / L = 1.1e-6 of its volume: 5e-5 expected per core point, 1.5 over 30000 core points.  Eight
          are allowed (a Poisson count of mean 1.5 exceeds 8 with probability 1e-5), counted per core point from the two calls'
          per-point counts.
So: counts of valid and significant core points within K = 8 + U (+ the core points whose |distance| is within TOL_D of its level
of detection, for `significant`); an event moves one core point's distance by at most 2 L or takes it in or out of the valid ones,
so mean within TOL_D + K 2 L / valid and rms within sqrt(TOL_D^2 + K (2 L)^2 / valid), each plus the 5e-6 relative rounding of the
line's %.6g; max within TOL_D (and the rounding) when the core point that holds it is no event.  Away from the events every
per-point distance is within TOL_D.  The same line is also pinned bit for bit on Context.m3c2 with the library's own normals (the CLI
makes the same two calls): an extra, not the reference.  A bad value prints the one warning and leaves the parent's output."""
import os
import re
import subprocess

import numpy as np
import pytest

import scales_restate as R
import subsample_restate as SR
from plade_amd.plyio import write_ply
from plade_amd.synth import make_pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "plade_amd", "PLADE")
M3C2 = "0.25,0.5"
M3C2_LINE = "m3c2: %d of %d core points valid, %d significant (mean %.6g, rms %.6g, max %.6g)"
NORMALS_LINE = "m3c2 normals: %d of %d core points fitted (scales%s; largest neighbourhood %d)"
R_MIN, R_MAX = 0.15, 0.45
RADIUS, DEPTH = 0.25, 0.5
DELTA, EVENTS, PRINT = 2e-7, 8, 5e-6
TOL_D = 3e-7                           # >= 2 sqrt(R^2 + L^2) DELTA = 2.24e-7
LINE_RE = r"m3c2: (\d+) of (\d+) core points valid, (\d+) significant \(mean (\S+), rms (\S+), max (\S+)\)"


def radii(scales):
    return [R_MIN + (R_MAX - R_MIN) * s / (scales - 1) for s in range(scales)]


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
    d = tmp_path_factory.mktemp("scales_cli")
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

    m0, mres0 = run(PLADE_M3C2=M3C2)
    assert m0.returncode == 0 and "transformation:" in mres0 and len(lines(m0.stdout, "m3c2: ")) == 1, m0.stdout + m0.stderr
    return tg, sr, run, m0, mres0


def test_with_m3c2_alone_nothing_changes(pair):
    tg, sr, run, m0, mres0 = pair
    assert lines(m0.stdout, "m3c2 normals: ") == []
    r0, res0 = run()
    r1, res1 = run(PLADE_M3C2_NORMALS="0.15,0.45")                  # without PLADE_M3C2 the switch does nothing
    assert res1 == res0 and r1.stderr == r0.stderr and strip_time(r1.stdout) == strip_time(r0.stdout)


@pytest.fixture(scope="module")
def restated(pair):
    """the target at the four radii, mode 0 (computed once, never changed)"""
    return R.scales(pair[0], radii(4), mode=0, orient=1)


@pytest.mark.parametrize("value,scales,mode", [("0.15,0.45", 4, 0), ("0.15,0.45,4,1", 4, 1)])
def test_core_points_get_the_multi_scale_normals(pair, restated, ctx, value, scales, mode):
    tg, sr, run, m0, mres0 = pair
    ok, Tr = ctx.registration(tg, sr)                               # the CLI's registration, with all its digits
    assert ok and np.allclose(_matrix(mres0), Tr, rtol=2e-5, atol=2e-6)
    rr = radii(scales)
    ref = dict(restated)
    if mode == 1:
        ref["criterion"] = R.criterion(ref["features"], 1)
        ref["chosen"] = R.choose(ref["criterion"], ref["fitted"])
        ref["unsure"] = R.unsure(ref["criterion"], ref["fitted"], ref["count"], ref["eigenvalues"])
        ref["normal"] = R.pick(ref["normals"], ref["chosen"])
    assert ref["unsure"].mean() <= 0.01 and 0 < (ref["chosen"] >= 0).sum()     # on the restatement alone
    for core_value, q in ((None, None), ("0.3,5", SR.subsample(tg[:, :3], 0.3, 5)["kept_index"])):
        idx = np.arange(len(tg)) if q is None else np.asarray(q, np.int64)
        nrm, info = ctx.scale_features(tg, rr, mode=mode, orient=1, query_index=q)
        sure = ~ref["unsure"][idx]
        assert np.array_equal(info["chosen"][sure], ref["chosen"][idx][sure])
        assert np.array_equal(info["chosen"] >= 0, ref["chosen"][idx] >= 0)
        want = R.summary(info["chosen"], ref["count"][idx], scales)
        assert {k: info[k] for k in want} == want
        fitted = ref["chosen"][idx] >= 0
        clear = sure & fitted & (ref["gap"][idx, np.maximum(ref["chosen"][idx], 0)] > 1e-3)
        U = int((fitted & ~clear).sum())
        assert U <= 0.01 * fitted.sum()                                         # on the restatement alone
        a, b = nrm[clear].astype(np.float64), ref["normal"][idx][clear].astype(np.float64)
        ang = np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), (a * b).sum(1))        # the same side, too
        print(f"mode {mode}, core {core_value}: max angle to the restated normals {ang.max():.3e} (DELTA {DELTA}), unbounded {U}")
        assert ang.max() <= DELTA
        # the reference: M3C2 at the core points with the RESTATED normals
        core_ref = np.ascontiguousarray(np.concatenate([tg[idx, :3], ref["normal"][idx]], axis=1))
        d_ref, m_ref = ctx.m3c2(core_ref, tg, sr, RADIUS, DEPTH, T=Tr)
        core = np.ascontiguousarray(np.concatenate([tg[idx, :3], nrm], axis=1))
        d_lib, m = ctx.m3c2(core, tg, sr, RADIUS, DEPTH, T=Tr)
        event = (m["count"] != m_ref["count"]).any(axis=1) | (np.isnan(d_lib) != np.isnan(d_ref))
        calm = ~event & (clear | ~fitted)
        both = calm & ~np.isnan(d_ref)
        print(f"  events {int((event & clear).sum())} (allowed {EVENTS}), worst calm |d - d_ref| {np.abs(d_lib[both] - d_ref[both]).max():.3e} (TOL_D {TOL_D})")
        assert (event & clear).sum() <= EVENTS and not event[~fitted].any()
        assert (np.abs(d_lib[both] - d_ref[both]) <= TOL_D).all()
        extra = dict(PLADE_M3C2=M3C2, PLADE_M3C2_NORMALS=value)
        if core_value:
            extra["PLADE_M3C2_CORE"] = core_value
        r, res = run(**extra)
        hist = "".join(" %d" % h for h in want["chosen_hist"])
        assert lines(r.stdout, "m3c2 normals: ") == [NORMALS_LINE % (want["fitted"], len(idx), hist, want["max_count"])], r.stdout + r.stderr
        got = lines(r.stdout, "m3c2: ")
        assert len(got) == 1 and re.fullmatch(LINE_RE, got[0]), got
        w = re.fullmatch(LINE_RE, got[0]).groups()
        valid, cores, signif = int(w[0]), int(w[1]), int(w[2])
        mean, rms, mx = float(w[3]), float(w[4]), float(w[5])
        K = EVENTS + U
        ok_ref = ~np.isnan(d_ref)
        edge = int((np.abs(np.abs(d_ref[ok_ref]) - m_ref["lod"][ok_ref]) <= TOL_D).sum())
        print(f"  line {got[0]!r}; with the restated normals: valid {m_ref['valid']}, significant {m_ref['significant']}, "
              f"mean {m_ref['mean']!r}, rms {m_ref['rms']!r}, max {m_ref['max']!r}; K {K}, edge {edge}")
        assert cores == len(idx) == m_ref["m"]
        assert abs(valid - m_ref["valid"]) <= K and abs(signif - m_ref["significant"]) <= K + edge
        assert abs(mean - m_ref["mean"]) <= TOL_D + K * 2 * DEPTH / m_ref["valid"] + PRINT * abs(m_ref["mean"])
        assert abs(rms - m_ref["rms"]) <= np.sqrt(TOL_D ** 2 + K * (2 * DEPTH) ** 2 / m_ref["valid"]) + PRINT * m_ref["rms"]
        if calm[np.nanargmax(np.abs(d_ref))] and calm[np.nanargmax(np.abs(d_lib))]:
            assert abs(mx - m_ref["max"]) <= TOL_D + PRINT * m_ref["max"]
        # an extra: the CLI makes the same two calls as above, so its line is also that of the library's own normals, bit for bit
        assert got == [M3C2_LINE % (m["valid"], len(idx), m["significant"], m["mean"], m["rms"], m["max"])]
        assert r.stdout.index("m3c2 normals: ") < r.stdout.index("m3c2: ") and res == mres0 and r.stderr == m0.stderr
        assert got != lines(m0.stdout, "m3c2: ")                               # the normals matter


def test_bad_values_warn_once_and_are_ignored(pair):
    tg, sr, run, m0, mres0 = pair
    for badv in ("wide", "0.15", "0.45,0.15", "0.15,0.45,9", "0.15,0.45,4,2", "0.15,,4", "0.3,0.3"):
        rb, resb = run(PLADE_M3C2=M3C2, PLADE_M3C2_NORMALS=badv)
        assert rb.stderr.count(f"warning: PLADE_M3C2_NORMALS={badv} is not <r_min>,<r_max>[,<scales>[,<mode>]]") == 1, badv
        assert rb.stderr.count("the core points keep their normals") == 1, badv
        assert resb == mres0 and strip_time(rb.stdout) == strip_time(m0.stdout), badv
        assert "".join(l + "\n" for l in rb.stderr.split("\n")[:-1] if not l.startswith("warning: PLADE_M3C2_NORMALS=")) == m0.stderr, badv
