"""The penetration filter (plade_amd/csrc/k_penetration.hip) item by item against the oracle's seam (orc_penetration_items): which
triples (candidate k, source plane i1, target plane j1) reach the walks, every float of their common segment BIT-EQUAL, every
count of both walks, the verdicts, and the flags of an ordinary (non-audit) call.  No item is left out of a comparison.
Tables: the real ones of the golden scenes (K = 201) and the synthetic ones of tests/pen_cases.py."""
import numpy as np
import pytest

import plade_amd
import pen_cases
from oracle.oracle import PEN_WALKED

pytestmark = pytest.mark.gpu
MODES = [1, 0]          # plade_params.closest_point_mode: the reference's fp32 SVD solves (default) / the closed form
FLOORS = {"g8": (2000, 144), "g9": (2000, 4), "g9b": (2000, 0)}     # walked, penetrating triples (tests/test_penetration_items_host.py)
STATUS = ("gated out", "no intersection line", "no edge hits", "hit count other than 2", "no overlap", "walked")
FLOATS = ("plane1", "start", "direc", "length")


@pytest.fixture(scope="module")
def pctx():
    c = {m: plade_amd.Context(0, closest_point_mode=m) for m in MODES}
    yield c
    for v in c.values():
        v.close()


def oracle_items(oracle, tb, mode):
    oracle.set_closest_point_mode(mode)
    try:
        return tb.oracle_items(oracle)
    finally:
        oracle.reset_closest_point_mode()


def sorted_items(tb, items):
    ps, pt = len(tb.src[0]), len(tb.tgt[0])
    key = (items["k"].astype(np.int64) * ps + items["i1"]) * pt + items["j1"]
    order = np.argsort(key, kind="stable")
    return key[order], items[order]


def check(tb, rec, flags, items, plain, where):
    """GPU audit (flags, items) and the flags of a non-audit call (plain) against the oracle's records of the same tables."""
    K, ps, pt = len(tb.cand), len(tb.src[0]), len(tb.tgt[0])

    def name(q):
        return f"{where}: item (k {q // (ps * pt)}, i1 {q // pt % ps}, j1 {q % pt})"
    assert len(rec) == K * ps * pt
    want = np.nonzero(rec["status"] == PEN_WALKED)[0]
    key, it = sorted_items(tb, items)
    assert len(np.unique(key)) == len(key), f"{where}: an item was emitted twice"
    for q in np.setdiff1d(want, key)[:3]:
        raise AssertionError(f"{name(q)} is walked by the oracle and not emitted")
    for q in np.setdiff1d(key, want)[:3]:
        raise AssertionError(f"{name(q)} is emitted; the oracle has it as '{STATUS[rec['status'][q]]}'")
    o = rec[want]
    for f in FLOATS:
        a, b = np.atleast_2d(it[f].T).T, np.atleast_2d(o[f].T).T
        bad = np.nonzero((a.view(np.uint32) != b.view(np.uint32)).any(axis=1))[0]
        if len(bad):
            q = bad[0]
            raise AssertionError(f"{name(want[q])} field {f}: {a[q].tolist()} != oracle {b[q].tolist()} ({len(bad)} of {len(it)} items differ)")
    ints = (("nsteps", it["nsteps"], o["nsteps"]), ("pos", it["pos"], o["positive"]), ("neg", it["neg"], o["negative"]),
            ("gated", it["gated"], o["nsteps"][:, None] - o["skipped"]), ("verdict", it["verdict"], o["verdict"]))
    for f, a, b in ints:
        a, b = np.atleast_2d(a.T).T, np.atleast_2d(b.T).T
        bad = np.nonzero((a != b).any(axis=1))[0]
        if len(bad):
            q = bad[0]
            raise AssertionError(f"{name(want[q])} field {f}: {a[q].tolist()} != oracle {b[q].tolist()}; nsteps {o['nsteps'][q]}, "
                                 f"oracle pos {o['positive'][q].tolist()} neg {o['negative'][q].tolist()} ({len(bad)} of {len(it)} items differ)")
    by_or = np.zeros(K, np.int32)
    np.maximum.at(by_or, it["k"].astype(np.int64), it["verdict"])
    orc = rec["verdict"].reshape(K, -1).max(axis=1) if K and ps and pt else np.zeros(K, np.int32)
    assert np.array_equal(flags, by_or), f"{where}: audit flags != OR of the audit verdicts at k {np.nonzero(flags != by_or)[0][:5]}"
    assert np.array_equal(flags, orc), f"{where}: flags != oracle at k {np.nonzero(flags != orc)[0][:5]}"
    assert np.array_equal(plain, flags), f"{where}: non-audit flags != audit flags at k {np.nonzero(plain != flags)[0][:5]}"
    return o, it


def run(ctx, oracle, tb, mode, where):
    rec = oracle_items(oracle, tb, mode)
    flags, items = ctx.penetration_filter(tb.cand, tb.src, tb.tgt, tb.length_threshold, tb.angle_threshold, audit=True)
    plain = ctx.penetration_filter(tb.cand, tb.src, tb.tgt, tb.length_threshold, tb.angle_threshold)
    o, it = check(tb, rec, flags, items, plain, f"{where}, mode {mode}")
    return rec, o, it, flags


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", [n for n, _, _ in pen_cases.SCENES])
def test_real_tables_every_item_equals_the_oracle(pctx, oracle, name, mode):
    """K = 201 is no multiple of the 4 items of a workgroup, the triples no multiple of the 64 lanes of the pooled setup."""
    tb, loop_flags, rec, _ = pen_cases.scene(oracle, name, mode)
    assert len(tb.cand) == 201 and len(rec) % 64 != 0
    flags, items = pctx[mode].penetration_filter(tb.cand, tb.src, tb.tgt, tb.length_threshold, tb.angle_threshold, audit=True)
    plain = pctx[mode].penetration_filter(tb.cand, tb.src, tb.tgt, tb.length_threshold, tb.angle_threshold)
    o, it = check(tb, rec, flags, items, plain, f"{name}, mode {mode}")
    assert np.array_equal(flags, loop_flags)
    print(f"{name} mode {mode}: {len(it)} items, {int(it['verdict'].sum())} penetrating, {int(flags.sum())} candidates flagged")
    assert len(it) >= FLOORS[name][0] and int(it["verdict"].sum()) >= FLOORS[name][1]


@pytest.mark.parametrize("mode", MODES)
def test_synthetic_crossings_rotations_and_a_far_frame(pctx, oracle, mode):
    tb = pen_cases.rotation_tables()
    rec, o, it, _ = run(pctx[mode], oracle, tb, mode, "rotations 0 44 45 46 90 180")
    assert len(it) == 6 and it["verdict"].all()
    # the walk's major axis in the target grid: u up to 45 degrees, v from 46 on; 180 degrees walks the other way
    d = it["direc"]
    assert (np.abs(d[[0, 1], 0]) > np.abs(d[[0, 1], 1])).all() and (np.abs(d[[3, 4], 0]) < np.abs(d[[3, 4], 1])).all()
    assert np.sign(d[0, 0]) == -np.sign(d[5, 0])
    if mode == 0:   # exact operands: points at exactly r/2 and exactly r from step points exist, and the strict < leaves them out
        r = float(tb.length_threshold)
        t, s = tb.tgt[3].astype(np.float64), tb.src[3].astype(np.float64)
        step = it["start"][0].astype(np.float64) + r * np.arange(it["nsteps"][0])[:, None] * it["direc"][0].astype(np.float64)
        d2t = ((step[:, None, :] - t[None]) ** 2).sum(-1)
        d2s = ((step[:, None, :] - s[None]) ** 2).sum(-1)
        assert (d2t == (r / 2) ** 2).any() and (d2s == r * r).any()
        assert it["gated"][0, 0] == ((d2t < (r / 2) ** 2).sum(1) >= 2).sum()
        near = ((d2s < r * r) & ((d2t < (r / 2) ** 2).sum(1) >= 2)[:, None]).any(0)
        assert it["pos"][0, 0] == (near & (s[:, 2] > r / 2)).sum() and it["neg"][0, 0] == (near & (s[:, 2] < -r / 2)).sum()
    rec, o, it, _ = run(pctx[mode], oracle, pen_cases.far_frame_tables(), mode, "far frame")
    assert len(it) == 2 and it["verdict"].all()


@pytest.mark.parametrize("mode", MODES)
def test_oblique_walks_through_a_dense_cloud(pctx, oracle, mode):
    """Candidates chosen so that a counted point sits in a cell which a column reaches only with the full `pad` of pen_visit."""
    rec, o, it, _ = run(pctx[mode], oracle, pen_cases.pad_tables(), mode, "oblique walks")
    assert len(it) == len(pen_cases.PAD_CANDIDATES) and (it["pos"][:, 1] >= 100).all()     # pass 1 counts the target points


@pytest.mark.parametrize("mode", MODES)
def test_long_segments_up_to_the_step_limit(pctx, oracle, mode):
    want = [140, 280, 600, 1023, 1024]
    rec, o, it, _ = run(pctx[mode], oracle, pen_cases.long_tables(want), mode, "long segments")
    assert it["nsteps"].tolist() == want and it["verdict"].all()
    assert np.array_equal(it["gated"], np.repeat(it["nsteps"][:, None], 2, axis=1))
    tb = pen_cases.long_tables([1025])
    assert oracle_items(oracle, tb, mode)["nsteps"].tolist() == [1025]
    for audit in (False, True):
        with pytest.raises(plade_amd.PladeError) as e:
            pctx[mode].penetration_filter(tb.cand, tb.src, tb.tgt, tb.length_threshold, tb.angle_threshold, audit=audit)
        assert e.value.code == plade_amd.PLADE_ELIMIT
    run(pctx[mode], oracle, pen_cases.long_tables([140]), mode, "after the refused call")     # the context is still usable


@pytest.mark.parametrize("mode", MODES)
def test_crowded_and_sparse_cells(pctx, oracle, mode):
    rec, o, it, _ = run(pctx[mode], oracle, pen_cases.crowded_tables(), mode, "crowded / sparse")
    assert len(it) == 2
    assert it["pos"][0].min() > 600 and it["neg"][0].min() > 600            # the crowded cell is counted, duplicates included
    n = int(it["nsteps"][1])
    assert 0 < it["gated"][1, 0] < n and 0 < it["gated"][1, 1] < n         # one point is no gate, two are
    assert it["pos"][1].max() <= n                                          # a point within r of two steps is counted once
    if mode == 0:   # exact operands: steps x = r, 2r, ... 32r; two gate points at x = i r where i % 3 == 2 (pass 0) / i odd (pass 1)
        assert it["gated"][1].tolist() == [10, 16]


@pytest.mark.parametrize("mode", MODES)
def test_thresholds_on_either_side(pctx, oracle, mode):
    tb = pen_cases.threshold_tables()
    rec, o, it, flags = run(pctx[mode], oracle, tb, mode, "thresholds")
    n = len(pen_cases.THRESHOLD_CASES)
    assert len(it) == n and flags.tolist() == [1]
    for q, (c0, c1) in enumerate(pen_cases.THRESHOLD_CASES):
        got = it[(it["i1"] == q) & (it["j1"] == q)][0]
        assert ((got["pos"][0], got["neg"][0]), (got["pos"][1], got["neg"][1])) == (c0, c1), f"pair {q}"
        assert got["verdict"] == pen_cases.reference_rule(c0, c1), f"pair {q}: counts {c0} {c1}"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", [("tgt", "major"), ("src", "major"), ("tgt", "minor"), ("src", "minor")], ids="-".join)
def test_walk_beyond_the_grid_cap(pctx, oracle, which, mode):
    """A plane of 5120 cells on an axis whose grid stops at 4096: every point beyond lies in the last cell, and a walk out there
    has to look into it.  (Before the clamp of ca0 / cb0 in pen_visit it visited no cell and counted nothing.)"""
    rec, o, it, _ = run(pctx[mode], oracle, pen_cases.cap_tables(which), mode, f"grid cap {which}")
    assert len(it) == 1 and it["verdict"][0] == 1 and it["pos"].min() >= 64 and (it["gated"] == it["nsteps"][0]).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["no_candidates", "no_source_planes", "no_target_planes", "empty_plane", "gated", "parallel",
                                  "edge_parallel", "corner"])
def test_degenerate_tables(pctx, oracle, kind, mode):
    tb = pen_cases.degenerate_tables(kind)
    rec, o, it, flags = run(pctx[mode], oracle, tb, mode, kind)
    if kind in ("no_candidates", "no_source_planes", "no_target_planes", "gated", "parallel"):
        assert len(it) == 0 and not flags.any()
    if kind in ("gated", "parallel"):
        assert rec["status"].tolist() == [{"gated": 0, "parallel": 1}[kind]]
    if kind == "empty_plane":
        # (the two empty planes meet as well: an item whose walks see nothing)
        assert [(q["i1"], q["j1"], q["verdict"], q["pos"].sum() + q["neg"].sum() + q["gated"].sum() > 0) for q in it] == [(0, 1, 0, False), (1, 0, 1, True)]
    if kind == "corner" and mode == 0:
        assert rec["status"].tolist() == [3] and len(it) == 0


@pytest.mark.parametrize("mode", MODES)
def test_repetition_and_a_second_context(pctx, oracle, mode):
    tb = pen_cases.scene(oracle, "g9", mode)[0]
    args = (tb.cand, tb.src, tb.tgt, tb.length_threshold, tb.angle_threshold)
    f0, a0 = pctx[mode].penetration_filter(*args, audit=True)
    f1, a1 = pctx[mode].penetration_filter(*args, audit=True)
    other = plade_amd.Context(0, closest_point_mode=mode)
    try:
        f2, a2 = other.penetration_filter(*args, audit=True)
    finally:
        other.close()
    ref = sorted_items(tb, a0)[1].tobytes()
    assert sorted_items(tb, a1)[1].tobytes() == ref and sorted_items(tb, a2)[1].tobytes() == ref
    assert np.array_equal(f0, f1) and np.array_equal(f0, f2)
