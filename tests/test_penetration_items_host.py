"""The oracle's item-by-item seam of the penetration filter (orc_penetration_items) against the oracle's own short-circuited loop
(orc_registration) and its single walk (orc_pen_walk, pinned against FLANN in test_oracle_golden.py / test_oracle_vs_ref.py).
CPU only.  The GPU filter is compared with this seam record by record in tests/test_gpu_penetration.py."""
import numpy as np
import pytest

import pen_cases
from oracle.oracle import PEN_WALKED

# the short-circuited loop already walks 4501 / 2855 / 3567 pairs and flags 144 / 4 / 0 candidates: the full seam gives no fewer
FLOORS = {"g8": (2000, 144), "g9": (2000, 4), "g9b": (2000, 0)}
scene = pen_cases.scene


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("name", [n for n, _, _ in pen_cases.SCENES])
def test_or_of_item_verdicts_is_the_loops_flag(oracle, name, mode):
    tb, flags, rec, dt = scene(oracle, name, mode)
    K, ps, pt = len(tb.cand), len(tb.src[0]), len(tb.tgt[0])
    assert K == len(flags) and len(rec) == K * ps * pt
    k, i1, j1 = np.unravel_index(np.arange(len(rec)), (K, ps, pt))
    assert np.array_equal(rec["k"], k) and np.array_equal(rec["i1"], i1) and np.array_equal(rec["j1"], j1)
    walked = rec["status"] == PEN_WALKED
    assert not rec["verdict"][~walked].any()
    got = rec["verdict"].reshape(K, -1).max(axis=1)
    assert np.array_equal(got, flags), np.nonzero(got != flags)[0]
    n_walked, n_pen = int(walked.sum()), int(rec["verdict"].sum())
    print(f"{name} mode {mode}: K {K}, {ps} x {pt} planes, statuses {np.bincount(rec['status'], minlength=6).tolist()}, "
          f"{n_pen} penetrating, seam {dt:.2f} s")
    assert n_walked >= FLOORS[name][0] and n_pen >= FLOORS[name][1]


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("name", [n for n, _, _ in pen_cases.SCENES])
def test_walked_records_equal_the_single_walk(oracle, name, mode):
    """Both walks of a sample of walked records (every penetrating one, the longest, and a stride of the rest) through orc_pen_walk
    on the same operands."""
    tb, _, rec, _ = scene(oracle, name, mode)
    w = np.nonzero(rec["status"] == PEN_WALKED)[0]
    pick = set(w[:: max(1, len(w) // 60)].tolist()) | set(w[rec["verdict"][w] == 1][:40].tolist())
    pick |= set(w[np.argsort(rec["nsteps"][w])[-10:]].tolist())
    r = np.float32(np.float64(tb.length_threshold))
    md = np.float32(np.float64(tb.length_threshold) / 2)
    both = 0
    for q in sorted(pick):
        it = rec[q]
        c = tb.cand[it["k"]]
        R, T = c[:9].reshape(3, 3), c[9:]
        sp = tb.src[3][tb.src[4][it["i1"]]:tb.src[4][it["i1"] + 1]]
        # pcl::transformPointCloud: (R00 x + R01 y + R02 z) + T0, left to right in fp32
        moved = ((R[:, 0] * sp[:, :1] + R[:, 1] * sp[:, 1:2]) + R[:, 2] * sp[:, 2:3]) + T
        tp = tb.tgt[3][tb.tgt[4][it["j1"]]:tb.tgt[4][it["j1"] + 1]]
        w0 = oracle.pen_walk(moved, tp, tb.tgt[0][it["j1"]], it["start"], it["direc"], it["length"], r, md)
        w1 = oracle.pen_walk(tp, moved, it["plane1"], it["start"], it["direc"], it["length"], r, md)
        for wi, got in enumerate((w0, w1)):
            want = (it["positive"][wi], it["negative"][wi], it["skipped"][wi])
            assert got == want, f"item (k {it['k']}, i1 {it['i1']}, j1 {it['j1']}) walk {wi}: {got} != record {want}"
        assert it["skipped"].max() <= it["nsteps"]
        both += (it["positive"][0] < 10 or it["negative"][0] < 10) and (it["positive"][1] + it["negative"][1] > 0)
    assert both > 0, "no sampled record shows a second walk behind a failed first one"
