"""The restatement of DBSCAN (tests/dbscan_restate.py) pinned without a GPU: against a plain-Python textbook DBSCAN over the float32
predicate, its two edge paths against each other, min_points = 1 against the components, the library's documented defaults; and
the two switches of the CLI (PLADE_DBSCAN, PLADE_M3C2_CLUSTERS: cli_switches.h) through a stand-alone program built with the address
and undefined-behaviour sanitizers (tests/cxx/dbscan_switch_harness.cpp)."""
import os
import subprocess
from collections import deque

import numpy as np
import pytest

import plade_amd
import components_restate as CR
import dbscan_restate as DR

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def textbook_dbscan(P, r, min_points):
    """(label, kind): region queries one float32 predicate at a time, clusters expanded from seeds in ascending index through core
    points only, then every non-core point with a core point in its region re-attached by the (d, j) rule."""
    X = np.asarray(P, F32)[:, :3]
    n = len(X)
    r2 = F32(r) * F32(r)

    def d2(i, j):
        dx, dy, dz = X[i, 0] - X[j, 0], X[i, 1] - X[j, 1], X[i, 2] - X[j, 2]
        return F32(F32(F32(dx * dx) + F32(dy * dy)) + F32(dz * dz))

    region = [[j for j in range(n) if d2(i, j) < r2] for i in range(n)]        # (the point itself: d = 0 < r2)
    core = [len(region[i]) >= min_points for i in range(n)]
    label = [-1] * n
    c = 0
    for s in range(n):                       # ascending: a new cluster is met at its smallest core index
        if not core[s] or label[s] >= 0:
            continue
        label[s] = c
        todo = deque([s])
        while todo:
            i = todo.popleft()
            for j in region[i]:
                if core[j] and label[j] < 0:
                    label[j] = c
                    todo.append(j)
        c += 1
    kind = [2 if core[i] else 0 for i in range(n)]
    for i in range(n):
        if core[i]:
            continue
        cand = [(d2(i, j), j) for j in region[i] if core[j]]
        if cand:
            label[i] = label[min(cand)[1]]
            kind[i] = 1
    return np.asarray(label, np.int32), np.asarray(kind, np.uint8)


def test_restatement_against_textbook_dbscan():
    rng = np.random.default_rng(11)
    seen = set()
    for n, r, mp in ((1, 0.1, 1), (1, 0.1, 2), (2, 0.5, 2), (2, 0.5, 3), (60, 0.2, 3), (60, 0.25, 5), (150, 0.12, 3), (150, 0.17, 5),
                     (150, 0.2, 8)):
        P = rng.random((n, 3)).astype(F32)
        P[n // 2] = P[0]                     # a duplicate
        label, kind = textbook_dbscan(P, r, mp)
        out = DR.dbscan(P, r, mp)
        assert np.array_equal(out["label"], label) and np.array_equal(out["kind"], kind), (n, r, mp)
        C = label.max() + 1
        assert out["clusters"] == C and np.array_equal(out["size"], np.bincount(label[label >= 0], minlength=C).astype(np.uint32))
        assert (out["core"], out["border"], out["noise"]) == tuple(int((kind == k).sum()) for k in (2, 1, 0))
        assert out["kept"] == int((label >= 0).sum()) and np.array_equal(out["keep"], label >= 0)
        seen |= set(kind.tolist())
    assert seen == {0, 1, 2}


def test_border_tie_goes_to_the_smaller_index():
    q, a, b = [[0, 0, 0]], [[-0.5, 0, 0]] + [[-1, 0, 0]] * 5, [[0.5, 0, 0]] + [[1, 0, 0]] * 5
    for rows in (q + a + b, q + b + a):      # q is 0.5 from both inner points: it joins whichever comes first
        P = np.array(rows, F32)
        out = DR.dbscan(P, 0.625, 5)
        assert out["label"].tolist() == [0] * 7 + [1] * 6 and out["kind"].tolist() == [1] + [2] * 12
        assert out["contested"] == 1
        label, kind = textbook_dbscan(P, 0.625, 5)
        assert np.array_equal(label, out["label"]) and np.array_equal(kind, out["kind"])


def test_both_edge_paths_agree_on_5k():
    rng = np.random.default_rng(5)
    P = (rng.random((5000, 3)) * np.array([4.0, 3.0, 0.05])).astype(F32)   # a noisy slab: about 13 points within r
    r = 0.1
    a, b = CR.edges_brute(P, r), CR.edges_kdtree(P, r)
    assert len(a) > 20000 and np.array_equal(a, b)
    da, db = DR.dbscan(P, r, 12, edge_list=a), DR.dbscan(P, r, 12, edge_list=b)
    assert min(da["core"], da["border"], da["noise"]) > 0
    for k in da:
        assert np.array_equal(da[k], db[k]), k


def test_min_points_1_is_the_components():
    rng = np.random.default_rng(6)
    P = (rng.random((3000, 3)) * np.array([2.0, 2.0, 0.1])).astype(F32)
    for sel in (dict(), dict(min_size=3, keep_largest=4)):
        c, d = CR.components(P, 0.04, **sel), DR.dbscan(P, 0.04, 1, **sel)
        assert c["components"] == d["clusters"] > 10 and (d["kind"] == 2).all()
        for k in ("label", "size", "keep", "kept_index", "rows", "kept", "largest"):
            assert np.array_equal(c[k], d[k]), k
        assert c["kept_components"] == d["kept_clusters"]


def test_default_params():
    assert plade_amd.dbscan_default_params() == {"radius": 0.0, "min_points": 4, "min_size": 1, "max_size": 0, "keep_largest": 0}
    assert set(("plade_dbscan_default_params", "plade_cluster_dbscan", "plade_cloud_cluster_dbscan_dev")) <= set(plade_amd.ABI_SYMBOLS)


# ---- the two switches ------------------------------------------------------------------------------------------------------------
OFF = (0, 0.0, 4, 1, 0)
W_DBSCAN = (" is not <radius>,<min_points>[,<min_size>[,<keep_largest>]] with radius > 0 (its square not below FLT_MIN),"
            " min_points >= 1, min_size >= 1 and keep_largest >= 0; no clustering")
W_M3C2 = (" is not <radius>[,<min_points>[,<min_size>]] with radius > 0 (its square not below FLT_MIN), min_points >= 1"
          " and min_size >= 1; no clusters of change")
# (variable, text, (on, radius, min_points, min_size, keep_largest) or None when rejected); ARITY: required fields, fields
ARITY = {"PLADE_DBSCAN": (2, 4), "PLADE_M3C2_CLUSTERS": (1, 3)}
TAIL = {"PLADE_DBSCAN": W_DBSCAN, "PLADE_M3C2_CLUSTERS": W_M3C2}
CASES = [
    ("PLADE_DBSCAN", None, OFF),
    ("PLADE_DBSCAN", "0.25,8", (1, 0.25, 8, 1, 0)),
    ("PLADE_DBSCAN", "0.25,8,50", (1, 0.25, 8, 50, 0)),
    ("PLADE_DBSCAN", "0.25,8,50,3", (1, 0.25, 8, 50, 3)),
    ("PLADE_DBSCAN", " 1e-3,+1,1,0", (1, 1e-3, 1, 1, 0)),
    ("PLADE_DBSCAN", "0.25", None),                   # min_points is required
    ("PLADE_DBSCAN", "0,8,50,3", None),               # each field in turn
    ("PLADE_DBSCAN", "-0.25,8", None),
    ("PLADE_DBSCAN", "nan,8", None),
    ("PLADE_DBSCAN", "inf,8", None),
    ("PLADE_DBSCAN", "1e-30,8", None),                # its fp32 square is below FLT_MIN
    ("PLADE_DBSCAN", "1e30,8", None),                 # its fp32 square is not finite
    ("PLADE_DBSCAN", "0.25,0", None),
    ("PLADE_DBSCAN", "0.25,0,50,3", None),
    ("PLADE_DBSCAN", "0.25,8.5", None),
    ("PLADE_DBSCAN", "0.25,8,0", None),
    ("PLADE_DBSCAN", "0.25,8,0,3", None),
    ("PLADE_DBSCAN", "0.25,8,50,-1", None),
    ("PLADE_DBSCAN", "0.25,8,50,3,1", None),          # a fifth field
    ("PLADE_DBSCAN", "0.25,8,", None),                # a trailing comma is no empty field
    ("PLADE_DBSCAN", "0.25,,50", None),
    ("PLADE_DBSCAN", "", None),
    ("PLADE_DBSCAN", "x", None),
    ("PLADE_M3C2_CLUSTERS", None, OFF),
    ("PLADE_M3C2_CLUSTERS", "0.5", (1, 0.5, 4, 1, 0)),
    ("PLADE_M3C2_CLUSTERS", "0.5,6", (1, 0.5, 6, 1, 0)),
    ("PLADE_M3C2_CLUSTERS", "0.5,6,20", (1, 0.5, 6, 20, 0)),
    ("PLADE_M3C2_CLUSTERS", "0", None),
    ("PLADE_M3C2_CLUSTERS", "0,6,20", None),
    ("PLADE_M3C2_CLUSTERS", "-1", None),
    ("PLADE_M3C2_CLUSTERS", "1e-30", None),
    ("PLADE_M3C2_CLUSTERS", "0.5,0", None),
    ("PLADE_M3C2_CLUSTERS", "0.5,0,20", None),
    ("PLADE_M3C2_CLUSTERS", "0.5,6,0", None),
    ("PLADE_M3C2_CLUSTERS", "0.5,6,20,1", None),      # no keep_largest here
    ("PLADE_M3C2_CLUSTERS", "0.5,,20", None),
    ("PLADE_M3C2_CLUSTERS", "", None),
]


def test_the_switch_table_cannot_pass_vacuously():
    """Every variable has an accepted value of every length it allows, and for every field a rejected value that differs from an
    accepted one in that field alone."""
    assert {c[0] for c in CASES} == set(ARITY) and len({c[:2] for c in CASES}) == len(CASES)
    for var, (required, n) in ARITY.items():
        assert (var, None, OFF) in CASES
        mine = [c for c in CASES if c[0] == var and c[1] is not None]
        good = {tuple(c[1].split(",")) for c in mine if c[2] is not None}
        bad = {tuple(c[1].split(",")) for c in mine if c[2] is None}
        assert {len(g) for g in good} == set(range(required, n + 1)), var
        for k in range(n):
            assert any(len(b) == len(g) and [i for i in range(len(b)) if b[i] != g[i]] == [k] for b in bad for g in good), (var, k)
        assert any(",," in c[1] for c in mine), var


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dbscan_switches") / "dbscan_switch_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "plade_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "dbscan_switch_harness.cpp"), "-o", exe])
    return exe


def test_the_two_parsers(harness):
    """Every field of the parsed struct and the warning byte for byte, all rows in one process (nothing is latched in the header)."""
    feed = "".join(var + ("" if text is None else "\t" + text) + "\n" for var, text, _ in CASES)
    r = subprocess.run([harness], input=feed, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    got = r.stdout.split("\n")
    assert got[-1] == "" and len(got) == len(CASES) + 1
    for (var, text, want), line in zip(CASES, got):
        fields, warning = line.split("\t", 1)
        on, radius, min_points, min_size, keep_largest = fields.split(" ")
        have = (int(on), float(radius), int(min_points), int(min_size), int(keep_largest))
        if want is None:
            assert have == OFF and warning == f"warning: {var}={text}{TAIL[var]}", (var, text, line)
        else:
            assert have == want and warning == "", (var, text, line)


def test_the_latches_and_their_place_in_the_load():
    """One latch per switch in plade_host.cpp; PLADE_DBSCAN filters after PLADE_KEEP_COMPONENTS and before PLADE_SMOOTH."""
    host = open(os.path.join(ROOT, "plade_amd", "csrc", "plade_host.cpp")).read()
    assert host.count('getenv("PLADE_DBSCAN")') == 1 and host.count('getenv("PLADE_M3C2_CLUSTERS")') == 1
    assert "!keep_components_in_place(buf) || !dbscan_in_place(buf) || !smooth_in_place(buf)" in host
