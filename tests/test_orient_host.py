"""The restatement of the consistent normal orientation (tests/orient_restate.py) against itself, and the parser of
PLADE_CONSISTENT_NORMALS (plade_amd/csrc/cli_switches.h) through a stand-alone program built with the address and
undefined-behaviour sanitizers (tests/cxx/orient_switch_harness.cpp).  No GPU.

The key of a pair with |dot32| = 1 is 0x7F800000 - 0x3F800000 = 0x40000000 (orient_restate.KEY_FLAT), that of a pair with
dot32 = 0 is 0x7F800000 (KEY_TOP).
"""
import os
import subprocess

import numpy as np
import pytest

import orient_restate as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def noisy_sheet(n, seed, sigma=0.3):
    N = np.tile(np.asarray([0, 0, 1], np.float64), (n, 1)) + sigma * np.random.default_rng(seed).normal(size=(n, 3))
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    return OR.with_normals(OR.sheet(n, seed=seed), OR.random_flips(N, seed=seed + 1)), N


def one_side(rows, truth):
    d = np.einsum("ij,ij->i", rows[:, 3:6].astype(np.float64), np.asarray(truth, np.float64))
    return 1 if (d > 0).all() else -1 if (d < 0).all() else 0


# ---- Kruskal == Boruvka under the same order -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,radius,seed", [(1, 1.5, 1), (2, 5.0, 2), (65, 1.5, 3), (300, 1.5, 4), (300, 3.0, 5), (150, 30.0, 6)])
def test_kruskal_is_boruvka(n, radius, seed):
    rows, _ = noisy_sheet(n, seed)
    rows[::17, 4] = np.nan                                         # some points are no vertices
    if n >= 150:
        rows[100:140, 3:] = [0.0, 0.0, 1.0]                        # a patch of ties
    lo, hi, key, s = OR.weighted_edges(rows, radius)
    tk, uk = OR.kruskal(n, lo, hi, key, s)
    tb, ub, rounds = OR.boruvka(n, lo, hi, key, s)
    assert np.array_equal(tk, tb) and int(key[tk].sum()) == int(key[tb].sum())
    assert 1 <= rounds <= int(np.ceil(np.log2(max(n, 1)))) + 1
    for mode in (OR.VOTE, OR.EXTREME):
        a = OR.orient(rows, radius, mode=mode, viewpoint=(3.0, 2.0, 40.0), forest=(lo, hi, key, s, tk, uk))
        b = OR.orient(rows, radius, mode=mode, viewpoint=(3.0, 2.0, 40.0), forest=(lo, hi, key, s, tb, ub))
        assert np.array_equal(a["flip"], b["flip"]) and np.array_equal(a["label"], b["label"])
        assert a["rows"].tobytes() == b["rows"].tobytes() and a["tree_key_sum"] == b["tree_key_sum"]
        ok = OR.valid_points(rows)
        assert a["tree_edges"] == ok.sum() - a["components"] and (a["label"][~ok] == -1).all()
        t = a["tree"]                                              # along every forest edge flip_i ^ flip_j = s_ij
        with np.errstate(all="ignore"):
            d = OR.dot32(rows[:, 3:6], t[:, 0], t[:, 1])
        assert np.array_equal(a["flip"][t[:, 0]] ^ a["flip"][t[:, 1]], (d < 0).astype(np.uint8))
        assert (OR.dot32(a["rows"][:, 3:6], t[:, 0], t[:, 1]) >= 0).all()   # so no forest edge joins opposed normals afterwards


# ---- a plane and a sphere come out on one side ----------------------------------------------------------------------------------------
def test_plane_with_flipped_normals_is_one_side():
    rows, N = noisy_sheet(1500, 7, sigma=0.1)
    r = OR.orient(rows, 3.0, viewpoint=(0.0, 0.0, 30.0))
    assert r["components"] == 1 and one_side(r["rows"], N) == 1 and 600 < r["flipped"] < 900
    assert one_side(OR.orient(rows, 3.0, viewpoint=(0.0, 0.0, -30.0))["rows"], N) == -1
    assert one_side(OR.orient(rows, 3.0, mode=OR.EXTREME)["rows"], N) == 1
    assert one_side(OR.orient(rows, 3.0, mode=OR.EXTREME, inward=1)["rows"], N) == -1


def test_sphere_with_flipped_normals_is_one_side():
    P, U = OR.sphere(2000)
    rows = OR.with_normals(P, OR.random_flips(U))
    r = OR.orient(rows, 2.0, mode=OR.EXTREME)
    assert r["components"] == 1 and one_side(r["rows"], U) == 1    # outward: the top point's normal has a component along +z
    assert one_side(OR.orient(rows, 2.0, mode=OR.EXTREME, inward=1)["rows"], U) == -1
    assert one_side(OR.orient(rows, 2.0)["rows"], U) == -1         # every outward normal faces away from the centre
    # the per-point viewpoint test from a viewpoint outside cannot do this: it leaves the far half inward
    seen = np.where(OR.flip_test(OR.with_normals(P, U), (0.0, 0.0, 30.0)) < 0, -1.0, 1.0)[:, None] * U
    assert one_side(OR.with_normals(P, seen), U) == 0


# ---- the keys ------------------------------------------------------------------------------------------------------------------------
def test_key_constants():
    assert int(OR.key32(F32(0.0))) == 0x7F800000 == OR.KEY_TOP and int(OR.key32(F32(-0.0))) == OR.KEY_TOP
    assert int(OR.key32(F32(1.0))) == 0x7F800000 - 0x3F800000 == 0x40000000 == OR.KEY_FLAT and int(OR.key32(F32(-1.0))) == OR.KEY_FLAT
    d = np.asarray([0.0, 1e-30, 0.25, 0.5, 0.99999994, 1.0, 2.0, 3e36], F32)
    assert (np.diff(OR.key32(d)) < 0).all() and (OR.key32(d) >= 0).all()   # the flatter pair has the smaller key


def test_plane_of_identical_normals_is_all_ties():
    P = OR.sheet(800, seed=9)
    rows = OR.with_normals(P, np.tile(np.asarray([0, 0, 1], F32), (800, 1)))
    lo, hi, key, s = OR.weighted_edges(rows, 2.0)
    assert (key == OR.KEY_FLAT).all() and not s.any()
    r = OR.orient(rows, 2.0, viewpoint=(0.0, 0.0, -5.0))
    assert r["tree_key_sum"] == r["tree_edges"] * OR.KEY_FLAT and r["flip"].all()
    # under ties the indices decide: Kruskal over (lo, hi) alone, so every tree edge is the smallest-index way into its subtree
    assert np.array_equal(r["tree"], np.stack([lo, hi], 1)[OR.kruskal(800, lo, hi, key, s)[0]])
    tb, _, _ = OR.boruvka(800, lo, hi, key, s)
    assert np.array_equal(np.stack([lo[tb], hi[tb]], 1), r["tree"])


def test_ordering_by_index_alone_gives_a_larger_key_sum():
    rows, _ = noisy_sheet(400, 11)
    lo, hi, key, s = OR.weighted_edges(rows, 2.5)
    tk, _ = OR.kruskal(400, lo, hi, key, s)
    by_index = np.lexsort((hi, lo))
    ti, _ = OR.kruskal(400, lo[by_index], hi[by_index], key[by_index], s[by_index])
    tb, _, _ = OR.boruvka(400, lo, hi, key, s, order=by_index)
    assert len(ti) == len(tk) == len(tb)                           # the same components, another forest
    assert int(key[by_index][ti].sum()) > int(key[tk].sum()) and int(key[tb].sum()) > int(key[tk].sum())


# ---- the switch ----------------------------------------------------------------------------------------------------------------------
VAR = "PLADE_CONSISTENT_NORMALS"
TAIL = " is not <radius>[,<mode>[,<inward>]] with radius >= 0 (its square not below FLT_MIN), mode 0 or 1 and inward 0 or 1; no orientation"
OFF = (0.0, 0, 0)
# (text, (radius, mode, inward) or None when the value is rejected)
VALUES = [(None, OFF), ("0.25", (0.25, 0, 0)), ("0.25,1", (0.25, 1, 0)), ("0.25,1,1", (0.25, 1, 1)), ("0.25,0,1", (0.25, 0, 1)),
          (" +5e-1,+1", (0.5, 1, 0)), ("0x1p-2", (0.25, 0, 0)), ("0", OFF), ("0,1,1", (0.0, 1, 1)), ("-0", OFF), ("1e-18", (1e-18, 0, 0)),
          ("", None), ("wide", None), ("0.25,", None), ("0.25,,1", None), ("0.25,1.0", None), ("0.25,2", None), ("0.25,-1", None),
          ("0.25,1,2", None), ("0.25,1,1,0", None), ("0.25x", None), ("inf", None), ("nan", None), ("-0.25", None), ("1e30", None),
          ("1e-30", None)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("orient_switch") / "orient_switch_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "plade_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cxx", "orient_switch_harness.cpp"), "-o", exe])
    return exe


def test_switch_values(harness):
    feed = "".join(VAR + ("" if text is None else "\t" + text) + "\n" for text, _ in VALUES)
    r = subprocess.run([harness], input=feed, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    got = r.stdout.split("\n")
    assert got[-1] == "" and len(got) == len(VALUES) + 1
    for (text, want), line in zip(VALUES, got):
        fields, warning = line.split("\t")
        radius, mode, inward = fields.split(" ")
        value = (float.fromhex(radius), int(mode), int(inward))
        if want is None:                                           # rejected: the switch's "off" and the one warning
            assert value == OFF and warning == f"warning: {VAR}={text}{TAIL}", (text, line)
        else:
            assert value == want and warning == "", (text, line)


def test_the_switch_is_documented_at_its_latch():
    host = open(os.path.join(ROOT, "plade_amd", "csrc", "plade_host.cpp")).read()
    assert host.count(f'getenv("{VAR}")') == 1 and host.count("cli_switches::parse_consistent_normals(") == 1
    assert f"// {VAR}=<radius>[,<mode>[,<inward>]]" in host
