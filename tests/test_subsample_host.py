"""The minimum-spacing subsample on the CPU (tests/subsample_restate.py): the sequential greedy walk that defines the kept set is the
fixed point of the synchronous rounds the GPU runs; the set is separated and maximal by brute force; mix64 against constants; and
the documented reason for the hashed order -- a sorted scan line takes a handful of rounds hashed and n rounds in index order."""
import numpy as np
import pytest

import subsample_restate as SR

SHEETS = [(n, s) for n in (257, 2000) for s in (0.5, 2.0, 10.0)]


@pytest.fixture(scope="module")
def restated():
    return {(n, s): (SR.sheet(n), SR.subsample(SR.sheet(n), s, seed=7)) for n, s in SHEETS}


def test_mix64_constants():
    # splitmix64 seeded with 0: its first two outputs are the finaliser of 1 x and 2 x the golden-ratio increment, i.e.
    # common.h's mix64 (which adds the increment first) of 0 and of the increment; the third by hand from the definition
    assert SR.mix64_int(0) == 0xE220A8397B1DCDAF
    assert SR.mix64_int(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert SR.mix64_int(0xFFFFFFFFFFFFFFFF) == 0xE4D971771B652C20
    z = np.array([0, 0x9E3779B97F4A7C15, 0xFFFFFFFFFFFFFFFF], np.uint64)
    assert [int(v) for v in SR.mix64(z)] == [SR.mix64_int(int(v)) for v in z]


def test_keys_are_distinct_and_seeded():
    a, b = SR.keys(5000, 0), SR.keys(5000, 1)
    assert len(np.unique(a)) == 5000 and len(np.unique(b)) == 5000 and not np.array_equal(a, b)
    assert int(a[3]) == SR.mix64_int(SR.mix64_int(0) ^ 3)


@pytest.mark.parametrize("n,spacing", SHEETS)
def test_greedy_is_the_fixed_point_of_the_rounds(restated, n, spacing):
    P, ref = restated[(n, spacing)]
    print(f"n {n} spacing {spacing}: kept {ref['kept']}, rounds {ref['rounds']}")
    assert np.array_equal(ref["keep"], ref["greedy"])
    assert ref["round"].min() >= 1 and ref["round"].max() == ref["rounds"]
    assert ref["keep"][ref["first"]] and ref["round"][ref["first"]] == 1   # the smallest key is kept at once
    assert ref["rounds"] <= 12


@pytest.mark.parametrize("n,spacing", SHEETS)
def test_separation_and_maximality(restated, n, spacing):
    P, ref = restated[(n, spacing)]
    assert SR.separated(P, ref["keep"], spacing) and SR.maximal(P, ref["keep"], spacing)
    # the checks can fail: one more point breaks the separation, one fewer the maximality (a kept point has no kept neighbour)
    more = ref["keep"].copy()
    dropped = np.flatnonzero(~more)
    if len(dropped):
        more[dropped[0]] = True
        assert not SR.separated(P, more, spacing)
    fewer = ref["keep"].copy()
    fewer[np.flatnonzero(fewer)[0]] = False
    assert not SR.maximal(P, fewer, spacing)


def test_index_order_is_another_set(restated):
    P, ref = restated[(2000, 2.0)]
    other = SR.subsample(P, 2.0, order="index")
    assert np.array_equal(other["keep"], other["greedy"]) and SR.separated(P, other["keep"], 2.0) and SR.maximal(P, other["keep"], 2.0)
    assert not np.array_equal(other["keep"], ref["keep"])
    assert not np.array_equal(SR.subsample(P, 2.0, seed=8)["keep"], ref["keep"])


def test_sorted_chain_hashed_against_index_order():
    P = SR.chain(3000, 0.6)
    hashed = SR.subsample(P, 1.0, seed=7)
    index = SR.subsample(P, 1.0, order="index")
    print(f"chain of 3000: hashed {hashed['rounds']} rounds, index order {index['rounds']}")
    assert hashed["rounds"] <= 8
    assert index["rounds"] == 3000 and np.array_equal(index["keep"], np.arange(3000) % 2 == 0)
    for r in (hashed, index):
        assert np.array_equal(r["keep"], r["greedy"]) and SR.separated(P, r["keep"], 1.0) and SR.maximal(P, r["keep"], 1.0)
