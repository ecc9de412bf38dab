"""The minimum-spacing subsample on the GPU (plade_subsample_spacing / plade_cloud_subsample_dev, plade_amd/csrc/k_subsample.hip)
against the restatement of its semantics (tests/subsample_restate.py: the float32 graph, the hashed keys, the synchronous rounds).
keep, kept_index, round, rounds and the kept rows are compared bit for bit: the kept set is an exact set and the rounds are part of
the result, so there is no tolerance anywhere in this file.  Separation and maximality are checked once more by brute force that
knows nothing of keys or rounds.
"""
import ctypes

import numpy as np
import pytest

import plade_amd
import grid_shapes as GS
import subsample_restate as SR
from outlier_restate import flann_d2
from conftest import ORIENTED

pytestmark = pytest.mark.gpu

F32 = np.float32
SUMMARY = ("n", "kept", "rounds")
STATS = ("subsample_grid_s", "subsample_rounds_s", "subsample_compact_s", "subsample_rounds", "subsample_kept", "subsample_grid_dx",
         "subsample_grid_dy", "subsample_grid_dz", "subsample_grid_cell")
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 4099)
SPACINGS = (0.5, 2.0, 10.0)            # x the mean point spacing of SR.sheet (1)

# the messages of the errors
E_EMPTY = "subsample_spacing: the cloud is empty (n = 0)"
E_STRIDE = "subsample_spacing: stride must be >= 3 floats"
E_NULL = "plade_subsample_spacing: NULL cloud"
E_NULL_DEV = "plade_cloud_subsample_dev: NULL cloud"
E_FINITE = "the point cloud contains non-finite coordinates (NaN or infinity)"
E_SPACING = "subsample_spacing: spacing must be finite and > 0, its fp32 square finite and not below FLT_MIN"


@pytest.fixture(scope="module")
def sctx():
    c = plade_amd.Context(0, **ORIENTED)
    yield c
    c.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def rows_of(P, stride):
    """(n, stride): x y z, then columns of arbitrary words -- NaNs with a payload in the first of them"""
    P = np.ascontiguousarray(P, F32)
    out = np.empty((len(P), stride), F32)
    out[:, :3] = P[:, :3]
    if stride > 3:
        w = np.random.default_rng(stride).integers(0, 1 << 32, (len(P), stride - 3), dtype=np.uint64).astype(np.uint32)
        w[:, 0] = np.uint32(0x7FC00000) + (np.arange(len(P), dtype=np.uint32) & np.uint32(0xFFFF)) + np.uint32(1)
        out[:, 3:] = w.view(F32)
        assert np.isnan(out[:, 3]).all()
    return out


def valid_set(P, keep, spacing):
    """separation and maximality by brute force over the float32 distances"""
    r2 = F32(spacing) * F32(spacing)
    A = flann_d2(P[:, :3], P[:, :3]) < r2
    np.fill_diagonal(A, False)
    assert not A[np.ix_(keep, keep)].any(), "two kept points are closer than the spacing"
    assert A[np.ix_(~keep, keep)].any(1).all(), "a dropped point has no kept point closer than the spacing"


def assert_same(got, ref, rows):
    out, kept, info = got
    for k in SUMMARY:
        assert info[k] == ref[k], (k, info[k], ref[k])
    assert np.array_equal(info["keep"], ref["keep"])
    assert info["round"].dtype == np.uint32 and same_bits(info["round"], ref["round"])
    assert kept.dtype == np.uint32 and same_bits(kept, ref["kept_index"]) and (np.diff(kept.astype(np.int64)) > 0).all()
    assert out.shape == (len(kept), rows.shape[1]) and same_bits(out.view(np.uint32), rows[kept].view(np.uint32))


def check(ctx, P, spacing, seed=0, strides=(3, 6, 7)):
    """every stride through the host form, twice; stride 6 through the resident form.  Returns (restated, info of the last call)"""
    P = np.ascontiguousarray(P, F32)
    ref = SR.subsample(P, spacing, seed)
    assert np.array_equal(ref["keep"], ref["greedy"])
    info = None
    for stride in strides:
        rows = rows_of(P, stride)
        got = ctx.subsample(rows, spacing, seed)
        info = got[2]
        print(f"n {len(P)} spacing {float(spacing):.6g} seed {seed} stride {stride}: kept {info['kept']} (restated {ref['kept']}), rounds "
              f"{info['rounds']} (restated {ref['rounds']})")
        assert_same(got, ref, rows)
        valid_set(P, info["keep"], spacing)
        s = ctx.stats()
        assert all(k in s for k in STATS), [k for k in STATS if k not in s]
        assert s["subsample_rounds"] == info["rounds"] and s["subsample_kept"] == info["kept"]
        assert_same(ctx.subsample(rows, spacing, seed), ref, rows)               # a second call: the same bits
        if stride == 6:
            c = ctx.upload(rows)
            try:
                f, kept, dinfo = ctx.subsample_dev(c, spacing, seed, info=True)
                try:
                    assert f.n == ref["kept"] and same_bits(kept, ref["kept_index"]) and np.array_equal(dinfo["keep"], ref["keep"])
                    assert all(dinfo[k] == ref[k] for k in SUMMARY)
                    assert same_bits(f.download().view(np.uint32), rows[kept].view(np.uint32))
                finally:
                    f.free()
            finally:
                c.free()
    return ref, info


# ---- seeded sheets: sizes around the wavefront and the workgroup, several workgroups; three densities of the graph ---------------
@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("n", SIZES)
def test_sheets(sctx, n, spacing):
    ref, info = check(sctx, SR.sheet(n), spacing, seed=7)
    assert info["keep"][ref["first"]] and info["round"][ref["first"]] == 1


def test_two_seeds_give_two_valid_sets(sctx):
    P = SR.sheet(2000)
    a, ia = check(sctx, P, 2.0, seed=7, strides=(3,))
    b, ib = check(sctx, P, 2.0, seed=8, strides=(3,))
    assert not np.array_equal(ia["keep"], ib["keep"])


# ---- the predicate ----------------------------------------------------------------------------------------------------------------
def test_64_copies_of_one_point(sctx):
    P = np.tile(np.array([[0.25, -1.5, 3.0]], F32), (64, 1))
    ref, info = check(sctx, P, 0.5, seed=3)
    assert info["kept"] == 1 and np.flatnonzero(info["keep"]).tolist() == [ref["first"]]
    assert ref["first"] == int(np.argmin(SR.keys(64, 3)))


def test_pair_exactly_at_the_spacing_and_one_ulp_closer(sctx):
    a = np.array([1.0, 2.0, 3.0], F32)
    at = a + np.array([0.5, 0.0, 0.0], F32)                        # d = 0.25 = 0.5^2, every step exact in fp32
    below = at.copy()
    below[0] = np.nextafter(at[0], F32(0.0))
    assert flann_d2(a[None], at[None])[0, 0] == F32(0.25) and flann_d2(a[None], below[None])[0, 0] < F32(0.25)
    _, i_at = check(sctx, np.stack([a, at]), 0.5)
    ref, i_below = check(sctx, np.stack([a, below]), 0.5)
    assert i_at["kept"] == 2 and i_at["rounds"] == 1
    assert i_below["kept"] == 1 and np.flatnonzero(i_below["keep"]).tolist() == [ref["first"]] and i_below["rounds"] == 2


def test_spacing_above_the_diameter_keeps_the_first_key(sctx):
    P = SR.sheet(257)
    ref, info = check(sctx, P, 100.0, seed=11)                     # the diagonal of the sheet is 23
    assert info["kept"] == 1 and np.flatnonzero(info["keep"]).tolist() == [ref["first"]] and info["rounds"] == 2


def test_spacing_below_the_smallest_gap_keeps_everything(sctx):
    P = SR.sheet(257)
    d = flann_d2(P, P)
    np.fill_diagonal(d, np.inf)
    spacing = 0.5 * float(np.sqrt(d.min()))
    ref, info = check(sctx, P, spacing)
    assert info["kept"] == 257 and info["rounds"] == 1 and info["keep"].all()


def test_sorted_chain_of_3000(sctx):
    ref, info = check(sctx, SR.chain(3000, 0.6), 1.0, seed=7, strides=(3, 6))
    assert info["rounds"] == ref["rounds"] <= 8                    # (3000 in index order: test_subsample_host.py)


# ---- the grid shapes of DESIGN.md section 22 ----------------------------------------------------------------------------------------
def test_single_row_grid(sctx):
    P = GS.cloud("row0")
    ref, info = check(sctx, P, GS.R, seed=1, strides=(3, 6))
    s = sctx.stats()
    assert (s["subsample_grid_dy"], s["subsample_grid_dz"]) == (1, 1) and s["subsample_grid_dx"] > 100


def test_one_cell_thick_grid(sctx):
    P = GS.cloud("sheet2")
    ref, info = check(sctx, P, GS.R, seed=1, strides=(3, 6))
    s = sctx.stats()
    assert s["subsample_grid_dz"] == 1 and s["subsample_grid_dx"] > 1 and s["subsample_grid_dy"] > 1


def test_capped_grid(sctx):
    rng = np.random.default_rng(9)
    clump = 0.02 * rng.random((200, 3))
    far = clump[::-1] + 1e4 / np.sqrt(3.0)                         # 1e4 away along the diagonal: every axis is long
    P = np.ascontiguousarray(np.concatenate([clump, far]).astype(F32))
    spacing = 1e-3
    ref, info = check(sctx, P, spacing, seed=2, strides=(3, 6))
    assert 2 <= info["kept"] < 400
    s = sctx.stats()
    dims = (s["subsample_grid_dx"], s["subsample_grid_dy"], s["subsample_grid_dz"])
    assert GS.is_capped(s["subsample_grid_cell"], dims, GS.radius_cell(P, r=spacing)), (s["subsample_grid_cell"], dims)


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def test_errors(sctx):
    P = SR.sheet(300)
    ref = SR.subsample(P, 2.0)
    nan, inf = P.copy(), P.copy()
    nan[17, 1] = np.nan
    inf[299, 2] = np.inf
    cases = [(np.zeros((0, 3), F32), 2.0, E_EMPTY), (nan, 2.0, E_FINITE), (inf, 2.0, E_FINITE), (P, 0.0, E_SPACING), (P, -1.0, E_SPACING),
             (P, float("nan"), E_SPACING), (P, 1e30, E_SPACING), (P, 1e-30, E_SPACING), (P, float("inf"), E_SPACING)]
    for arr, spacing, msg in cases:
        with pytest.raises(plade_amd.PladeError) as e:
            sctx.subsample(arr, spacing)
        assert e.value.code == plade_amd.PLADE_EINVAL and str(e.value).endswith(": " + msg), (spacing, str(e.value))
        assert_same(sctx.subsample(P, 2.0), ref, P)                # the next call on the same context succeeds
    # stride < 3, a NULL cloud and the defaults (no spacing) through the C ABI itself
    prm = plade_amd.SubsampleParams(2.0, 0)
    summ = plade_amd.SubsampleSummary()
    L, h = sctx.L, sctx.h
    two = np.zeros((10, 2), F32)
    rc = L.plade_subsample_spacing(h, two.ctypes.data, 10, 2, ctypes.byref(prm), None, None, None, None, ctypes.byref(summ))
    assert rc == plade_amd.PLADE_EINVAL and L.plade_last_error(h).decode() == E_STRIDE
    rc = L.plade_subsample_spacing(h, None, 10, 3, ctypes.byref(prm), None, None, None, None, ctypes.byref(summ))
    assert rc == plade_amd.PLADE_EINVAL and L.plade_last_error(h).decode() == E_NULL
    rc = L.plade_subsample_spacing(h, P.ctypes.data, len(P), 3, None, None, None, None, None, ctypes.byref(summ))
    assert rc == plade_amd.PLADE_EINVAL and L.plade_last_error(h).decode() == E_SPACING
    out = ctypes.c_void_p()
    rc = L.plade_cloud_subsample_dev(h, None, ctypes.byref(prm), ctypes.byref(out), None, None, ctypes.byref(summ))
    assert rc == plade_amd.PLADE_EINVAL and L.plade_last_error(h).decode() == E_NULL_DEV and not out.value
    c = sctx.upload(rows_of(P, 6))
    try:
        with pytest.raises(plade_amd.PladeError) as e:
            sctx.subsample_dev(c, 0.0)
        assert e.value.code == plade_amd.PLADE_EINVAL and str(e.value).endswith(": " + E_SPACING)
    finally:
        c.free()
    # every output is optional
    rc = L.plade_subsample_spacing(h, P.ctypes.data, len(P), 3, ctypes.byref(prm), None, None, None, None, ctypes.byref(summ))
    assert rc == 0 and (summ.n, summ.kept, summ.rounds) == (300, ref["kept"], ref["rounds"])
    assert L.plade_subsample_spacing(h, P.ctypes.data, len(P), 3, ctypes.byref(prm), None, None, None, None, None) == 0


def test_defaults():
    assert plade_amd.subsample_default_params() == {"spacing": 0.0, "seed": 0}
