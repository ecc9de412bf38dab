"""The nine tools that search TargetGrid's dense row index (normals, both outlier filters, distances, smoothing, components, FPFH,
M3C2 and the ICP / GICP seams) on the three grid shapes of grid_shapes.py: a single row of cells, a grid one cell thick and a grid
whose cell the cap on the padded rows enlarged to five times what the tool asked for.

Every case checks the result with the tool's own checker and restatement, at that checker's tolerances (nothing here is new), and
proves from the "<tool>_grid_*" stats that the library built the shape the case was written for, with the inequalities that
test_grid_shapes_host.py asserts on the CPU model; the kNN tools on a row also prove that every query took the ring kernel.
"""
import numpy as np
import pytest

import plade_amd
import components_restate as CR
import fpfh_restate as FR
import grid_shapes as GS
import icp_restate as IR
import m3c2_restate as MR
import outlier_restate as OR
import smooth_restate as SR
from conftest import ORIENTED
from test_gpu_components import assert_same
from test_gpu_distances import _check as check_distances
from test_gpu_fpfh import check_integers, check_sums
from test_gpu_gicp import _check_seam as check_gicp_seam
from test_gpu_icp import _check_seam as check_icp_seam
from test_gpu_m3c2 import check_against, check_derived
from test_gpu_normals import check_against_ref
from test_gpu_outliers import check_outputs, check_statistical
from test_gpu_smooth import same_bits

pytestmark = pytest.mark.gpu

R = GS.R
MIN_NB = 4                                                          # smoothing: a point of a row has five neighbours, itself included


@pytest.fixture(scope="module")
def gctx():
    c = plade_amd.Context(0, **ORIENTED)
    yield c
    c.close()


@pytest.fixture(scope="module")
def keys():
    """the restated neighbour keys of every shape, computed once"""
    return {name: OR.neighbours(GS.cloud(name), kmax=16)[0] for name in GS.SHAPES}


def met(ctx, tool, name, asked=None, capped=None):
    """The grid `tool` reports, printed; asserts the shape `name` stands for: its unit axes, and -- where the tool asked for the
    cell `asked` -- that the cap decided the cell exactly when `capped` says so (default: on the capped cloud)."""
    s = ctx.stats()
    dims = [int(s[f"{tool}_grid_d{a}"]) for a in "xyz"]
    cell = s[f"{tool}_grid_cell"]
    ring = f", ring queries {s[tool + '_ring_queries']:.0f}" if tool + "_ring_queries" in s else ""
    print(f"{tool} on {name}: grid {dims[0]} x {dims[1]} x {dims[2]}, cell {cell:.5g}" + (f" (asked {asked:.5g})" if asked else "")
          + f", padded rows {GS.padded_rows(dims):.3e}" + ring)
    for a in GS.unit_axes(name):
        assert dims[a] == 1, (tool, name, dims)
    assert sorted(dims)[len(GS.unit_axes(name))] > 1, (tool, name, dims)
    if asked is not None:
        assert GS.is_capped(cell, dims, asked) == ((name == "capped") if capped is None else capped), (tool, name, cell, asked, dims)
    return dims, cell


def knn_met(ctx, tool, name, n):
    """a kNN tool: on a row the cap decides the cell and every query goes to the ring kernel; the far points of capped do"""
    dims, cell = met(ctx, tool, name)
    ring = ctx.stats()[f"{tool}_ring_queries"]
    if name in GS.ROWS:
        assert ring == n and GS.CELL_CAP / 1.26 ** 3 < GS.padded_rows(dims) <= GS.CELL_CAP
    if name == "capped":
        assert ring >= len(GS.FAR)


# ---- normals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [(s, 16) for s in GS.SHAPES] + [("row1", 64)])
def test_normals(gctx, name, k):
    """Neighbour lists equal, curvature, the finite / NaN rule; the normal itself where the restated eigenvalue gap allows: every
    query of a sheet (asserted on pca_ref by test_grid_shapes_host.py), none of a row -- there the covariance has two zero
    eigenvalues by construction and only the lists, the curvature and the finite / NaN rule remain."""
    P = GS.cloud(name)
    out, curv, nbr = gctx.estimate_normals(P, k=k, curvature=True, neighbours=True)
    knn_met(gctx, "normals", name, len(P))
    assert np.array_equal(out[:, :3].view(np.uint32), P.view(np.uint32))
    checked = check_against_ref(P, out, curv, nbr, np.arange(len(P)), k)
    print(f"normals on {name}, k = {k}: {checked} of {len(P)} normals compared")
    if name in GS.SHEETS:
        assert checked == len(P)
    if name in GS.ROWS:
        assert checked == 0


# ---- outliers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GS.SHAPES)
def test_statistical_outliers(gctx, keys, name):
    P = GS.cloud(name)
    info, _ = check_statistical(gctx, P, 16, 1.0, keys[name], name)
    knn_met(gctx, "outliers", name, len(P))
    if name == "capped":
        assert not info["keep"][GS.N_PATCH:].any()


@pytest.mark.parametrize("name", GS.SHAPES)
def test_radius_outliers(gctx, name):
    P = GS.cloud(name)
    want, keep = OR.radius(P, R, 4)
    out, kept, info = gctx.remove_outliers(P, mode="radius", radius=R, min_neighbours=4)
    met(gctx, "outliers", name, GS.radius_cell(P))
    assert info["count"].dtype == np.uint32 and np.array_equal(info["count"], want)
    assert np.array_equal(info["keep"], keep)
    check_outputs(P, out, kept, info)
    out2, kept2, info2 = gctx.remove_outliers(P, mode="radius", radius=R, min_neighbours=4, per_point=False)   # the early stop
    assert np.array_equal(info2["keep"], keep) and same_bits(out, out2)


# ---- distances ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", [R, 40 * R])
@pytest.mark.parametrize("name", GS.SHAPES)
def test_distances(gctx, name, bound):
    """bound R: the radius grid (capped: enlarged; a row: the collapsed density cell, every far probe in the ring kernel); 40 R
    reaches the probes in empty space across empty cells"""
    tgt, src = GS.with_normals(GS.cloud(name)), GS.distance_source(name)
    idx = check_distances(gctx, tgt, src, bound)[0]
    dims, cell = met(gctx, "distances", name, GS.radius_cell(tgt[:, :3]) if bound == R and name not in GS.ROWS else None)
    if name in GS.ROWS:
        assert GS.CELL_CAP / 1.26 ** 3 < GS.padded_rows(dims) <= GS.CELL_CAP and cell < 0.01
    assert (idx[:-4] >= 0).all()
    assert (idx[-4:] >= 0).sum() == (0 if bound == R else 2 if name == "capped" else 4)


# ---- smoothing ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GS.SHAPES)
def test_smoothing(gctx, name):
    """counts and the fitted flag bit for bit, the moments and the projection at the tolerances of test_gpu_smooth.py"""
    P = GS.cloud(name)
    ref = SR.smooth(P, R, MIN_NB)
    rows, info = gctx.smooth_cloud(P, R, min_neighbours=MIN_NB, moments=True)
    met(gctx, "smooth", name, GS.radius_cell(P))
    assert info["count"].dtype == np.uint32 and np.array_equal(info["count"], ref["count"])
    assert np.array_equal(info["fitted_mask"], ref["fitted"]) and info["fitted"] == int(ref["fitted"].sum())
    err = np.abs(info["moments"] - ref["moments"])
    print(f"smoothing on {name}: fitted {info['fitted']} of {len(P)}, worst |moment - restated| / sum |terms| = "
          f"{float(np.max(err / np.maximum(ref['mag'], 1e-300))):.3e}")
    assert (err <= 1e-12 * ref["mag"]).all()
    f, d = ref["fitted"], info["displacement"]
    want = P[f].astype(np.float64) + d[f, None] * rows[f, 3:].astype(np.float64)
    tol = np.spacing(np.abs(rows[f, :3])).astype(np.float64) + 2.0 ** -23 * np.abs(d[f, None])
    assert (np.abs(rows[f, :3].astype(np.float64) - want) <= tol).all()
    assert (np.abs(d[f] - ref["delta"][f]) <= np.linalg.norm(ref["mu"][f], axis=1) * 1e-4 + 1e-12 * R).all()
    u = ~f
    assert same_bits(rows[u, :3], P[u]) and np.isnan(rows[u, 3:]).all() and (d[u] == 0).all()
    assert f.sum() >= len(P) - 4 and (name != "capped" or u[GS.N_PATCH:].all())


# ---- components ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1.25, R])
@pytest.mark.parametrize("name", GS.SHAPES)
def test_components(gctx, name, r):
    """exact.  At r = 1.25 a row falls into many pieces; the far points of capped are components of their own: three single
    points at 1.25 (the two neighbours are 1.58 apart), the corner and the pair at 2.5"""
    P = GS.cloud(name)
    ref = CR.components(P, r)
    got = gctx.connected_components(P, r)
    met(gctx, "components", name, GS.radius_cell(P, r))
    print(f"components on {name}, r = {r}: {got[2]['components']} (restated {ref['components']}), largest {got[2]['largest']}")
    assert_same(got, ref, P)
    if name in GS.ROWS:
        assert got[2]["components"] > 100 if r < R else got[2]["components"] == 1
    if name == "capped":
        lab = got[2]["label"][GS.N_PATCH:]
        assert sorted(got[2]["size"][lab]) == ([1, 1, 1] if r < R else [1, 2, 2]) and len(set(lab)) == (3 if r < R else 2)


# ---- FPFH ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GS.SHEETS + ("capped", "row1"))
def test_fpfh(gctx, name):
    cloud = GS.with_normals(GS.cloud(name))
    mp = GS.fpfh_min_pairs(name)
    ref = FR.fpfh(cloud, R, min_pairs=mp)
    assert ref["edge_near"].sum() <= 0.01 * len(cloud)              # (on the restatement alone)
    got = gctx.fpfh(cloud, R, min_pairs=mp, seams=True)
    met(gctx, "fpfh", name, GS.radius_cell(cloud[:, :3]))
    print(f"fpfh on {name}: described {got[1]['described']} of {len(cloud)}, max pairs {got[1]['max_pairs']}")
    check_integers(got, ref, name)
    check_sums(got, ref, name)
    assert got[1]["described"] >= len(cloud) - 3


# ---- M3C2 ---------------------------------------------------------------------------------------------------------------------
def check_m3c2(ctx, name, core, A, B, params):
    refs = MR.m3c2(core, A, B, params, min_points=GS.M3C2_MIN_POINTS)
    for (r, L), ref in zip(params, refs):
        got = ctx.m3c2(core, A, B, r, L, min_points=GS.M3C2_MIN_POINTS, moments=True)
        for side, X in (("m3c2_a", A), ("m3c2_b", B)):
            met(ctx, side, name, GS.radius_cell(X[:, :3]))
        print(f"m3c2 on {name}, (R, L) = ({r}, {L}), {len(core)} core points: valid {int(ref['valid'].sum())}, "
              f"max c_A {ref['count'][:, 0].max()}, max c_B {ref['count'][:, 1].max()}")
        check_against(got, ref, L, f"{name} ({r}, {L})")
        check_derived(got, ref["has_axis"], min_points=GS.M3C2_MIN_POINTS)
        assert ref["valid"].sum() >= 0.3 * len(core)


@pytest.mark.parametrize("name", GS.SHAPES)
def test_m3c2(gctx, name):
    """L = 10 on every shape; L = 60 on capped and row0: the cylinder crosses several enlarged cells and runs off both ends of a
    one-cell axis.  On capped one core point lies in the empty middle of the box and one at the far corner."""
    core, A, B = GS.m3c2_inputs(name)
    check_m3c2(gctx, name, core, A, B, GS.m3c2_params(name))


@pytest.mark.parametrize("name", ["capped", "sheet2"])
def test_m3c2_axis_aligned(gctx, name):
    """the six axis-aligned normals on 200 core points"""
    _, A, B = GS.m3c2_inputs(name)
    check_m3c2(gctx, name, GS.m3c2_axis_core(name), A, B, GS.m3c2_params(name)[:1])


# ---- the ICP and GICP seams ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["capped", "sheet2"])
def test_icp_seam(gctx, name):
    tgt, src, T = GS.seam_inputs(name)
    corr, _ = check_icp_seam(gctx, IR.Target(tgt), tgt, np.ascontiguousarray(src[:, :3]), T, R)
    met(gctx, "icp", name, GS.radius_cell(tgt[:, :3], factor=1.01))
    assert (corr >= 0).sum() >= 495 and (name != "capped" or (corr[-3:] >= GS.N_PATCH).all())


@pytest.mark.parametrize("name", ["capped", "sheet2"])
def test_gicp_seam(gctx, name):
    tgt, src, T = GS.seam_inputs(name)
    for eps in (1e-3, 1.0):
        corr, _ = check_gicp_seam(gctx, IR.Target(tgt), tgt, src, T, R, eps)
        met(gctx, "gicp", name, GS.radius_cell(tgt[:, :3], factor=1.01))
        assert (corr >= 0).sum() >= 495 and (name != "capped" or (corr[-3:] >= GS.N_PATCH).all())
