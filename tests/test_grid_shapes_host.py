"""The clouds of grid_shapes.py produce the three grid shapes they are named for, in every grid the GPU tests build over them, and
stay inside every exclusion cap of the tolerant checks those tests reuse.  Checked on the CPU model of the grids and of the ring
walk (ring_scene.py) and on the brute-force restatements alone (no GPU); test_gpu_grid_shapes.py asserts the same inequalities on
the grids the library reports."""
import numpy as np
import pytest

import components_restate as CR
import distance_restate as DR
import fpfh_restate as FR
import grid_shapes as GS
import m3c2_restate as MR
import outlier_restate as OR
import ring_scene as S
from test_gpu_normals import knn_ref, pca_ref


def test_the_generators_give_what_they_say():
    for a in range(3):
        P = GS.row(a)
        assert P.shape == (GS.N_ROW, 3) and P.dtype == np.float32
        for b in GS.unit_axes(f"row{a}"):
            assert (P[:, b] == np.float32(GS.CONST[b])).all()
        assert np.abs(P[:, a] - np.arange(GS.N_ROW)).max() <= 0.2001
    for f in (2, 0):
        P = GS.sheet(f)
        assert P.shape == (GS.N_SHEET, 3) and (P[:, f] == np.float32(GS.CONST[f])).all()
    P = GS.capped()
    assert P.shape == (GS.N_PATCH + 3, 3) and np.array_equal(P[GS.N_PATCH:], GS.FAR)
    for name in GS.SHAPES:                                          # deterministic; another seed is another sampling
        assert np.array_equal(GS.cloud(name), GS.cloud(name)) and not np.array_equal(GS.cloud(name), GS.cloud(name, seed=1))
        assert len(np.unique(GS.cloud(name), axis=0)) == len(GS.cloud(name))


@pytest.mark.parametrize("name", GS.SHAPES)
def test_radius_grids(name):
    """the grid of every radius tool (radius_cell(R); the ICP's factor 1.01 gives the same shape)"""
    P = GS.cloud(name)
    for factor in (1.03, 1.01):
        asked = GS.radius_cell(P, factor=factor)
        cell, dims = S.build(P, asked)
        print(f"{name} x{factor}: asked {asked:.4f}, cell {cell:.4f}, dims {tuple(dims)}, padded rows {GS.padded_rows(dims):.3e}")
        for a in GS.unit_axes(name):
            assert dims[a] == 1
        assert sorted(dims)[len(GS.unit_axes(name))] >= 19          # ... and only those
        assert GS.is_capped(cell, dims, asked) == (name == "capped")


@pytest.mark.parametrize("name", GS.ROWS)
@pytest.mark.parametrize("k", [16, 64])
def test_knn_grids_and_walks_of_the_rows(name, k):
    """the cap decides the cell, a middle point's walk takes at least 20 steps, and the blocks of a row along y or z are single
    columns of more than 10 000 rows"""
    P = GS.cloud(name)
    cell, dims = S.knn_grid(P, k)
    assert [a for a in range(3) if dims[a] == 1] == GS.unit_axes(name)
    assert GS.CELL_CAP / 1.26 ** 3 < GS.padded_rows(dims) <= GS.CELL_CAP and cell < 0.01
    d = np.sqrt(OR.key_d2(OR.neighbours(P, [GS.N_ROW // 2, 0], kmax=k)[0]).astype(np.float64))
    for q, row in zip((GS.N_ROW // 2, 0), d):
        for need in (row[k - 2], row[k - 1]):                       # normals count the point itself, the outlier filter does not
            steps = S.walk(P, P[q], cell, dims, need)
            print(f"{name} k={k} query {q}: {len(steps)} steps, last (rout, rows, whole, side, clipped) = {steps[-1]}")
            assert len(steps) >= 20
            assert steps[-1][1] == 1 if name == "row0" else steps[-1][1] > 10000
            assert steps[-1][4] >= 4                                # clipped on both sides of both unit axes


def test_knn_grid_and_walk_of_the_capped_cloud():
    P = GS.capped()
    cell, dims = S.knn_grid(P, 16)
    d = np.sqrt(OR.key_d2(OR.neighbours(P, [GS.N_PATCH], kmax=16)[0]).astype(np.float64))[0]
    steps = S.walk(P, P[GS.N_PATCH], cell, dims, d[14])
    print(f"capped k=16: cell {cell:.3f}, dims {tuple(dims)}, far corner: {len(steps)} steps, last {steps[-1]}")
    assert len(steps) >= 12 and steps[-1][1] > 80000 and S.does_everything(steps)


@pytest.mark.parametrize("name", GS.SHAPES)
def test_distance_grids_and_probes(name):
    """bound R: the radius grid (rows: the collapsed density cell); the probes lie beyond R, at least two within 40 R of the target"""
    T = GS.cloud(name)
    src = GS.distance_source(name)
    assert src.shape == (len(T) + 4, 3) and src.dtype == np.float32
    nn = np.sqrt(DR.flann_d2(src[-4:], T).min(1).astype(np.float64))
    assert (nn > GS.R).all() and (nn < 40 * GS.R).sum() >= 2       # (capped: the two probes in the middle of the box find nothing)
    cell, dims = S.distance_grid(T, GS.R)
    for a in GS.unit_axes(name):
        assert dims[a] == 1
    if name == "capped":
        assert GS.is_capped(cell, dims, GS.radius_cell(T))
    if name in GS.ROWS:
        assert cell < 0.01 and GS.padded_rows(dims) > GS.CELL_CAP / 1.26 ** 3


@pytest.mark.parametrize("name", GS.SHAPES)
def test_normals_gate(name):
    """check_against_ref compares the normal itself where (w1 - w0) / s > 1e-3: every query of a sheet, none of a row"""
    P = GS.cloud(name)
    q = np.arange(len(P))
    nbr = knn_ref(P, q, 16)
    gate = np.empty(len(P), bool)
    for i in q:
        w, _ = pca_ref(P, i, nbr[i])
        assert w.sum() > 0
        gate[i] = (w[1] - w[0]) / w.sum() > 1e-3
    if name in GS.SHEETS:
        assert gate.all()
    if name in GS.ROWS:
        assert not gate.any()


@pytest.mark.parametrize("name", GS.SHAPES)
def test_no_mean_distance_sits_on_the_threshold(name):
    """what check_statistical asserts before it compares keep flags"""
    P = GS.cloud(name)
    ref = OR.statistical(P, 16, 1.0)
    assert OR.nearest_gap(ref["m"], ref["threshold"]) > 1e-9
    c, keep = OR.radius(P, GS.R, 4)
    assert keep.sum() >= len(P) - 4 and (name != "capped" or not keep[GS.N_PATCH:].any())   # (a row loses its two ends twice)


@pytest.mark.parametrize("name", GS.SHAPES)
def test_components_of_the_shapes(name):
    """r = 1.25: a row falls into many pieces; the far points of the capped cloud are components of their own at both radii (one
    each at 1.25, where the two neighbours are 1.58 apart; the corner and the pair at 2.5)"""
    P = GS.cloud(name)
    small, large = CR.components(P, 1.25), CR.components(P, GS.R)
    print(f"{name}: {small['components']} components at r = 1.25, {large['components']} at r = {GS.R}")
    if name in GS.ROWS:
        assert small["components"] > 100 and large["components"] == 1
    if name == "capped":
        far = np.arange(GS.N_PATCH, GS.N_PATCH + 3)
        assert len(set(small["label"][far])) == 3 and (small["size"][small["label"][far]] == 1).all()
        assert large["components"] == 3 and sorted(large["size"]) == [1, 2, GS.N_PATCH]
        assert large["label"][far[1]] == large["label"][far[2]] != large["label"][far[0]]


@pytest.mark.parametrize("name", GS.SHEETS + ("capped", "row1"))
def test_fpfh_bin_edges(name):
    """check_integers leaves out the points with a feature within 1e-9 of a bin edge: at most 1 %"""
    ref = FR.fpfh(GS.with_normals(GS.cloud(name)), GS.R, min_pairs=GS.fpfh_min_pairs(name))
    assert ref["edge_near"].sum() <= 0.01 * len(ref["edge_near"])
    assert ref["described"].sum() >= len(ref["described"]) - 3      # (all but the far points, or a row's ends)


def band_excluded(ref, L):
    v = ref["valid"]
    return int((np.abs(np.abs(ref["distance"][v]) - ref["lod"][v]) < 1e-9 * L).sum()), int(v.sum())


@pytest.mark.parametrize("name", GS.SHAPES)
def test_m3c2_band(name):
    """check_against leaves out the core points with | |distance| - lod | < 1e-9 L and caps them at 1 %"""
    core, A, B = GS.m3c2_inputs(name)
    params = GS.m3c2_params(name)
    cases = [(core, params)]
    if name in ("capped", "sheet2"):
        cases.append((GS.m3c2_axis_core(name), [params[0]]))
    for c, prm in cases:
        for (R, L), ref in zip(prm, MR.m3c2(c, A, B, prm, min_points=GS.M3C2_MIN_POINTS)):
            out, valid = band_excluded(ref, L)
            print(f"{name} (R, L) = ({R}, {L}), {len(c)} core points: valid {valid}, in the band {out}")
            assert valid >= 0.3 * len(c) and out <= 0.01 * valid


@pytest.mark.parametrize("name", ["capped", "sheet2"])
def test_seam_sources_correspond(name):
    tgt, src, T = GS.seam_inputs(name)
    corr = GS.IR.Target(tgt).match(GS.IR.transform_f32(T, src[:, :3]), GS.R)
    assert src.shape == (500, 6) and (corr >= 0).sum() >= 495
    if name == "capped":
        assert (corr[-3:] >= GS.N_PATCH).all()                      # the far points find far points
