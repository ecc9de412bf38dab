"""Three grid shapes that the room-like scenes of the other tests never produce, and the inputs every grid tool gets on them
(test_gpu_grid_shapes.py); test_grid_shapes_host.py qualifies them on the CPU model of ring_scene.py.

  row(axis)     3000 points on an axis-aligned line: two axes of the grid have one cell.  build_knn_grid's area term collapses, the
                cap on the padded rows decides the cell (about 600 times smaller than the spacing), and every query goes to the
                ring kernel, which grows its block more than twenty times.
  sheet(flat)   a 64 x 48 lattice with one coordinate exactly constant: the grid is one cell thick.
  capped()      a 48 x 48 patch and three points 4000 away: TargetGrid::build enlarges the cell seven times, to five times the
                cell the tool asked for.

Deterministic, float32, spacing 1; the search radius of every radius tool is R."""
import numpy as np

import icp_restate as IR

F32 = np.float32
R = 2.5
N_ROW, N_SHEET, N_PATCH = 3000, 3072, 2304
CONST = (2.5, -1.25, 0.75)          # the coordinates a row or a sheet holds exactly, in x, y, z order
FAR = np.array([[4000, 4000, 4000], [4000, 10, 5], [4001.5, 10.5, 5]], F32)
MIDDLE = (2000.0, 2000.0, 2000.0)   # the empty middle of capped's box
ROWS = ("row0", "row1", "row2")
SHEETS = ("sheet2", "sheet0")
SHAPES = ROWS + SHEETS + ("capped",)
CELL_CAP = 48.0e6                   # TargetGrid::build: padded rows
M3C2_SHIFT = 0.3                    # B = a second sampling of the shape, moved this far along +z
M3C2_MIN_POINTS = 4
AXES6 = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))


def row(axis, seed=0):
    """coordinate `axis` = i + U(-0.2, 0.2), the other two exactly constant"""
    rng = np.random.default_rng(100 + 10 * seed + axis)
    P = np.tile(np.asarray(CONST, F32), (N_ROW, 1))
    P[:, axis] = (np.arange(N_ROW) + rng.uniform(-0.2, 0.2, N_ROW)).astype(F32)
    return np.ascontiguousarray(P)


def sheet(flat, seed=0):
    """a 64 x 48 lattice jittered by U(-0.3, 0.3) in the two other axes (64 along the first of them), coordinate `flat` constant"""
    rng = np.random.default_rng(200 + 10 * seed + flat)
    g = np.stack(np.meshgrid(np.arange(64), np.arange(48), indexing="ij"), -1).reshape(-1, 2).astype(np.float64)
    P = np.full((N_SHEET, 3), CONST[flat], F32)
    P[:, [a for a in range(3) if a != flat]] = (g + rng.uniform(-0.3, 0.3, g.shape)).astype(F32)
    return np.ascontiguousarray(P)


def capped(seed=0):
    """a 48 x 48 jittered patch with z in U(0, 0.3), then FAR"""
    rng = np.random.default_rng(300 + 10 * seed)
    g = np.stack(np.meshgrid(np.arange(48), np.arange(48), indexing="ij"), -1).reshape(-1, 2).astype(np.float64)
    patch = np.concatenate([g + rng.uniform(-0.3, 0.3, g.shape), rng.uniform(0.0, 0.3, (len(g), 1))], 1)
    return np.ascontiguousarray(np.concatenate([patch.astype(F32), FAR]))


def cloud(name, seed=0):
    """(n, 3) float32 of the shape `name` of SHAPES"""
    if name.startswith("row"):
        return row(int(name[3]), seed)
    if name.startswith("sheet"):
        return sheet(int(name[5]), seed)
    return capped(seed)


def with_normals(P):
    """(n, 6): +z on every point"""
    t = np.zeros((len(P), 6), F32)
    t[:, :3] = P
    t[:, 5] = 1
    return t


def unit_axes(name):
    """the axes on which the grid of the shape has one cell"""
    if name.startswith("row"):
        return [a for a in range(3) if a != int(name[3])]
    if name.startswith("sheet"):
        return [int(name[5])]
    return []


# ---- the inputs of the tools that take more than the cloud --------------------------------------------------------------------
def distance_source(name):
    """(n + 4, 3): the shape's points moved by U(-0.4, 0.4), then four probes in empty space: one beyond each end of a row (the
    other two nearer to them), above and below a sheet, in the middle of capped's box and near its points"""
    P = cloud(name)
    rng = np.random.default_rng(400 + SHAPES.index(name))
    near = P + rng.uniform(-0.4, 0.4, P.shape).astype(F32)
    if name.startswith("row"):
        a = int(name[3])
        probes = np.tile(np.asarray(CONST, F32), (4, 1))
        probes[:, a] = (-30.0, N_ROW + 30.0, -7.0, N_ROW + 6.0)
    elif name.startswith("sheet"):
        f = int(name[5])
        probes = np.empty((4, 3), F32)
        probes[:, [a for a in range(3) if a != f]] = ((10.3, 20.2), (40.1, 7.7), (63.2, 46.9), (-0.4, -0.3))
        probes[:, f] = np.asarray((30.0, -30.0, 6.0, -5.0), F32) + F32(CONST[f])
    else:
        probes = np.array([MIDDLE, (2100, 1900, 2050), (3950, 30, 20), (30, 30, 50)], F32)
    return np.ascontiguousarray(np.concatenate([near, probes]))


def fpfh_min_pairs(name):
    """a point of a row has four neighbours within R (two at the ends): below the default of 5, nothing would be described"""
    return 3 if name in ROWS else 5


def m3c2_inputs(name):
    """(core, A, B): A = the shape with +z normals, B = a second sampling of it moved M3C2_SHIFT along +z, core = every fourth
    point of A with random non-unit axes on every second of them; on capped also one core point in the empty middle of the box and
    one at the far corner"""
    A = with_normals(cloud(name))
    B = with_normals(cloud(name, seed=1))
    B[:, 2] = (B[:, 2].astype(np.float64) + M3C2_SHIFT).astype(F32)
    core = np.ascontiguousarray(A[::4])
    rng = np.random.default_rng(500 + SHAPES.index(name))
    v = rng.normal(size=(len(core), 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v *= rng.uniform(0.5, 2.0, len(core))[:, None]
    core[1::2, 3:] = v[1::2].astype(F32)
    if name == "capped":
        extra = with_normals(np.array([MIDDLE, FAR[0]], F32))
        extra[:, 3:] = np.array([[0.3, -0.5, 1.1], [-0.6, 0.2, -0.9]], F32)
        core = np.concatenate([core, extra])
    return np.ascontiguousarray(core), A, B


def m3c2_params(name):
    """the (R, L) of the shape: L = 60 crosses several enlarged cells and runs off both ends of a one-cell axis"""
    return [(R, 10.0), (R, 60.0)] if name in ("capped", "row0") else [(R, 10.0)]


def m3c2_axis_core(name):
    """the six axis-aligned normals on the first 200 core points"""
    core = m3c2_inputs(name)[0][:200]
    core = np.concatenate([core] * 6)
    core[:, 3:] = np.repeat(np.asarray(AXES6, F32), 200, axis=0)
    return np.ascontiguousarray(core)


def seam_inputs(name):
    """(target (n, 6), source (500, 6), T (4, 4) float64): 500 target points, the last points of the cloud among them (capped: the
    far ones), and the small rigid transform that moves them"""
    tgt = with_normals(cloud(name))
    rng = np.random.default_rng(600 + SHAPES.index(name))
    pick = np.sort(np.concatenate([rng.choice(len(tgt) - 3, 497, replace=False), np.arange(len(tgt) - 3, len(tgt))]))
    return tgt, np.ascontiguousarray(tgt[pick]), IR.perturb(np.eye(4), 1e-4, 0.3, seed=7)


# ---- what a grid has to look like to count as the shape --------------------------------------------------------------------------
def padded_rows(dims):
    return float(np.prod(np.asarray(dims, np.float64) + 4.0))


def is_capped(cell, dims, asked):
    """the cap decided the cell: at least 4 x the cell that was asked for, and the padded rows just under the cap"""
    return cell >= 4.0 * asked and CELL_CAP / 1.26 ** 3 < padded_rows(dims) <= CELL_CAP


def radius_cell(P, r=R, factor=1.03):
    """grid_walk.h's radius_cell for the cloud P"""
    amax = float(np.abs(np.concatenate([P.min(0), P.max(0)])).max())
    return float(F32(factor * r + 4e-6 * amax))
