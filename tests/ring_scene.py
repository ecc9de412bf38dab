"""One small scene that makes the shared ring walk (plade_amd/csrc/grid_walk.h: ring_step) do everything it can do, and a CPU
model of the walk that says so (test_ring_scene_host.py).  A 64 x 64 jittered planar patch in the low corner of the box and eight
isolated points far from it along different axes, the last one the box's high corner.  The three ring consumers use it:
test_gpu_normals.py, test_gpu_outliers.py, test_gpu_distances.py."""
import numpy as np

N_PATCH, N_FAR = 4096, 8
FAR = np.array([[150, 20, 0.1], [30, 160, 0.2], [20, 30, 140], [140, 150, 0.0], [150, 10, 130], [10, 150, 140], [160, 90, 5],
                [170, 170, 170]], np.float32)
PROBES = np.array([[129, 109, 99], [100, 73, 76], [119, 100, 96], [90, 94, 105], [113, 102, 82], [115, 143, 83], [85, 83, 95],
                   [83, 138, 85]], np.float32)
GAP = 80.0                       # every probe of PROBES is farther than this from every point of the scene
RADII = (70.0, 120.0)            # the distance test's bounds: below and above the gap


def scene():
    """(4104, 3) fp32: the patch, then FAR"""
    rng = np.random.default_rng(11)
    g = np.stack(np.meshgrid(np.arange(64), np.arange(64), indexing="ij"), -1).reshape(-1, 2).astype(np.float64)
    patch = np.concatenate([g + rng.uniform(-0.3, 0.3, g.shape), rng.uniform(0.0, 0.3, (len(g), 1))], 1)
    return np.ascontiguousarray(np.concatenate([patch.astype(np.float32), FAR]))


def target():
    """the scene as a target cloud (n x 6, normals +z)"""
    t = np.zeros((N_PATCH + N_FAR, 6), np.float32)
    t[:, :3] = scene()
    t[:, 5] = 1
    return t


def probes():
    """(264, 3) fp32 source of the distance test: 256 points near the patch, then PROBES in the empty middle of the box"""
    rng = np.random.default_rng(12)
    P = scene()
    near = P[rng.choice(N_PATCH, 256, replace=False)] + rng.uniform(-0.2, 0.2, (256, 3)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([near, PROBES]))


# ---- a model of the grids and of the walk -------------------------------------------------------------------------------------
# The functions below restate TargetGrid::build, build_knn_grid, distances_dev's cell and ring_step, constants included.  They are
# no reference for the library: they only qualify the scene (does a walk over it meet every case?), and have to follow the C++
# when it changes.  What the GPU computes is compared with the independent brute-force restatements, never with these.
def build(P, min_cell):
    """TargetGrid::build's cell and cell counts for the cloud P"""
    mn, mx = P.min(0), P.max(0)
    cell = np.float32(min_cell) * np.float32(1.001)
    while True:
        dims = np.floor((mx - mn) / cell).astype(np.int64) + 1
        if np.prod(dims + 4.0) <= 48.0e6:
            return float(cell), dims
        cell *= np.float32(1.26)


def cells_of(P, Q, cell, dims):
    c = np.floor((Q - P.min(0)) * np.float32(1.0 / cell)).astype(np.int64)
    return np.clip(c, 0, dims - 1)


def knn_grid(P, k):
    """build_knn_grid's cell and cell counts"""
    n = len(P)
    e = np.maximum(1e-9, P.max(0).astype(np.float64) - P.min(0))
    area, goal = 2 * (e[0] * e[1] + e[1] * e[2] + e[0] * e[2]), 0.7 * k
    want = np.float32(1.5 * np.sqrt(k * area / (np.pi * n)))
    for attempt in range(4):
        cell, dims = build(P, want)
        if attempt == 3 or n <= 4 * k:
            break
        occ = len(np.unique(cells_of(P, P, cell, dims), axis=0))
        mean = n / max(occ, 1)
        if mean > 2 * goal and cell <= want * 1.01:
            want = np.float32(cell * max(0.25, np.sqrt(goal / mean)))
        elif mean < 0.5 * goal and occ < n:
            want = np.float32(cell * min(4.0, np.sqrt(goal / mean)))
        else:
            break
    return cell, dims


def distance_grid(T, d):
    """distances_dev's cell and cell counts for the target T"""
    e = np.maximum(1e-9, T.max(0).astype(np.float64) - T.min(0))
    area = 2 * (e[0] * e[1] + e[1] * e[2] + e[0] * e[2])
    amax = float(np.abs(np.concatenate([T.min(0), T.max(0)])).max())
    return build(T, min(1.5 * np.sqrt(8.0 * area / (np.pi * len(T))), 1.03 * d + 4e-6 * amax))


def walk(P, q, cell, dims, need):
    """The steps of ring_step for the query q until every point outside the block is farther than `need` (the k-th distance, or
    the search bound) -- the kernels stop no earlier: their k-th key of what they have scanned is no smaller.  Per step:
    (rout, rows of the block, rows with whole runs, rows with side runs, sides clipped by the grid's edge)."""
    c = cells_of(P, q[None], cell, dims)[0]
    mn = P.min(0).astype(np.float64)
    steps, rin, rout = [], -1, 1
    while True:
        lo, hi = np.maximum(c - rout, 0), np.minimum(c + rout, dims - 1)
        y, z = np.meshgrid(np.arange(lo[1], hi[1] + 1), np.arange(lo[2], hi[2] + 1), indexing="ij")
        whole = (np.abs(y - c[1]) > rin) | (np.abs(z - c[2]) > rin)
        sides = (c[0] - rin - 1 >= lo[0]) or (c[0] + rin + 1 <= hi[0])
        clipped = int((c - rout < 0).sum() + (c + rout > dims - 1).sum())
        steps.append((rout, whole.size, int(whole.sum()), int((~whole).sum()) if sides else 0, clipped))
        reach = np.inf
        for t in range(3):
            if c[t] - rout > 0:
                reach = min(reach, q[t] - (mn[t] + (c[t] - rout) * cell))
            if c[t] + rout < dims[t] - 1:
                reach = min(reach, (mn[t] + (c[t] + rout + 1) * cell) - q[t])
        if reach == np.inf or reach - 0.01 * cell > need:      # (the kernels' margin is a little larger: they stop no earlier)
            return steps
        rin, rout = rout, rout + max(1, rout // 2)


def does_everything(steps):
    """the row loop runs more than once, a step has whole-row and side runs, three growth steps, a step clipped on a side"""
    return (max(s[1] for s in steps) > 64 and any(s[2] > 0 and s[3] > 0 for s in steps) and len(steps) >= 4
            and any(s[4] > 0 for s in steps))
