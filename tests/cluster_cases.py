"""The candidate sets of the clustering tests, built once and shared: tests/test_cluster_host.py pins the restatement
(tests/cluster_restate.py) on every one of them against the oracle without a GPU, tests/test_gpu_cluster.py runs them through the
seam plade_cluster_transforms.  case(name) = (t_xyz, euler, dist_threshold, angle_gate), reference(name) = the restatement's
(cluster_of, n_clusters); both are cached and read-only.

Also here: the cell coordinate of k_t_keys restated in numpy, in the float64 form the kernel uses and in the float32 form it used
before, for the checks that a case really reaches the part of the hash it is aimed at.
"""
import functools

import numpy as np

import cluster_restate as KR

F32 = np.float32
R = 0.06          # lengthThreshold / 2 of the golden registrations
GATE = 0.004
BLOBS = (5, 17, 80, 81)   # candidates in the x-row window of a node: 16 walked by the lane itself, the rest 64 per wavefront step


# ---- the hash of cluster_transforms / k_t_keys ---------------------------------------------------------------------------
def grid_of(t_xyz, r):
    """(mn float32[3], cell float32): the corner and the cell edge after the doubling loop of cluster_transforms."""
    T = np.asarray(t_xyz, F32).reshape(-1, 3)
    mn, mx = T.min(0), T.max(0)
    cell = F32(r) * F32(1.001)
    if not cell > 0:
        cell = F32(1)
    ext = float((mx.astype(np.float64) - mn.astype(np.float64)).max())
    while not ext / float(cell) + 4 < float(1 << 21):
        cell = F32(cell * F32(2))
    return mn, cell


def cells_f64(t_xyz, r):
    """(m, 3) int64: floor((double(t) - double(mn)) * (1.0 / double(cell))) + 1, the kernel's cell coordinates."""
    T = np.asarray(t_xyz, F32).reshape(-1, 3)
    mn, cell = grid_of(T, r)
    return np.floor((T.astype(np.float64) - mn.astype(np.float64)) * (1.0 / np.float64(cell))).astype(np.int64) + 1


def cells_f32(t_xyz, r):
    """The same in float32 throughout, floorf((t - mn) * (1.f / cell)) + 1: what k_t_keys computed before it went to float64."""
    T = np.asarray(t_xyz, F32).reshape(-1, 3)
    mn, cell = grid_of(T, r)
    inv = F32(1) / cell
    return np.floor((T - mn) * inv).astype(np.int64) + 1


def x_window_counts(t_xyz, r):
    """Per candidate: how many candidates lie in the cells (cx - 1 .. cx + 1, cy, cz) -- the length of the span that one lane of
    k_cluster_edges walks for the candidate's own row."""
    c = cells_f64(t_xyz, r)
    cnt = {}
    for k in map(tuple, c):
        cnt[k] = cnt.get(k, 0) + 1
    return np.array([sum(cnt.get((x + d, y, z), 0) for d in (-1, 0, 1)) for (x, y, z) in map(tuple, c)], np.int64)


# ---- the candidate sets ----------------------------------------------------------------------------------------------------
def _mixed(m, seed=3):
    """m candidates of mixed content.  From 255 on: a corner candidate that fixes the grid's origin; four blobs of BLOBS candidates,
    each inside one cell of the same x-row of cells, ten cells apart, each split in two by its Euler angles; isolated candidates in
    cells of their own; exact duplicates of isolated ones, half with the same angles (they join) and half with others (they do not);
    for what is left a slab of random candidates near the percolation threshold with noisy angles.  Indices shuffled."""
    rng = np.random.default_rng(seed)
    if m == 1:
        return np.array([[0.25, -1.5, 3.0]], F32), np.array([[0.1, 0.2, 0.3]], F32)
    if m == 2:
        return np.array([[0.25, -1.5, 3.0], [0.25 + 0.5 * R, -1.5, 3.0]], F32), np.zeros((2, 3), F32)
    assert m >= 255
    cell = np.float64(F32(R) * F32(1.001))
    c0 = np.array([-2.0, -2.5, -0.25])
    T, E = [c0], [np.zeros(3)]
    for k, nb in enumerate(BLOBS):
        centre = c0 + (np.array([10 + 10 * k, 5, 5]) + 0.5) * cell
        T += list(centre + (rng.random((nb, 3)) - 0.5) * 0.4 * cell)
        E += [np.array([0.5 * (i >= nb // 2), 0.0, 0.0]) for i in range(nb)]
    n_dup, n_slab = 20, max(0, m - 257)
    n_iso = m - 1 - sum(BLOBS) - n_dup - n_slab
    iso = [c0 + (np.array([2 * i, 12 + 2 * (i % 3), 0]) + 0.5) * cell for i in range(n_iso)]
    T += iso
    E += [np.zeros(3)] * n_iso
    T += iso[:n_dup]
    E += [np.array([0.0, 0.5 * (i % 2), 0.0]) for i in range(n_dup)]
    if n_slab:
        T += list(c0 + np.array([0.0, 30 * cell, 0.0]) + rng.random((n_slab, 3)) * np.array([3.0, 2.0, 0.2]))
        E += list(rng.normal(0.0, 0.03, (n_slab, 3)) * (rng.random((n_slab, 1)) < 0.5))
    p = rng.permutation(m)
    return np.asarray(T, F32)[p], np.asarray(E, F32)[p]


def _dense():
    """3000 candidates inside one cell (a 0.05 cube, r = 0.06), one Euler angle from five values 0.5 apart: five clusters, spans of
    thousands, every union contended."""
    rng = np.random.default_rng(7)
    t = (rng.random((3000, 3)) * 0.05).astype(F32)
    e = np.zeros((3000, 3), F32)
    e[:, 0] = rng.integers(0, 5, 3000) * 0.5
    return t, e


CHAIN_R = 0.0625   # a power of two: a link of exactly r can be written down
CHAIN_SEED = 11


def _chain(cut):
    """4000 candidates 0.99 r apart along the diagonal, indices shuffled: parent chains as deep as the union-find makes them.  cut: the
    link after candidate 2500 is (r, 0, 0) exactly -- float32 d^2 == r^2, no edge under the strict <."""
    rng = np.random.default_rng(CHAIN_SEED)
    s = F32(0.99 * CHAIN_R / np.sqrt(3.0))
    k = np.arange(4000)
    if cut:
        base = F32(2500) * s
        x = np.where(k <= 2500, k.astype(F32) * s, (base + F32(CHAIN_R)) + (k - 2501).astype(F32) * s).astype(F32)
        yz = np.where(k <= 2500, k.astype(F32) * s, base + (k - 2501).astype(F32) * s).astype(F32)
        t = np.stack([x, yz, yz], 1)
    else:
        t = np.repeat((k.astype(F32) * s)[:, None], 3, 1)
    p = rng.permutation(4000)
    return t[p].astype(F32), np.zeros((4000, 3), F32)


def _lattice():
    """9 x 9 x 9 candidates exactly on multiples of the cell edge (the grid's origin is one of them), each with a partner up to r away:
    below, above and diagonally across the cell boundary the candidate sits on."""
    cell = F32(R) * F32(1.001)
    g = np.arange(9).astype(F32) * cell
    L = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(F32)
    off = np.array([[-0.5, 0, 0], [0, -0.5, 0], [0, 0, -0.5], [0.5, 0, 0], [-0.4, -0.4, -0.4], [0.999, 0, 0], [0, 0.999, 0],
                    [0, 0, 0.999]]) * R
    P = (L.astype(np.float64) + off[np.arange(len(L)) % len(off)]).astype(F32)
    return np.concatenate([L, P]), np.zeros((2 * len(L), 3), F32)


def _same_spot(two):
    t = np.tile(np.array([[1.5, -2.25, 0.75]], F32), (1000, 1))
    e = np.zeros((1000, 3), F32)
    if two:
        e[:, 1] = (np.arange(1000) % 2) * 0.5
    return t, e


WIDE_PAIRS = 3000


def _wide(axis, far=False):
    """An anchor and 3000 pairs (a, b) along one axis, b - a just inside r in float32, over an extent of 60 000: 10^6 cells, where a
    float32 cell coordinate is good to 0.06 cells and the probe of +-1 cell has a margin of 0.001.  Candidates: the anchor, all a, all
    b; pair k at (k, k mod 7) on the other two axes.  far: the anchor 4 10^6 away on all three axes instead -- the cell doubles five
    times and the key takes 63 bits."""
    rng = np.random.default_rng(5)
    f = F32
    r = f(R)
    r2 = KR.r2_of(R)
    a = f(rng.random(WIDE_PAIRS) * 30000 + 7800)
    b = f(a + f(0.99995) * r)
    for _ in range(8):
        late = ~((b - a) * (b - a) < r2)
        b = np.where(late, np.nextafter(b, f(-np.inf)), b).astype(f)
    assert ((b - a) * (b - a) < r2).all() and (b > a).all()
    k = np.arange(WIDE_PAIRS)
    pair = lambda x: np.stack([x, k.astype(f), (k % 7).astype(f)], 1)
    anchor = [-(4.0e6 - 37800), -(4.0e6 - 3000), -(4.0e6 - 6)] if far else [-0.37 * 60000, 0, 0]
    t = np.concatenate([np.array([anchor], f), pair(a), pair(b)]).astype(f)
    return np.roll(t, axis, axis=1), np.zeros((len(t), 3), f)


def _by_gate_only():
    rng = np.random.default_rng(13)
    t = ((rng.random((300, 3)) - 0.5) * 100).astype(F32)
    e = (rng.normal(0, 0.005, (300, 3))).astype(F32)
    e[:, 2] += (rng.integers(0, 3, 300) * 0.5).astype(F32)
    return t, e


def _shifted():
    t, e = _mixed(5000)
    return (t + np.array([1000, -2000, 500], F32)).astype(F32), e


PERM_SEED = 17


def _permuted():
    t, e = _mixed(5000)
    p = np.random.default_rng(PERM_SEED).permutation(len(t))
    return t[p], e[p]


def _pair_x(x, e1=(0, 0, 0)):
    return np.array([[0, 0, 0], [x, 0, 0]], F32), np.array([[0, 0, 0], e1], F32)


def _nan_euler():
    t = np.array([[0, 0, 0], [0.01, 0, 0], [0.02, 0, 0], [0.02, 0, 0]], F32)
    e = np.zeros((4, 3), F32)
    e[1, 1] = np.nan
    return t, e


_BUILD = {
    "mixed_1": lambda: _mixed(1) + (R, GATE),
    "mixed_2": lambda: _mixed(2) + (R, GATE),
    "mixed_255": lambda: _mixed(255) + (R, GATE),
    "mixed_256": lambda: _mixed(256) + (R, GATE),
    "mixed_257": lambda: _mixed(257) + (R, GATE),
    "mixed_5000": lambda: _mixed(5000) + (R, GATE),
    "dense": lambda: _dense() + (R, GATE),
    "chain": lambda: _chain(False) + (CHAIN_R, GATE),
    "chain_cut": lambda: _chain(True) + (CHAIN_R, GATE),
    "r_apart": lambda: _pair_x(0.5) + (0.5, GATE),
    "r_joined": lambda: _pair_x(np.nextafter(F32(0.5), F32(0))) + (0.5, GATE),
    "gate_apart": lambda: _pair_x(0.01, (0, 0.5, 0)) + (R, 0.25),
    "gate_joined": lambda: _pair_x(0.01, (0, 0.5, 0)) + (R, float(np.nextafter(F32(0.25), F32(1)))),
    "nan_euler": lambda: _nan_euler() + (R, GATE),
    "shifted_5000": lambda: _shifted() + (R, GATE),
    "permuted_5000": lambda: _permuted() + (R, GATE),
    "lattice": lambda: _lattice() + (R, GATE),
    "same_spot_one": lambda: _same_spot(False) + (R, GATE),
    "same_spot_two": lambda: _same_spot(True) + (R, GATE),
    "wide_x": lambda: _wide(0) + (R, GATE),
    "wide_y": lambda: _wide(1) + (R, GATE),
    "wide_z": lambda: _wide(2) + (R, GATE),
    "far_63bit": lambda: _wide(0, far=True) + (R, GATE),
    "r_zero": lambda: _mixed(257) + (0.0, GATE),
    "r_inf": lambda: _by_gate_only() + (float("inf"), GATE),
}
NAMES = tuple(_BUILD)


@functools.lru_cache(maxsize=None)
def case(name):
    t, e, r, gate = _BUILD[name]()
    t, e = np.ascontiguousarray(t, F32), np.ascontiguousarray(e, F32)
    t.setflags(write=False)
    e.setflags(write=False)
    return t, e, float(r), float(gate)


@functools.lru_cache(maxsize=None)
def reference(name):
    lab, n = KR.cluster(*case(name))
    lab.setflags(write=False)
    return lab, n
