"""Tables of the penetration filter (code/PLADE/util.cpp:450-519) for tests/test_penetration_items_host.py and
tests/test_gpu_penetration.py: the real ones out of the oracle's registration dump, and small synthetic ones whose every
coordinate is a dyadic rational, so that distances of exactly r/2 and r occur and are exact in fp32."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ANGLE_THRESHOLD = np.float32(5.0 / 180 * np.pi)       # plade.cpp:49
SCENES = (("g8", "g8_polyhedron.npz", ""), ("g9", "g9_room.npz", ""), ("g9b", "g9_room.npz", "b"))


class Tables:
    """What both seams take: cand K x 12; src / tgt = (coef, center, four, pts, off); the two thresholds."""

    def __init__(self, cand, src, tgt, length_threshold, angle_threshold=ANGLE_THRESHOLD):
        self.cand = np.ascontiguousarray(cand, np.float32).reshape(-1, 12)
        self.src, self.tgt = self._side(src), self._side(tgt)
        self.length_threshold = np.float32(length_threshold)
        self.angle_threshold = np.float32(angle_threshold)

    @staticmethod
    def _side(s):
        coef, center, four, pts, off = s
        return (np.ascontiguousarray(coef, np.float32).reshape(-1, 4), np.ascontiguousarray(center, np.float32).reshape(-1, 3),
                np.ascontiguousarray(four, np.float32).reshape(-1, 12), np.ascontiguousarray(pts, np.float32).reshape(-1, 3),
                np.ascontiguousarray(off, np.int32))

    def oracle_items(self, oracle):
        return oracle.penetration_items(self.cand, self.src, self.tgt, self.length_threshold, self.angle_threshold)


def real_tables(oracle, fixture, pre):
    """-> (Tables, pen_flags of the oracle's own short-circuited loop) of one golden scene."""
    g = np.load(os.path.join(GOLDEN, fixture))
    tp = (g[f"t{pre}_coef"], g[f"t{pre}_off"], g[f"t{pre}_idx"])
    sp = (g[f"s{pre}_coef"], g[f"s{pre}_off"], g[f"s{pre}_idx"])
    ok, _, d = oracle.registration(g["target"], g["source"], tp, sp, voxel_sort_mode=1)
    assert ok

    def side(tag, coef):
        return (coef, d[f"{tag}_plane_center_radius"].reshape(-1, 4)[:, :3], d[f"{tag}_plane_four"], d[f"{tag}_plane_ds"],
                d[f"{tag}_plane_ds_offsets"])
    lt = np.float32(d["average_spacing"][0]) * np.float32(5)      # plade.cpp:48
    return Tables(d["pen_candidates"], side("src", sp[0]), side("tgt", tp[0]), lt), d["pen_flags"]


_scene_cache = {}


def scene(oracle, name, mode):
    """-> (Tables, pen_flags of the oracle's loop, the oracle seam's records, its CPU seconds) of golden scene `name` under
    closest-point mode `mode`; computed once per session and left unchanged."""
    import time
    key = (name, mode)
    if key not in _scene_cache:
        fixture, pre = next((f, p) for n, f, p in SCENES if n == name)
        oracle.set_closest_point_mode(mode)
        try:
            tb, flags = real_tables(oracle, fixture, pre)
            t0 = time.perf_counter()
            rec = tb.oracle_items(oracle)
            dt = time.perf_counter() - t0
        finally:
            oracle.reset_closest_point_mode()
        _scene_cache[key] = (tb, flags, rec, dt)
    return _scene_cache[key]


# ---- synthetic crossings -------------------------------------------------------------------------------------------------
# The canonical pair: a TARGET patch in the plane z = 0 (its rectangle's first edge along x) and a SOURCE patch in the plane
# y = y0 (first edge along x, second along z).  They meet in the line (t, y0, 0); the common segment is the overlap of the
# two rectangles' x ranges.  A cloud is given in (t, w): t along the line, w = the in-plane offset from it (y - y0 for the
# target, z for the source).  With the walk's radius r = lengthThreshold and minDistance = r / 2, a point with |w| <= r / 2
# is never classified, and |w| < r / 2 makes it a gate point of the steps near its t.
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)


def band(t0, t1, pitch, rows):
    """(t, w) for t = t0, t0 + pitch, ... <= t1 and every w of rows."""
    t = t0 + pitch * np.arange(int(np.floor((t1 - t0) / pitch + 1e-9)) + 1)
    return np.array([(a, w) for w in rows for a in t], np.float64).reshape(-1, 2)


def crossing(t_tw, s_tw, t_x, s_x, y0=0.0, t_y=(-1.0, 1.0), s_z=(-1.0, 1.0)):
    """One canonical pair -> (source plane, target plane), each (coef 4, four 4 x 3, pts n x 3).  t_x / s_x: the x ranges of
    the two rectangles, t_y: the target rectangle's y range relative to y0, s_z: the source rectangle's z range."""
    t_tw, s_tw = np.asarray(t_tw, np.float64).reshape(-1, 2), np.asarray(s_tw, np.float64).reshape(-1, 2)
    tgt = (np.array([0, 0, 1, 0.0]),
           np.array([(t_x[0], y0 + t_y[0], 0), (t_x[1], y0 + t_y[0], 0), (t_x[1], y0 + t_y[1], 0), (t_x[0], y0 + t_y[1], 0)], np.float64),
           np.stack([t_tw[:, 0], y0 + t_tw[:, 1], np.zeros(len(t_tw))], 1))
    src = (np.array([0, 1, 0, -y0]),
           np.array([(s_x[0], y0, s_z[0]), (s_x[1], y0, s_z[0]), (s_x[1], y0, s_z[1]), (s_x[0], y0, s_z[1])], np.float64),
           np.stack([s_tw[:, 0], np.full(len(s_tw), y0), s_tw[:, 1]], 1))
    return src, tgt


def moved(plane, R, T):
    """The plane's tables under x -> R x + T (fp64; exact for signed permutations and dyadic T)."""
    coef, four, pts = plane
    R, T = np.asarray(R, np.float64).reshape(3, 3), np.asarray(T, np.float64)
    n = R @ coef[:3]
    return np.append(n, coef[3] - n @ T), four @ R.T + T, pts @ R.T + T


def tables(src_planes, tgt_planes, cands, r):
    def side(planes):
        off = np.cumsum([0] + [len(p[2]) for p in planes])
        four = np.array([p[1] for p in planes], np.float32).reshape(-1, 12)
        center = (four[:, 0:3] + four[:, 6:9]) / np.float32(2)
        pts = np.concatenate([np.asarray(p[2], np.float64).reshape(-1, 3) for p in planes]) if planes else np.zeros((0, 3))
        return np.array([p[0] for p in planes], np.float32).reshape(-1, 4), center, four, pts, off
    return Tables(np.asarray(cands, np.float32).reshape(-1, 12), side(src_planes), side(tgt_planes), r)


def rot_z(deg):
    """Candidate (R, T = 0) turning the source about z; exact entries at multiples of 90 degrees."""
    c, s = {0: (1, 0), 90: (0, 1), 180: (-1, 0), 270: (0, -1)}.get(deg % 360, (np.cos(np.radians(deg)), np.sin(np.radians(deg))))
    return np.array([c, -s, 0, s, c, 0, 0, 0, 1, 0, 0, 0], np.float32)


def gate_rows(t0, t1, r):
    """Two rows at w = +- r / 4, pitch r / 4: every step between t0 and t1 finds at least two of them within r / 2, and none
    of them is ever classified (|w| < minDistance)."""
    return band(t0, t1, r / 4, (-r / 4, r / 4))


def counted(n_pos, n_neg, r, t0=None):
    """n_pos points at w = +3r/4 and n_neg at w = -3r/4, at t = t0 (r/2), t0 + r/2, ...: each within r of a step (the nearest
    is at most r/2 away along the line: (1/4 + 9/16) r^2 < r^2) and farther than minDistance = r/2 from the other plane."""
    t0 = r / 2 if t0 is None else t0
    return np.array([(t0 + i * r / 2, 0.75 * r) for i in range(n_pos)] + [(t0 + i * r / 2, -0.75 * r) for i in range(n_neg)],
                    np.float64).reshape(-1, 2)


def threshold_pair(c0, c1, r, y0, length=4.0):
    """A pair whose pass 0 counts (pos, neg) = c0 and pass 1 counts = c1, every step gated in both passes."""
    g = gate_rows(0.0, length, r)
    return crossing(np.concatenate([g, counted(c1[0], c1[1], r)]), np.concatenate([g, counted(c0[0], c0[1], r)]),
                    (0.0, length), (0.0, length), y0=y0)


def reference_rule(c0, c1, min_points=10):
    """AreTwoPlanesPenetrable's thresholds (util.cpp:1407-1415, 1444-1452) on given counts."""
    def ratio(p, n):
        m = min(p, n + 1)
        return np.inf if m == 0 else max(p, n) / m
    if c0[0] < min_points or c0[1] < min_points or ratio(*c0) > 5:
        return 0
    if (c1[0] < min_points and c1[1] < min_points) or ratio(*c1) > 5:
        return 0
    return 1


THRESHOLD_CASES = [((9, 10), (10, 10)), ((10, 9), (10, 10)), ((10, 10), (10, 10)), ((55, 10), (10, 10)), ((56, 10), (10, 10)),
                   ((10, 55), (10, 10)), ((10, 10), (9, 9)), ((10, 10), (9, 10)), ((10, 10), (10, 0)), ((10, 10), (0, 10)),
                   ((10, 10), (55, 10)), ((10, 10), (56, 10))]


def threshold_tables(r=2.0 ** -3):
    """Pair q (source plane q, target plane q, 16 apart in y) carries THRESHOLD_CASES[q]; one candidate, the identity."""
    pairs = [threshold_pair(c0, c1, r, 16.0 * q) for q, (c0, c1) in enumerate(THRESHOLD_CASES)]
    return tables([p[0] for p in pairs], [p[1] for p in pairs], [IDENTITY], r)


def lattice_rows(r, half_width):
    """w = multiples of r/2 up to +- half_width, and +- r/4, +- 3r/4 (with the pitch r/2 alone every point off the line is at
    exactly minDistance or at r and beyond: nothing would ever be counted)."""
    n = int(round(half_width / (r / 2)))
    return sorted(set((r / 2 * np.arange(-n, n + 1)).tolist()) | {-0.75 * r, -0.25 * r, 0.25 * r, 0.75 * r})


def rotation_tables(r=2.0 ** -3):
    """Synthetic crossings: a 4 x 4 target lattice of pitch r/2 (so distances of exactly r/2 and r to step points occur) and a
    2 x 1 source patch through its middle; candidates turn the source about the target's normal by 0, 44, 45, 46, 90 and 180
    degrees: the walk's major axis in the target grid switches at slope 1, and 180 degrees reverses the direction."""
    h = r / 2
    g = h * np.arange(-32, 33)
    t_tw = np.concatenate([np.array([(a, b) for a in g for b in g]), band(-2.0, 2.0, h, (-0.75 * r, -0.25 * r, 0.25 * r, 0.75 * r)),
                           np.array([(b, a) for a, b in band(-2.0, 2.0, h, (-0.75 * r, -0.25 * r, 0.25 * r, 0.75 * r))])])
    s_tw = band(-1.0, 1.0, h, lattice_rows(r, 0.5))
    # (the rectangle is higher than wide: at 45 degrees the line leaves through its sides, not through its corners)
    s, t = crossing(t_tw, s_tw, (-2.0, 2.0), (-1.0, 1.0), t_y=(-2.5, 2.5), s_z=(-0.5, 0.5))
    return tables([s], [t], [rot_z(a) for a in (0, 44, 45, 46, 90, 180)], r)


def far_frame_tables(r=2.0 ** -3):
    """The same crossing seen through a general rotation with |T| about 1000: the source tables are the canonical ones under the
    candidate's inverse, so the moved source meets the target where the canonical one does, up to fp32 rounding out there."""
    h = r / 2
    s, t = crossing(band(-2.0, 2.0, h, lattice_rows(r, 1.0)), band(-1.0, 1.0, h, lattice_rows(r, 0.5)), (-2.0, 2.0), (-1.0, 1.0),
                    s_z=(-0.5, 0.5))
    ax = np.array([0.36, 0.48, 0.8])
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * K @ K
    T = np.array([640.0, -480.0, 600.0])
    R32, T32 = R.astype(np.float32), T.astype(np.float32)
    Rd = R32.astype(np.float64)
    s_own = moved(s, Rd.T, -Rd.T @ T)
    return tables([s_own], [t], [np.concatenate([R32.ravel(), T32]), np.concatenate([R32.ravel(), T32 + np.float32(r / 4)])], r)


def long_tables(nsteps_list, r=2.0 ** -3):
    """Pairs 16 apart in y whose common segments are (n - 1/2) r long: n steps each.  Cell = 2 r, so 140 / 280 / 600 steps are
    70 / 140 / 300 columns of the in-plane grids: the second, third and fifth 64-column round of a walk."""
    S, T = [], []
    for q, n in enumerate(nsteps_list):
        L = (n - 0.5) * r
        pts = np.concatenate([gate_rows(0.0, L, r), band(0.0, L, r / 2, (-0.75 * r, 0.75 * r))])
        s, t = crossing(pts, pts, (0.0, L), (-1.0, L + 1.0), y0=16.0 * q)
        S.append(s); T.append(t)
    return tables(S, T, [IDENTITY], r)


def crowded_tables(r=2.0 ** -3, seed=5):
    """Pair 0: one cell (2r x 2r) of each cloud holds 3000 points on a 2^-10 lattice, a third of them duplicates: its column
    hands out far more than 64 points per round.  Pair 1: the gate cloud of pass 0 has no point near step k when k % 3 == 0,
    exactly one within r/2 when k % 3 == 1, exactly two when k % 3 == 2 (that of pass 1 alternates one and two), and the classified points
    sit midway between two steps, within r of both: counted once, and only where one of the two steps is gated."""
    rng = np.random.default_rng(seed)
    q = 2.0 ** -10

    def crowd():
        p = np.stack([1.0 + q * rng.integers(0, int(2 * r / q), 2000), q * rng.integers(-int(r / q), int(r / q), 2000)], 1)
        return np.concatenate([p, p[:1000]])
    base = np.concatenate([gate_rows(0.0, 4.0, r), band(0.0, 4.0, r / 2, (-0.75 * r, 0.75 * r))])
    s0, t0 = crossing(np.concatenate([base, crowd()]), np.concatenate([base, crowd()]), (0.0, 4.0), (0.0, 4.0))
    k = np.arange(32)
    mid = np.array([(r * (i + 0.5), w) for i in k for w in (-0.75 * r, 0.75 * r)])
    # (where a step has one gate point it has a second one at EXACTLY r/2, which the strict < leaves out)
    t_gate = np.array([(r * i, w) for i in k for w in ((), (0.25 * r, -0.5 * r), (-0.25 * r, 0.25 * r))[i % 3]])
    s_gate = np.array([(r * i, w) for i in k for w in ((0.25 * r, -0.5 * r), (-0.25 * r, 0.25 * r))[i % 2]])
    s1, t1 = crossing(np.concatenate([t_gate, mid]), np.concatenate([s_gate, mid]), (0.0, 4.0), (0.0, 4.0), y0=16.0)
    return tables([s0, s1], [t0, t1], [IDENTITY], r)


def cap_tables(which, r=2.0 ** -6):
    """A plane longer than the 4096 cells an in-plane grid has per axis (cell = 2 r = 2^-5: 160 units are 5120 cells), the other
    plane short, points only near the far end: the walk lies beyond cell 4095 of the long plane's grid.
    which = (side whose plane is long, "major" | "minor": the grid axis that is capped, seen from the walk)."""
    side, axis = which
    rows = lattice_rows(r, 4 * r)
    pts = band(159.0, 159.5, r / 2, rows)
    long_x, short_x = ((0.0, 160.0), (159.0, 159.5)) if axis == "major" else ((158.0, 160.0), (159.0, 159.5))
    far = (-159.25, 0.75) if axis == "minor" else (-1.0, 1.0)     # minor: the line lies 159.25 up the rectangle's second edge
    if side == "tgt":
        s, t = crossing(pts, pts, long_x, short_x, t_y=far)
    else:
        s, t = crossing(pts, pts, short_x, long_x, s_z=far)
    return tables([s], [t], [IDENTITY], r)


def degenerate_tables(kind, r=2.0 ** -3):
    pts = np.concatenate([gate_rows(0.0, 4.0, r), band(0.0, 4.0, r / 2, (-0.75 * r, 0.75 * r))])
    s, t = crossing(pts, pts, (0.0, 4.0), (0.0, 4.0))
    if kind == "no_candidates":
        return tables([s], [t], np.zeros((0, 12)), r)
    if kind == "no_source_planes":
        return tables([], [t], [IDENTITY], r)
    if kind == "no_target_planes":
        return tables([s], [], [IDENTITY], r)
    if kind == "empty_plane":                   # a second source plane and a second target plane without points, 16 up in y
        s2, t2 = crossing(np.zeros((0, 2)), np.zeros((0, 2)), (0.0, 4.0), (0.0, 4.0), y0=16.0)
        return tables([s2, s], [t, t2], [IDENTITY], r)
    if kind == "gated":                         # source and target in the same plane: the gate of util.cpp:487-492 drops the pair
        return tables([(t[0].copy(), t[1].copy(), t[2].copy())], [t], [IDENTITY], r)
    if kind == "parallel":                      # a second target plane z = 1/2 against a source plane z = 0: no intersection line
        s2 = (t[0].copy(), t[1].copy(), t[2].copy())
        t2 = moved(t, np.eye(3), (0.0, 0.0, 0.5))
        return tables([s2], [t2], [IDENTITY], r)
    if kind == "edge_parallel":                 # the target rectangle turned by 0.5 degrees about z: two of its edges are within
        a = np.radians(0.5)                     # the 0.9999 rule of the line, the other two are hit: still two hits, walked
        Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        return tables([s], [moved(t, Rz, (0.0, 0.0, 0.0))], [IDENTITY], r)
    if kind == "corner":                        # the target rectangle turned by 45 degrees about its corner on the line: the line
        c, s_ = np.sqrt(0.5), np.sqrt(0.5)      # passes through that corner and meets two edges there and a third further on
        Rz = np.array([[c, -s_, 0], [s_, c, 0], [0, 0, 1]])
        t2 = (t[0], (np.array([(0, 0, 0), (2, 0, 0), (2, 2, 0), (0, 2, 0.0)]) @ Rz.T) + np.array([1.0, -np.sqrt(2.0), 0]), t[2])
        return tables([s], [t2], [IDENTITY], r)
    raise KeyError(kind)


# (angle in 1/64 degree, T_x, T_y in 2^-9) of candidates under which a counted target point lies in a grid cell that the walk
# reaches only through the sqrt(2) of pen_visit's `pad` (found with an fp64 model of its cell selection; such points are rare:
# a handful of items among the 17 000 of the golden tables)
PAD_CANDIDATES = [(3458, 53, -15), (3605, -58, -49), (2460, 4, 15), (3038, -38, 46), (3301, -2, -48), (2721, 39, 30)]


def pad_tables(r=2.0 ** -3, seed=7):
    """Oblique walks through a dense random target cloud (12 000 points on a 2^-9 lattice over 4 x 4)."""
    rng = np.random.default_rng(seed)
    q = 2.0 ** -9
    t_tw = np.stack([q * rng.integers(-1024, 1025, 12000), q * rng.integers(-1024, 1025, 12000)], 1)
    s, t = crossing(t_tw, band(-1.5, 1.5, r / 2, lattice_rows(r, 0.5)), (-2.0, 2.0), (-1.5, 1.5), t_y=(-2.5, 2.5), s_z=(-0.5, 0.5))
    cands = []
    for a64, tx, ty in PAD_CANDIDATES:
        c = rot_z(a64 / 64.0)
        c[9], c[10] = q * tx, q * ty
        cands.append(c)
    return tables([s], [t], cands, r)
