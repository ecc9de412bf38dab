"""numpy + plain Python restatement of the consistent normal orientation (plade_amd/csrc/orient.h).

Vertices: the valid points (all three normal components finite and |component| <= float32(1e18)).  Edges: components_restate.edges --
the exact float32 radius graph -- between valid points.  dot32 = (nx nx' + ny ny') + nz nz' in float32 (numpy does not contract);
key32 = 0x7F800000 - bits(|dot32|); the order of the edges is (key32, min(i,j), max(i,j)).  The forest is Kruskal's over that order
with a union-find that carries a parity bit; boruvka() is the same forest by synchronous rounds, the form the GPU runs.  The anchors
(VOTE, EXTREME), `inward`, the labels and the summary are plain numpy.  No tolerance anywhere: every output is an exact function of
the rows and the parameters.
"""
import numpy as np

import components_restate as CR

F32 = np.float32
VOTE, EXTREME = 0, 1
KEY_TOP = 0x7F800000
KEY_FLAT = 0x40000000                  # |dot| = 1
NORMAL_MAX = F32(1e18)


def valid_points(rows):
    N = np.asarray(rows, F32)[:, 3:6]
    with np.errstate(invalid="ignore"):
        return (np.abs(N) <= NORMAL_MAX).all(1)        # (False for NaN and inf)


def dot32(N, i, j):
    a, b = N[i], N[j]
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def key32(d):
    return (np.int64(KEY_TOP) - np.abs(np.asarray(d, F32)).view(np.uint32).astype(np.int64))


def weighted_edges(rows, radius):
    """(lo, hi, key, s) of every edge between valid points, sorted by (key, lo, hi): int64, int64, int64, uint8."""
    rows = np.ascontiguousarray(rows, F32)
    ok = valid_points(rows)
    e = CR.edges(rows[:, :3], radius)
    e = e[ok[e[:, 0]] & ok[e[:, 1]]]
    lo, hi = e[:, 0], e[:, 1]
    with np.errstate(all="ignore"):
        d = dot32(rows[:, 3:6], lo, hi)
    key = key32(d)
    order = np.lexsort((hi, lo, key))
    return lo[order], hi[order], key[order], (d[order] < F32(0)).astype(np.uint8)


class ParityForest:
    """union-find over n points; find(i) -> (root, parity of i relative to the root)"""

    def __init__(self, n):
        self.parent = list(range(n))
        self.par = [0] * n

    def find(self, i):
        path = []
        while self.parent[i] != i:
            path.append(i)
            i = self.parent[i]
        p = 0
        for x in reversed(path):                        # compress: every node of the path directly under the root
            p ^= self.par[x]
            self.parent[x], self.par[x] = i, p
        return i, (self.par[path[0]] if path else 0)

    def union(self, i, j, s):
        """false: already in one tree.  Otherwise joins them so that parity_i ^ parity_j = s holds"""
        ri, pi = self.find(i)
        rj, pj = self.find(j)
        if ri == rj:
            return False
        self.parent[ri], self.par[ri] = rj, pi ^ pj ^ s
        return True


def kruskal(n, lo, hi, key, s, chunk=4096):
    """The forest over edges sorted by (key, lo, hi): (tree edge positions, ParityForest).  Edges inside one tree are dropped a chunk
    at a time with the roots of the chunk's start (a tree only grows: what was inside stays inside)."""
    uf = ParityForest(n)
    tree = []
    for c0 in range(0, len(lo), chunk):
        root = np.asarray(uf.parent, np.int64)
        while not np.array_equal(root, root[root]):
            root = root[root]
        l, h = lo[c0:c0 + chunk], hi[c0:c0 + chunk]
        for k in np.flatnonzero(root[l] != root[h]):
            if uf.union(int(l[k]), int(h[k]), int(s[c0 + k])):
                tree.append(c0 + int(k))
    return np.asarray(tree, np.int64), uf


def boruvka(n, lo, hi, key, s, order=None):
    """The same forest by synchronous rounds: every component picks its smallest outgoing edge of the previous round's components.
    order: the positions of the edges in the order that decides (default: as they are sorted).  Returns (sorted tree edge positions,
    ParityForest, rounds)."""
    rank = np.arange(len(lo)) if order is None else np.argsort(np.asarray(order), kind="stable")
    uf = ParityForest(n)
    tree, rounds = [], 0
    while True:
        rounds += 1
        root = [uf.find(i)[0] for i in range(n)]
        pick = {}
        for k in range(len(lo)):
            a, b = root[lo[k]], root[hi[k]]
            if a != b:
                for r in (a, b):
                    if r not in pick or rank[k] < rank[pick[r]]:
                        pick[r] = k
        hooks = 0
        for k in sorted(set(pick.values())):
            if uf.union(int(lo[k]), int(hi[k]), int(s[k])):
                tree.append(k)
                hooks += 1
        if not hooks:
            return np.asarray(sorted(tree), np.int64), uf, rounds


def labels_of(n, ok, uf):
    """(label int32 with -1 on invalid points, root per point, parity per point): ids in ascending order of the smallest index"""
    label = np.full(n, -1, np.int32)
    root, par = np.zeros(n, np.int64), np.zeros(n, np.uint8)
    ids = {}
    for i in range(n):
        if ok[i]:
            r, p = uf.find(i)
            root[i], par[i] = r, p
            label[i] = ids.setdefault(r, len(ids))
    return label, root, par


def flip_test(rows, v):
    """t_i of normals.h in fp64 from the float32 inputs: ((vx - px) nx + (vy - py) ny) + (vz - pz) nz"""
    R = np.asarray(rows, F32).astype(np.float64)
    v = np.asarray(v, F32).astype(np.float64)
    return ((v[0] - R[:, 0]) * R[:, 3] + (v[1] - R[:, 1]) * R[:, 4]) + (v[2] - R[:, 2]) * R[:, 5]


def along(X, d):
    X = np.asarray(X, F32).astype(np.float64)
    d = np.asarray(d, F32).astype(np.float64)
    return (X[:, 0] * d[0] + X[:, 1] * d[1]) + X[:, 2] * d[2]


def flipped_rows(rows, flip):
    out = np.ascontiguousarray(rows, F32).copy()
    w = out.view(np.uint32)
    w[:, 3:6] ^= (np.asarray(flip, np.uint32) << np.uint32(31))[:, None]
    return out


def orient(rows, radius, mode=VOTE, inward=0, viewpoint=(0, 0, 0), direction=(0, 0, 1), forest=None):
    """dict rows, flip (uint8), label (int32), the summary fields n, unoriented, components, flipped, tree_edges, tree_key_sum, and
    tree (m, 2) = the forest's edges.  forest: (lo, hi, key, s, tree positions, ParityForest) to anchor another forest than Kruskal's."""
    rows = np.ascontiguousarray(rows, F32)
    n = len(rows)
    ok = valid_points(rows)
    if forest is None:
        lo, hi, key, s = weighted_edges(rows, radius)
        tree, uf = kruskal(n, lo, hi, key, s)
    else:
        lo, hi, key, s, tree, uf = forest
    label, root, par = labels_of(n, ok, uf)
    flip = np.zeros(n, np.uint8)
    with np.errstate(all="ignore"):
        t = flip_test(rows, viewpoint)
        e = along(rows[:, :3], direction)
        g = along(rows[:, 3:6], direction)
    for c in range(label.max() + 1 if n else 0):
        m = np.flatnonzero(label == c)
        if mode == VOTE:
            f = par[m] ^ par[m[0]]                      # anchored at flip 0 on the smallest index
            tt = np.where(f == 1, -t[m], t[m])
            toggle = int((tt < 0).sum() > (tt > 0).sum()) ^ inward
            flip[m] = f ^ toggle
        else:
            a = m[e[m] == e[m].max()][0]                # the largest e, then the smaller index
            flip[m] = par[m] ^ par[a] ^ int(g[a] < 0) ^ inward
    return {"rows": flipped_rows(rows, flip), "flip": flip, "label": label, "n": n, "unoriented": int((~ok).sum()),
            "components": int(label.max() + 1) if n else 0, "flipped": int(flip.sum()), "tree_edges": len(tree),
            "tree_key_sum": int(key[tree].sum()) if len(tree) else 0, "tree": np.stack([lo[tree], hi[tree]], 1)}


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def sheet(n, seed=5):
    """n seeded points on a thin sheet: x, y uniform in a square of side sqrt(n) (mean point spacing 1), z in U(0, 0.1)"""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.c_[np.sqrt(n) * rng.random((n, 2)), 0.1 * rng.random(n)].astype(F32))


def with_normals(P, N):
    return np.ascontiguousarray(np.c_[np.asarray(P, F32)[:, :3], np.asarray(N, F32)], F32)


def random_normals(n, seed=1):
    N = np.random.default_rng(seed).normal(size=(n, 3))
    return (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(F32)


def random_flips(N, seed=2):
    """the normals N with every second one, at random, negated"""
    sign = np.where(np.random.default_rng(seed).random(len(N)) < 0.5, -1.0, 1.0)
    return (np.asarray(N, np.float64) * sign[:, None]).astype(F32)


def sphere(n, radius=10.0, seed=3):
    """(points, outward unit normals) of n seeded points on a sphere about the origin"""
    U = np.random.default_rng(seed).normal(size=(n, 3))
    U /= np.linalg.norm(U, axis=1, keepdims=True)
    return (radius * U).astype(F32), U.astype(F32)
