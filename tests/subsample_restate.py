"""The minimum-spacing subsample (plade_amd/csrc/subsample.h) restated in numpy: the splitmix64 finaliser, the
priority keys, the float32 graph "closer than spacing", the sequential greedy walk that DEFINES the kept set, and the synchronous
rounds whose fixed point it is, with the round that decides each point.  Brute force over all pairs for the clouds of the tests (a
few thousand points); for the 30 000-point clouds of the CLI tests a kd-tree proposes the pairs and the same fp32 expression decides."""
import numpy as np

F32 = np.float32
M64 = (1 << 64) - 1


def mix64_int(z):
    """common.h's mix64 on a Python int"""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def mix64(z):
    """the same on a uint64 array (the products wrap)"""
    z = np.atleast_1d(np.asarray(z, np.uint64)).copy()
    with np.errstate(over="ignore"):
        z += np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def keys(n, seed=0, order="hash"):
    """the first component of the keys (the second is the index): mix64(mix64(seed) ^ i); order = "index" (the mutation the tests
    compare with): the index itself"""
    i = np.arange(n, dtype=np.uint64)
    return mix64(np.uint64(mix64_int(int(seed))) ^ i) if order == "hash" else i


def rank_of(key):
    """rank[i] = the position of point i in ascending (key, index) order"""
    order = np.lexsort((np.arange(len(key)), key))
    rank = np.empty(len(key), np.int64)
    rank[order] = np.arange(len(key))
    return rank, order


def d2(P):
    """(n, n) float32: (dx*dx + dy*dy) + dz*dz, every step rounded to fp32"""
    P = np.ascontiguousarray(P, F32)[:, :3]
    dx = P[:, None, 0] - P[None, :, 0]
    dd = dx * dx
    dx = P[:, None, 1] - P[None, :, 1]
    dd += dx * dx
    dx = P[:, None, 2] - P[None, :, 2]
    dd += dx * dx
    assert dd.dtype == F32
    return dd


def graph(P, spacing):
    """(n, n) bools: i != j and d(i, j) < (float)spacing * (float)spacing"""
    r2 = F32(spacing) * F32(spacing)
    A = d2(P) < r2
    np.fill_diagonal(A, False)
    return A


def edges(P, spacing, chunk=1024):
    """(i, j) of every ordered pair i != j with d(i, j) < r2, rows of the distance matrix `chunk` at a time (tens of thousands of
    points stay affordable)"""
    P = np.ascontiguousarray(P, F32)[:, :3]
    r2 = F32(spacing) * F32(spacing)
    if len(P) > 6000:
        return edges_tree(P, spacing)
    ii, jj = [], []
    for a in range(0, len(P), chunk):
        Q = P[a:a + chunk]
        dx = Q[:, None, 0] - P[None, :, 0]
        dd = dx * dx
        dx = Q[:, None, 1] - P[None, :, 1]
        dd += dx * dx
        dx = Q[:, None, 2] - P[None, :, 2]
        dd += dx * dx
        i, j = np.nonzero(dd < r2)
        i += a
        ii.append(i[i != j])
        jj.append(j[i != j])
    return np.concatenate(ii), np.concatenate(jj)


def edges_tree(P, spacing):
    """the same pairs for the clouds of the CLI tests (tens of thousands of points): a kd-tree proposes every pair within 1.001 x
    spacing in fp64 -- a superset: the fp32 expression is off by a few 1e-7 of itself --, the fp32 expression decides"""
    from scipy.spatial import cKDTree
    r2 = F32(spacing) * F32(spacing)
    pr = cKDTree(P.astype(np.float64)).query_pairs(1.001 * float(F32(spacing)) + 1e-30, output_type="ndarray")
    a, b = P[pr[:, 0]], P[pr[:, 1]]
    dx = a[:, 0] - b[:, 0]
    dd = dx * dx
    dx = a[:, 1] - b[:, 1]
    dd += dx * dx
    dx = a[:, 2] - b[:, 2]
    dd += dx * dx
    assert dd.dtype == F32
    pr = pr[dd < r2]
    i, j = np.concatenate([pr[:, 0], pr[:, 1]]), np.concatenate([pr[:, 1], pr[:, 0]])
    o = np.argsort(i, kind="stable")
    return i[o], j[o]


def greedy(n, i, j, rank, order):
    """the definition: walk in ascending key order, keep a point when no kept point is its neighbour"""
    start = np.searchsorted(i, np.arange(n + 1))             # (i ascending: the rows of the chunks in order)
    keep = np.zeros(n, bool)
    for p in order:
        if not keep[j[start[p]:start[p + 1]]].any():         # (a kept neighbour was walked earlier: it has a smaller key)
            keep[p] = True
    return keep


def rounds(n, i, j, rank):
    """the synchronous rounds: (keep, round[i], rounds).  Edge lists, so that a long chain in index order (n rounds) stays cheap"""
    low = rank[j] < rank[i]
    r, c = i[low], j[low]                                    # c: a neighbour of r with a smaller key
    state = np.zeros(n, np.int8)                             # 0 undecided, 1 kept, 2 dropped
    rnd = np.zeros(n, np.uint32)
    t = 0
    while (state == 0).any():
        t += 1
        live = state[r] == 0
        r, c = r[live], c[live]
        has_kept = np.bincount(r, weights=state[c] == 1, minlength=n) > 0
        has_und = np.bincount(r, weights=state[c] == 0, minlength=n) > 0
        und = state == 0
        drop = und & has_kept
        take = und & ~has_kept & ~has_und
        state[drop] = 2
        state[take] = 1
        rnd[drop | take] = t
    return state == 1, rnd, t


def subsample(P, spacing, seed=0, order="hash"):
    """dict: keep (n bools), kept_index (uint32, ascending), round (n uint32), rounds, n, kept, first (the point with the smallest
    key) -- and greedy, the sequential walk's set, for the callers that compare the two"""
    P = np.ascontiguousarray(P, F32)
    n = len(P)
    i, j = edges(P, spacing)
    rank, by_key = rank_of(keys(n, seed, order))
    keep, rnd, t = rounds(n, i, j, rank)
    return {"keep": keep, "kept_index": np.flatnonzero(keep).astype(np.uint32), "round": rnd, "rounds": t, "n": n,
            "kept": int(keep.sum()), "greedy": greedy(n, i, j, rank, by_key), "first": int(by_key[0])}


def separated(P, keep, spacing):
    """no kept pair with d < r2 (brute force, independent of the keys)"""
    A = graph(P, spacing)
    return not A[np.ix_(keep, keep)].any()


def maximal(P, keep, spacing):
    """every dropped point has a kept point with d < r2"""
    A = graph(P, spacing)
    return bool(A[np.ix_(~keep, keep)].any(1).all())


# ---- the clouds of the tests ------------------------------------------------------------------------------------------------------
def sheet(n, seed=5, width=None):
    """n seeded points on a thin sheet: x, y uniform in a square of side sqrt(n) (mean point spacing 1), z in U(0, 0.1)"""
    rng = np.random.default_rng(seed)
    side = np.sqrt(n) if width is None else width
    return np.ascontiguousarray(np.c_[side * rng.random((n, 2)), 0.1 * rng.random(n)].astype(F32))


def chain(n=3000, step=0.6):
    """the sorted collinear chain: a scan line.  x = i * step (spacing 1: only the two direct neighbours are closer)"""
    P = np.zeros((n, 3), F32)
    P[:, 0] = (np.arange(n) * step).astype(F32)
    return P
