"""numpy + scipy restatement of the connected components (plade_amd/csrc/components.h).

Edge: i ~ j when i != j and d(i, j) = ((dx dx + dy dy) + dz dz) in float32 < float32(r) * float32(r).  The edge set is exact on both
paths: brute force over all pairs (outlier_restate.flann_d2) for small clouds; for larger ones the candidate pairs of
cKDTree.query_pairs(1.001 r) in float64 -- a superset of the edges: the float32 expression is off from the true squared distance by
a few ulps of the largest squared coordinate difference, far less than the 0.2 % the candidate radius gives away -- each re-decided
with the float32 expression.  No tolerance, no excluded pairs.  The components are scipy's, renumbered by their smallest index; the
selection rule is plain numpy.
"""
import numpy as np

from outlier_restate import flann_d2

F32 = np.float32
BRUTE_MAX = 8192


def _xyz(points):
    return np.ascontiguousarray(np.asarray(points, F32)[:, :3])


def r2_of(r):
    return F32(r) * F32(r)


def pair_d2(X, i, j):
    """float32 ((dx dx + dy dy) + dz dz) of the pairs (i, j)."""
    a, b = X[i], X[j]
    dx = a[:, 0] - b[:, 0]
    dd = dx * dx
    dx = a[:, 1] - b[:, 1]
    dd = dd + dx * dx
    dx = a[:, 2] - b[:, 2]
    dd = dd + dx * dx
    return dd


def edges_brute(points, r, pairs=1 << 24):
    """All edges (i < j) by brute force: (m, 2) int64, sorted."""
    X = _xyz(points)
    n = len(X)
    r2 = r2_of(r)
    out = []
    step = max(1, pairs // max(n, 1))
    for c0 in range(0, n, step):
        dd = flann_d2(X[c0:c0 + step], X)
        ii, jj = np.nonzero(dd < r2)
        ii += c0
        m = ii < jj
        out.append(np.stack([ii[m], jj[m]], 1))
    e = np.concatenate(out) if out else np.zeros((0, 2), np.int64)
    return e[np.lexsort((e[:, 1], e[:, 0]))].astype(np.int64)


def edges_kdtree(points, r):
    """The same edge set from k-d tree candidates (float64, 1.001 r) re-decided in float32."""
    from scipy.spatial import cKDTree
    X = _xyz(points)
    cand = cKDTree(X.astype(np.float64)).query_pairs(1.001 * float(F32(r)), output_type="ndarray").astype(np.int64)
    if len(cand) == 0:
        return np.zeros((0, 2), np.int64)
    lo, hi = np.minimum(cand[:, 0], cand[:, 1]), np.maximum(cand[:, 0], cand[:, 1])
    m = pair_d2(X, lo, hi) < r2_of(r)
    e = np.stack([lo[m], hi[m]], 1)
    return e[np.lexsort((e[:, 1], e[:, 0]))]


def edges(points, r):
    return edges_brute(points, r) if len(points) <= BRUTE_MAX else edges_kdtree(points, r)


def labels_from_edges(n, e):
    """(label int32, size uint32): the components of the undirected graph, ids in ascending order of the smallest index."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    g = coo_matrix((np.ones(len(e), np.uint8), (e[:, 0], e[:, 1])), shape=(n, n))
    _, lab = connected_components(g, directed=False)
    first = np.full(lab.max() + 1, n, np.int64)
    np.minimum.at(first, lab, np.arange(n))
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    label = rank[lab].astype(np.int32)
    return label, np.bincount(label).astype(np.uint32)


def select(size, min_size=1, max_size=0, keep_largest=0):
    """kept (C bools): the components that pass, with keep_largest = m > 0 only the first m of them by (size descending, id)."""
    size = np.asarray(size, np.int64)
    ok = (size >= min_size) & ((size <= max_size) if max_size else True)
    if keep_largest > 0:
        ids = np.nonzero(ok)[0]
        ids = ids[np.lexsort((ids, -size[ids]))][:keep_largest]
        ok = np.zeros(len(size), bool)
        ok[ids] = True
    return ok


def components(points, r, min_size=1, max_size=0, keep_largest=0, edge_list=None):
    """dict label, size, keep, kept_index, rows and the summary fields n, components, kept_components, kept, largest."""
    P = np.asarray(points, F32)
    n = len(P)
    e = edges(P, r) if edge_list is None else edge_list
    label, size = labels_from_edges(n, e)
    kept_c = select(size, min_size, max_size, keep_largest)
    keep = kept_c[label]
    idx = np.nonzero(keep)[0].astype(np.uint32)
    return {"label": label, "size": size, "keep": keep, "kept_index": idx, "rows": P[idx],
            "n": n, "components": len(size), "kept_components": int(kept_c.sum()), "kept": len(idx), "largest": int(size.max())}
