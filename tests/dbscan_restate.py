"""numpy + scipy restatement of DBSCAN as the library defines it (plade_amd/csrc/dbscan.h), built on the exact
float32 edge set of components_restate.py.

count(i) = 1 (the point itself) + the edges at i; core: count >= min_points.  The clusters are scipy's components of the core-core
edges, renumbered by their smallest core index.  A non-core point with a core neighbour is a border point and takes the label of
the core neighbour with the smallest (d, j), d the float32 expression of the edge: a lexsort on (i, d, j).  Everything else is
noise, label -1.  The selection is components_restate.select on the sizes (core and border members).  No tolerance anywhere.
"""
import numpy as np

import components_restate as CR

F32 = np.float32
NOISE, BORDER, CORE = 0, 1, 2


def counts_from_edges(n, e):
    """count(i): the points closer than r, the point itself included."""
    return 1 + np.bincount(e[:, 0], minlength=n) + np.bincount(e[:, 1], minlength=n)


def core_labels(n, e, core):
    """(label int32 with -1 off the core points, C): the components of the core-core edges, ids by smallest core index."""
    label = np.full(n, -1, np.int32)
    idx = np.flatnonzero(core)
    if len(idx) == 0:
        return label, 0
    compact = np.full(n, -1, np.int64)
    compact[idx] = np.arange(len(idx))                      # monotone: the smallest compact index is the smallest core index
    ee = e[core[e[:, 0]] & core[e[:, 1]]]
    lab, size = CR.labels_from_edges(len(idx), np.stack([compact[ee[:, 0]], compact[ee[:, 1]]], 1))
    label[idx] = lab
    return label, len(size)


def border_pairs(X, e, core):
    """(i, j, d): every (non-core i, core j) pair of the edge set with its float32 distance, sorted by (i, d, j)."""
    a = np.concatenate([e[:, 0], e[:, 1]])
    b = np.concatenate([e[:, 1], e[:, 0]])
    m = ~core[a] & core[b]
    i, j = a[m], b[m]
    d = CR.pair_d2(X, i, j)
    o = np.lexsort((j, d, i))
    return i[o], j[o], d[o]


def dbscan(points, r, min_points=4, min_size=1, max_size=0, keep_largest=0, edge_list=None):
    """dict label, kind, size, keep, kept_index, rows, the summary fields n, clusters, core, border, noise, kept_clusters, kept,
    largest, and `contested`: the border points with core neighbours in more than one cluster."""
    P = np.asarray(points, F32)
    X = CR._xyz(P)
    n = len(P)
    e = CR.edges(P, r) if edge_list is None else edge_list
    core = counts_from_edges(n, e) >= min_points
    label, C = core_labels(n, e, core)
    kind = np.where(core, CORE, NOISE).astype(np.uint8)
    bi, bj, _ = border_pairs(X, e, core)
    contested = 0
    if len(bi):
        first = np.ones(len(bi), bool)
        first[1:] = bi[1:] != bi[:-1]                       # the smallest (d, j) of each i
        label[bi[first]] = label[bj[first]]
        kind[bi[first]] = BORDER
        seen = np.unique(np.stack([bi, label[bj].astype(np.int64)], 1), axis=0)
        contested = int((np.bincount(seen[:, 0]) > 1).sum())
    size = np.bincount(label[label >= 0], minlength=C).astype(np.uint32)
    kept_c = CR.select(size, min_size, max_size, keep_largest) if C else np.zeros(0, bool)
    keep = np.zeros(n, bool)
    keep[label >= 0] = kept_c[label[label >= 0]]
    idx = np.flatnonzero(keep).astype(np.uint32)
    return {"label": label, "kind": kind, "size": size, "keep": keep, "kept_index": idx, "rows": P[idx], "n": n, "clusters": C,
            "core": int(core.sum()), "border": int((kind == BORDER).sum()), "noise": int((kind == NOISE).sum()),
            "kept_clusters": int(kept_c.sum()), "kept": len(idx), "largest": int(size.max()) if C else 0, "contested": contested}
