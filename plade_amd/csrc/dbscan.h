// plade_amd/csrc/dbscan.h -- density-based clustering of a point cloud (DBSCAN) and the selection of its clusters by size
// (k_dbscan.hip).
//
// Semantics (include/plade_hip.h; no reference counterpart -- Open3D ships it as cluster_dbscan, scikit-learn
// as DBSCAN, CloudCompare and PDAL under the same name).  Input: n >= 1 points, rows of `stride` >= 3 floats, x y z first, all
// coordinates finite.  d(i, j) = flann_d2(p_i, p_j), the fp32 expression of common.h; r2 = (float)r * (float)r.
//   parameters   radius r: finite and > 0, also as fp32, with r2 a normal fp32 number (radius_ok(r, true): a point must be its own
//                neighbour; no automatic value); min_points >= 1 (default 4: with 1 the tool is the components tool); min_size >= 1
//                (default 1), max_size: 0 = no upper bound, else >= min_size (default 0) and keep_largest >= 0 (default 0) as in
//                plade_component_params
//   count        count(i) = |{ j : d(i, j) < r2 }|, the strict `<` of every radius tool, the point itself included (Open3D's and
//                scikit-learn's convention).  i is a core point iff count(i) >= min_points.  The count is no output
//   clusters     the connected components of the graph on the core points alone, i ~ j iff both are core and d(i, j) < r2: an
//                exact set.  Ids run 0 .. C - 1 in ascending order of a cluster's smallest core index
//   border       a non-core point with at least one core point closer than r is a border point and takes the label of the core
//                neighbour j with the smallest key (d(i, j), j) (make_key of grid_walk.h: d >= 0, so the u64 order is the pair
//                order).  Textbook DBSCAN leaves this to the visiting order; here the result is a function of the point set and the
//                parameters.  A border point never connects two clusters
//   noise        everything else: label -1
//   selection    on size (core and border members) exactly as for the components (components.h); noise is never kept
//   output       label (n int32); kind (n bytes: 0 noise, 1 border, 2 core); size (C uint32, room for n); keep (n bytes 0 / 1);
//                kept_index: the kept original indices, ascending; the kept rows in that order, every float of a row copied bit for
//                bit; the summary n, clusters = C, core, border, noise, kept_clusters, kept, largest
//   errors       PLADE_EINVAL: n = 0, stride < 3, a NULL cloud, a non-finite coordinate, a bad radius, min_points < 1, min_size < 1,
//                max_size in (0, min_size), keep_largest < 0.  All noise, or a selection that keeps nothing, is PLADE_OK with
//                kept = 0; a resident result of 0 points is PLADE_EFAIL (plade_cloud has no empty form).  Bad input leaves the
//                outputs untouched and the context usable.  The grid refuses nothing of its own (components.h)
// The result depends on the point set and the parameters only: not on the grid's cell, the launch shapes, the order in which the
// unions happen, or whether the input is a host array or a resident cloud; the same bits on every run.  With min_points = 1 every
// point is core: label, size, keep, kept_index and the rows are those of plade_label_components bit for bit, kind is 2 everywhere.
#pragma once
#include "ctx.h"
