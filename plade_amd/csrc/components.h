// plade_amd/csrc/components.h -- connected components of a point cloud's radius graph and their selection by size
// (k_components.hip).
//
// Semantics (include/plade_hip.h; no reference counterpart -- PCL ships it as EuclideanClusterExtraction,
// Open3D as cluster_dbscan with min_points = 1).  Input: n >= 1 points, rows of `stride` >= 3 floats, x y z first, all coordinates
// finite.  d(i, j) = flann_d2(p_i, p_j), the fp32 expression of common.h.
//   parameters   radius r > 0 and finite with (float)r * (float)r finite (no automatic value); min_size >= 1 (default 1);
//                max_size: 0 = no upper bound, else >= min_size (default 0); keep_largest >= 0: 0 = no such selection (default 0)
//   edge         i ~ j when i != j and d(i, j) < (float)r * (float)r: the strict `<` of the radius filter.  d is symmetric in i and
//                j, so the graph is undirected; duplicates (d = 0) are connected; a pair at exactly d = r^2 is not
//   components   the connected components of that graph: an exact set.  Their ids run 0 .. C - 1 in ascending order of the
//                component's smallest original index.  label[i] (int32) = the id of i's component; size[c] (uint32) = its points
//   selection    component c passes when min_size <= size[c] and (max_size = 0 or size[c] <= max_size).  keep_largest = m > 0: only
//                the m passing components that come first in the order (size descending, id ascending) are kept; m = 0: all
//                passing components.  A point is kept when its component is
//   output       label (n); size (C entries, room for n); keep: n bytes 0 / 1; kept_index: the kept original indices, ascending;
//                the kept rows in that order, every float of a row copied bit for bit; the summary n, components = C,
//                kept_components, kept, largest = the largest size
//   errors       PLADE_EINVAL: n = 0, stride < 3, a NULL cloud, a non-finite coordinate, a bad radius, min_size < 1, max_size in
//                (0, min_size), keep_largest < 0.  A selection that keeps nothing is PLADE_OK with kept = 0; a resident result of 0
//                points is PLADE_EFAIL (plade_cloud has no empty form).  The grid refuses nothing of its own: where r asks for more cells
//                than it holds (48e6), its cell grows; a tiny r on a wide cloud then fills a row table of up to 192 MB per call
// The result depends on the point set and the parameters only: not on the grid's cell, the launch shapes, the order in which the
// unions happen, or whether the input is a host array or a resident cloud.
#pragma once
#include "ctx.h"
