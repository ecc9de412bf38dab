// plade_amd/csrc/scales.h -- multi-scale normals and dimensionality features of a point cloud (k_scales.hip): the normal-scale step
// of M3C2 (Lague, Brodu, Leroux 2013).
//
// Semantics (include/plade_hip.h; no reference counterpart).  Input: n >= 1 points, rows of `stride` >= 3 floats,
// x y z first, all coordinates finite.  The queries are all n points, or query_index: k >= 1 strictly ascending indices < n (what
// plade_subsample_spacing's kept_index gives); every output is by query, in the order of that list.  1 <= S <= 8 radii r_s, each
// accepted by radius_ok(r, true), their fp32 squares r2_s = (float)r_s * (float)r_s strictly ascending; min_neighbours >= 3; mode and
// orient in {0, 1}; orient = 1 needs stride >= 6 and reads words 3..5 of a row as its normal g; a finite viewpoint v.
//   neighbourhoods  N(i, s) = { j : flann_d2(p_i, p_j) < r2_s } (the fp32 expression of common.h, the `<` of sections 10 to 15); the
//                   point itself belongs to every one of them.  c(i, s) = |N(i, s)|, an exact integer
//   moments         unweighted, fp64, about the query, q_j = double(p_j) - double(p_i): per scale the nine sums of q (3) and of
//                   q_a q_b (6: xx xy xz yy yz zz).  Each scale adds the terms of the neighbours that pass ITS OWN test, in the order
//                   the walk meets them: the nine runs of for_block27 (z outer, y inner) on the grid built for the largest radius,
//                   ascending sorted position within a run.  No atomics.  So the moments of a scale do not depend on which smaller
//                   scales were asked for
//   fit at scale s  mu = sum q / c, C = M / c - mu mu^T in the expression order of k_smooth_fit with (double)c in place of W;
//                   l1 >= l2 >= l3 from sym3_eigenvalues (pca_eig.h) on the six entries of C, each clamped with fmax(., 0) (always:
//                   c >= 1); n from pca_eig on the same six entries.  The scale is fitted iff c >= min_neighbours, pca_eig returns
//                   true and l1 > 0; the normal of an unfitted scale is NaN
//   features        fp64: linearity (l1 - l2) / l1, planarity (l2 - l3) / l1, sphericity l3 / l1, variation l3 / ((l1 + l2) + l3)
//   choice          over the fitted scales in ascending s: mode 0 keeps the largest planarity (M3C2's rule), mode 1 the smallest
//                   variation; a later scale replaces the current one only on a strict improvement (ties keep the smaller radius);
//                   chosen = -1 when no scale is fitted
//   orientation     of every scale's normal.  orient = 0: k_smooth_fit's viewpoint test, n is flipped when (v - p_i) . n < 0.
//                   orient = 1: t = (g_x n_x + g_y n_y) + g_z n_z with g as doubles; flipped when t < 0; when t is 0 or not finite the
//                   viewpoint test decides
//   output          by query, every array optional: chosen (int32), normal (3 fp32, the chosen scale's, NaN when -1), features
//                   (4 fp32 in the order above, the chosen scale's, NaN when -1); per scale count (S uint32), fitted (S uint8),
//                   eigenvalues (S x 3 fp64: l1 l2 l3), normals (S x 3 fp32), moments (S x 9 fp64 -- the test seam); the summary:
//                   queries, fitted (chosen >= 0), chosen_hist[8], the largest count, a reserved word -- integers in the fixed
//                   order of fixed_reduce.h
//   errors          PLADE_EINVAL: n = 0; stride < 3, or < 6 with orient = 1; a non-finite coordinate or viewpoint; S outside 1..8; a
//                   radius radius_ok refuses; squares not strictly ascending; min_neighbours < 3; mode or orient out of range; k = 0; a
//                   query index >= n or not ascending
// No eigenentropy: log has no bit-exact restatement.  The same input gives the same bits on every run, on every context and from
// the host and the resident entry points; counts, fitted flags and -- away from ties -- chosen depend on the point set and the radii
// only.
#pragma once
#include "ctx.h"

namespace plade {

constexpr int SCALES_MAX = 8;
constexpr int SCALES_MIN_NEIGHBOURS = 3;

}  // namespace plade
