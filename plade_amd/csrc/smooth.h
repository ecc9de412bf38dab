// plade_amd/csrc/smooth.h -- moving-least-squares plane projection of a point cloud (k_smooth.hip).
//
// Semantics (include/plade_hip.h; no reference counterpart -- the reference's vendored PCL has no `surface`
// module).  Input: n points, rows of `stride` >= 3 floats, x y z first, all coordinates finite.  r > 0 and finite with r2 a normal fp32
// number (finite, >= FLT_MIN: d = 0 < r2 must hold for the point itself), min_neighbours >= 3, a finite viewpoint v.  r2 = (float)r * (float)r; d(i, j) = flann_d2(p_i, p_j), the fp32 expression of common.h.
//   neighbourhood N_i = { j : d(i, j) < r2 } (the `<` of sections 10 to 12); the point itself belongs to it (d = 0).  c_i = |N_i|,
//                 an exact integer
//   weights       u = (double)d / (double)r2, w = (1 - u) * (1 - u) in fp64: compact support, no exp
//   moments       fp64 about the query, q_j = double(p_j) - double(p_i): W = sum w, S = sum w q (3), M = sum (w q_a) q_b (6, upper
//                 triangle: xx xy xz yy yz zz), each added term by term in the order the walk meets the neighbours: the nine runs
//                 of for_block27 (z outer, y inner), ascending sorted position within a run.  No atomics.  mu = S / W,
//                 C = M / W - mu mu^T
//   fit           pca_eig (pca_eig.h, the eigen-solve of k_normals): n = the unit eigenvector of C's smallest eigenvalue l0,
//                 curvature = max(l0, 0) / trace; n is flipped when (v - p_i) . n < 0
//   projection    delta_i = n . mu in fp64 (the signed distance from p_i to the fitted plane along n);
//                 p_i' = fp32(double(p_i) + delta_i * n) per coordinate
//   unfitted      c_i < min_neighbours, or C exactly zero: the position is copied bit for bit, normal and curvature are NaN,
//                 delta = 0, fitted = 0
//   output        by original index: smoothed xyz (n x 3 fp32), normal (n x 3 fp32), curvature (fp32), displacement (fp64), count
//                 (uint32), fitted (uint8), moments (n x 10 fp64: W, S, M -- the test seam); the summary n, fitted, rms and max of
//                 |delta| over the fitted points (0 when there is none; a fixed-order fp64 reduction over the original index) and
//                 the largest c_i
//   errors        PLADE_EINVAL: n = 0, stride < 3, a non-finite coordinate or viewpoint, r <= 0 or not finite, r2 not finite
//                 or below FLT_MIN, min_neighbours < 3
// The same input gives the same bits on every run, on every context and from the host and the resident entry points.  c_i and
// fitted depend on the point set and r only; the fp64 sums follow the grid's order, so under a permutation of the input (or another
// bounding box) their last bits may differ.
#pragma once
#include "ctx.h"

namespace plade {

constexpr int SMOOTH_MIN_NEIGHBOURS = 3;

}  // namespace plade
