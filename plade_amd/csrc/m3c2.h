// plade_amd/csrc/m3c2.h -- M3C2 distances between two registered clouds (k_m3c2.hip): per core point a cylinder along the local
// normal, the mean position of each cloud inside it along that normal, their difference and its 95 % level of detection
// (Lague, Brodu, Leroux 2013).
//
// Semantics (include/plade_hip.h; no reference counterpart).  Input: m >= 1 core points, rows x y z nx ny nz
// with finite coordinates (the normals need not be unit and may be non-finite); the reference cloud A and the compared cloud B,
// n >= 1 points each, rows of `stride` >= 3 floats, x y z first, finite; T: row-major fp32 4 x 4, B -> the frame of A and the core
// points (NULL: the identity, which goes through the same arithmetic).  R = radius > 0, L = depth > 0 (the cylinder's half-length),
// reg_error >= 0, min_points >= 2.
//   transform    B' = ((r0 x + r1 y) + r2 z) + t per row in fp32 (the rule of distances.h)
//   axis         len2 = (nx nx + ny ny) + nz nz in fp64; n^ = double(n) / sqrt(len2).  len2 not finite or 0: no axis -- both
//                counts 0, the moments 0, every derived output NaN, significant 0 (not an error)
//   membership   fp64 from the fp32 inputs, no contraction: q = double(p) - double(c); t = (q_x n^_x + q_y n^_y) + q_z n^_z;
//                e = q - t n^ per coordinate; rho2 = (e_x e_x + e_y e_y) + e_z e_z; p is in the cylinder iff
//                fabs(t) <= L && rho2 < R * R (the strict `<` of sections 10 to 15 on the radius, closed ends)
//   moments      per core point and cloud X: c_X (exact), S1_X = sum t, S2_X = sum t t; fp64 sums in the order of the grid walk
//                (lane by lane, then one xor butterfly).  No atomics
//   result       valid iff there is an axis and c_A, c_B >= min_points.  mean_X = S1_X / c_X;
//                var_X = max(S2_X - S1_X mean_X, 0) / (c_X - 1); sigma_X = sqrt(var_X); distance = mean_B - mean_A;
//                lod = 1.96 (sqrt(var_A / c_A + var_B / c_B) + reg_error); significant = |distance| > lod.  Not valid: distance,
//                lod and sigma NaN, significant 0; the counts and moments are still reported when there is an axis
//   output       by core index, each optional: distance (m fp64), lod (m fp64), significant (m uint8), count (m x 2 uint32: A, B),
//                sigma (m x 2 fp64), moments (m x 4 fp64: S1_A S2_A S1_B S2_B -- the test seam); the summary m, valid,
//                significant, the mean of distance, the rms of distance and the max of |distance| over the valid core points
//                (NaN when there is none; a fixed-order fp64 reduction over the core index) and the largest count
//   errors       PLADE_EINVAL: a NULL cloud, params or summary, m = 0 or n = 0, stride < 3, a non-finite coordinate or T, R or L
//                <= 0 or not finite, R * R not finite, reg_error < 0 or not finite, min_points < 2
// The same input gives the same bits on every run, on every context and from the host and the resident entry points.  The counts
// depend on the point sets, the axes, R and L only; the last bits of the sums follow the grid (another bounding box, a permutation).
#pragma once
#include "ctx.h"

namespace plade {

constexpr int M3C2_MIN_POINTS = 2;

}  // namespace plade
