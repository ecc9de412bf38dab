// plade_amd/csrc/distances.h -- cloud-to-cloud distances and registration fitness (k_distances.hip).
//
// Semantics (include/plade_hip.h; no reference counterpart).  Target: n_t points x y z nx ny nz (normals
// may be NaN); source: n_s points x y z, `stride` floats apart; T: the row-major 4 x 4 source -> target transform in fp32
// (NULL: the identity); d = max_dist, fp32, finite and > 0.
//   transform   p'_i = fp32(R) s_i + fp32(t), each row ((r0 x + r1 y) + r2 z) + t in fp32 (-ffp-contract=off): ICP's match rule
//   nearest     j_i = the argmin over ALL target points of the key (flann_d2(p'_i, q_j), j) -- ties go to the smaller index
//   corresp.    i has one when flann_d2(p'_i, q_j_i) < (float)d * (float)d.  An exact set: independent of the grid's cell size,
//               the source order and the launch shapes
//   per point   idx[i] = j_i or -1; d2[i] = that fp32 flann_d2 or +inf; plane[i] = fp32 of
//               r_i = (n0 (p0 - q0) + n1 (p1 - q1)) + n2 (p2 - q2) with p = double(T) double(s_i) in fp64 (the same row order),
//               NaN without a correspondence or when n_j is not finite
//   summary     n = n_s, count, fitness = count / n, rmse = sqrt(sum d2 / count), mean = sum sqrt(d2) / count, max = max sqrt(d2),
//               plane_count = the correspondences with a finite n_j, plane_rmse = sqrt(sum r^2 / plane_count); the sums are fp64
//               over double(d2) and r in a fixed order of the original index i (no fp64 atomics): bit-identical from run to run,
//               with or without per-point outputs, for host or resident clouds.  count = 0: rmse, mean and max are NaN (fitness
//               0); plane_count = 0: plane_rmse is NaN
//   errors      PLADE_EINVAL: NULL clouds or summary, n = 0, non-finite coordinates or T, d <= 0 or not finite, stride < 3
#pragma once
#include "ctx.h"
