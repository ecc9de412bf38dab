// plade_amd/csrc/corr_pose.h -- a rigid pose from point correspondences: RANSAC over triples with an edge-length prerejection, an
// exhaustive inlier count per surviving hypothesis and a least-squares refit of the best one (k_corr_pose.hip; Fischler, Bolles 1981;
// the prerejection: Buch, Kraft, Kamarainen, Petersen, Krueger 2013; the refit: Horn 1987).
//
// Semantics (include/plade_hip.h; no reference counterpart).  Input: source points (ns rows) and target points
// (nt rows), fp32 x y z at a stride >= 3 floats, finite; M correspondences as int32 pairs (s, t), 0 <= s < ns, 0 <= t < nt.  S_m and
// Q_m are the two points of correspondence m widened to fp64.  Everything below is fp64 from those values, + - * / sqrt only, no
// contraction, every dot product (a_x b_x + a_y b_y) + a_z b_z and every cross product (a_y b_z - a_z b_y, a_z b_x - a_x b_z,
// a_x b_y - a_y b_x): tests/corr_pose_restate.py reproduces every step up to the refit bit for bit.
//   sample        base = mix64(seed) (common.h); for k = 0, 1, 2: z = mix64(base ^ (4 h + k)), index = ((z >> 32) * M) >> 32; the
//                 triple (a, b, c).  status 1 when two of them are equal; there is no redraw
//   prerejection  for the edges (a, b), (b, c), (c, a): ls = sqrt(|S_i - S_j|^2), lt likewise from Q; status 2 when
//                 fmin(ls, lt) < edge_similarity * fmax(ls, lt) on any edge
//   transform     per side u = p_b - p_a, v = p_c - p_a; e1 = u / sqrt(u.u); w = u x v, e3 = w / sqrt(w.w); e2 = e3 x e1.  status 3
//                 when sqrt(w.w) is 0 or not finite on either side.  R_ij = (e1t_i e1s_j + e2t_i e2s_j) + e3t_i e3s_j;
//                 c_s = ((S_a + S_b) + S_c) / 3.0, c_t likewise; t_i = c_t,i - ((R_i0 c_s0 + R_i1 c_s1) + R_i2 c_s2).  status 0: scored
//   score         count_h = #{ m : d2_m < inlier_dist * inlier_dist }, x'_i = ((R_i0 S_0 + R_i1 S_1) + R_i2 S_2) + t_i, d = x' - Q,
//                 d2 = (d_x d_x + d_y d_y) + d_z d_z.  Integers: independent of any order
//   best          the scored hypothesis with the largest count, ties to the smallest h (the maximum of count << 32 | ~h).
//                 PLADE_EFAIL, T = identity and a failure code when M < 3, nothing is scored or the best count is below min_inliers
//   refinement    at most refine_iterations times, from T = the best hypothesis' and its flags F (d2 < inlier_dist^2 under T):
//                   n, sum S, sum Q and sum d2 over F; s = sum S / n, q = sum Q / n; C_ij = sum over F of (Q - q)_i (S - s)_j --
//                   the terms in correspondence order (0 where the flag is not set), summed in the fixed order of fixed_reduce.h
//                   with workgroups of 256 (tests/fixed_order.py replays them);
//                   R' = the rotation of Horn's unit quaternion: the eigenvector of the largest eigenvalue of the symmetric 4 x 4
//                   matrix N(C), found by CORR_JACOBI_SWEEPS cyclic Jacobi sweeps in the order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3),
//                   normalised; a unit quaternion gives det R' = +1 whatever C is, so a mirrored set cannot produce a reflection;
//                   t' = q - R' s;
//                   T' is accepted iff it is finite and its inlier count is >= T's (the result's `refinements` counts these);
//                   otherwise T stays and the loop stops.  The loop stops as well after an accepted T' whose flags equal T's
//   output        T16 = fp32 of the fp64 T; inliers, rmse = sqrt(sum d2 / inliers) and fitness = inliers / M under the final T
// The same input gives the same bits on every run, on every context and from the host and the resident entry points.
#pragma once
#include "ctx.h"

namespace plade {

constexpr int CORR_SUM_TPB = 256;       // the workgroup of the refinement's sums: part of the semantics (the order of the sums)
constexpr int CORR_JACOBI_SWEEPS = 12;  // a 4 x 4 symmetric matrix is diagonal to the last bit after 6 or 7; fixed, so no data-dependent exit
constexpr int CORR_SCORE_TILE = 64;     // correspondences per LDS tile of k_hyp_score
constexpr int CORR_SCORE_CHUNK = 256;   // the smallest number of correspondences per workgroup (blockIdx.y)
constexpr int CORR_MOMENTS = 17;        // n, s (3), q (3), C (9), sum d2: plade_corr_pose_moments

}  // namespace plade
