// plade_amd/csrc/icp.h -- point-to-plane ICP refinement of a registration (k_icp.hip).
//
// Semantics (include/plade_hip.h; no reference counterpart -- the reference returns the Umeyama fit of its
// matched descriptors).  D = the diagonal of the target's bounding box; a parameter that is 0 takes the value in brackets.
//   sample     S = the VoxelGrid downsample (voxel.h, plade_voxel_downsample) of the source's x y z with leaf source_leaf [0.005 D]
//   iterate    T_k in fp64, T_0 = T_in; the stage distance d starts at max_dist [0.025 D]
//   centre     s-bar = the fp64 mean of S (summed once in a fixed order); c_k = T_k s-bar in fp64, rows as below
//   match      p' = fp32(R) s + fp32(t), each row ((r0 x + r1 y) + r2 z) + t in fp32 (-ffp-contract=off); j = the argmin over all
//              target points of the key (flann_d2(p', q_j), j); s has a correspondence when flann_d2 < (float)d * (float)d and
//              the normal n_j is finite.  An exact set: a numpy float32 restatement reproduces it bit for bit, whatever the grid's
//              cell size or the launch shape.
//   linearise  fp64 over the correspondences, with p = T_k double(s) (rows ((r0 x + r1 y) + r2 z) + t), n = double(n_j),
//              q = double(q_j): r = (n0 (p0 - q0) + n1 (p1 - q1)) + n2 (p2 - q2), J = [(p - c_k) x n, n] (about the
//              centre: the rotation columns do not grow with the distance of the scene from the origin); moments = the 21 values of
//              J^T J (row-major upper triangle), the 6 of J^T r, sum r^2 and the count.  Fixed summation order (lanes, waves,
//              workgroups, then the partials in order): bit-identical from run to run, no fp64 atomics.
//   solve      J^T J x = -J^T r by fp64 Cholesky; pivot j <= 1e-12 A[j][j] (its own diagonal entry; an exactly zero column
//              counts) -> degenerate.  Unchanged when a column is rescaled: the same answer in mm or km.
//   update     T_{k+1} = [R | (c_k - R c_k) + x3..5] T_k in fp64, R = Rodrigues(x0..2): a rotation about c_k, and x3..5 is the
//              motion of the centre
//   schedule   A = the target's max |coordinate|; eps_t = max(eps_translation [1e-6 D], 4 2^-23 A), eps_r = max(eps_rotation
//              [1e-6], 4 2^-23 A / D) (the floor: one fp32 ulp of the coordinates, below which steps cannot shrink; it applies to
//              given values too).  Converged stage: |x0..2| < eps_r and |x3..5| < eps_t; then d = max(min_dist, d / 2)
//              while d > min_dist [0.0025 D], else stop (converged); at most max_iterations [60] updates (converged = 0, PLADE_OK)
//   failure    fewer than min_correspondences [100] correspondences, or degenerate: PLADE_EFAIL, T_out = T_in
#pragma once
#include "ctx.h"

namespace plade {

constexpr int ICP_MOMENTS = 29;      // 21 J^T J, 6 J^T r, sum r^2, count
constexpr int ICP_MAX_STAGES = 16;

}  // namespace plade
