// plade_amd/csrc/gicp.h -- plane-to-plane (generalized) ICP refinement of a registration (k_gicp.hip).
//
// Semantics (include/plade_hip.h; the library's own -- the reference refines nothing).  Segal's Generalized ICP
// with the covariances built from the normals, C = I - (1 - eps) n n^T (variance eps along the normal, 1 in the tangent plane): every
// correspondence is weighted by M = (C_t + R C_s R^T)^-1.  D, A, the automatic values, the stage distances, the tolerances with
// their fp32 floors and the limit of 16 stages are those of icp.h, word for word.
//   input      target n_t rows x y z nx ny nz; source n_s rows x y z nx ny nz; T_in source -> target, row-major 4 x 4 fp32
//   epsilon    0 < eps <= 1, finite; 0 selects 1e-3.  eps = 1: M = I / 2 exactly, point-to-point ICP
//   sample     S = the source alone, voxel-fused under merge.h's rules at leaf source_leaf [0.005 D] (plade_merge_clouds_dev of one
//              cloud under the identity): fp64 mean position, normalised fp64 sum of the finite normals, ascending voxel order.
//              Every sample point carries a normal m (or three NaNs).  Not the xyz-only sample of icp.h
//   centre     s-bar = the fp64 mean of S, summed once in the fixed order; c_k = T_k s-bar in fp64 (icp.h)
//   match      p' in fp32 and j = the argmin over all target points of the key (flann_d2(p', q_j), j), as icp.h.  s has a
//              correspondence when flann_d2 < (float)d * (float)d, n_j is finite with ln2 = (n0 n0 + n1 n1) + n2 n2 > 0 in fp64,
//              and m is finite with lm2 = (m0 m0 + m1 m1) + m2 m2 > 0 in fp64.  No second choice is looked for
//   linearise  fp64, every term a fixed expression of + - * / sqrt (-ffp-contract=off); T = T_k, rows T[4 r + c]:
//                p_r  = ((T[4r] X + T[4r+1] Y) + T[4r+2] Z) + T[4r+3]       (X Y Z = double(s))
//                e_r  = p_r - double(q_r),   u_r = p_r - c_r
//                nh_r = n_r / sqrt(ln2)
//                a_r  = (T[4r] m0 + T[4r+1] m1) + T[4r+2] m2,   ah_r = a_r / sqrt((a0 a0 + a1 a1) + a2 a2)
//                k    = 1 - eps
//                S_ij = (dd - k (nh_i nh_j)) - k (ah_i ah_j),  dd = 2 on the diagonal, 0 off it       (Sigma, six entries)
//                C00 = S11 S22 - S12 S12   C01 = S02 S12 - S01 S22   C02 = S01 S12 - S02 S11          (cofactors)
//                C11 = S00 S22 - S02 S02   C12 = S01 S02 - S00 S12   C22 = S00 S11 - S01 S01
//                det = (S00 C00 + S01 C01) + S02 C02,   M_ij = C_ij / det
//                w_r  = (M_r0 e0 + M_r1 e1) + M_r2 e2                                                 (M e)
//                G_r0 = M_r2 u1 - M_r1 u2,  G_r1 = M_r0 u2 - M_r2 u0,  G_r2 = M_r1 u0 - M_r0 u1,  G_r(3+c) = M_rc   (M J, 3 x 6)
//                with J = [-[u]x | I] (the rotation acts about c_k) and, for a 3-vector v,
//                  K0(v) = v2 u1 - v1 u2,  K1(v) = v0 u2 - v2 u0,  K2(v) = v1 u0 - v0 u1                  (the rows of -[u]x^T)
//                H_ab = Ka(G_0b, G_1b, G_2b) for a < 3, G_(a-3)b for a >= 3      (J^T M J, b >= a: 21 values, row-major)
//                g_a  = Ka(w) for a < 3, w_(a-3) for a >= 3                       (J^T M e, 6 values)
//                cost = (e0 w0 + e1 w1) + e2 w2,   ee = (e0 e0 + e1 e1) + e2 e2
//              moments = H (21), g (6), sum cost, sum ee, count: GICP_MOMENTS = 30.  numpy float64 reproduces every term bit for
//              bit; only the order of the summation differs.  The eigenvalues of Sigma lie in [2 eps, 2]: det >= 8 eps^2 > 0
//   summation  icp.h's: lanes by butterfly, the waves in order, one partial per workgroup, the partials by one wavefront.  No fp64
//              atomics; the same bits on every run
//   solve, update, schedule, failure   icp.h's, on the 21 + 6 moments.  The isotropic part of M makes a single plane or a crease
//              non-degenerate here (an in-plane pull at relative weight eps is inherent to GICP); PLADE_ICP_DEGENERATE remains for
//              the truly singular cases, e.g. a sample on one straight line through c_k
//   output     T_out = fp32 of the fp64 iterate, T_in on failure; rmse = sqrt(sum ee / count) (point-to-point), cost = sum cost /
//              count, fitness = count / |S|, all of the last linearisation
#pragma once
#include "ctx.h"

namespace plade {

constexpr int GICP_MOMENTS = 30;     // 21 J^T M J, 6 J^T M e, sum e^T M e, sum |e|^2, count

}  // namespace plade
