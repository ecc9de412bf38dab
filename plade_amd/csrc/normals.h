// plade_amd/csrc/normals.h -- k-nearest-neighbour PCA normals of an unoriented xyz cloud (k_normals.hip).
//
// Semantics (DESIGN.md section "Normal estimation"; no reference counterpart -- the reference requires oriented normals in its
// input and its vendored PCL has no `features` module):
//   neighbours  N_k(i) = the k_eff = min(k, n) points j, i itself included, with the smallest d(i, j) = flann_d2(p_i, p_j) (the
//               fp32 expression of common.h), ties broken by the smaller original index j, listed in ascending (d, j) order;
//   PCA         fp64 on q_j = double(p_j) - double(p_i), accumulated in the listed order: mu = sum q_j / m,
//               C = sum (q_j - mu)(q_j - mu)^T / m; the normal is the unit eigenvector of the smallest eigenvalue l0 (written as
//               fp32), the curvature l0 / (l0 + l1 + l2);
//   orientation n is flipped when (v - p_i) . n < 0 (PCL's flipNormalTowardsViewpoint), v = the viewpoint;
//   degenerate  k_eff < 3 or C == 0 exactly (all neighbours coincide): normal and curvature NaN.
// The result depends only on the point set, k and v -- not on the grid's cell size, the launch shape or which of the two search
// kernels finished a point.
#pragma once
#include "ctx.h"

namespace plade {

constexpr int NORMALS_K_MIN = 3, NORMALS_K_MAX = 64;

struct NormalsWork;

// d_xyz: n points of `stride` floats on the device, finite (bbmin / bbmax: their bounding box, bbox_host).  Writes n x 6 floats
// (x y z nx ny nz, the input coordinates copied bit for bit) to d_out; d_curv (n floats) and d_nbr (n x k int32, -1 behind the
// k_eff neighbours when n < k) may be nullptr.  Queued on ctx->stream; the caller syncs.  Records the grid build and the
// search + PCA with HIP events; normals_stats() reads them after the sync.
void estimate_normals_dev(plade_ctx *ctx, NormalsWork &W, const float *d_xyz, uint32_t n, uint32_t stride, const float bbmin[3],
                          const float bbmax[3], int k, const float view[3], float *d_out, float *d_curv, int32_t *d_nbr);
// after the caller's sync: stats "normals_grid_s" (grid builds, including the host waits of the cell adaptation), "normals_search_s",
// "normals_grid_builds", "normals_ring_queries" and the grid of the last build (grid_stats of grid_walk.h)
void normals_stats(plade_ctx *ctx, NormalsWork &W);

// argument checks of the entry points (PLADE_EINVAL): n >= 1, stride >= 3, k in [3, 64], a finite viewpoint (bbox_host checks
// the coordinates)
void normals_check_args(uint32_t n, uint32_t stride, int k, const float *view);

}  // namespace plade
