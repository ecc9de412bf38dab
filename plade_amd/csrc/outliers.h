// plade_amd/csrc/outliers.h -- statistical and radius outlier removal of a point cloud (k_outliers.hip).
//
// Semantics (include/plade_hip.h; no reference counterpart -- the reference's vendored PCL has no `filters`
// module).  Input: n points, rows of `stride` >= 3 floats, x y z first, all coordinates finite.  d(i, j) = flann_d2(p_i, p_j), the
// fp32 expression of common.h.
//   statistical  k in [1, 64], alpha >= 0 and finite
//     neighbours the k_eff = min(k, n - 1) points j != i with the smallest keys (d(i, j), j).  The point itself is left out by its
//                index, not by its distance: a duplicate of i is a neighbour at distance 0.  An exact set
//     m_i        (sum of sqrt(double(d(i, j))) over the neighbours in ascending key order) / k_eff in fp64; n = 1: m_0 = 0
//     mu, sigma  mu = sum m_i / n; sigma = sqrt(sum (m_i - mu)^2 / (n - 1)) in a second pass (n = 1: 0); fp64, summed in a fixed
//                order of the original index (no fp64 atomics): the same bits on every run
//     keep       t = mu + alpha * sigma in fp64; point i is kept when m_i <= t
//   radius       r > 0 and finite, min_neighbours >= 1
//     c_i        the number of j != i with d(i, j) < (float)r * (float)r (the `<` of sections 10 and 11); exact integers
//     keep       point i is kept when c_i >= min_neighbours
//   output       keep: n bytes 0 / 1; kept_index: the kept original indices, ascending; the filtered cloud: the kept rows in that
//                order, every float of a row copied bit for bit; per point m (fp64) or c (uint32); the summary n, kept, mu, sigma,
//                threshold (NaN in radius mode)
//   errors       PLADE_EINVAL: n = 0, stride < 3, a non-finite coordinate, k outside [1, 64], alpha negative or not finite,
//                r <= 0 or not finite, min_neighbours < 1.  A filter that keeps nothing is PLADE_OK with kept = 0; a resident
//                result of 0 points is PLADE_EFAIL (plade_cloud has no empty form)
// The result depends on the point set and the parameters only: not on the grid's cell, the launch shape, or which of the two
// search kernels finished a point.
#pragma once
#include "ctx.h"

namespace plade {

constexpr int OUTLIERS_K_MIN = 1, OUTLIERS_K_MAX = 64;

}  // namespace plade
