// plade_amd/csrc/keypoints.h -- Intrinsic Shape Signatures keypoints of a cloud (k_keypoints.hip; Zhong 2009, as PCL's
// ISSKeypoint3D defines the scatter) and the row gather of a descriptor table that puts them in front of the feature match.
//
// Semantics (include/plade_hip.h; no reference counterpart).  Input: n >= 1 rows of `stride` >= 3 floats, x y z
// first, all finite; normals are not used.  salient_radius rs > 0 and finite, (float)rs * (float)rs finite and >= FLT_MIN (the rule of
// smooth.h; no default); non_max_radius rn: 0 means rs, otherwise the same rule; gamma21, gamma32 finite and in (0, 1] (default
// 0.975); min_neighbours >= 1 (default 5).  d(i, j) = flann_d2(p_i, p_j), the fp32 expression of common.h; rs2, rn2 = the fp32 squares.
//   scatter      N_i = { j : d(i, j) < rs2 } (the strict `<` of sections 10 to 18; the point itself belongs to it), c_i = |N_i|, exact.
//                q_j = double(p_j) - double(p_i); M_i = sum q_a q_b: six fp64 sums xx xy xz yy yz zz, each added term by term in the
//                order the walk meets the neighbours: the nine runs of for_block27 (z outer, y inner), ascending sorted position
//                within a run.  No atomics.  C_i = M_i / double(c_i) entry by entry: the scatter about the QUERY POINT, not about the
//                centroid (neighbours that share a neighbour set would share a centroid scatter up to rounding, and the suppression
//                below would be a coin toss between them)
//   eigenvalues  l1 >= l2 >= l3 of C_i: sym3_eigenvalues of pca_eig.h, the trigonometric closed form of pca_eig
//   salient      c_i >= 3 && l1 > 0 && l2 < gamma21 * l1 && l3 < gamma32 * l2 && l3 > 1e-9 * l1: products and comparisons in fp64, no
//                division (collinear and coplanar neighbourhoods are flat by arithmetic, not by the sign of a rounding error).
//                saliency_i = l3 when salient, else 0
//   suppression  B_i = { j : d(i, j) < rn2 }, i included; m_i = |B_i|.  i is a keypoint iff it is salient, m_i - 1 >= min_neighbours and
//                no j in B_i, j != i, has saliency_j > saliency_i, or saliency_j == saliency_i with j < i: an exact function of the
//                points and the saliency array
//   output       by original index, each optional: keypoint (n uint8), the ascending index list with its exact length (PLADE_ECAP
//                with the first `cap` entries when the capacity is smaller), saliency (n fp64), eigenvalues (n x 3 fp64, descending),
//                count (n uint32: c_i), nms_count (n uint32: m_i) and the test seam scatter (n x 6 fp64: M_i).  The summary: n,
//                salient, keypoints, the largest c_i
//   errors       PLADE_EINVAL: NULL arguments, n = 0, stride < 3, a non-finite coordinate, a bad radius or gamma, min_neighbours < 1
// c, m and -- given the saliencies -- the flags depend on the point set and the radii only; the last bits of M follow the grid.  The
// same input gives the same bits on every run, on every context and from the host and the resident entry points.
//
// One grid serves both walks: its cell is radius_cell(max(rs, rn)), each walk filters the same 27-cell block by its own radius.
#pragma once
#include "fpfh.h"

namespace plade {

// The steps plade_register_keypoints chains (k_corr_pose.hip), device to device.
// The detector on n device rows (`stride` floats apart, x y z first) with a known bounding box: returns the device list of the
// keypoints' original indices, ascending (valid until the context's next detection), its length in *n_keypoints, fills the summary
// (the bits of plade_cloud_keypoints_iss).
const uint32_t *iss_list_dev(plade_ctx *ctx, const float *d_rows, uint32_t n, uint32_t stride, const float bbmin[3], const float bbmax[3],
                             const plade_iss_params &p, plade_iss_summary *summary, uint32_t *n_keypoints);
// out row o = in row d_index[o], o < k (k >= 1; the indices are below in.n): the bits of plade_features_select
void features_select_dev(plade_ctx *ctx, const plade_features &in, const uint32_t *d_index, uint32_t k, plade_features &out);
// the pairs (s, t) of a device list with s replaced by d_index[s]: returns a device list of m pairs (valid until the next call)
const int32_t *corr_map_source_dev(plade_ctx *ctx, const int32_t *d_corr, uint64_t m, const uint32_t *d_index);

}  // namespace plade
