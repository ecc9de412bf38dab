// plade_amd/csrc/fpfh.h -- Fast Point Feature Histograms of a cloud with normals and the nearest-neighbour match of two sets of
// them in feature space (k_fpfh.hip; Rusu, Blodow, Beetz 2009).
//
// Semantics (include/plade_hip.h; no reference counterpart).  Input: n >= 1 rows x y z nx ny nz in fp32 with
// finite coordinates (the normals need not be unit and may be non-finite).  radius r > 0 and finite, r2 = (float)r * (float)r finite
// and >= FLT_MIN (the rule of smooth.h; no default), min_pairs >= 1.
//   neighbours   d(i, j) = flann_d2(p_i, p_j), the fp32 expression of common.h; N_i = { j : 0 < d(i, j) < r2 } (the strict `<` of
//                sections 10 to 17; coincident points, i itself included, are no neighbours)
//   axis         len2 = (nx nx + ny ny) + nz nz in fp64; n^ = double(n) / sqrt(len2).  len2 zero or not finite: no axis -- the point
//                has no descriptor and is nobody's neighbour
//   pair (i, j)  j in N_i, both with an axis; fp64 from the fp32 inputs, no contraction, every dot product (a_x b_x + a_y b_y) + a_z b_z:
//                q = double(p_j) - double(p_i); l = sqrt(q.q); e = q / l; a_i = n^_i.e; a_j = n^_j.e;
//                (n1, n2, dp) = fabs(a_i) < fabs(a_j) ? (n^_j, n^_i, -e) : (n^_i, n^_j, e);
//                f3 = n1.dp; v = dp x n1; |v| = sqrt(v.v): 0 -> the pair is not counted; v /= |v|; w = n1 x v; f2 = v.n2;
//                f1 = atan2(w.n2, n1.n2);
//                b1 = clamp((int)floor(11.0 * ((f1 + pi) / (2.0 * pi))), 0, 10), b2 = clamp((int)floor(11.0 * ((f2 + 1.0) * 0.5)), 0, 10),
//                b3 from f3 as b2 (pi = M_PI; a NaN maps to bin 0); H_i[b1], H_i[11 + b2], H_i[22 + b3] each grow by one
//   SPFH         H_i (33 x uint32) and c_i, the number of counted pairs: exact integers, independent of any order.  i is
//                described iff it has an axis and c_i >= min_pairs
//   FPFH         for a described i over the described j in N_i: w_ij = (double)r2 / (double)d(i, j); W_i = sum w_ij;
//                R_i[b] = sum w_ij * (double(H_j[b]) / double(c_j)) -- fp64 sums in the order of the grid walk, no atomics.
//                W_i > 0: F_i[b] = fp32(50.0 * (double(H_i[b]) / double(c_i) + R_i[b] / W_i));
//                W_i = 0: F_i[b] = fp32((100.0 * double(H_i[b])) / double(c_i)).  A point that is not described: 33 NaNs
//   output       by original index, each optional: desc (n x 33 fp32), described (n uint8), pairs (n uint32: c_i), spfh (n x 33
//                uint32) and raw (n x 34 fp64: W_i, R_i; zeros where not described) -- the last two are test seams; the summary: n,
//                described, the largest c_i, the mean c_i over the described points (an exact integer sum, one division; 0 when
//                nothing is described)
//   errors       PLADE_EINVAL: a NULL cloud or summary, n = 0, a non-finite coordinate, a bad radius, min_pairs < 1
// H, c and `described` depend on the point set and r only (permuted exactly under a permutation of the rows); the last bits of raw
// follow the grid.  The same input gives the same bits on every run, on every context and from the host and the resident entry points.
//
// Match.  Source descriptors ns x 33 fp32, target descriptors nt x 33, ns, nt >= 1.  A row is valid iff its first value is not NaN.
//   distance     delta(s, t) = sum over b = 0 .. 32, in that order, of (S_b - T_b) * (S_b - T_b): fp32, no contraction.  A target
//                whose delta is NaN (a valid row with a NaN further in) is passed over
//   neighbours   per valid source row the two smallest keys (delta, t) over the valid targets (make_key of grid_walk.h: ties go to the
//                smaller index): nn[s] (int32, -1: none), d2[s] (2 floats; NaN where there is none)
//   mutual       (default on) the same search target -> source gives back[t]; s is kept iff back[nn[s]] == s
//   max_ratio    (default 0 = off) otherwise s is kept iff it has no second neighbour or d2[s][0] < (ratio * ratio) * d2[s][1] in fp32
//   output       nn, d2, back (nt int32; computed when wanted or mutual) and the kept (s, nn[s]) ascending in s with the exact
//                n_corr; PLADE_ECAP when the list's capacity is smaller (the first `cap` pairs are written)
//   errors       PLADE_EINVAL: a NULL table, params' max_ratio negative or not finite, ns = 0 or nt = 0, n_corr NULL
// Integers and fp32 bit patterns only: the same on every run and for every split of the targets over workgroups.
#pragma once
#include "ctx.h"

namespace plade {

constexpr int FPFH_BINS = 11, FPFH_DIM = 33;
constexpr int FEAT_TILE = 64;     // targets per LDS tile of k_feat_match
constexpr int FEAT_CHUNK = 512;   // the smallest number of targets per workgroup (blockIdx.y)

}  // namespace plade

// a resident descriptor table: n x 33 fp32, rows of NaN where a point is not described
struct plade_features {
    plade::DBuf<float> desc;
    uint32_t n = 0;
};

namespace plade {
// The steps plade_register_features chains (k_corr_pose.hip), device to device: the descriptors of n device rows x y z nx ny nz with
// a known bounding box into `out` (grow-only; the bits of plade_cloud_fpfh), and the match of two such tables -- returns the device
// list of the kept (s, t) pairs (valid until the context's next match) and their number (the bits of plade_match_features).
void fpfh_table_dev(plade_ctx *ctx, const float *d_rows, uint32_t n, const float bbmin[3], const float bbmax[3],
                    const plade_fpfh_params &p, plade_features &out, plade_fpfh_summary *summary);
const int32_t *feature_corr_dev(plade_ctx *ctx, const plade_features &src, const plade_features &tgt, const plade_feature_match_params &p,
                                uint64_t *n_corr);
}  // namespace plade
