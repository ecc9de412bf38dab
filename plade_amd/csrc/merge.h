// plade_amd/csrc/merge.h -- merge registered clouds into one voxel-fused cloud (k_merge.hip).
//
// Semantics (include/plade_hip.h; the library's own -- no reference counterpart).
//   input      k clouds, 1 <= k <= 16; cloud c has n_c >= 1 rows x y z nx ny nz with finite coordinates (normals may be NaN) and a
//              row-major fp32 4 x 4 T_c into the output frame (a NULL table or entry: the identity, through the same arithmetic);
//              leaf >= 0 (fp32)
//   transform  p' = ((r0 x + r1 y) + r2 z) + t and n' = (r0 nx + r1 ny) + r2 nz, row by row in fp32 (the match rule of sections 10
//              and 11).  n' gets no translation and is not renormalised; a normal with a non-finite component stays non-finite
//   leaf = 0   the output is the transformed concatenation in (cloud, index) order; count = 1 and mask = 1 << c for every row
//   leaf > 0   inv = 1.f / leaf; the voxel of p' is floor(p' * inv) per axis in fp32 minus floor(min * inv) of the bounding box of
//              all p' (the key of plade_voxel_downsample); one output row per occupied voxel, in ascending (k, j, i)
//     position fp64 sum of double(p') over the voxel's points, one after the other in ascending (cloud, index) order; divided by
//              the count in fp64 and rounded to fp32
//     normal   s = the fp64 sum of double(n'), same order, over the points whose n' is finite; q = (sx sx + sy sy) + sz sz; three
//              NaNs when there is no such point or q == 0, else fp32(s / sqrt(q)).  A plain sum (PCL's normal accumulator):
//              opposite normals cancel
//     count    uint32 points of the voxel; mask: uint32, bit c set when cloud c contributed
//   summary    n_in = sum n_c, n_out = output rows, n_shared = rows whose mask has two or more bits, max_count
//   errors     PLADE_EINVAL: k outside [1, 16], a NULL cloud, n_c = 0, a non-finite coordinate or T, leaf negative or not finite;
//              PLADE_ELIMIT: more than 2^18 leaves along an axis, sum n_c >= 2^31.  The context stays usable
// The result depends on the inputs only -- not on launch shapes, not on host or resident clouds -- and is the same bits on every
// run: the sums are taken by one lane per voxel in the order a stable sort leaves the points in; there are no floating-point
// atomics.
#pragma once
#include "ctx.h"

namespace plade {

constexpr int MERGE_MAX_CLOUDS = 16;

struct MergeWork;

// The voxel fuse of ONE device cloud (n x 6 rows) under the identity at leaf > 0 -- plade_merge_clouds_dev of one cloud -- for the
// stages that sample a cloud with its normals (gicp.h): returns the number of fused rows and leaves them, n_out x 6, behind *d_out in
// the context's MergeWork, where they stay until the next merge on the context.  Waits for the stream.  What the merge refuses (a
// non-finite coordinate, more than 2^18 leaves along an axis, a leaf that is 0 in fp32) is reported under the name `who`.
uint32_t merge_fuse_one(plade_ctx *ctx, const float *d_rows, uint32_t n, float leaf, const float **d_out, const char *who);

}  // namespace plade
