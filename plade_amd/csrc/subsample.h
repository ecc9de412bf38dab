// plade_amd/csrc/subsample.h -- a subset of a cloud's own points at a minimum spacing (k_subsample.hip).
//
// Semantics (include/plade_hip.h; no reference counterpart -- CloudCompare ships it as "Subsample -> Space"
// and takes M3C2's core points from it).  Input: n >= 1 points, rows of `stride` >= 3 floats, x y z first, all coordinates finite.
// d(i, j) = flann_d2(p_i, p_j), the fp32 expression of common.h; r2 = (float)spacing * (float)spacing.
//   parameters   spacing > 0 with r2 finite and >= FLT_MIN (no automatic value); seed (default 0)
//   priority     point i has the key (mix64(mix64(seed) ^ i), i), mix64 of common.h.  Keys compare lexicographically: no two are
//                equal (mix64 is a bijection of the 64-bit words, so the first components already differ)
//   kept set     walk the points in ascending key order; a point is kept if and only if no already-kept point j has d(i, j) < r2
//                -- the strict `<` of the radius filter: of duplicate points exactly one is kept, a pair at exactly d = r2 keeps
//                both.  This is the lexicographically first maximal independent set of the graph "closer than spacing": no two kept
//                points are closer than spacing, every dropped point has a kept point closer than spacing, and the set is unique
//   rounds       the same set as the fixed point of a synchronous iteration.  In round t = 1, 2, ... every undecided point looks at
//                its neighbours with d < r2 and a smaller key AS THEY STOOD AT THE END OF ROUND t - 1: one of them is kept -> the
//                point is dropped; otherwise none of them is undecided -> the point is kept; otherwise it waits.  round[i] = the
//                round in which i was decided, rounds = max round[i].  The undecided point with the smallest key is decided in
//                every round, so rounds <= n; with the hashed keys a handful (2 .. 8 on small sheets and on a sorted scan line,
//                where the index order would take n; 11 .. 12 on a room of 1M points)
//   output       keep: n bytes 0 / 1; kept_index: the kept original indices, ascending; the kept rows in that order, every float
//                of a row copied bit for bit; round (n uint32); the summary n, kept, rounds
//   errors       PLADE_EINVAL: n = 0 (or n >= 2^31: a state word holds round << 1 | kept), stride < 3, a NULL cloud, a non-finite
//                coordinate, a bad spacing.  At least one point is always kept (the one with the smallest key): the resident form
//                has no empty result.  The grid refuses nothing of its own: where the spacing asks for more cells than it holds,
//                its cell grows and the walk stays exact
// The result -- keep, round and rounds -- depends on the points, spacing and seed only: not on the grid's cell, the launch shapes,
// the order of the active lists, or whether the input is a host array or a resident cloud.
#pragma once
#include "ctx.h"
