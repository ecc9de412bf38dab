// plade_amd/csrc/orient.h -- one side of the surface for every normal of a cloud, without a viewpoint per point (k_orient.hip).
//
// Semantics (include/plade_hip.h; no reference counterpart -- Open3D ships it as
// orient_normals_consistent_tangent_plane, CloudCompare as its MST orientation; both follow Hoppe et al. 1992).  Input: n >= 1 rows
// x y z nx ny nz, n < 2^31, all coordinates finite.  d(i, j) = flann_d2(p_i, p_j), the fp32 expression of common.h;
// r2 = (float)radius * (float)radius, finite and >= FLT_MIN (radius_sq32 of cli_switches.h).
//   valid point  its three normal components are finite and each |component| <= 1e18f: every fp32 expression below is then finite.
//                Every other point is left bit for bit as it is, gets flip = 0 and label = -1 and is counted in `unoriented`
//   graph        the vertices are the valid points; i ~ j when i != j and d(i, j) < r2 -- the strict `<` and the 27-cell block of
//                section 14: duplicates are joined, a pair at exactly d = r2 is not
//   edge weight  dot32(i, j) = (nx_i*nx_j + ny_i*ny_j) + nz_i*nz_j in fp32 without contraction, symmetric in i and j;
//                a = fabsf(dot32); key32 = 0x7F800000u - bits(a): the smaller key is the flatter pair, Hoppe's 1 - |n_i . n_j| as a
//                total order on the bits (a = 1: 0x40000000; a = 0: 0x7F800000).  Edges are ordered by (key32, min(i,j), max(i,j)):
//                no two are equal.  On synthetic planes almost every key ties: the index tie-break is part of the definition
//   tree         the minimum spanning forest of the graph under that order: unique
//   flips        s_ij = 1 when dot32(i, j) < 0.0f, else 0; along every forest edge flip_i ^ flip_j = s_ij.  That fixes the flips of
//                a component up to one bit; the component's anchor fixes the bit
//   anchor VOTE  (mode PLADE_ORIENT_VOTE = 0, the default; viewpoint v, default the origin).  Anchored provisionally at flip = 0 on
//                the component's valid point of smallest index, t_i = ((vx - px) * nx + (vy - py) * ny) + (vz - pz) * nz in fp64 from
//                the fp32 inputs -- the flip test of normals.h in the arithmetic of k_normals.hip -- on the provisionally flipped
//                normal.  towards = #{t_i > 0}, away = #{t_i < 0}: integers, the same in any order.  away > towards toggles the
//                whole component; a tie toggles nothing
//   anchor EXTREME (mode PLADE_ORIENT_EXTREME = 1; direction `dir`, default +z, not zero).  e_i = ((double)x*dx + (double)y*dy) +
//                (double)z*dz; the anchor is the component's valid point with the largest (e_i, then the smaller index); with g the
//                same fp64 form on its normal, the anchor is flipped when g < 0 (it ends with g >= 0; g == 0 keeps it as it is)
//   inward = 1   inverts the decision of either mode (the toggle of VOTE, the anchor's flip of EXTREME): a room scanned from the
//                inside wants this with EXTREME
//   output       the n rows: a flipped point's three normal floats have their sign bit toggled, every other float is copied bit for
//                bit; flip (n bytes); label (n int32, -1 for invalid points; ids ascending in the order of each component's smallest
//                index, as section 14); the summary n, unoriented, components, flipped, tree_edges (= valid points - components),
//                tree_key_sum (the uint64 sum of key32 over the forest's edges: it pins minimality) and rounds
//   errors       PLADE_EINVAL: n = 0 (or n >= 2^31: a state word holds root << 1 | parity), a NULL cloud, a non-finite coordinate,
//                a bad radius, a non-finite viewpoint or direction, direction = 0, a mode other than 0 or 1, inward not 0 or 1.  A
//                cloud without any valid point is PLADE_OK with everything copied.  The grid refuses nothing of its own: where the
//                radius asks for more cells than it holds, its cell grows and the walk stays exact
// Two parallel sheets of opposite orientation that are closer than `radius` are joined by edges with |dot| = 1, the flattest there
// are, and end on the SAME side.  This is inherent to the method: `radius` must stay below the thinnest wall of the scene.
// The result -- everything but `rounds` -- depends on the rows and the parameters only: not on the grid's cell, the launch shapes,
// the order of the active lists, or whether the input is a host array or a resident cloud.
#pragma once
#include "ctx.h"
