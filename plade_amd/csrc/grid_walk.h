// plade_amd/csrc/grid_walk.h -- the pieces every search of TargetGrid's dense row index shares (k_normals, k_outliers,
// k_distances, k_icp): the (d, j) keys, the cell assignment, the 27-cell block, the growing blocks of the ring kernels, the
// register and wave top-K lists and the hand-over from a lane kernel to its ring kernel.  Each kernel keeps its own policy (what
// a candidate is, when a query is finished, what is stored); only the walk is here, once.
//
// The index (overlap.h): the points sorted by their linear cell id in a grid padded by two cells on every side, x fastest, float4
// with the original index in w; row_start[L] = number of points in cells < L.  Cells x0 .. x1 of one (y, z) row are the contiguous
// run [row_start[r + x0], row_start[r + x1 + 1]) of `sorted`, r = row_base(g, y, z) + 2; the padding makes every row next to a
// cell of the grid valid.
#pragma once
#include "overlap.h"

namespace plade {

// the dense row index and its cell assignment (k_cell_ids), as the kernels take it
struct GridView {
    const float4 *sorted;            // the points in cell order: x y z, bit-cast original index
    const uint32_t *row_start;
    float mnx, mny, mnz, inv;
    int dx, dy, dz, DX, DY;          // cells, padded row pitch
    double mn[3], cell;              // the same origin and 1 / inv in fp64 (block_reach)
};

// who: the entry point a refusal names
inline void require_dense(const TargetGrid &G, const char *who) {
    PLADE_REQUIRE(G.dense, PLADE_EINVAL, std::string(who) + ": needs the dense row index (unset PLADE_OVERLAP_INDEX_COMPACT)");
}
inline GridView view_of(const TargetGrid &G, const char *who) {
    require_dense(G, who);
    GridView g;
    g.sorted = G.sorted.p; g.row_start = G.row_start.p;
    g.mnx = G.gp.mnx; g.mny = G.gp.mny; g.mnz = G.gp.mnz; g.inv = G.gp.inv;
    g.dx = G.gp.dx; g.dy = G.gp.dy; g.dz = G.gp.dz; g.DX = G.DX; g.DY = G.DY;
    g.mn[0] = G.gp.mnx; g.mn[1] = G.gp.mny; g.mn[2] = G.gp.mnz;
    g.cell = 1.0 / (double)G.gp.inv;
    return g;
}

// The grid a tool met, for its stats: "<tool>_grid_dx", "_dy", "_dz" (cells) and "_grid_cell" (1 / inv: build() may have enlarged
// the cell that was asked for).  Called where the tool publishes its other stats, with the grid it built
inline void grid_stats(plade_ctx *ctx, const char *tool, const TargetGrid &G) {
    const std::string t(tool);
    ctx->stats.set(t + "_grid_dx", G.gp.dx);
    ctx->stats.set(t + "_grid_dy", G.gp.dy);
    ctx->stats.set(t + "_grid_dz", G.gp.dz);
    ctx->stats.set(t + "_grid_cell", 1.0 / (double)G.gp.inv);
}

// the largest |coordinate| of a bounding box
inline double amax_of(const float mn[3], const float mx[3]) {
    double a = 0.0;
    for (int t = 0; t < 3; ++t) a = std::max(a, std::max(std::fabs((double)mn[t]), std::fabs((double)mx[t])));
    return a;
}

// what block_reach gives away for the fp32 cell assignment: (x - mn) * inv is off by a few ulps of the coordinates (bbmin / bbmax:
// the bounding box of the grid's points); 1 % of a cell on top
inline double grid_margin(const GridView &g, const float bbmin[3], const float bbmax[3]) {
    return 0.01 * g.cell + 1e-6 * amax_of(bbmin, bbmax);
}

// The cell of a search with radius r over points in the box [mn, mx]: at this cell the 27-cell block around a point holds every
// point closer than r, exactly (the rule of DESIGN.md section 10).  A point at distance r lies less than one cell away along
// every axis only if cell > r by more than the fp32 cell assignment can be off: (x - mn) * inv carries a few ulps of the
// coordinates, 2^-23 max|coordinate| each -- 4e-6 max|coordinate| covers them with room to spare -- and `factor` adds a share of
// r itself (3 %; the ICP's stage grids take 1 %, build() adds 0.1 % and may enlarge the cell, never shrink it).  The bound 1e37
// keeps 1 / cell a normal fp32 number; it binds for k_m3c2 alone, whose radius is checked in fp64.  The other radius tools
// require (float)r * (float)r finite, so r < 1.9e19 and 4e-6 max|coordinate| <= 1.4e33; k_distances takes the smaller of this and
// its density cell and is exact at any cell.
inline float radius_cell(double r, const float mn[3], const float mx[3], double factor = 1.03) {
    return (float)std::min(factor * r + 4e-6 * amax_of(mn, mx), 1e37);
}
// The radius of such a search as its entry point accepts it: finite and > 0, also as fp32, and r2 = (float)r * (float)r finite.
// square_not_below_flt_min: r2 a normal fp32 number too, for the tools in which a point must be its own neighbour -- d = 0 < r2 has
// to hold, and a subnormal r2 carries few bits.
inline bool radius_ok(double radius, bool square_not_below_flt_min) {
    const float r = (float)radius;
    return std::isfinite(radius) && std::isfinite(r) && r > 0.f && std::isfinite(r * r) && (!square_not_below_flt_min || r * r >= FLT_MIN);
}

// The grid of a k-nearest-neighbour search over d_rows (n points, `stride` floats apart, bounding box known).  The cell: a
// surface-like cloud spread over the faces of its box has r_k = sqrt(k A / (pi n)) (A = the box's area); the cell is 1.5 r_k, so
// that an occupied cell holds ~0.7 k points, then adapted to the measured mean occupancy (clouds that are lines, slabs or clumps):
// up to four builds.  d_occ: one device word for the count of occupied cells.  Returns the number of builds.
int build_knn_grid(plade_ctx *ctx, TargetGrid &G, const float *d_rows, uint32_t n, uint32_t stride, const float bbmin[3],
                   const float bbmax[3], int k, uint32_t *d_occ, const char *who);

typedef unsigned long long u64;
constexpr u64 EMPTY = ~0ull;

// (d, j) as one word d_bits << 32 | j: ordered exactly like (d, j) because d >= 0
__device__ __forceinline__ u64 make_key(float d, uint32_t j) { return ((u64)__float_as_uint(d) << 32) | (u64)j; }
__device__ __forceinline__ float key_d(u64 key) { return __uint_as_float((uint32_t)(key >> 32)); }   // EMPTY: NaN

__device__ __forceinline__ void cell_of(const GridView &g, f3 q, int &cx, int &cy, int &cz) {   // = k_cell_ids
    cx = min(max((int)floorf((q.x - g.mnx) * g.inv), 0), g.dx - 1);
    cy = min(max((int)floorf((q.y - g.mny) * g.inv), 0), g.dy - 1);
    cz = min(max((int)floorf((q.z - g.mnz) * g.inv), 0), g.dz - 1);
}

// the padded index of the first cell (x = -2) of row (y, z)
__device__ __forceinline__ uint32_t row_base(const GridView &g, int y, int z) {
    return (uint32_t)g.DX * ((uint32_t)(y + 2) + (uint32_t)g.DY * (uint32_t)(z + 2));
}

// f(j0, j1) for the nine runs of three cells around (cx, cy, cz), z outer, y inner
template <class F>
__device__ __forceinline__ void for_block27(const GridView &g, int cx, int cy, int cz, F &&f) {
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy) {
            const uint32_t r = (uint32_t)(cx + 1) + row_base(g, cy + dy, cz + dz);
            f(g.row_start[r], g.row_start[r + 3]);
        }
}

// distance from q to the outside of the block of cells [c - R, c + R]^3 (no bound where the block reaches the grid's edge: cell
// ids are clamped there, nothing lies beyond), less the margin; +inf: the block covers the grid
__device__ __forceinline__ double block_reach(const GridView &g, f3 q, int cx, int cy, int cz, int R, double margin) {
    double b = INFINITY;
    const double qv[3] = {q.x, q.y, q.z};
    const int c[3] = {cx, cy, cz}, d[3] = {g.dx, g.dy, g.dz};
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        if (c[t] - R > 0) b = fmin(b, qv[t] - (g.mn[t] + (double)(c[t] - R) * g.cell));
        if (c[t] + R < d[t] - 1) b = fmin(b, (g.mn[t] + (double)(c[t] + R + 1) * g.cell) - qv[t]);
    }
    return b == INFINITY ? b : b - margin;
}
// true: every point outside the block is farther than d (squared distance)
__device__ __forceinline__ bool inside_reach(float d, double reach) {
    if (reach == INFINITY) return true;
    return reach > 0.0 && d < (float)(reach * reach);
}

// a lane's K best keys as a sorted list in registers (statically indexed: no scratch)
template <int K>
__device__ __forceinline__ void insert(u64 (&best)[K], u64 key) {
    if (key < best[K - 1]) {
        // top down, in place: the new entry b depends only on the old entries b - 1 and b (no second copy of the list)
#pragma unroll
        for (int b = K - 1; b > 0; --b) best[b] = key < best[b - 1] ? best[b - 1] : (key < best[b] ? key : best[b]);
        best[0] = key < best[0] ? key : best[0];
    }
}

// The wave's 64 smallest keys: lane r holds the r-th.  Merged with one key per lane (EMPTY: none): the new keys are sorted across
// the wave (bitonic, 21 steps), reversed and merged with the list (the element-wise minimum of an ascending and a descending
// sequence is a bitonic sequence that holds the 64 smallest of both, 6 more steps).  Two u64 registers per lane, whatever k is.
__device__ __forceinline__ u64 wave_merge(u64 list, u64 key, int lane) {
    u64 v = key;
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1)
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const u64 o = __shfl_xor(v, stride, 64);
            const bool keep_min = ((lane & stride) == 0) == ((lane & size) == 0);
            v = keep_min ? (o < v ? o : v) : (o < v ? v : o);
        }
    const u64 r = __shfl(v, 63 - lane, 64);
    u64 t = list < r ? list : r;
#pragma unroll
    for (int stride = 32; stride > 0; stride >>= 1) {
        const u64 o = __shfl_xor(t, stride, 64);
        t = (lane & stride) == 0 ? (o < t ? o : t) : (o < t ? t : o);
    }
    return t;
}

__device__ __forceinline__ u64 wave_min(u64 v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const u64 w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}

// The ring walk.  A ring kernel gives one wavefront to each query its lane kernel could not finish and scans the block
// [c - rout, c + rout]^3 in growing steps (rin = -1, rout = 1; then rin = rout, rout += max(1, rout / 2): the radius grows by half
// per step).  One step -- this function, called by the whole wave -- reads only what the previous block [c - rin, c + rin]^3 did
// not hold: whole x runs of the rows outside the old block's y-z square, the two x runs left and right of it in the rows inside.
// So a step costs one or two row look-ups per in-grid row of the new block (its y-z square, not its volume), and an isolated
// point's search costs O(rows of the final block), i.e. O(R^2) look-ups, not the O(R^3) of ring-by-ring cells.  Lane l takes row
// t0 + l; the candidates of all lanes' runs are handed out 64 at a time (a wave-wide prefix sum over the run lengths, each lane
// finding its run by binary search over the lanes): on_batch(valid, p) is called by all lanes, p = this lane's candidate when
// valid.  What a batch is reduced to, and when the query is finished, are the caller's.
template <class F>
__device__ __forceinline__ void ring_step(const GridView &g, int cx, int cy, int cz, int rin, int rout, int lane, F &&on_batch) {
    const int y0 = max(cy - rout, 0), y1 = min(cy + rout, g.dy - 1), z0 = max(cz - rout, 0), z1 = min(cz + rout, g.dz - 1);
    const int ny = y1 - y0 + 1, rows = ny * (z1 - z0 + 1);
    const int xo0 = max(cx - rout, 0), xo1 = min(cx + rout, g.dx - 1);   // x range of the new block
    for (int t0 = 0; t0 < rows; t0 += 64) {                              // (wave-uniform)
        const int t = t0 + lane;
        uint32_t a0 = 0, la = 0, b0 = 0, lb = 0;                         // up to two runs of this lane's row
        if (t < rows) {
            const int y = y0 + t % ny, z = z0 + t / ny;
            const uint32_t row = row_base(g, y, z) + 2u;
            if (abs(y - cy) > rin || abs(z - cz) > rin) {                // outside the old block's y-z square: the whole run
                a0 = g.row_start[row + (uint32_t)xo0];
                la = g.row_start[row + (uint32_t)xo1 + 1u] - a0;
            } else {                                                     // inside: left and right of the old block
                if (cx - rin - 1 >= xo0) {
                    a0 = g.row_start[row + (uint32_t)xo0];
                    la = g.row_start[row + (uint32_t)(cx - rin)] - a0;
                }
                if (cx + rin + 1 <= xo1) {
                    b0 = g.row_start[row + (uint32_t)(cx + rin + 1)];
                    lb = g.row_start[row + (uint32_t)xo1 + 1u] - b0;
                }
            }
        }
        const uint32_t len = la + lb;
        uint32_t incl = len;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(incl, d, 64); if (lane >= d) incl += o; }
        const uint32_t pre = incl - len, cand_total = __shfl(incl, 63, 64);
        for (uint32_t c0 = 0; c0 < cand_total; c0 += 64) {               // (wave-uniform)
            const uint32_t idx = c0 + (uint32_t)lane;
            int o = 0;                                                   // the last lane whose run starts at or before idx
#pragma unroll
            for (int st = 32; st >= 1; st >>= 1) if (__shfl(pre, o + st, 64) <= idx) o += st;
            const uint32_t off = idx - __shfl(pre, o, 64), la_o = __shfl(la, o, 64);
            const uint32_t a0_o = __shfl(a0, o, 64), b0_o = __shfl(b0, o, 64);
            const bool valid = idx < cand_total;
            float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid) p = g.sorted[off < la_o ? a0_o + off : b0_o + (off - la_o)];
            on_batch(valid, p);
        }
    }
}

// The hand-out of ring_step on its own, for a walk that is no growing block (k_m3c2_walk): lane l offers one run of `sorted`,
// [a0, a0 + len) (len = 0: none).  The candidates of all lanes' runs are handed out 64 at a time in lane order, ascending sorted
// position within a run (the same prefix sum over the run lengths and binary search over the lanes): on_batch(valid, p) is
// called by all lanes, p = this lane's candidate when valid.  Wave-uniform control flow; no LDS.
template <class F>
__device__ __forceinline__ void hand_out_runs(const GridView &g, uint32_t a0, uint32_t len, int lane, F &&on_batch) {
    uint32_t incl = len;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(incl, d, 64); if (lane >= d) incl += o; }
    const uint32_t pre = incl - len, cand_total = __shfl(incl, 63, 64);
    for (uint32_t c0 = 0; c0 < cand_total; c0 += 64) {                   // (wave-uniform)
        const uint32_t idx = c0 + (uint32_t)lane;
        int o = 0;                                                       // the last lane whose run starts at or before idx
#pragma unroll
        for (int st = 32; st >= 1; st >>= 1) if (__shfl(pre, o + st, 64) <= idx) o += st;
        const uint32_t off = idx - __shfl(pre, o, 64), a0_o = __shfl(a0, o, 64);
        const bool valid = idx < cand_total;
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
        if (valid) p = g.sorted[a0_o + off];
        on_batch(valid, p);
    }
}

// wave-aggregated append of the failing lanes' values to a list (a lane kernel's hand-over to its ring kernel): one atomic per
// wavefront.  Called by all lanes
__device__ __forceinline__ void fail_append(bool fail, uint32_t value, uint32_t *list, uint32_t *count) {
    const u64 mask = __ballot(fail);
    if (mask) {
        const uint32_t lane = threadIdx.x & 63u, leader = (uint32_t)__ffsll((long long)mask) - 1u;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(count, (uint32_t)__popcll(mask));
        base = __shfl(base, (int)leader, 64);
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        if (fail) list[base + rank] = value;
    }
}

}  // namespace plade
