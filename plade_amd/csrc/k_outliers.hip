// plade_amd/csrc/k_outliers.hip -- statistical and radius outlier removal on gfx950 (semantics: outliers.h).
//
// Layout
//   grid     the dense row index of TargetGrid (overlap.h).  Statistical mode: the cell of k_normals (an occupied cell holds about
//            0.7 k points, adapted to the measured occupancy).  Radius mode: the cell is 1.03 r + 4e-6 max|coordinate| (the rule of
//            DESIGN.md section 10), so the 27-cell block around a point holds everything closer than r.
//   search   k_outliers_grid<K>: one lane per point in the grid's sorted order keeps its K best (d, j) keys -- 64-bit words
//            d_bits << 32 | j -- as a sorted list in registers, the point itself left out by its index.  A point whose k-th key is
//            closer than the outside of its 27-cell block is finished: m_i is summed from the registers in ascending key order.
//            The others are appended to a compacted list.
//   rings    k_outliers_ring: one wavefront per listed point, the growing blocks of k_normals_ring (one key per lane, bitonic
//            merges).  m_i is summed in the same order by a broadcast per key: the same bits as the grid kernel would give.
//   radius   k_outliers_radius: one lane per point in grid order counts the points of its 27-cell block closer than r.  Without
//            the per-point counts a lane stops at the end of the row run that reaches min_neighbours.
//   mu sigma k_outliers_sum / k_outliers_final, twice: a butterfly per wave, the waves in order, one partial per workgroup; one
//            wavefront sums the partials (lane l: partials l, l + 64, ..., then a butterfly).  No fp64 atomics.  mu, sigma and the
//            threshold stay on the device for the next kernel.
//   keep     k_outliers_flags; compact_flags (one scan) gives the ascending kept list; k_outliers_gather copies the kept rows
//            word by word.
#include "outliers.h"
#include "overlap.h"
#include "prims.h"
#include "stages.h"
#include "voxel.h"
#include <functional>

namespace plade {

namespace {

typedef unsigned long long u64;
constexpr u64 EMPTY = ~0ull;
constexpr int GRID_TPB = 128, RING_WAVES = 4, RAD_TPB = 256, SUM_TPB = 256, ROW_TPB = 256;

// the dense row index and its cell assignment (k_cell_ids)
struct GridView {
    const float4 *sorted;            // the points in cell order: x y z, bit-cast original index
    const uint32_t *row_start;
    uint32_t n;
    float mnx, mny, mnz, inv;
    int dx, dy, dz, DX, DY;          // cells, padded row pitch
};

struct StatArgs {
    GridView g;
    int m;                           // k_eff = min(k, n - 1) >= 1
    double mn[3], cell, margin;
    double *mean;                    // m_i by original index
    uint32_t *fail, *fail_count;
};

struct RadArgs {
    GridView g;
    float r2;                        // (float)r * (float)r
    uint32_t min_nb, stop;           // stop: the count at which a lane may end (0xffffffff: count everything)
    uint32_t *count;                 // c_i by original index, or nullptr
    uint8_t *keep;
    uint32_t *flags;
};

__device__ __forceinline__ u64 make_key(float d, uint32_t j) { return ((u64)__float_as_uint(d) << 32) | (u64)j; }
__device__ __forceinline__ float key_d(u64 key) { return __uint_as_float((uint32_t)(key >> 32)); }   // EMPTY: NaN

__device__ __forceinline__ void cell_of(const GridView &g, f3 q, int &cx, int &cy, int &cz) {   // = k_cell_ids
    cx = min(max((int)floorf((q.x - g.mnx) * g.inv), 0), g.dx - 1);
    cy = min(max((int)floorf((q.y - g.mny) * g.inv), 0), g.dy - 1);
    cz = min(max((int)floorf((q.z - g.mnz) * g.inv), 0), g.dz - 1);
}

template <int K>
__device__ __forceinline__ void insert(u64 (&best)[K], u64 key) {
    if (key < best[K - 1]) {
        // top down, in place: the new entry b depends only on the old entries b - 1 and b
#pragma unroll
        for (int b = K - 1; b > 0; --b) best[b] = key < best[b - 1] ? best[b - 1] : (key < best[b] ? key : best[b]);
        best[0] = key < best[0] ? key : best[0];
    }
}

// distance from q to the outside of the block of cells [c - R, c + R]^3 (no bound where the block reaches the grid's edge: cell
// ids are clamped there, nothing lies beyond), less the margin; +inf: the block covers the grid
__device__ __forceinline__ double block_reach(const StatArgs &a, f3 q, int cx, int cy, int cz, int R) {
    double b = INFINITY;
    const double qv[3] = {q.x, q.y, q.z};
    const int c[3] = {cx, cy, cz}, d[3] = {a.g.dx, a.g.dy, a.g.dz};
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        if (c[t] - R > 0) b = fmin(b, qv[t] - (a.mn[t] + (double)(c[t] - R) * a.cell));
        if (c[t] + R < d[t] - 1) b = fmin(b, (a.mn[t] + (double)(c[t] + R + 1) * a.cell) - qv[t]);
    }
    return b == INFINITY ? b : b - a.margin;
}
// true: every point outside the block is farther than d (squared distance)
__device__ __forceinline__ bool inside_reach(float d, double reach) {
    if (reach == INFINITY) return true;
    return reach > 0.0 && d < (float)(reach * reach);
}

template <int K>
__global__ __launch_bounds__(GRID_TPB) void k_outliers_grid(const StatArgs a) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    bool fail = false;
    if (s < a.g.n) {
        const float4 q4 = a.g.sorted[s];
        const f3 q(q4.x, q4.y, q4.z);
        const uint32_t self = __float_as_uint(q4.w);
        int cx, cy, cz;
        cell_of(a.g, q, cx, cy, cz);
        u64 best[K];
#pragma unroll
        for (int b = 0; b < K; ++b) best[b] = EMPTY;
        // nine runs of three cells; the padding of the row index makes every row of the block valid
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy) {
                const uint32_t r = (uint32_t)(cx + 1) + (uint32_t)a.g.DX * ((uint32_t)(cy + dy + 2) + (uint32_t)a.g.DY * (uint32_t)(cz + dz + 2));
                const uint32_t j1 = a.g.row_start[r + 3];
                for (uint32_t j = a.g.row_start[r]; j < j1; ++j) {
                    const float4 p = a.g.sorted[j];
                    const uint32_t orig = __float_as_uint(p.w);
                    if (orig != self) insert<K>(best, make_key(flann_d2(q, f3(p.x, p.y, p.z)), orig));
                }
            }
        u64 kth = EMPTY;
#pragma unroll
        for (int b = 0; b < K; ++b) if (b == a.m - 1) kth = best[b];
        if (kth != EMPTY && inside_reach(key_d(kth), block_reach(a, q, cx, cy, cz, 1))) {
            double sum = 0.0;
#pragma unroll
            for (int b = 0; b < K; ++b) if (b < a.m) sum += sqrt((double)key_d(best[b]));
            a.mean[self] = sum / (double)a.m;
        } else
            fail = true;
    }
    // wave-aggregated append to the list of the ring pass
    const u64 mask = __ballot(fail);
    if (mask) {
        const uint32_t lane = threadIdx.x & 63u, leader = (uint32_t)__ffsll((long long)mask) - 1u;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(a.fail_count, (uint32_t)__popcll(mask));
        base = __shfl(base, (int)leader, 64);
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        if (fail) a.fail[base + rank] = s;
    }
}

// The wave's 64 smallest keys: lane r holds the r-th.  Merged with one key per lane (EMPTY: none): the new keys are sorted across
// the wave (bitonic, 21 steps), reversed and merged with the list (the element-wise minimum of an ascending and a descending
// sequence is a bitonic sequence that holds the 64 smallest of both, 6 more steps).
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

// One wavefront per point the grid kernel could not finish (persistent workgroups; the list's length stays on the device).  The
// block [c - rout, c + rout]^3 grows by half its radius per step; a step reads whole x runs of the rows outside the old block's
// y-z square and the two x runs left and right of it in the rows inside (one or two row look-ups per row: O(R^2) per step).  The
// candidates of all lanes' runs are handed out 64 at a time (a wave prefix sum over the run lengths, each lane finding its run by
// a binary search over the lanes); a batch is merged only when one of its keys is below the current k-th.  The point is finished
// when the k-th key is closer than the outside of the block, or the block covers the grid (then all n - 1 >= k_eff other points
// have been scanned).
__global__ __launch_bounds__(64 * RING_WAVES) void k_outliers_ring(const StatArgs a) {
    const int lane = (int)(threadIdx.x & 63u), wv = (int)(threadIdx.x >> 6);
    const uint32_t total = *a.fail_count, stride_w = gridDim.x * RING_WAVES;
    for (uint32_t i = blockIdx.x * RING_WAVES + (uint32_t)wv; i < total; i += stride_w) {
        const uint32_t s = a.fail[i];
        const float4 q4 = a.g.sorted[s];
        const f3 q(q4.x, q4.y, q4.z);
        const uint32_t self = __float_as_uint(q4.w);
        int cx, cy, cz;
        cell_of(a.g, q, cx, cy, cz);
        u64 list = EMPTY;
        for (int rin = -1, rout = 1;; rin = rout, rout += max(1, rout / 2)) {
            const int y0 = max(cy - rout, 0), y1 = min(cy + rout, a.g.dy - 1), z0 = max(cz - rout, 0), z1 = min(cz + rout, a.g.dz - 1);
            const int ny = y1 - y0 + 1, rows = ny * (z1 - z0 + 1);
            const int xo0 = max(cx - rout, 0), xo1 = min(cx + rout, a.g.dx - 1);   // x range of the new block
            for (int t0 = 0; t0 < rows; t0 += 64) {                                // (wave-uniform)
                const int t = t0 + lane;
                uint32_t a0 = 0, la = 0, b0 = 0, lb = 0;                           // up to two runs of this lane's row
                if (t < rows) {
                    const int y = y0 + t % ny, z = z0 + t / ny;
                    const uint32_t row = (uint32_t)a.g.DX * ((uint32_t)(y + 2) + (uint32_t)a.g.DY * (uint32_t)(z + 2)) + 2u;
                    if (abs(y - cy) > rin || abs(z - cz) > rin) {                  // outside the old block's y-z square: the whole run
                        a0 = a.g.row_start[row + (uint32_t)xo0];
                        la = a.g.row_start[row + (uint32_t)xo1 + 1u] - a0;
                    } else {                                                       // inside: left and right of the old block
                        if (cx - rin - 1 >= xo0) {
                            a0 = a.g.row_start[row + (uint32_t)xo0];
                            la = a.g.row_start[row + (uint32_t)(cx - rin)] - a0;
                        }
                        if (cx + rin + 1 <= xo1) {
                            b0 = a.g.row_start[row + (uint32_t)(cx + rin + 1)];
                            lb = a.g.row_start[row + (uint32_t)xo1 + 1u] - b0;
                        }
                    }
                }
                const uint32_t len = la + lb;
                uint32_t incl = len;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(incl, d, 64); if (lane >= d) incl += o; }
                const uint32_t pre = incl - len, cand_total = __shfl(incl, 63, 64);
                for (uint32_t c0 = 0; c0 < cand_total; c0 += 64) {                 // (wave-uniform)
                    const uint32_t idx = c0 + (uint32_t)lane;
                    int o = 0;                                                     // the last lane whose run starts at or before idx
#pragma unroll
                    for (int st = 32; st >= 1; st >>= 1) if (__shfl(pre, o + st, 64) <= idx) o += st;
                    const uint32_t off = idx - __shfl(pre, o, 64), la_o = __shfl(la, o, 64);
                    const uint32_t a0_o = __shfl(a0, o, 64), b0_o = __shfl(b0, o, 64);
                    u64 key = EMPTY;
                    if (idx < cand_total) {
                        const float4 p = a.g.sorted[off < la_o ? a0_o + off : b0_o + (off - la_o)];
                        const uint32_t orig = __float_as_uint(p.w);
                        if (orig != self) key = make_key(flann_d2(q, f3(p.x, p.y, p.z)), orig);
                    }
                    const u64 kth = __shfl(list, a.m - 1, 64);
                    if (__ballot(key < kth)) list = wave_merge(list, key, lane);
                }
            }
            const double reach = block_reach(a, q, cx, cy, cz, rout);
            if (reach == INFINITY) break;
            if (inside_reach(key_d(__shfl(list, a.m - 1, 64)), reach)) break;   // (EMPTY: NaN, not inside)
        }
        // the grid kernel's sum: the keys in ascending order, one after the other
        const double term = lane < a.m ? sqrt((double)key_d(list)) : 0.0;
        double sum = 0.0;
        for (int r = 0; r < a.m; ++r) sum += __shfl(term, r, 64);
        if (lane == 0) a.mean[self] = sum / (double)a.m;
    }
}

__global__ __launch_bounds__(RAD_TPB) void k_outliers_radius(const RadArgs a) {
    const uint32_t s = blockIdx.x * RAD_TPB + threadIdx.x;
    if (s >= a.g.n) return;
    const float4 q4 = a.g.sorted[s];
    const f3 q(q4.x, q4.y, q4.z);
    const uint32_t self = __float_as_uint(q4.w);
    int cx, cy, cz;
    cell_of(a.g, q, cx, cy, cz);
    uint32_t c = 0;
    for (int t = 0; t < 9 && c < a.stop; ++t) {
        const int dy = t % 3 - 1, dz = t / 3 - 1;
        const uint32_t r = (uint32_t)(cx + 1) + (uint32_t)a.g.DX * ((uint32_t)(cy + dy + 2) + (uint32_t)a.g.DY * (uint32_t)(cz + dz + 2));
        const uint32_t j1 = a.g.row_start[r + 3];
        for (uint32_t j = a.g.row_start[r]; j < j1; ++j) {
            const float4 p = a.g.sorted[j];
            c += (__float_as_uint(p.w) != self && flann_d2(q, f3(p.x, p.y, p.z)) < a.r2) ? 1u : 0u;
        }
    }
    const uint32_t keep = c >= a.min_nb ? 1u : 0u;
    if (a.count) a.count[self] = c;
    a.keep[self] = (uint8_t)keep;
    a.flags[self] = keep;
}

// pass 0: the partial sums of m_i; pass 1: of (m_i - mu)^2 with mu = stat[0].  Fixed order: a butterfly across the wave, the
// waves in order
__global__ __launch_bounds__(SUM_TPB) void k_outliers_sum(const double *__restrict__ mean, uint32_t n, const double *__restrict__ stat,
                                                          int pass, double *__restrict__ partial) {
    __shared__ double s_red[SUM_TPB / 64];
    const uint32_t i = blockIdx.x * SUM_TPB + threadIdx.x;
    double v = 0.0;
    if (i < n) {
        v = mean[i];
        if (pass) { const double e = v - stat[0]; v = e * e; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = s_red[0];
#pragma unroll
        for (int w = 1; w < SUM_TPB / 64; ++w) t += s_red[w];
        partial[blockIdx.x] = t;
    }
}

// stat[0] = mu (pass 0); stat[1] = sigma, stat[2] = mu + alpha sigma (pass 1)
__global__ __launch_bounds__(64) void k_outliers_final(const double *__restrict__ partial, uint32_t blocks, uint32_t n, int pass,
                                                       double alpha, double *__restrict__ stat) {
    const int lane = threadIdx.x;
    double v = 0.0;
    for (uint32_t b = (uint32_t)lane; b < blocks; b += 64) v += partial[b];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane != 0) return;
    if (!pass) { stat[0] = v / (double)n; return; }
    const double sigma = n > 1 ? sqrt(v / (double)(n - 1)) : 0.0;
    stat[1] = sigma;
    stat[2] = stat[0] + alpha * sigma;
}

__global__ __launch_bounds__(ROW_TPB) void k_outliers_flags(const double *__restrict__ mean, uint32_t n, const double *__restrict__ stat,
                                                            uint8_t *__restrict__ keep, uint32_t *__restrict__ flags) {
    const uint32_t i = blockIdx.x * ROW_TPB + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = mean[i] <= stat[2] ? 1u : 0u;
    keep[i] = (uint8_t)k;
    flags[i] = k;
}

// out row o = in row kept[o], word by word (whatever the floats hold: NaN normals keep their bits)
__global__ __launch_bounds__(ROW_TPB) void k_outliers_gather(const uint32_t *__restrict__ in, uint32_t stride, const uint32_t *__restrict__ kept,
                                                             uint32_t total, uint32_t *__restrict__ out) {
    const size_t w = (size_t)blockIdx.x * ROW_TPB + threadIdx.x;
    if (w >= (size_t)total * stride) return;
    const uint32_t o = (uint32_t)(w / stride), c = (uint32_t)(w - (size_t)o * stride);
    out[w] = in[(size_t)kept[o] * stride + c];
}

// occ[0] += occupied cells (distinct sorted keys)
__global__ __launch_bounds__(256) void k_outliers_cells(const uint32_t *__restrict__ keys, uint32_t n, uint32_t *__restrict__ occ) {
    uint32_t c = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        c += (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(occ, c);
}

template <int K>
void launch_search(plade_ctx *ctx, const StatArgs &a) {
    hipLaunchKernelGGL(k_outliers_grid<K>, dim3(cdiv(a.g.n, GRID_TPB)), dim3(GRID_TPB), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_outliers_ring, dim3(std::min(cdiv(a.g.n, RING_WAVES), 2048u)), dim3(64 * RING_WAVES), 0, ctx->stream, a);
}

GridView view_of(const TargetGrid &G, uint32_t n) {
    GridView g;
    g.sorted = G.sorted.p; g.row_start = G.row_start.p; g.n = n;
    g.mnx = G.gp.mnx; g.mny = G.gp.mny; g.mnz = G.gp.mnz; g.inv = G.gp.inv;
    g.dx = G.gp.dx; g.dy = G.gp.dy; g.dz = G.gp.dz; g.DX = G.DX; g.DY = G.DY;
    return g;
}

}  // namespace

struct OutlierWork {
    TargetGrid grid;
    DBuf<uint32_t> fail, count, flags, pos, kept, nbr_count;
    DBuf<float> in, out;             // the host-pointer entry point's device copies (grow-only)
    DBuf<double> mean, partial, stat;
    DBuf<uint8_t> keep;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int builds = 0;
    uint32_t h_count = 0;
    double h_stat[3] = {0.0, 0.0, 0.0};
    ~OutlierWork() { for (hipEvent_t &e : ev) if (e) (void)hipEventDestroy(e); }
};
OutlierWork *outlier_work_create() { return new OutlierWork; }
void outlier_work_destroy(OutlierWork *w) { delete w; }

namespace {

void check_params(uint32_t n, uint32_t stride, const plade_outlier_params &p) {
    PLADE_REQUIRE(n >= 1, PLADE_EINVAL, "filter_outliers: the cloud is empty (n = 0)");
    PLADE_REQUIRE(stride >= 3, PLADE_EINVAL, "filter_outliers: stride must be >= 3 floats");
    PLADE_REQUIRE(p.mode == PLADE_OUTLIER_STATISTICAL || p.mode == PLADE_OUTLIER_RADIUS, PLADE_EINVAL, "filter_outliers: unknown mode");
    if (p.mode == PLADE_OUTLIER_STATISTICAL) {
        PLADE_REQUIRE(p.k >= OUTLIERS_K_MIN && p.k <= OUTLIERS_K_MAX, PLADE_EINVAL, "filter_outliers: k must be in [1, 64]");
        PLADE_REQUIRE(std::isfinite(p.alpha) && p.alpha >= 0.0, PLADE_EINVAL, "filter_outliers: alpha must be finite and >= 0");
    } else {
        const float r = (float)p.radius;
        PLADE_REQUIRE(std::isfinite(p.radius) && std::isfinite(r) && r > 0.f && std::isfinite(r * r), PLADE_EINVAL,
                      "filter_outliers: radius must be finite and > 0");
        PLADE_REQUIRE(p.min_neighbours >= 1, PLADE_EINVAL, "filter_outliers: min_neighbours must be >= 1");
    }
}

// The filter on a device cloud of `stride` floats per point with a known bounding box.  Leaves keep (n bytes), the kept list and
// m or c (want_values) in W, gathers the kept rows into dst(kept) -- not called when nothing is kept --, waits, fills the summary
// and the stats.  Returns the number of kept points.
uint32_t filter_dev(plade_ctx *ctx, OutlierWork &W, const float *d_rows, uint32_t n, uint32_t stride, const float bbmin[3],
                    const float bbmax[3], const plade_outlier_params &p, bool want_values, const std::function<float *(uint32_t)> &dst,
                    plade_outlier_summary *summary) {
    for (hipEvent_t &e : W.ev) if (!e) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventRecord(W.ev[0], ctx->stream));
    TargetGrid &G = W.grid;
    const bool stat = p.mode == PLADE_OUTLIER_STATISTICAL;
    const double ex = std::max(1e-9, (double)bbmax[0] - bbmin[0]), ey = std::max(1e-9, (double)bbmax[1] - bbmin[1]),
                 ez = std::max(1e-9, (double)bbmax[2] - bbmin[2]);
    double amax = 0.0;
    for (int t = 0; t < 3; ++t) amax = std::max(amax, std::max(std::fabs((double)bbmin[t]), std::fabs((double)bbmax[t])));
    uint32_t *d_cnt = W.count.ensure(4);   // [0]: the ring list's length, [1]: occupied cells
    uint8_t *d_keep = W.keep.ensure((size_t)n + 4);
    uint32_t *d_flags = W.flags.ensure((size_t)n + 1);
    double *d_stat = W.stat.ensure(4);
    W.builds = 0;
    W.h_count = 0;
    ctx->fill_async(d_cnt, 0, 4);
    ctx->fill_async(d_flags + n, 0, 4);    // compact_flags scans n + 1 entries
    if (stat) {
        const int k = p.k, m = (int)std::min<uint32_t>((uint32_t)k, n - 1);
        double *d_mean = W.mean.ensure(n);
        if (m == 0) {                      // n = 1: m_0 = 0
            ctx->fill_async(d_mean, 0, 8);
            HIP_TRY(hipEventRecord(W.ev[1], ctx->stream));
        } else {
            // cell: k_normals' -- a surface-like cloud spread over the faces of its box has r_k = sqrt(k A / (pi n)); the cell is
            // 1.5 r_k (an occupied cell holds ~0.7 k points), then adapted to the measured mean occupancy
            const double area = 2 * (ex * ey + ey * ez + ex * ez), target = 0.7 * k;
            float cell = (float)(1.5 * std::sqrt((double)k * area / (M_PI * (double)n)));
            if (!(cell > 0.f) || !std::isfinite(cell)) cell = 1.f;
            for (int attempt = 0;; ++attempt) {
                G.build(ctx, d_rows, n, stride, cell, bbmin, bbmax, true);
                ++W.builds;
                PLADE_REQUIRE(G.dense, PLADE_EINVAL, "filter_outliers: needs the dense row index (unset PLADE_OVERLAP_INDEX_COMPACT)");
                if (attempt == 3 || n <= (uint32_t)(4 * k)) break;
                ctx->fill_async(d_cnt + 1, 0, 4);
                hipLaunchKernelGGL(k_outliers_cells, dim3(std::min(cdiv(n, 1024), 512u)), dim3(256), 0, ctx->stream, G.keys2.p, n, d_cnt + 1);
                HIP_TRY(hipGetLastError());
                uint32_t occ = 0;
                ctx->d2h(&occ, d_cnt + 1, 4);
                ctx->sync();
                const double mean = (double)n / std::max(occ, 1u);
                const float built = 1.f / G.gp.inv;          // build() enlarges the cell when the cell budget is hit
                if (mean > 2.0 * target && built <= cell * 1.01f) cell = built * (float)std::max(0.25, std::sqrt(target / mean));   // too coarse
                else if (mean < 0.5 * target && occ < n) cell = built * (float)std::min(4.0, std::sqrt(target / mean));          // too fine
                else break;
            }
            HIP_TRY(hipEventRecord(W.ev[1], ctx->stream));
            StatArgs a;
            memset(&a, 0, sizeof(a));
            a.g = view_of(G, n);
            a.m = m;
            a.mn[0] = G.gp.mnx; a.mn[1] = G.gp.mny; a.mn[2] = G.gp.mnz;
            a.cell = 1.0 / (double)G.gp.inv;
            a.margin = 0.01 * a.cell + 1e-6 * amax;   // fp32 cell assignment: a few ulps of the coordinates, 1 % of a cell on top
            a.mean = d_mean;
            a.fail = W.fail.ensure(n); a.fail_count = d_cnt;
            if (k <= 8) launch_search<8>(ctx, a);
            else if (k <= 16) launch_search<16>(ctx, a);
            else if (k <= 32) launch_search<32>(ctx, a);
            else launch_search<64>(ctx, a);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(W.ev[2], ctx->stream));
        const uint32_t blocks = cdiv(n, SUM_TPB);
        double *d_partial = W.partial.ensure(blocks);
        for (int pass = 0; pass < 2; ++pass) {
            hipLaunchKernelGGL(k_outliers_sum, dim3(blocks), dim3(SUM_TPB), 0, ctx->stream, d_mean, n, d_stat, pass, d_partial);
            hipLaunchKernelGGL(k_outliers_final, dim3(1), dim3(64), 0, ctx->stream, d_partial, blocks, n, pass, p.alpha, d_stat);
        }
        hipLaunchKernelGGL(k_outliers_flags, dim3(cdiv(n, ROW_TPB)), dim3(ROW_TPB), 0, ctx->stream, d_mean, n, d_stat, d_keep, d_flags);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(W.h_stat, d_stat, sizeof(W.h_stat), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(&W.h_count, d_cnt, 4, hipMemcpyDeviceToHost, ctx->stream));
    } else {
        const float r = (float)p.radius;
        G.build(ctx, d_rows, n, stride, (float)(1.03 * (double)r + 4e-6 * amax), bbmin, bbmax, true);
        ++W.builds;
        PLADE_REQUIRE(G.dense, PLADE_EINVAL, "filter_outliers: needs the dense row index (unset PLADE_OVERLAP_INDEX_COMPACT)");
        HIP_TRY(hipEventRecord(W.ev[1], ctx->stream));
        RadArgs a;
        memset(&a, 0, sizeof(a));
        a.g = view_of(G, n);
        a.r2 = r * r;
        a.min_nb = (uint32_t)p.min_neighbours;
        a.stop = want_values ? 0xffffffffu : a.min_nb;
        a.count = want_values ? W.nbr_count.ensure(n) : nullptr;
        a.keep = d_keep; a.flags = d_flags;
        hipLaunchKernelGGL(k_outliers_radius, dim3(cdiv(n, RAD_TPB)), dim3(RAD_TPB), 0, ctx->stream, a);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(W.ev[2], ctx->stream));
    }
    HIP_TRY(hipEventRecord(W.ev[3], ctx->stream));
    const uint32_t total = compact_flags(ctx, d_flags, n, W.pos, W.kept);   // (waits for the count)
    if (total) {
        float *d_out = dst(total);
        const size_t words = (size_t)total * stride;
        hipLaunchKernelGGL(k_outliers_gather, dim3(cdiv(words, ROW_TPB)), dim3(ROW_TPB), 0, ctx->stream,
                           reinterpret_cast<const uint32_t *>(d_rows), stride, W.kept.p, total, reinterpret_cast<uint32_t *>(d_out));
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(W.ev[4], ctx->stream));
    ctx->sync();
    if (summary) {
        summary->n = n;
        summary->kept = total;
        summary->mu = stat ? W.h_stat[0] : NAN;
        summary->sigma = stat ? W.h_stat[1] : NAN;
        summary->threshold = stat ? W.h_stat[2] : NAN;
    }
    float ms[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < 4; ++k) HIP_TRY(hipEventElapsedTime(&ms[k], W.ev[k], W.ev[k + 1]));
    ctx->stats.clear();
    ctx->stats.add("outliers_grid_s", 1e-3 * ms[0]);
    ctx->stats.add("outliers_search_s", 1e-3 * ms[1]);
    ctx->stats.add("outliers_reduce_s", 1e-3 * ms[2]);
    ctx->stats.add("outliers_compact_s", 1e-3 * ms[3]);
    ctx->stats.add("outliers_grid_builds", W.builds);
    ctx->stats.add("outliers_ring_queries", W.h_count);
    ctx->stats.add("outliers_kept", total);
    return total;
}

OutlierWork &work_of(plade_ctx *ctx) {
    if (!ctx->outlier_work) ctx->outlier_work = outlier_work_create();
    return *ctx->outlier_work;
}

}  // namespace
}  // namespace plade

using namespace plade;

// ---- C ABI (include/plade_hip.h) ---------------------------------------------------------------------------------------------
extern "C" void plade_outlier_default_params(plade_outlier_params *p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->mode = PLADE_OUTLIER_STATISTICAL;
    p->k = 16;
    p->alpha = 1.0;
    p->radius = 0.0;
    p->min_neighbours = 1;
}

extern "C" int plade_filter_outliers(plade_ctx *ctx, const float *rows, uint32_t n, uint32_t stride, const plade_outlier_params *params,
                                     uint8_t *keep_out, uint32_t *kept_index_out, float *rows_out, double *mean_dist_out,
                                     uint32_t *count_out, plade_outlier_summary *summary) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(rows, PLADE_EINVAL, "plade_filter_outliers: NULL cloud");
        plade_outlier_params p;
        if (params) p = *params; else plade_outlier_default_params(&p);
        check_params(n, stride, p);
        OutlierWork &W = work_of(ctx);
        W.in.ensure((size_t)n * stride + 4);
        HIP_TRY(hipMemcpyAsync(W.in.p, rows, (size_t)n * stride * 4, hipMemcpyHostToDevice, ctx->stream));
        float mn[3], mx[3];
        bbox_host(ctx, W.in.p, n, stride, mn, mx);   // (waits; refuses non-finite coordinates)
        const bool stat = p.mode == PLADE_OUTLIER_STATISTICAL;
        const bool want_values = stat ? mean_dist_out != nullptr : count_out != nullptr;
        const uint32_t total = filter_dev(ctx, W, W.in.p, n, stride, mn, mx, p, want_values,
                                          [&](uint32_t kept) { return W.out.ensure((size_t)kept * stride + 4); }, summary);
        if (keep_out) HIP_TRY(hipMemcpyAsync(keep_out, W.keep.p, n, hipMemcpyDeviceToHost, ctx->stream));
        if (kept_index_out && total) HIP_TRY(hipMemcpyAsync(kept_index_out, W.kept.p, (size_t)total * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (rows_out && total) HIP_TRY(hipMemcpyAsync(rows_out, W.out.p, (size_t)total * stride * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (stat && mean_dist_out) HIP_TRY(hipMemcpyAsync(mean_dist_out, W.mean.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (!stat && count_out) HIP_TRY(hipMemcpyAsync(count_out, W.nbr_count.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        return PLADE_OK;
    });
}

extern "C" int plade_cloud_filter_outliers_dev(plade_ctx *ctx, plade_cloud *cloud, const plade_outlier_params *params, plade_cloud **out,
                                               uint8_t *keep_out, uint32_t *kept_index_out, plade_outlier_summary *summary) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(cloud && out, PLADE_EINVAL, "plade_cloud_filter_outliers_dev: NULL cloud");
        *out = nullptr;
        plade_outlier_params p;
        if (params) p = *params; else plade_outlier_default_params(&p);
        const CloudDev &in = cloud->dev;
        check_params(in.n, 6, p);
        OutlierWork &W = work_of(ctx);
        plade_cloud *c = new plade_cloud;
        try {
            const uint32_t total = filter_dev(ctx, W, in.aos.p, in.n, 6, in.bbmin, in.bbmax, p, false,
                                              [&](uint32_t kept) { cloud_shape(c->dev, kept); return c->dev.aos.p; }, summary);
            if (keep_out) HIP_TRY(hipMemcpyAsync(keep_out, W.keep.p, in.n, hipMemcpyDeviceToHost, ctx->stream));
            if (kept_index_out && total) HIP_TRY(hipMemcpyAsync(kept_index_out, W.kept.p, (size_t)total * 4, hipMemcpyDeviceToHost, ctx->stream));
            ctx->sync();
            PLADE_REQUIRE(total >= 1, PLADE_EFAIL, "plade_cloud_filter_outliers_dev: the filter keeps no point (a resident cloud cannot be empty)");
            cloud_finish_device(ctx, c->dev);   // SoA planes + bounding box of the resident cloud, as plade_cloud_upload
        } catch (...) { delete c; throw; }
        *out = c;
        return PLADE_OK;
    });
}
