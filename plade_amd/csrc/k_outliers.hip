// plade_amd/csrc/k_outliers.hip -- statistical and radius outlier removal on gfx950 (semantics: outliers.h).
//
// Layout
//   grid     the dense row index of TargetGrid, walked with the pieces of grid_walk.h.  Statistical mode: the cell of k_normals
//            (build_knn_grid: an occupied cell holds about 0.7 k points, adapted to the measured occupancy).  Radius mode: the cell
//            is radius_cell(r) of grid_walk.h (the rule of DESIGN.md section 10), so the 27-cell block around a point holds
//            everything closer than r.
//   search   k_outliers_grid<K>: one lane per point in the grid's sorted order keeps its K best (d, j) keys -- 64-bit words
//            d_bits << 32 | j -- as a sorted list in registers, the point itself left out by its index.  A point whose k-th key is
//            closer than the outside of its 27-cell block is finished: m_i is summed from the registers in ascending key order.
//            The others are appended to a compacted list.
//   rings    k_outliers_ring: one wavefront per listed point, the growing blocks of k_normals_ring (ring_step; one key per lane,
//            wave_merge).  m_i is summed in the same order by a broadcast per key: the same bits as the grid kernel would give.
//   radius   k_outliers_radius: one lane per point in grid order counts the points of its 27-cell block closer than r.  Without
//            the per-point counts a lane stops at the end of the row run that reaches min_neighbours.
//   mu sigma k_outliers_sum / k_outliers_final, twice, in the fixed order of fixed_reduce.h.  mu, sigma and the threshold stay on
//            the device for the next kernel.
//   keep     k_outliers_flags; compact_flags (one scan) gives the ascending kept list; gather_rows (prims.h) copies the kept
//            rows word by word.
#include "outliers.h"
#include "cloud_tool.h"
#include "fixed_reduce.h"
#include "grid_walk.h"
#include "voxel.h"

namespace plade {

namespace {

constexpr int GRID_TPB = 128, RING_WAVES = 4, RAD_TPB = 256, SUM_TPB = 256, ROW_TPB = 256;

struct StatArgs {
    GridView g;
    uint32_t n;
    int m;                           // k_eff = min(k, n - 1) >= 1
    double margin;                   // grid_margin
    double *mean;                    // m_i by original index
    uint32_t *fail, *fail_count;
};

struct RadArgs {
    GridView g;
    uint32_t n;
    float r2;                        // (float)r * (float)r
    uint32_t min_nb, stop;           // stop: the count at which a lane may end (0xffffffff: count everything)
    uint32_t *count;                 // c_i by original index, or nullptr
    uint8_t *keep;
    uint32_t *flags;
};

template <int K>
__global__ __launch_bounds__(GRID_TPB) void k_outliers_grid(const StatArgs a) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    bool fail = false;
    if (s < a.n) {
        const float4 q4 = a.g.sorted[s];
        const f3 q(q4.x, q4.y, q4.z);
        const uint32_t self = __float_as_uint(q4.w);
        int cx, cy, cz;
        cell_of(a.g, q, cx, cy, cz);
        u64 best[K];
#pragma unroll
        for (int b = 0; b < K; ++b) best[b] = EMPTY;
        // for_block27's runs, written out (as in k_normals_grid: the register list is not handed to a lambda)
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy) {
                const uint32_t r = (uint32_t)(cx + 1) + row_base(a.g, cy + dy, cz + dz);
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
        if (kth != EMPTY && inside_reach(key_d(kth), block_reach(a.g, q, cx, cy, cz, 1, a.margin))) {
            double sum = 0.0;
#pragma unroll
            for (int b = 0; b < K; ++b) if (b < a.m) sum += sqrt((double)key_d(best[b]));
            a.mean[self] = sum / (double)a.m;
        } else
            fail = true;
    }
    fail_append(fail, s, a.fail, a.fail_count);   // to the list of the ring pass
}

// One wavefront per point the grid kernel could not finish (persistent workgroups; the list's length stays on the device): the
// growing blocks of ring_step, the point itself left out.  A batch is merged only when one of its keys is below the current k-th.
// The point is finished when the k-th key is closer than the outside of the block, or the block covers the grid (then all
// n - 1 >= k_eff other points have been scanned).
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
            ring_step(a.g, cx, cy, cz, rin, rout, lane, [&](bool valid, float4 p) {
                const uint32_t orig = __float_as_uint(p.w);
                const u64 key = valid && orig != self ? make_key(flann_d2(q, f3(p.x, p.y, p.z)), orig) : EMPTY;
                const u64 kth = __shfl(list, a.m - 1, 64);
                if (__ballot(key < kth)) list = wave_merge(list, key, lane);
            });
            const double reach = block_reach(a.g, q, cx, cy, cz, rout, a.margin);
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
    if (s >= a.n) return;
    const float4 q4 = a.g.sorted[s];
    const f3 q(q4.x, q4.y, q4.z);
    const uint32_t self = __float_as_uint(q4.w);
    int cx, cy, cz;
    cell_of(a.g, q, cx, cy, cz);
    uint32_t c = 0;
    for (int t = 0; t < 9 && c < a.stop; ++t) {
        const int dy = t % 3 - 1, dz = t / 3 - 1;
        const uint32_t r = (uint32_t)(cx + 1) + row_base(a.g, cy + dy, cz + dz);   // for_block27's runs, with an early end
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

// pass 0: the partial sums of m_i; pass 1: of (m_i - mu)^2 with mu = stat[0] (the order: fixed_reduce.h)
__global__ __launch_bounds__(SUM_TPB) void k_outliers_sum(const double *__restrict__ mean, uint32_t n, const double *__restrict__ stat,
                                                          int pass, double *__restrict__ partial) {
    __shared__ double s_red[SUM_TPB / 64][1];
    const uint32_t i = blockIdx.x * SUM_TPB + threadIdx.x;
    double v[1] = {0.0};
    if (i < n) {
        v[0] = mean[i];
        if (pass) { const double e = v[0] - stat[0]; v[0] = e * e; }
    }
    block_reduce<SUM_TPB>(v, s_red, partial, SumOp());
}

// stat[0] = mu (pass 0); stat[1] = sigma, stat[2] = mu + alpha sigma (pass 1)
__global__ __launch_bounds__(64) void k_outliers_final(const double *__restrict__ partial, uint32_t blocks, uint32_t n, int pass,
                                                       double alpha, double *__restrict__ stat) {
    double s[1];
    final_reduce(partial, blocks, s, SumOp());
    if (threadIdx.x != 0) return;
    const double v = s[0];
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

template <int K>
void launch_search(plade_ctx *ctx, const StatArgs &a) {
    hipLaunchKernelGGL(k_outliers_grid<K>, dim3(cdiv(a.n, GRID_TPB)), dim3(GRID_TPB), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_outliers_ring, dim3(std::min(cdiv(a.n, RING_WAVES), 2048u)), dim3(64 * RING_WAVES), 0, ctx->stream, a);
}

}  // namespace

struct OutlierWork : KeepWork {
    TargetGrid grid;
    DBuf<uint32_t> fail, count, nbr_count;
    DBuf<double> mean, partial, stat;
    EventSpans<5> spans;             // grid, search, reduce, compact
    int builds = 0;
    uint32_t h_count = 0;
    double h_stat[3] = {0.0, 0.0, 0.0};
};

namespace {

void check_params(uint32_t n, uint32_t stride, const plade_outlier_params &p) {
    PLADE_REQUIRE(n >= 1, PLADE_EINVAL, "filter_outliers: the cloud is empty (n = 0)");
    PLADE_REQUIRE(stride >= 3, PLADE_EINVAL, "filter_outliers: stride must be >= 3 floats");
    PLADE_REQUIRE(p.mode == PLADE_OUTLIER_STATISTICAL || p.mode == PLADE_OUTLIER_RADIUS, PLADE_EINVAL, "filter_outliers: unknown mode");
    if (p.mode == PLADE_OUTLIER_STATISTICAL) {
        PLADE_REQUIRE(p.k >= OUTLIERS_K_MIN && p.k <= OUTLIERS_K_MAX, PLADE_EINVAL, "filter_outliers: k must be in [1, 64]");
        PLADE_REQUIRE(std::isfinite(p.alpha) && p.alpha >= 0.0, PLADE_EINVAL, "filter_outliers: alpha must be finite and >= 0");
    } else {
        PLADE_REQUIRE(radius_ok(p.radius, false), PLADE_EINVAL, "filter_outliers: radius must be finite and > 0");
        PLADE_REQUIRE(p.min_neighbours >= 1, PLADE_EINVAL, "filter_outliers: min_neighbours must be >= 1");
    }
}

// The filter on a device cloud of `stride` floats per point with a known bounding box.  Leaves keep (n bytes), the kept list and
// m or c (want_values) in W, gathers the kept rows into dst(kept) -- not called when nothing is kept --, waits, fills the summary
// and the stats.  Returns the number of kept points.
uint32_t filter_dev(plade_ctx *ctx, OutlierWork &W, const float *d_rows, uint32_t n, uint32_t stride, const float bbmin[3],
                    const float bbmax[3], const plade_outlier_params &p, bool want_values, const KeepRows &dst,
                    plade_outlier_summary *summary) {
    W.spans.mark(ctx, 0);
    TargetGrid &G = W.grid;
    const bool stat = p.mode == PLADE_OUTLIER_STATISTICAL;
    uint32_t *d_cnt = W.count.ensure(4);   // [0]: the ring list's length, [1]: occupied cells
    uint8_t *d_keep = W.keep.ensure((size_t)n + 4);
    double *d_stat = W.stat.ensure(4);
    W.builds = 0;
    W.h_count = 0;
    ctx->fill_async(d_cnt, 0, 4);
    uint32_t *d_flags = keep_flags(ctx, W, n);
    if (stat) {
        const int k = p.k, m = (int)std::min<uint32_t>((uint32_t)k, n - 1);
        double *d_mean = W.mean.ensure(n);
        if (m == 0) {                      // n = 1: m_0 = 0
            ctx->fill_async(d_mean, 0, 8);
            W.spans.mark(ctx, 1);
        } else {
            W.builds = build_knn_grid(ctx, G, d_rows, n, stride, bbmin, bbmax, k, d_cnt + 1, "filter_outliers");
            W.spans.mark(ctx, 1);
            StatArgs a;
            memset(&a, 0, sizeof(a));
            a.g = view_of(G, "filter_outliers");
            a.n = n; a.m = m;
            a.margin = grid_margin(a.g, bbmin, bbmax);
            a.mean = d_mean;
            a.fail = W.fail.ensure(n); a.fail_count = d_cnt;
            if (k <= 8) launch_search<8>(ctx, a);
            else if (k <= 16) launch_search<16>(ctx, a);
            else if (k <= 32) launch_search<32>(ctx, a);
            else launch_search<64>(ctx, a);
            HIP_TRY(hipGetLastError());
        }
        W.spans.mark(ctx, 2);
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
        G.build(ctx, d_rows, n, stride, radius_cell((double)r, bbmin, bbmax), bbmin, bbmax, true);
        ++W.builds;
        W.spans.mark(ctx, 1);
        RadArgs a;
        memset(&a, 0, sizeof(a));
        a.g = view_of(G, "filter_outliers");
        a.n = n; a.r2 = r * r;
        a.min_nb = (uint32_t)p.min_neighbours;
        a.stop = want_values ? 0xffffffffu : a.min_nb;
        a.count = want_values ? W.nbr_count.ensure(n) : nullptr;
        a.keep = d_keep; a.flags = d_flags;
        hipLaunchKernelGGL(k_outliers_radius, dim3(cdiv(n, RAD_TPB)), dim3(RAD_TPB), 0, ctx->stream, a);
        HIP_TRY(hipGetLastError());
        W.spans.mark(ctx, 2);
    }
    W.spans.mark(ctx, 3);
    const uint32_t total = keep_compact_gather(ctx, W, d_rows, n, stride, dst);
    W.spans.mark(ctx, 4);
    ctx->sync();
    if (summary) {
        summary->n = n;
        summary->kept = total;
        summary->mu = stat ? W.h_stat[0] : NAN;
        summary->sigma = stat ? W.h_stat[1] : NAN;
        summary->threshold = stat ? W.h_stat[2] : NAN;
    }
    W.spans.collect();
    ctx->stats.clear();
    ctx->stats.add("outliers_grid_s", W.spans.seconds(0));
    ctx->stats.add("outliers_search_s", W.spans.seconds(1));
    ctx->stats.add("outliers_reduce_s", W.spans.seconds(2));
    ctx->stats.add("outliers_compact_s", W.spans.seconds(3));
    ctx->stats.add("outliers_grid_builds", W.builds);
    ctx->stats.add("outliers_ring_queries", W.h_count);
    if (W.builds) grid_stats(ctx, "outliers", G);
    ctx->stats.add("outliers_kept", total);
    return total;
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
        const plade_outlier_params p = params_or_default(params, plade_outlier_default_params);
        check_params(n, stride, p);
        OutlierWork &W = work_in<OutlierWork>(ctx->outlier_work);
        float mn[3], mx[3];
        upload_rows(ctx, W.in, rows, n, stride, mn, mx);
        const bool stat = p.mode == PLADE_OUTLIER_STATISTICAL;
        const bool want_values = stat ? mean_dist_out != nullptr : count_out != nullptr;
        const uint32_t total = filter_dev(ctx, W, W.in.p, n, stride, mn, mx, p, want_values, keep_rows_host(W, stride), summary);
        keep_copy_out(ctx, W, n, total, stride, keep_out, kept_index_out, rows_out);
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
        const plade_outlier_params p = params_or_default(params, plade_outlier_default_params);
        const CloudDev &in = cloud->dev;
        check_params(in.n, 6, p);
        OutlierWork &W = work_in<OutlierWork>(ctx->outlier_work);
        resident_result(ctx, out, [&](CloudDev &c) {
            const uint32_t total = filter_dev(ctx, W, in.aos.p, in.n, 6, in.bbmin, in.bbmax, p, false, keep_rows_cloud(c), summary);
            keep_copy_out(ctx, W, in.n, total, 6, keep_out, kept_index_out, nullptr);
            ctx->sync();
            require_kept(total, "plade_cloud_filter_outliers_dev: the filter");
        });
        return PLADE_OK;
    });
}
