// plade_amd/csrc/k_distances.hip -- exact bounded nearest-neighbour distances of a source against a target on gfx950
// (semantics: distances.h).
//
// Layout
//   grid    one dense row index of TargetGrid over the target, walked with the pieces of grid_walk.h.  The cell follows the
//           target's density (about five points per occupied cell of a surface), or d plus a margin when d is smaller: then one
//           27-cell block holds every target point closer than d.  The cell never grows to a large d -- a d-sized cell would
//           hand each probe thousands of candidates (the ICP's coarse stage).
//   order   k_distances_keys forms p' and its padded cell id in that grid; the radix sort orders the probes by cell, so the 64
//           lanes of a wavefront probe neighbouring cells and share their candidate runs.  Outputs go back by original index.
//   lane    k_distances_lane: one lane per probe scans its 27-cell block for the (d2, j) argmin key.  The probe is finished when
//           that key is closer than the block's outside, or the outside is at least d away (both less a margin for the fp32 cell
//           assignment).  A probe at least d from the target's bounding box ends before any load of the grid.  The rest is
//           appended to a compacted list (one atomic per wavefront).
//   ring    k_distances_ring: one wavefront per listed probe grows the block as k_normals_ring does (ring_step); the 64 keys of a
//           batch are reduced by a wave min.  It stops at the first block whose outside is at least min(best, d) away, or that
//           covers the grid.
//   summary k_distances_summary: one lane per original index forms the plane residual in fp64 and the six summary terms, reduced
//           per workgroup and then by k_distances_final in the fixed order of fixed_reduce.h.  No fp64 atomics.
#include "distances.h"
#include "fixed_reduce.h"
#include "grid_walk.h"
#include "prims.h"
#include "voxel.h"

namespace plade {

namespace {

constexpr int KEY_TPB = 256, LANE_TPB = 256, SUM_TPB = 256, RING_WAVES = 4;
constexpr int SUM_TERMS = 6;   // count, sum d2, sum sqrt(d2), max sqrt(d2), plane_count, sum r^2

struct DistArgs {
    GridView g;                      // over the target
    double margin;                   // grid_margin
    double bmn[3], bmx[3];           // the target's bounding box
    float d2;                        // (float)d * (float)d
    const float4 *probe;             // n probes in the original order: p', bit-cast original index
    const uint32_t *order;           // the original indices in cell order
    uint32_t n;
    int32_t *idx;
    float *dd;
    uint32_t *fail, *fail_count;
};

// margin of one probe: the grid's (1 % of a cell, ulps of the target's coordinates) and a few ulps of the probe's own
__device__ __forceinline__ double margin_of(const DistArgs &a, f3 q) {
    return a.margin + 1e-6 * (double)fmaxf(fabsf(q.x), fmaxf(fabsf(q.y), fabsf(q.z)));
}

// true: the best key so far is final -- it is closer than every point outside the block, or every point outside the block is
// at least d away (then a correspondence can only come from inside it)
__device__ __forceinline__ bool finished(const DistArgs &a, float best, double reach) {
    if (reach == INFINITY) return true;
    if (!(reach > 0.0)) return false;
    const float R2 = (float)(reach * reach);
    return best < R2 || a.d2 <= R2;      // (best NaN: no key yet)
}

__device__ __forceinline__ void store(const DistArgs &a, uint32_t orig, u64 best) {
    const float bd = key_d(best);
    const bool hit = best != EMPTY && bd < a.d2;
    a.idx[orig] = hit ? (int32_t)(uint32_t)best : -1;
    a.dd[orig] = hit ? bd : INFINITY;
}

// p' and its padded cell id in the target grid (k_cell_ids' formula, clamped: probes outside the grid sort to its edge)
__global__ __launch_bounds__(KEY_TPB) void k_distances_keys(const float *__restrict__ src, uint32_t n, uint32_t stride, const float *__restrict__ Tf,
                                                            DistArgs a, uint32_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                            float4 *__restrict__ probe) {
    const uint32_t i = blockIdx.x * KEY_TPB + threadIdx.x;
    if (i >= n) return;
    const float *s = src + (size_t)i * stride;
    const float x = s[0], y = s[1], z = s[2];
    const f3 q(((Tf[0] * x + Tf[1] * y) + Tf[2] * z) + Tf[3], ((Tf[4] * x + Tf[5] * y) + Tf[6] * z) + Tf[7],
               ((Tf[8] * x + Tf[9] * y) + Tf[10] * z) + Tf[11]);
    int cx, cy, cz;
    cell_of(a.g, q, cx, cy, cz);
    keys[i] = (uint32_t)(cx + 2) + row_base(a.g, cy, cz);
    vals[i] = i;
    probe[i] = make_float4(q.x, q.y, q.z, __uint_as_float(i));
}

__global__ __launch_bounds__(LANE_TPB) void k_distances_lane(const DistArgs a) {
    const uint32_t s = blockIdx.x * LANE_TPB + threadIdx.x;
    bool fail = false;
    uint32_t orig = 0;
    if (s < a.n) {
        orig = a.order[s];
        const float4 q4 = a.probe[orig];
        const f3 q(q4.x, q4.y, q4.z);
        const double mg = margin_of(a, q);
        // gap to the target's bounding box: a probe at least d away has no correspondence and loads nothing of the grid
        double g2 = 0.0;
        const double qv[3] = {q.x, q.y, q.z};
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const double g = fmax(fmax(a.bmn[t] - qv[t], qv[t] - a.bmx[t]), 0.0);
            g2 += g * g;
        }
        const double gap = sqrt(g2) - mg;
        u64 best = EMPTY;
        if (!(gap > 0.0 && a.d2 <= (float)(gap * gap))) {
            int cx, cy, cz;
            cell_of(a.g, q, cx, cy, cz);
            for_block27(a.g, cx, cy, cz, [&](uint32_t j0, uint32_t j1) {
                for (uint32_t j = j0; j < j1; ++j) {
                    const float4 p = a.g.sorted[j];
                    const u64 key = make_key(flann_d2(q, f3(p.x, p.y, p.z)), __float_as_uint(p.w));
                    best = key < best ? key : best;
                }
            });
            fail = !finished(a, key_d(best), block_reach(a.g, q, cx, cy, cz, 1, mg));
        }
        if (!fail) store(a, orig, best);
    }
    fail_append(fail, orig, a.fail, a.fail_count);   // to the list of the ring pass
}

// One wavefront per probe of the list (persistent workgroups; the list's length stays on the device): the growing blocks of
// ring_step, each batch reduced by a wave min of (d2, j) keys.
__global__ __launch_bounds__(64 * RING_WAVES) void k_distances_ring(const DistArgs a) {
    const int lane = (int)(threadIdx.x & 63u), wv = (int)(threadIdx.x >> 6);
    const uint32_t total = *a.fail_count, stride_w = gridDim.x * RING_WAVES;
    for (uint32_t i = blockIdx.x * RING_WAVES + (uint32_t)wv; i < total; i += stride_w) {
        const uint32_t orig = a.fail[i];
        const float4 q4 = a.probe[orig];
        const f3 q(q4.x, q4.y, q4.z);
        const double mg = margin_of(a, q);
        int cx, cy, cz;
        cell_of(a.g, q, cx, cy, cz);
        u64 best = EMPTY;
        for (int rin = -1, rout = 1;; rin = rout, rout += max(1, rout / 2)) {
            ring_step(a.g, cx, cy, cz, rin, rout, lane, [&](bool valid, float4 p) {
                const u64 m = wave_min(valid ? make_key(flann_d2(q, f3(p.x, p.y, p.z)), __float_as_uint(p.w)) : EMPTY);
                best = m < best ? m : best;
            });
            if (finished(a, key_d(best), block_reach(a.g, q, cx, cy, cz, rout, mg))) break;
        }
        if (lane == 0) store(a, orig, best);
    }
}

struct SumArgs {
    const int32_t *idx;
    const float *dd;
    const float *tgt;                // n_t x 6: the normals are gathered by j
    const float *src;                // `stride` floats per point
    uint32_t stride, n;
    double T[12];                    // double(T16), rows 0..2
    float *plane;                    // n or nullptr
    double *partial;                 // gridDim.x x SUM_TERMS
};

struct SumMax3 {                     // term 3 is a maximum, the others are sums
    __device__ __forceinline__ double operator()(int k, double a, double b) const { return k == 3 ? fmax(a, b) : a + b; }
};

__global__ __launch_bounds__(SUM_TPB) void k_distances_summary(const SumArgs a) {
    __shared__ double s_red[SUM_TPB / 64][SUM_TERMS];
    const uint32_t i = blockIdx.x * SUM_TPB + threadIdx.x;
    double m[SUM_TERMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (i < a.n) {
        const int32_t j = a.idx[i];
        double r = NAN;
        if (j >= 0) {
            const double d2 = (double)a.dd[i], dist = sqrt(d2);
            m[0] = 1.0; m[1] = d2; m[2] = dist; m[3] = dist;
            const float *t = a.tgt + (size_t)j * 6;
            const double n0 = t[3], n1 = t[4], n2 = t[5];
            if (isfinite(n0) && isfinite(n1) && isfinite(n2)) {
                const float *s = a.src + (size_t)i * a.stride;
                const double X = s[0], Y = s[1], Z = s[2];
                const double *T = a.T;
                const double p0 = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[3];
                const double p1 = ((T[4] * X + T[5] * Y) + T[6] * Z) + T[7];
                const double p2 = ((T[8] * X + T[9] * Y) + T[10] * Z) + T[11];
                r = (n0 * (p0 - (double)t[0]) + n1 * (p1 - (double)t[1])) + n2 * (p2 - (double)t[2]);
                m[4] = 1.0; m[5] = r * r;
            }
        }
        if (a.plane) a.plane[i] = (float)r;
    }
    block_reduce<SUM_TPB>(m, s_red, a.partial, SumMax3());
}

__global__ __launch_bounds__(64) void k_distances_final(const double *__restrict__ partial, uint32_t blocks, double *__restrict__ out) {
    double m[SUM_TERMS];
    final_reduce(partial, blocks, m, SumMax3());
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < SUM_TERMS; ++k) out[k] = m[k];
}

}  // namespace

struct DistWork {
    TargetGrid grid;
    DBuf<float> in_t, in_s, Tf;      // the host-pointer entry points' device copies (grow-only); the fp32 transform
    DBuf<uint32_t> keys, keys2, vals, vals2, fail, count;
    DBuf<float4> probe;
    DBuf<int32_t> idx;
    DBuf<float> dd, plane;
    DBuf<double> partial, out;
    EventSpans<6> spans;             // grid, sort, lane, ring, summary
    float h_T[16];                   // the upload's source (kept until the call's sync)
    double h_out[SUM_TERMS];
    uint32_t h_count = 0;
};

namespace {

const float kIdentity[16] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};

void check_args(const float *T16, float max_dist) {
    for (int k = 0; k < 16; ++k) PLADE_REQUIRE(std::isfinite(T16[k]), PLADE_EINVAL, "cloud_distances: T must be finite");
    PLADE_REQUIRE(std::isfinite(max_dist) && max_dist > 0.f, PLADE_EINVAL, "cloud_distances: max_dist must be finite and > 0");
}

// the distances on device clouds: target n_t x 6, source `stride` floats per point, the target's bounding box known
void distances_dev(plade_ctx *ctx, DistWork &W, const float *d_tgt, uint32_t n_t, const float tmn[3], const float tmx[3],
                   const float *d_src, uint32_t n_s, uint32_t stride, const float *T16, float max_dist, int32_t *idx_out,
                   float *d2_out, float *plane_out, plade_distance_summary *summary) {
    W.spans.mark(ctx, 0);
    // cell: ~5 points per occupied cell of a surface spread over the faces of the target's box (k_normals' estimate at k = 8); a
    // d of less than that takes the radius cell of d (radius_cell), so one 27-cell block holds every point within d
    const double ex = std::max(1e-9, (double)tmx[0] - tmn[0]), ey = std::max(1e-9, (double)tmx[1] - tmn[1]),
                 ez = std::max(1e-9, (double)tmx[2] - tmn[2]);
    const double area = 2 * (ex * ey + ey * ez + ex * ez);
    const double dense_cell = 1.5 * std::sqrt(8.0 * area / (M_PI * (double)n_t));
    TargetGrid &G = W.grid;
    G.build(ctx, d_tgt, n_t, 6, std::min((float)dense_cell, radius_cell((double)max_dist, tmn, tmx)), tmn, tmx, true);
    W.spans.mark(ctx, 1);

    DistArgs a;
    memset(&a, 0, sizeof(a));
    a.g = view_of(G, "cloud_distances");
    a.margin = grid_margin(a.g, tmn, tmx);
    for (int t = 0; t < 3; ++t) { a.bmn[t] = tmn[t]; a.bmx[t] = tmx[t]; }
    a.d2 = max_dist * max_dist;
    a.n = n_s;
    a.probe = W.probe.ensure(n_s);
    a.idx = W.idx.ensure(n_s); a.dd = W.dd.ensure(n_s);
    a.fail = W.fail.ensure(n_s); a.fail_count = W.count.ensure(4);
    memcpy(W.h_T, T16, sizeof(W.h_T));
    HIP_TRY(hipMemcpyAsync(W.Tf.ensure(16), W.h_T, sizeof(W.h_T), hipMemcpyHostToDevice, ctx->stream));
    W.keys.ensure(n_s); W.keys2.ensure(n_s); W.vals.ensure(n_s); W.vals2.ensure(n_s);
    hipLaunchKernelGGL(k_distances_keys, dim3(cdiv(n_s, KEY_TPB)), dim3(KEY_TPB), 0, ctx->stream, d_src, n_s, stride, W.Tf.p, a, W.keys.p,
                       W.vals.p, W.probe.p);
    HIP_TRY(hipGetLastError());
    int bits = 1;
    while (((size_t)1 << bits) < G.ncells) ++bits;
    sort_pairs_u32(ctx, W.keys.p, W.keys2.p, W.vals.p, W.vals2.p, n_s, bits);
    a.order = W.vals2.p;
    ctx->fill_async(a.fail_count, 0, 4);
    W.spans.mark(ctx, 2);
    hipLaunchKernelGGL(k_distances_lane, dim3(cdiv(n_s, LANE_TPB)), dim3(LANE_TPB), 0, ctx->stream, a);
    W.spans.mark(ctx, 3);
    hipLaunchKernelGGL(k_distances_ring, dim3(std::min(cdiv(n_s, RING_WAVES), 2048u)), dim3(64 * RING_WAVES), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    W.spans.mark(ctx, 4);

    SumArgs sa;
    memset(&sa, 0, sizeof(sa));
    const uint32_t blocks = cdiv(n_s, SUM_TPB);
    sa.idx = a.idx; sa.dd = a.dd; sa.tgt = d_tgt; sa.src = d_src; sa.stride = stride; sa.n = n_s;
    for (int k = 0; k < 12; ++k) sa.T[k] = (double)T16[k];
    sa.plane = plane_out ? W.plane.ensure(n_s) : nullptr;
    sa.partial = W.partial.ensure((size_t)blocks * SUM_TERMS);
    double *d_out = W.out.ensure(SUM_TERMS);
    hipLaunchKernelGGL(k_distances_summary, dim3(blocks), dim3(SUM_TPB), 0, ctx->stream, sa);
    hipLaunchKernelGGL(k_distances_final, dim3(1), dim3(64), 0, ctx->stream, sa.partial, blocks, d_out);
    HIP_TRY(hipGetLastError());
    W.spans.mark(ctx, 5);
    HIP_TRY(hipMemcpyAsync(W.h_out, d_out, sizeof(W.h_out), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(&W.h_count, a.fail_count, 4, hipMemcpyDeviceToHost, ctx->stream));
    if (idx_out) HIP_TRY(hipMemcpyAsync(idx_out, a.idx, (size_t)n_s * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (d2_out) HIP_TRY(hipMemcpyAsync(d2_out, a.dd, (size_t)n_s * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (plane_out) HIP_TRY(hipMemcpyAsync(plane_out, sa.plane, (size_t)n_s * 4, hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();

    const double *o = W.h_out;
    plade_distance_summary r;
    memset(&r, 0, sizeof(r));
    r.n = n_s;
    r.count = (uint64_t)o[0];
    r.plane_count = (uint64_t)o[4];
    r.fitness = (double)r.count / (double)r.n;
    r.rmse = r.count ? std::sqrt(o[1] / (double)r.count) : NAN;
    r.mean = r.count ? o[2] / (double)r.count : NAN;
    r.max = r.count ? o[3] : NAN;
    r.plane_rmse = r.plane_count ? std::sqrt(o[5] / (double)r.plane_count) : NAN;
    *summary = r;

    W.spans.collect();
    ctx->stats.clear();
    ctx->stats.add("distances_grid_s", W.spans.seconds(0));
    ctx->stats.add("distances_sort_s", W.spans.seconds(1));
    ctx->stats.add("distances_search_s", W.spans.seconds(2) + W.spans.seconds(3));
    ctx->stats.add("distances_lane_s", W.spans.seconds(2));
    ctx->stats.add("distances_ring_s", W.spans.seconds(3));
    ctx->stats.add("distances_summary_s", W.spans.seconds(4));
    ctx->stats.add("distances_ring_queries", W.h_count);
    grid_stats(ctx, "distances", G);
}

}  // namespace
}  // namespace plade

using namespace plade;

// ---- C ABI (include/plade_hip.h) ---------------------------------------------------------------------------------------------
extern "C" int plade_cloud_distances(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t, const float *src_xyz, uint32_t n_s,
                                     uint32_t stride, const float *T16, float max_dist, int32_t *idx_out, float *d2_out,
                                     float *plane_out, plade_distance_summary *summary) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(tgt_pos_nrm && src_xyz && summary, PLADE_EINVAL, "plade_cloud_distances: NULL cloud or summary");
        PLADE_REQUIRE(n_t >= 1 && n_s >= 1, PLADE_EINVAL, "plade_cloud_distances: empty cloud (n = 0)");
        PLADE_REQUIRE(stride >= 3, PLADE_EINVAL, "plade_cloud_distances: stride must be >= 3 floats");
        const float *T = T16 ? T16 : kIdentity;
        check_args(T, max_dist);
        DistWork &W = work_in<DistWork>(ctx->dist_work);
        float tmn[3], tmx[3], smn[3], smx[3];
        upload_rows(ctx, W.in_t, tgt_pos_nrm, n_t, 6, tmn, tmx);
        upload_rows(ctx, W.in_s, src_xyz, n_s, stride, smn, smx);
        distances_dev(ctx, W, W.in_t.p, n_t, tmn, tmx, W.in_s.p, n_s, stride, T, max_dist, idx_out, d2_out, plane_out, summary);
        return PLADE_OK;
    });
}

extern "C" int plade_cloud_distances_dev(plade_ctx *ctx, plade_cloud *tgt, plade_cloud *src, const float *T16, float max_dist,
                                         int32_t *idx_out, float *d2_out, float *plane_out, plade_distance_summary *summary) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(tgt && src && summary, PLADE_EINVAL, "plade_cloud_distances_dev: NULL cloud or summary");
        PLADE_REQUIRE(tgt->dev.n >= 1 && src->dev.n >= 1, PLADE_EINVAL, "plade_cloud_distances_dev: empty cloud (n = 0)");
        const float *T = T16 ? T16 : kIdentity;
        check_args(T, max_dist);
        DistWork &W = work_in<DistWork>(ctx->dist_work);
        const CloudDev &t = tgt->dev, &s = src->dev;
        distances_dev(ctx, W, t.aos.p, t.n, t.bbmin, t.bbmax, s.aos.p, s.n, 6, T, max_dist, idx_out, d2_out, plane_out, summary);
        return PLADE_OK;
    });
}
