// plade_amd/csrc/k_keypoints.hip -- ISS keypoints and the row gather of a descriptor table on gfx950 (semantics: keypoints.h).
//
// Layout
//   grid     the dense row index of TargetGrid, built as k_smooth.hip builds it, with the cell radius_cell(max(rs, rn)) of grid_walk.h:
//            the 27-cell block around a point holds everything closer than either radius, and both walks filter it by their own.
//   scatter  k_iss_scatter: one lane per point in the grid's sorted order (the 64 queries of a wavefront share their runs, as in
//            k_smooth_fit).  A lane walks the nine runs of for_block27 with six fp64 accumulators and a count in registers, solves
//            the eigenvalues (sym3_eigenvalues of pca_eig.h), applies the salient test and writes M, the eigenvalues, c and the
//            saliency by original index -- and the saliency once more in sorted order, so that the second walk reads it from the run
//            it reads the positions from, not through an index gather.  No LDS, no atomics.
//   nms      k_iss_nms: the second walk, over rn: counts m_i and looks for a neighbour that beats the point (the tie rule needs the
//            neighbour's original index: the w of its float4).  No early exit: m_i is an output.
//   list     the flags through exclusive_scan_u32 of prims.h, k_iss_compact writes the ascending indices (the pattern of
//            k_feat_compact).
//   summary  k_iss_sum / k_iss_final, the fixed order of fixed_reduce.h on integers (exact, whatever the order).
//   select   k_feat_select: out row o = in row index[o], 33 floats a row, copied as words.  k_corr_map: the source column of a
//            correspondence list over a selected table back to the original indices.
#include "keypoints.h"
#include "fixed_reduce.h"
#include "grid_walk.h"
#include "pca_eig.h"
#include "prims.h"
#include "voxel.h"

namespace plade {

namespace {

constexpr int ISS_TPB = 256, SUM_TPB = 256;
constexpr double ISS_FLAT = 1e-9;    // l3 > ISS_FLAT * l1: below it the neighbourhood counts as a line or a plane

struct ScatterArgs {
    GridView g;
    uint32_t n;
    float r2;                        // (float)rs * (float)rs
    double g21, g32;
    double *saliency, *eig;          // by original index: n, n x 3
    uint32_t *count;
    double *scatter;                 // n x 6 (or nullptr)
    double *sal_sorted;              // grid order
};

__global__ __launch_bounds__(ISS_TPB) void k_iss_scatter(const ScatterArgs a) {
    const uint32_t s = blockIdx.x * ISS_TPB + threadIdx.x;
    if (s >= a.n) return;
    const float4 q4 = a.g.sorted[s];
    const f3 q(q4.x, q4.y, q4.z);
    const uint32_t self = __float_as_uint(q4.w);
    int cx, cy, cz;
    cell_of(a.g, q, cx, cy, cz);
    const double px = q.x, py = q.y, pz = q.z;
    double m00 = 0.0, m01 = 0.0, m02 = 0.0, m11 = 0.0, m12 = 0.0, m22 = 0.0;
    uint32_t c = 0;
    for (int t = 0; t < 9; ++t) {
        const int dy = t % 3 - 1, dz = t / 3 - 1;
        const uint32_t r = (uint32_t)(cx + 1) + row_base(a.g, cy + dy, cz + dz);   // for_block27's runs, as k_smooth_fit
        const uint32_t j1 = a.g.row_start[r + 3];
        for (uint32_t j = a.g.row_start[r]; j < j1; ++j) {
            const float4 p = a.g.sorted[j];
            if (flann_d2(q, f3(p.x, p.y, p.z)) < a.r2) {
                const double qx = (double)p.x - px, qy = (double)p.y - py, qz = (double)p.z - pz;
                m00 += qx * qx; m01 += qx * qy; m02 += qx * qz;
                m11 += qy * qy; m12 += qy * qz; m22 += qz * qz;
                ++c;
            }
        }
    }
    const double cd = (double)c;     // (c >= 1: the point itself)
    double l1, l2, l3;
    sym3_eigenvalues(m00 / cd, m01 / cd, m02 / cd, m11 / cd, m12 / cd, m22 / cd, l1, l2, l3);
    const bool salient = c >= 3 && l1 > 0.0 && l2 < a.g21 * l1 && l3 < a.g32 * l2 && l3 > ISS_FLAT * l1;
    const double sal = salient ? l3 : 0.0;
    a.saliency[self] = sal;
    a.sal_sorted[s] = sal;
    double *e = a.eig + (size_t)self * 3;
    e[0] = l1; e[1] = l2; e[2] = l3;
    a.count[self] = c;
    if (a.scatter) {
        double *m = a.scatter + (size_t)self * 6;
        m[0] = m00; m[1] = m01; m[2] = m02; m[3] = m11; m[4] = m12; m[5] = m22;
    }
}

struct NmsArgs {
    GridView g;
    uint32_t n;
    float r2;                        // (float)rn * (float)rn
    uint32_t min_nb;
    const double *sal_sorted;        // grid order
    uint32_t *nms_count;             // by original index
    uint32_t *flags;                 // by original index, n + 1 words (the last one, the scan's extra slot, is zeroed by the host)
    uint8_t *keypoint;
};

__global__ __launch_bounds__(ISS_TPB) void k_iss_nms(const NmsArgs a) {
    const uint32_t s = blockIdx.x * ISS_TPB + threadIdx.x;
    if (s >= a.n) return;
    const float4 q4 = a.g.sorted[s];
    const f3 q(q4.x, q4.y, q4.z);
    const uint32_t self = __float_as_uint(q4.w);
    const double sal = a.sal_sorted[s];
    int cx, cy, cz;
    cell_of(a.g, q, cx, cy, cz);
    uint32_t m = 0;
    bool beaten = false;
    for (int t = 0; t < 9; ++t) {
        const int dy = t % 3 - 1, dz = t / 3 - 1;
        const uint32_t r = (uint32_t)(cx + 1) + row_base(a.g, cy + dy, cz + dz);
        const uint32_t j1 = a.g.row_start[r + 3];
        for (uint32_t j = a.g.row_start[r]; j < j1; ++j) {
            const float4 p = a.g.sorted[j];
            if (flann_d2(q, f3(p.x, p.y, p.z)) < a.r2) {
                ++m;
                const double sj = a.sal_sorted[j];
                if (j != s && (sj > sal || (sj == sal && __float_as_uint(p.w) < self))) beaten = true;
            }
        }
    }
    const bool key = sal > 0.0 && m - 1u >= a.min_nb && !beaten;   // (saliency > 0 iff salient: l3 > 1e-9 l1 > 0)
    a.nms_count[self] = m;
    a.flags[self] = key ? 1u : 0u;
    a.keypoint[self] = key ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_iss_compact(const uint32_t *__restrict__ flags, const uint32_t *__restrict__ offs, uint32_t n,
                                                     uint32_t *__restrict__ list) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !flags[i]) return;
    list[offs[i]] = i;
}

// per workgroup: pu[3 b] = its salient points, pu[3 b + 1] = its keypoints, pu[3 b + 2] = its largest c (the order: fixed_reduce.h;
// terms 0 and 1 are sums, term 2 a maximum)
struct SumMaxU64 {
    __device__ __forceinline__ u64 operator()(int k, u64 a, u64 b) const { return k == 2 ? (b > a ? b : a) : a + b; }
};

__global__ __launch_bounds__(SUM_TPB) void k_iss_sum(const double *__restrict__ saliency, const uint8_t *__restrict__ keypoint,
                                                     const uint32_t *__restrict__ count, uint32_t n, u64 *__restrict__ pu) {
    __shared__ u64 s_red[SUM_TPB / 64][3];
    const uint32_t i = blockIdx.x * SUM_TPB + threadIdx.x;
    u64 v[3] = {0, 0, 0};
    if (i < n) {
        v[0] = saliency[i] > 0.0 ? 1 : 0;
        v[1] = keypoint[i] ? 1 : 0;
        v[2] = count[i];
    }
    block_reduce<SUM_TPB>(v, s_red, pu, SumMaxU64());
}
__global__ __launch_bounds__(64) void k_iss_final(const u64 *__restrict__ pu, uint32_t blocks, u64 *__restrict__ ru) {
    u64 v[3];
    final_reduce(pu, blocks, v, SumMaxU64());
    if (threadIdx.x != 0) return;
    ru[0] = v[0]; ru[1] = v[1]; ru[2] = v[2];
}

// out[o * 33 + b] = in[index[o] * 33 + b] as words, one lane per word
__global__ __launch_bounds__(256) void k_feat_select(const uint32_t *__restrict__ in, const uint32_t *__restrict__ index, uint32_t k,
                                                     uint32_t *__restrict__ out) {
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= (size_t)k * FPFH_DIM) return;
    const uint32_t o = (uint32_t)(w / FPFH_DIM), b = (uint32_t)(w - (size_t)o * FPFH_DIM);
    out[w] = in[(size_t)index[o] * FPFH_DIM + b];
}

__global__ __launch_bounds__(256) void k_corr_map(const int32_t *__restrict__ corr, uint32_t m, const uint32_t *__restrict__ index,
                                                  int32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    out[2 * (size_t)i] = (int32_t)index[corr[2 * (size_t)i]];
    out[2 * (size_t)i + 1] = corr[2 * (size_t)i + 1];
}

}  // namespace

struct IssWork {
    TargetGrid grid;
    DBuf<float> in;                  // the host-pointer entry point's device copy (grow-only)
    DBuf<double> saliency, eig, scatter, sal_sorted;
    DBuf<uint32_t> count, nms_count, flags, offs, list;
    DBuf<uint8_t> keypoint;
    DBuf<u64> partial, res;
    DBuf<uint32_t> sel_index;        // plade_features_select: the index list on the device
    DBuf<int32_t> corr;              // corr_map_source_dev
    u64 h_u[3] = {0, 0, 0};
    uint32_t h_total = 0;
    EventSpans<4> spans;             // grid, scatter, nms (+ list and summary)
};

namespace {

struct Outputs {
    uint8_t *keypoint;
    uint32_t *index;
    uint64_t cap;
    uint64_t *n_keypoints;
    double *saliency, *eig;
    uint32_t *count, *nms_count;
    double *scatter;
};

void check_params(uint32_t n, uint32_t stride, const plade_iss_params &p) {
    PLADE_REQUIRE(n >= 1, PLADE_EINVAL, "keypoints_iss: the cloud is empty (n = 0)");
    PLADE_REQUIRE(stride >= 3, PLADE_EINVAL, "keypoints_iss: stride must be >= 3 floats");
    // r2 a normal fp32 number, as smooth_cloud: at 0 no point would be its own neighbour
    PLADE_REQUIRE(radius_ok(p.salient_radius, true), PLADE_EINVAL,
                  "keypoints_iss: salient_radius must be finite and > 0, and its fp32 square finite and not below FLT_MIN");
    PLADE_REQUIRE(p.non_max_radius == 0.0 || radius_ok(p.non_max_radius, true), PLADE_EINVAL,
                  "keypoints_iss: non_max_radius must be 0 (= salient_radius) or finite and > 0, its fp32 square finite and not below FLT_MIN");
    PLADE_REQUIRE(std::isfinite(p.gamma21) && p.gamma21 > 0.0 && p.gamma21 <= 1.0 && std::isfinite(p.gamma32) && p.gamma32 > 0.0 &&
                      p.gamma32 <= 1.0,
                  PLADE_EINVAL, "keypoints_iss: gamma21 and gamma32 must be finite and in (0, 1]");
    PLADE_REQUIRE(p.min_neighbours >= 1, PLADE_EINVAL, "keypoints_iss: min_neighbours must be >= 1");
}

// The detector on a device cloud of `stride` floats per point with a known bounding box: leaves every per-point array and the list in
// W, copies the wanted ones out, waits, fills the summary and the stats.  Returns PLADE_ECAP when the list did not fit.
int iss_dev(plade_ctx *ctx, IssWork &W, const float *d_rows, uint32_t n, uint32_t stride, const float bbmin[3], const float bbmax[3],
            const plade_iss_params &p, const Outputs &out, plade_iss_summary *summary) {
    W.spans.mark(ctx, 0);
    const float rs = (float)p.salient_radius, rn = p.non_max_radius == 0.0 ? rs : (float)p.non_max_radius;
    TargetGrid &G = W.grid;
    G.build(ctx, d_rows, n, stride, radius_cell((double)std::max(rs, rn), bbmin, bbmax), bbmin, bbmax, true);
    const GridView g = view_of(G, "keypoints_iss");
    W.spans.mark(ctx, 1);
    ScatterArgs a;
    memset(&a, 0, sizeof(a));
    a.g = g; a.n = n; a.r2 = rs * rs; a.g21 = p.gamma21; a.g32 = p.gamma32;
    a.saliency = W.saliency.ensure(n);
    a.eig = W.eig.ensure((size_t)n * 3);
    a.count = W.count.ensure(n);
    a.scatter = out.scatter ? W.scatter.ensure((size_t)n * 6) : nullptr;
    a.sal_sorted = W.sal_sorted.ensure(n);
    hipLaunchKernelGGL(k_iss_scatter, dim3(cdiv(n, ISS_TPB)), dim3(ISS_TPB), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    W.spans.mark(ctx, 2);
    NmsArgs b;
    memset(&b, 0, sizeof(b));
    b.g = g; b.n = n; b.r2 = rn * rn; b.min_nb = (uint32_t)p.min_neighbours;
    b.sal_sorted = a.sal_sorted;
    b.nms_count = W.nms_count.ensure(n);
    b.flags = W.flags.ensure((size_t)n + 1);
    b.keypoint = W.keypoint.ensure((size_t)n + 4);
    HIP_TRY(hipMemsetAsync(b.flags + n, 0, 4, ctx->stream));
    hipLaunchKernelGGL(k_iss_nms, dim3(cdiv(n, ISS_TPB)), dim3(ISS_TPB), 0, ctx->stream, b);
    HIP_TRY(hipGetLastError());
    uint32_t *d_offs = W.offs.ensure((size_t)n + 1), *d_list = W.list.ensure(n);
    exclusive_scan_u32(ctx, b.flags, d_offs, (size_t)n + 1);
    hipLaunchKernelGGL(k_iss_compact, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, (const uint32_t *)b.flags, (const uint32_t *)d_offs, n,
                       d_list);
    const uint32_t blocks = cdiv(n, SUM_TPB);
    u64 *d_pu = W.partial.ensure((size_t)3 * blocks), *d_ru = W.res.ensure(4);
    hipLaunchKernelGGL(k_iss_sum, dim3(blocks), dim3(SUM_TPB), 0, ctx->stream, (const double *)a.saliency, (const uint8_t *)b.keypoint,
                       (const uint32_t *)a.count, n, d_pu);
    hipLaunchKernelGGL(k_iss_final, dim3(1), dim3(64), 0, ctx->stream, (const u64 *)d_pu, blocks, d_ru);
    HIP_TRY(hipGetLastError());
    W.spans.mark(ctx, 3);
    HIP_TRY(hipMemcpyAsync(W.h_u, d_ru, sizeof(W.h_u), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(&W.h_total, d_offs + n, 4, hipMemcpyDeviceToHost, ctx->stream));
    if (out.keypoint) HIP_TRY(hipMemcpyAsync(out.keypoint, b.keypoint, n, hipMemcpyDeviceToHost, ctx->stream));
    if (out.saliency) HIP_TRY(hipMemcpyAsync(out.saliency, a.saliency, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (out.eig) HIP_TRY(hipMemcpyAsync(out.eig, a.eig, (size_t)n * 24, hipMemcpyDeviceToHost, ctx->stream));
    if (out.count) HIP_TRY(hipMemcpyAsync(out.count, a.count, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (out.nms_count) HIP_TRY(hipMemcpyAsync(out.nms_count, b.nms_count, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (out.scatter) HIP_TRY(hipMemcpyAsync(out.scatter, a.scatter, (size_t)n * 48, hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    const uint64_t total = W.h_total;
    if (out.n_keypoints) *out.n_keypoints = total;
    const uint64_t w = std::min<uint64_t>(total, out.cap);
    if (out.index && w) {
        HIP_TRY(hipMemcpyAsync(out.index, d_list, (size_t)w * 4, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
    }
    if (summary) {
        summary->n = n;
        summary->salient = W.h_u[0];
        summary->keypoints = W.h_u[1];
        summary->max_count = (uint32_t)W.h_u[2];
        summary->reserved = 0;
    }
    W.spans.collect();
    ctx->stats.clear();
    ctx->stats.add("iss_grid_s", W.spans.seconds(0));
    ctx->stats.add("iss_scatter_s", W.spans.seconds(1));
    ctx->stats.add("iss_nms_s", W.spans.seconds(2));
    ctx->stats.add("iss_salient", (double)W.h_u[0]);
    ctx->stats.add("iss_keypoints", (double)W.h_u[1]);
    grid_stats(ctx, "iss", W.grid);
    return (out.index && total > out.cap) ? PLADE_ECAP : PLADE_OK;
}

}  // namespace

// ---- the steps as plade_register_keypoints chains them (k_corr_pose.hip) ------------------------------------------------------------
const uint32_t *iss_list_dev(plade_ctx *ctx, const float *d_rows, uint32_t n, uint32_t stride, const float bbmin[3], const float bbmax[3],
                             const plade_iss_params &p, plade_iss_summary *summary, uint32_t *n_keypoints) {
    check_params(n, stride, p);
    IssWork &W = work_in<IssWork>(ctx->iss_work);
    const Outputs none = {nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    iss_dev(ctx, W, d_rows, n, stride, bbmin, bbmax, p, none, summary);
    *n_keypoints = W.h_total;
    return W.list.p;
}

void features_select_dev(plade_ctx *ctx, const plade_features &in, const uint32_t *d_index, uint32_t k, plade_features &out) {
    out.n = k;
    out.desc.ensure((size_t)k * FPFH_DIM + 4);
    hipLaunchKernelGGL(k_feat_select, dim3(cdiv((size_t)k * FPFH_DIM, 256)), dim3(256), 0, ctx->stream,
                       reinterpret_cast<const uint32_t *>(in.desc.p), d_index, k, reinterpret_cast<uint32_t *>(out.desc.p));
    HIP_TRY(hipGetLastError());
}

const int32_t *corr_map_source_dev(plade_ctx *ctx, const int32_t *d_corr, uint64_t m, const uint32_t *d_index) {
    IssWork &W = work_in<IssWork>(ctx->iss_work);
    int32_t *d_out = W.corr.ensure((size_t)m * 2 + 2);
    if (m) {
        hipLaunchKernelGGL(k_corr_map, dim3(cdiv(m, 256)), dim3(256), 0, ctx->stream, d_corr, (uint32_t)m, d_index, d_out);
        HIP_TRY(hipGetLastError());
    }
    return d_out;
}

}  // namespace plade

using namespace plade;

// ---- C ABI (include/plade_hip.h) ---------------------------------------------------------------------------------------------
extern "C" void plade_iss_default_params(plade_iss_params *p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->salient_radius = 0.0;
    p->non_max_radius = 0.0;
    p->gamma21 = 0.975;
    p->gamma32 = 0.975;
    p->min_neighbours = 5;
}

extern "C" int plade_cloud_keypoints_iss(plade_ctx *ctx, const float *rows, uint32_t n, uint32_t stride, const plade_iss_params *params,
                                         uint8_t *keypoint_out, uint32_t *index_out, uint64_t cap, uint64_t *n_keypoints,
                                         double *saliency_out, double *eigenvalues_out, uint32_t *count_out, uint32_t *nms_count_out,
                                         double *scatter_out, plade_iss_summary *summary) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(rows && params && summary, PLADE_EINVAL, "plade_cloud_keypoints_iss: NULL cloud, params or summary");
        check_params(n, stride, *params);
        IssWork &W = work_in<IssWork>(ctx->iss_work);
        float mn[3], mx[3];
        upload_rows(ctx, W.in, rows, n, stride, mn, mx);                 // (the bounding box checks the coordinates)
        const Outputs out = {keypoint_out, index_out, cap, n_keypoints, saliency_out, eigenvalues_out, count_out, nms_count_out, scatter_out};
        return iss_dev(ctx, W, W.in.p, n, stride, mn, mx, *params, out, summary);
    });
}

extern "C" int plade_cloud_keypoints_iss_dev(plade_ctx *ctx, plade_cloud *cloud, const plade_iss_params *params, uint8_t *keypoint_out,
                                             uint32_t *index_out, uint64_t cap, uint64_t *n_keypoints, double *saliency_out,
                                             double *eigenvalues_out, uint32_t *count_out, uint32_t *nms_count_out, double *scatter_out,
                                             plade_iss_summary *summary) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(cloud && params && summary, PLADE_EINVAL, "plade_cloud_keypoints_iss_dev: NULL cloud, params or summary");
        const CloudDev &c = cloud->dev;
        check_params(c.n, 6, *params);
        const Outputs out = {keypoint_out, index_out, cap, n_keypoints, saliency_out, eigenvalues_out, count_out, nms_count_out, scatter_out};
        return iss_dev(ctx, work_in<IssWork>(ctx->iss_work), c.aos.p, c.n, 6, c.bbmin, c.bbmax, *params, out, summary);
    });
}

extern "C" int plade_features_select(plade_ctx *ctx, plade_features *features, const uint32_t *index, uint32_t k, plade_features **out) {
    return guarded(ctx, [&]() -> int {
        if (out) *out = nullptr;
        PLADE_REQUIRE(features && index && out, PLADE_EINVAL, "plade_features_select: NULL table, index list or output");
        PLADE_REQUIRE(k >= 1, PLADE_EINVAL, "plade_features_select: the index list is empty (k = 0)");
        for (uint32_t o = 0; o < k; ++o)
            PLADE_REQUIRE(index[o] < features->n, PLADE_EINVAL,
                          "plade_features_select: index " + std::to_string(o) + " names a row that does not exist");
        IssWork &W = work_in<IssWork>(ctx->iss_work);
        uint32_t *d_index = W.sel_index.ensure(k);
        HIP_TRY(hipMemcpyAsync(d_index, index, (size_t)k * 4, hipMemcpyHostToDevice, ctx->stream));
        plade_features *f = new plade_features;
        try {
            features_select_dev(ctx, *features, d_index, k, *f);
            ctx->sync();
        } catch (...) { delete f; throw; }
        *out = f;
        return PLADE_OK;
    });
}
