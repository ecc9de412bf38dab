// plade_amd/csrc/k_scales.hip -- multi-scale normals and dimensionality features on gfx950 (semantics: scales.h).
//
// Layout
//   grid     the dense row index of TargetGrid at radius_cell(the largest radius): ONE grid and ONE walk for all S scales.
//   queries  all n points, or a list: the listed points are marked by original index (k_scales_mark: index -> query slot), the
//            sorted positions that hold a marked point are flagged (k_scales_flag) and compacted with the scan of compact_flags, so
//            that the walk's wavefronts stay full and the 64 queries of a wavefront are neighbours in the grid's order.
//   walk     k_scales_walk<CAP>: one lane per query in the grid's sorted order, as k_smooth_fit.  A lane walks the nine runs of
//            for_block27 with nine fp64 accumulators and a count PER SCALE, all statically indexed (CAP = 2, 4 or 8 scales, so that
//            a two-scale call keeps the occupancy an eight-scale call cannot have).  d is computed once per candidate; the nine
//            terms once per candidate closer than the largest radius; scale s adds them under d < r2_s.  It writes the moments and
//            counts by query slot.  No LDS, no atomics.
//   fit      k_scales_fit: one lane per query slot, a run-time loop over the scales that reads the moments (76 B per query and
//            scale) and solves each with sym3_eigenvalues and pca_eig; the choice, the orientation, the outputs and the per-workgroup
//            partials of the summary.  Kept out of the walk: CAP unrolled solves next to the walk's accumulators would cost the walk
//            its occupancy.
//   summary  k_scales_final, in the fixed order of fixed_reduce.h: fitted queries, the histogram of the chosen scale, the largest count.
#include "scales.h"
#include "cloud_tool.h"
#include "fixed_reduce.h"
#include "grid_walk.h"
#include "pca_eig.h"
#include "voxel.h"

namespace plade {

namespace {

constexpr int WALK_TPB = 256, FIT_TPB = 256, MARK_TPB = 256;
constexpr uint32_t NO_SLOT = ~0u;
constexpr int SUM_TERMS = 2 + SCALES_MAX;   // fitted, chosen_hist[8], the largest count

// slot[query_index[t]] = t (slot: n words, NO_SLOT before)
__global__ __launch_bounds__(MARK_TPB) void k_scales_mark(const uint32_t *__restrict__ qidx, uint32_t k, uint32_t *__restrict__ slot) {
    const uint32_t t = blockIdx.x * MARK_TPB + threadIdx.x;
    if (t < k) slot[qidx[t]] = t;
}
// flags[s] = the point at sorted position s is a query
__global__ __launch_bounds__(MARK_TPB) void k_scales_flag(const float4 *__restrict__ sorted, const uint32_t *__restrict__ slot, uint32_t n,
                                                          uint32_t *__restrict__ flags) {
    const uint32_t s = blockIdx.x * MARK_TPB + threadIdx.x;
    if (s < n) flags[s] = slot[__float_as_uint(sorted[s].w)] != NO_SLOT ? 1u : 0u;
}

struct WalkArgs {
    GridView g;
    uint32_t k, S;                   // queries, scales
    const uint32_t *pos;             // the sorted positions of the queries, ascending (nullptr: every position, k = n)
    const uint32_t *slot;            // original index -> query slot (nullptr: the index itself)
    float r2[SCALES_MAX];            // (float)r_s * (float)r_s, ascending; -1 behind the last one (d < -1 never holds)
    float r2max;                     // r2[S - 1]
    double *moments;                 // k x S x 9
    uint32_t *count;                 // k x S
};

template <int CAP>
__global__ __launch_bounds__(WALK_TPB) void k_scales_walk(const WalkArgs a) {
    const uint32_t t = blockIdx.x * WALK_TPB + threadIdx.x;
    if (t >= a.k) return;
    const uint32_t s = a.pos ? a.pos[t] : t;
    const float4 q4 = a.g.sorted[s];
    const f3 q(q4.x, q4.y, q4.z);
    const uint32_t self = __float_as_uint(q4.w);
    int cx, cy, cz;
    cell_of(a.g, q, cx, cy, cz);
    const double px = q.x, py = q.y, pz = q.z;
    double m[CAP][9];
    uint32_t c[CAP];
#pragma unroll
    for (int u = 0; u < CAP; ++u) {
        c[u] = 0;
#pragma unroll
        for (int e = 0; e < 9; ++e) m[u][e] = 0.0;
    }
    for (int w = 0; w < 9; ++w) {
        const int dy = w % 3 - 1, dz = w / 3 - 1;
        const uint32_t r = (uint32_t)(cx + 1) + row_base(a.g, cy + dy, cz + dz);   // for_block27's runs, as k_smooth_fit
        const uint32_t j1 = a.g.row_start[r + 3];
        for (uint32_t j = a.g.row_start[r]; j < j1; ++j) {
            const float4 p = a.g.sorted[j];
            const float d = flann_d2(q, f3(p.x, p.y, p.z));
            if (d < a.r2max) {
                const double qx = (double)p.x - px, qy = (double)p.y - py, qz = (double)p.z - pz;
                const double term[9] = {qx, qy, qz, qx * qx, qx * qy, qx * qz, qy * qy, qy * qz, qz * qz};
#pragma unroll
                for (int u = 0; u < CAP; ++u)
                    if (d < a.r2[u]) {
#pragma unroll
                        for (int e = 0; e < 9; ++e) m[u][e] += term[e];
                        ++c[u];
                    }
            }
        }
    }
    const size_t slot = a.slot ? a.slot[self] : self;
#pragma unroll
    for (int u = 0; u < CAP; ++u)
        if ((uint32_t)u < a.S) {
            double *o = a.moments + (slot * a.S + u) * 9;
#pragma unroll
            for (int e = 0; e < 9; ++e) o[e] = m[u][e];
            a.count[slot * a.S + u] = c[u];
        }
}

struct FitArgs {
    const float *rows;               // the cloud: point i at rows + i * stride
    uint32_t stride;
    const uint32_t *qidx;            // the queried indices by slot (nullptr: the slot itself)
    uint32_t k, S, min_nb;
    int32_t mode, orient;
    double view[3];
    const double *moments;           // k x S x 9
    const uint32_t *count;           // k x S
    int32_t *chosen;                 // k
    float *nrm;                      // the chosen normal of slot t: nrm + t * nrm_stride
    uint32_t nrm_stride;
    float *xyz;                      // the query's position, bit for bit: xyz + t * xyz_stride (or nullptr)
    uint32_t xyz_stride;
    float *feat;                     // k x 4 (or nullptr)
    uint8_t *fitted;                 // k x S (or nullptr)
    double *eig;                     // k x S x 3 (or nullptr)
    float *normals;                  // k x S x 3 (or nullptr)
    uint32_t *partial;               // per workgroup: SUM_TERMS words
};

// term 0: fitted queries; 1 .. 8: the histogram of the chosen scale; 9: the largest count (a maximum; the others are sums)
struct HistMaxU {
    __device__ __forceinline__ uint32_t operator()(int k, uint32_t a, uint32_t b) const { return k == SUM_TERMS - 1 ? max(a, b) : a + b; }
};

__global__ __launch_bounds__(FIT_TPB) void k_scales_fit(const FitArgs a) {
    __shared__ uint32_t s_u[FIT_TPB / 64][SUM_TERMS];
    const uint32_t t = blockIdx.x * FIT_TPB + threadIdx.x;
    uint32_t u[SUM_TERMS];
#pragma unroll
    for (int e = 0; e < SUM_TERMS; ++e) u[e] = 0;
    if (t < a.k) {
        const uint32_t i = a.qidx ? a.qidx[t] : t;
        const float *row = a.rows + (size_t)i * a.stride;
        const float fx = row[0], fy = row[1], fz = row[2];
        const double px = fx, py = fy, pz = fz;
        double gx = 0.0, gy = 0.0, gz = 0.0;
        if (a.orient) { gx = (double)row[3]; gy = (double)row[4]; gz = (double)row[5]; }
        int32_t chosen = -1;
        double best = 0.0;
        d3 bn = {NAN, NAN, NAN};
        double bf[4] = {NAN, NAN, NAN, NAN};
        uint32_t cmax = 0;
        for (uint32_t sc = 0; sc < a.S; ++sc) {
            const size_t at = (size_t)t * a.S + sc;
            const double *mo = a.moments + at * 9;
            const uint32_t c = a.count[at];
            cmax = max(cmax, c);
            const double W = (double)c;        // (the point itself is in N(i, s): c >= 1)
            const d3 mu = {mo[0] / W, mo[1] / W, mo[2] / W};
            const double c00 = mo[3] / W - mu.x * mu.x, c01 = mo[4] / W - mu.x * mu.y, c02 = mo[5] / W - mu.x * mu.z;
            const double c11 = mo[6] / W - mu.y * mu.y, c12 = mo[7] / W - mu.y * mu.z, c22 = mo[8] / W - mu.z * mu.z;
            double l1, l2, l3;
            sym3_eigenvalues(c00, c01, c02, c11, c12, c22, l1, l2, l3);
            l1 = fmax(l1, 0.0); l2 = fmax(l2, 0.0); l3 = fmax(l3, 0.0);
            d3 nv = {NAN, NAN, NAN};
            bool fit = false;
            if (c >= a.min_nb && l1 > 0.0) {
                double l0, tr;
                fit = pca_eig(c00, c01, c02, c11, c12, c22, nv, l0, tr);
            }
            if (fit) {
                bool flip = (a.view[0] - px) * nv.x + (a.view[1] - py) * nv.y + (a.view[2] - pz) * nv.z < 0.0;
                if (a.orient) {
                    const double along = (gx * nv.x + gy * nv.y) + gz * nv.z;
                    if (along < 0.0) flip = true;
                    else if (along > 0.0) flip = false;        // 0 or not finite: the viewpoint test stands
                }
                if (flip) nv = {-nv.x, -nv.y, -nv.z};
                const double lin = (l1 - l2) / l1, pla = (l2 - l3) / l1, sph = l3 / l1, var = l3 / ((l1 + l2) + l3);
                // larger is better: -var > -best is var < best exactly.  One comparison and selects, no branch per mode
                const double crit = a.mode == 0 ? pla : -var;
                const bool take = chosen < 0 || crit > best;
                chosen = take ? (int32_t)sc : chosen;
                best = take ? crit : best;
                bn = {take ? nv.x : bn.x, take ? nv.y : bn.y, take ? nv.z : bn.z};
                bf[0] = take ? lin : bf[0]; bf[1] = take ? pla : bf[1]; bf[2] = take ? sph : bf[2]; bf[3] = take ? var : bf[3];
            } else {
                nv = {NAN, NAN, NAN};
            }
            if (a.fitted) a.fitted[at] = fit ? 1 : 0;
            if (a.eig) { double *o = a.eig + at * 3; o[0] = l1; o[1] = l2; o[2] = l3; }
            if (a.normals) { float *o = a.normals + at * 3; o[0] = (float)nv.x; o[1] = (float)nv.y; o[2] = (float)nv.z; }
        }
        a.chosen[t] = chosen;
        float *on = a.nrm + (size_t)t * a.nrm_stride;
        on[0] = (float)bn.x; on[1] = (float)bn.y; on[2] = (float)bn.z;
        if (a.xyz) { float *o = a.xyz + (size_t)t * a.xyz_stride; o[0] = fx; o[1] = fy; o[2] = fz; }
        if (a.feat) {
            float *o = a.feat + (size_t)t * 4;
            o[0] = (float)bf[0]; o[1] = (float)bf[1]; o[2] = (float)bf[2]; o[3] = (float)bf[3];
        }
        u[0] = chosen >= 0 ? 1u : 0u;
#pragma unroll
        for (int e = 0; e < SCALES_MAX; ++e) u[1 + e] = chosen == e ? 1u : 0u;
        u[SUM_TERMS - 1] = cmax;
    }
    block_reduce<FIT_TPB>(u, s_u, a.partial, HistMaxU());
}

__global__ __launch_bounds__(64) void k_scales_final(const uint32_t *__restrict__ partial, uint32_t blocks, uint32_t *__restrict__ res) {
    uint32_t u[SUM_TERMS];
    final_reduce(partial, blocks, u, HistMaxU());
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int e = 0; e < SUM_TERMS; ++e) res[e] = u[e];
}

}  // namespace

struct ScalesWork {
    TargetGrid grid;
    DBuf<float> in, nrm, feat, normals;      // in, nrm: the host-pointer entry point's device copies (grow-only)
    DBuf<double> moments, eig;
    DBuf<uint32_t> count, qidx, slot, flags, scan, pos, partial, res;
    DBuf<int32_t> chosen;
    DBuf<uint8_t> fitted;
    EventSpans<4> spans;                     // grid (with the query list), walk + fit, reduce
    uint32_t h_u[SUM_TERMS] = {};
};

namespace {

void check_params(uint32_t n, uint32_t stride, const uint32_t *query_index, uint32_t k, const plade_scale_params &p) {
    PLADE_REQUIRE(n >= 1, PLADE_EINVAL, "scale_features: the cloud is empty (n = 0)");
    PLADE_REQUIRE(p.orient == 0 || p.orient == 1, PLADE_EINVAL, "scale_features: orient must be 0 or 1");
    PLADE_REQUIRE(stride >= 3, PLADE_EINVAL, "scale_features: stride must be >= 3 floats");
    PLADE_REQUIRE(p.orient == 0 || stride >= 6, PLADE_EINVAL, "scale_features: orient = 1 reads the rows' normals: stride must be >= 6 floats");
    PLADE_REQUIRE(p.scales >= 1 && p.scales <= SCALES_MAX, PLADE_EINVAL, "scale_features: the number of scales must be 1 .. 8");
    for (int s = 0; s < p.scales; ++s) {
        PLADE_REQUIRE(radius_ok(p.radii[s], true), PLADE_EINVAL,
                      "scale_features: every radius must be finite and > 0, and its fp32 square finite and not below FLT_MIN");
        if (s) {
            const float r0 = (float)p.radii[s - 1], r1 = (float)p.radii[s];
            PLADE_REQUIRE(r0 * r0 < r1 * r1, PLADE_EINVAL, "scale_features: the fp32 squares of the radii must be strictly ascending");
        }
    }
    PLADE_REQUIRE(p.min_neighbours >= SCALES_MIN_NEIGHBOURS, PLADE_EINVAL, "scale_features: min_neighbours must be >= 3");
    PLADE_REQUIRE(p.mode == 0 || p.mode == 1, PLADE_EINVAL, "scale_features: mode must be 0 (planarity) or 1 (surface variation)");
    PLADE_REQUIRE(std::isfinite(p.viewpoint[0]) && std::isfinite(p.viewpoint[1]) && std::isfinite(p.viewpoint[2]), PLADE_EINVAL,
                  "scale_features: the viewpoint must be finite");
    if (query_index) {
        PLADE_REQUIRE(k >= 1, PLADE_EINVAL, "scale_features: the query list is empty (k = 0)");
        for (uint32_t t = 0; t < k; ++t) {
            PLADE_REQUIRE(query_index[t] < n, PLADE_EINVAL, "scale_features: a query index is >= n");
            PLADE_REQUIRE(t == 0 || query_index[t - 1] < query_index[t], PLADE_EINVAL,
                          "scale_features: the query indices must be strictly ascending");
        }
    }
}

// The tool on a device cloud of `stride` floats per point with a known bounding box; query_index: the host's list (checked) or
// nullptr.  f: where the chosen normals (and positions) go and which optional arrays are wanted (nrm, xyz, feat, fitted, eig,
// normals; the rest is filled in here).  Leaves chosen, moments and count in W, waits, fills the summary and the stats.
void scales_dev(plade_ctx *ctx, ScalesWork &W, const float *d_rows, uint32_t n, uint32_t stride, const float bbmin[3], const float bbmax[3],
                const uint32_t *query_index, uint32_t k, const plade_scale_params &p, FitArgs f, plade_scale_summary *summary) {
    const uint32_t S = (uint32_t)p.scales;
    W.spans.mark(ctx, 0);
    TargetGrid &G = W.grid;
    const float rmax = (float)p.radii[S - 1];
    G.build(ctx, d_rows, n, stride, radius_cell((double)rmax, bbmin, bbmax), bbmin, bbmax, true);
    WalkArgs a;
    memset(&a, 0, sizeof(a));
    a.g = view_of(G, "scale_features");
    a.k = k; a.S = S;
    for (int s = 0; s < SCALES_MAX; ++s) {
        const float r = (uint32_t)s < S ? (float)p.radii[s] : 0.f;
        a.r2[s] = (uint32_t)s < S ? r * r : -1.f;
    }
    a.r2max = rmax * rmax;
    if (query_index) {
        uint32_t *d_qidx = W.qidx.ensure(k), *d_slot = W.slot.ensure(n), *d_flags = W.flags.ensure((size_t)n + 1);
        ctx->h2d(d_qidx, query_index, (size_t)k * 4);
        ctx->fill_async(d_slot, 0xff, (size_t)n * 4);
        ctx->fill_async(d_flags + n, 0, 4);
        hipLaunchKernelGGL(k_scales_mark, dim3(cdiv(k, MARK_TPB)), dim3(MARK_TPB), 0, ctx->stream, d_qidx, k, d_slot);
        hipLaunchKernelGGL(k_scales_flag, dim3(cdiv(n, MARK_TPB)), dim3(MARK_TPB), 0, ctx->stream, a.g.sorted, d_slot, n, d_flags);
        HIP_TRY(hipGetLastError());
        const uint32_t total = compact_flags(ctx, d_flags, n, W.scan, W.pos);
        PLADE_REQUIRE(total == k, PLADE_EFAIL, "scale_features: the query list and its sorted positions disagree");
        a.pos = W.pos.p; a.slot = d_slot;
        f.qidx = d_qidx;
    }
    W.spans.mark(ctx, 1);
    a.moments = W.moments.ensure((size_t)k * S * 9);
    a.count = W.count.ensure((size_t)k * S);
    const dim3 wg(cdiv(k, WALK_TPB)), wb(WALK_TPB);
    if (S <= 2) hipLaunchKernelGGL(k_scales_walk<2>, wg, wb, 0, ctx->stream, a);
    else if (S <= 4) hipLaunchKernelGGL(k_scales_walk<4>, wg, wb, 0, ctx->stream, a);
    else hipLaunchKernelGGL(k_scales_walk<8>, wg, wb, 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    const uint32_t blocks = cdiv(k, FIT_TPB);
    f.rows = d_rows; f.stride = stride;
    f.k = k; f.S = S;
    f.min_nb = (uint32_t)p.min_neighbours;
    f.mode = p.mode; f.orient = p.orient;
    for (int t = 0; t < 3; ++t) f.view[t] = p.viewpoint[t];
    f.moments = a.moments; f.count = a.count;
    f.chosen = W.chosen.ensure(k);
    f.partial = W.partial.ensure((size_t)SUM_TERMS * blocks);
    hipLaunchKernelGGL(k_scales_fit, dim3(blocks), dim3(FIT_TPB), 0, ctx->stream, f);
    HIP_TRY(hipGetLastError());
    W.spans.mark(ctx, 2);
    uint32_t *d_res = W.res.ensure(SUM_TERMS);
    hipLaunchKernelGGL(k_scales_final, dim3(1), dim3(64), 0, ctx->stream, f.partial, blocks, d_res);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(W.h_u, d_res, sizeof(W.h_u), hipMemcpyDeviceToHost, ctx->stream));
    W.spans.mark(ctx, 3);
    ctx->sync();
    if (summary) {
        summary->queries = k;
        summary->fitted = W.h_u[0];
        for (int e = 0; e < SCALES_MAX; ++e) summary->chosen_hist[e] = W.h_u[1 + e];
        summary->max_count = W.h_u[SUM_TERMS - 1];
        summary->reserved = 0;
    }
    W.spans.collect();
    ctx->stats.clear();
    ctx->stats.add("scales_grid_s", W.spans.seconds(0));
    ctx->stats.add("scales_walk_s", W.spans.seconds(1));
    ctx->stats.add("scales_reduce_s", W.spans.seconds(2));
    ctx->stats.add("scales_fitted", W.h_u[0]);
    grid_stats(ctx, "scales", W.grid);
}

}  // namespace
}  // namespace plade

using namespace plade;

// ---- C ABI (include/plade_hip.h) ---------------------------------------------------------------------------------------------
extern "C" void plade_scale_default_params(plade_scale_params *p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->scales = 0;
    p->min_neighbours = 6;
    p->mode = 0;
    p->orient = 0;
}

extern "C" int plade_cloud_scale_features(plade_ctx *ctx, const float *rows, uint32_t n, uint32_t stride, const uint32_t *query_index,
                                          uint32_t k, const plade_scale_params *params, int32_t *chosen_out, float *normal_out,
                                          float *features_out, uint32_t *count_out, uint8_t *fitted_out, double *eigenvalues_out,
                                          float *normals_out, double *moments_out, plade_scale_summary *summary) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(rows, PLADE_EINVAL, "plade_cloud_scale_features: NULL cloud");
        const plade_scale_params p = params_or_default(params, plade_scale_default_params);
        check_params(n, stride, query_index, k, p);
        if (!query_index) k = n;
        ScalesWork &W = work_in<ScalesWork>(ctx->scales_work);
        float mn[3], mx[3];
        upload_rows(ctx, W.in, rows, n, stride, mn, mx);
        const size_t S = (size_t)p.scales, kS = (size_t)k * S;
        FitArgs f;
        memset(&f, 0, sizeof(f));
        f.nrm = W.nrm.ensure((size_t)k * 3 + 4); f.nrm_stride = 3;
        if (features_out) f.feat = W.feat.ensure((size_t)k * 4);
        if (fitted_out) f.fitted = W.fitted.ensure(kS + 4);
        if (eigenvalues_out) f.eig = W.eig.ensure(kS * 3);
        if (normals_out) f.normals = W.normals.ensure(kS * 3 + 4);
        scales_dev(ctx, W, W.in.p, n, stride, mn, mx, query_index, k, p, f, summary);
        const auto out = [&](void *dst, const void *src, size_t bytes) {
            if (dst) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
        };
        out(chosen_out, W.chosen.p, (size_t)k * 4);
        out(normal_out, W.nrm.p, (size_t)k * 12);
        out(features_out, W.feat.p, (size_t)k * 16);
        out(count_out, W.count.p, kS * 4);
        out(fitted_out, W.fitted.p, kS);
        out(eigenvalues_out, W.eig.p, kS * 24);
        out(normals_out, W.normals.p, kS * 12);
        out(moments_out, W.moments.p, kS * 72);
        ctx->sync();
        return PLADE_OK;
    });
}

extern "C" int plade_cloud_scale_normals_dev(plade_ctx *ctx, plade_cloud *cloud, const uint32_t *query_index, uint32_t k,
                                             const plade_scale_params *params, plade_cloud **out, plade_scale_summary *summary) {
    return guarded(ctx, [&]() -> int {
        if (out) *out = nullptr;         // NULL after every refusal, the one below included
        PLADE_REQUIRE(cloud && out, PLADE_EINVAL, "plade_cloud_scale_normals_dev: NULL cloud");
        const plade_scale_params p = params_or_default(params, plade_scale_default_params);
        const CloudDev &in = cloud->dev;
        check_params(in.n, 6, query_index, k, p);
        if (!query_index) k = in.n;
        ScalesWork &W = work_in<ScalesWork>(ctx->scales_work);
        resident_result(ctx, out, [&](CloudDev &c) {
            cloud_shape(c, k);
            FitArgs f;
            memset(&f, 0, sizeof(f));
            f.xyz = c.aos.p; f.xyz_stride = 6;
            f.nrm = c.aos.p + 3; f.nrm_stride = 6;
            scales_dev(ctx, W, in.aos.p, in.n, 6, in.bbmin, in.bbmax, query_index, k, p, f, summary);
        });
        return PLADE_OK;
    });
}
