// plade_amd/csrc/k_smooth.hip -- moving-least-squares plane projection on gfx950 (semantics: smooth.h).
//
// Layout
//   grid     the dense row index of TargetGrid, built as the radius filter of k_outliers.hip builds it: the cell is
//            radius_cell(r) of grid_walk.h (the rule of DESIGN.md section 10; build() may enlarge it, never shrink it), so the 27-cell
//            block around a point holds everything closer than r.
//   fit      k_smooth_fit: one lane per point in the grid's sorted order (the 64 queries of a wavefront share their candidate runs,
//            as in k_outliers_radius).  A lane walks the nine runs of for_block27 with ten fp64 accumulators (W, S, M about the
//            query) and a count, then solves the fit with pca_eig (pca_eig.h, the eigen-solve of k_normals), projects the point
//            and writes its outputs by original index.  No LDS, no atomics.
//   summary  k_smooth_sum / k_smooth_final, in the fixed order of fixed_reduce.h: sum of delta^2 and max |delta| over the fitted
//            points, their number, the largest count.
#include "smooth.h"
#include "cloud_tool.h"
#include "fixed_reduce.h"
#include "grid_walk.h"
#include "pca_eig.h"
#include "voxel.h"

namespace plade {

namespace {

constexpr int FIT_TPB = 256, SUM_TPB = 256;

struct FitArgs {
    GridView g;
    uint32_t n;
    float r2;                        // (float)r * (float)r
    uint32_t min_nb;
    double view[3];
    float *xyz;                      // the smoothed position of point i: xyz + i * xyz_stride
    uint32_t xyz_stride;
    float *nrm;                      // the normal of point i: nrm + i * nrm_stride (or nullptr)
    uint32_t nrm_stride;
    const uint32_t *keep_nrm;        // rows of 6 words whose words 3..5 go to nrm instead of the fit's normal (or nullptr)
    float *curv;                     // or nullptr
    double *disp;
    uint32_t *count;
    uint8_t *fitted;
    double *moments;                 // n x 10 (or nullptr)
};

__global__ __launch_bounds__(FIT_TPB) void k_smooth_fit(const FitArgs a) {
    const uint32_t s = blockIdx.x * FIT_TPB + threadIdx.x;
    if (s >= a.n) return;
    const float4 q4 = a.g.sorted[s];
    const f3 q(q4.x, q4.y, q4.z);
    const uint32_t self = __float_as_uint(q4.w);
    int cx, cy, cz;
    cell_of(a.g, q, cx, cy, cz);
    const double px = q.x, py = q.y, pz = q.z, r2 = (double)a.r2;
    double W = 0.0, sx = 0.0, sy = 0.0, sz = 0.0, m00 = 0.0, m01 = 0.0, m02 = 0.0, m11 = 0.0, m12 = 0.0, m22 = 0.0;
    uint32_t c = 0;
    for (int t = 0; t < 9; ++t) {
        const int dy = t % 3 - 1, dz = t / 3 - 1;
        const uint32_t r = (uint32_t)(cx + 1) + row_base(a.g, cy + dy, cz + dz);   // for_block27's runs, as k_outliers_radius
        const uint32_t j1 = a.g.row_start[r + 3];
        for (uint32_t j = a.g.row_start[r]; j < j1; ++j) {
            const float4 p = a.g.sorted[j];
            const float d = flann_d2(q, f3(p.x, p.y, p.z));
            if (d < a.r2) {
                const double h = 1.0 - (double)d / r2, w = h * h;
                const double qx = (double)p.x - px, qy = (double)p.y - py, qz = (double)p.z - pz;
                const double wx = w * qx, wy = w * qy, wz = w * qz;
                W += w;
                sx += wx; sy += wy; sz += wz;
                m00 += wx * qx; m01 += wx * qy; m02 += wx * qz;
                m11 += wy * qy; m12 += wy * qz; m22 += wz * qz;
                ++c;
            }
        }
    }
    d3 nv = {NAN, NAN, NAN};
    double delta = 0.0, curvature = NAN;
    float ox = q.x, oy = q.y, oz = q.z;
    bool fit = false;
    if (c >= a.min_nb) {             // (the point itself is in N_i: W >= 1)
        const d3 mu = {sx / W, sy / W, sz / W};
        double l0, tr;
        if (pca_eig(m00 / W - mu.x * mu.x, m01 / W - mu.x * mu.y, m02 / W - mu.x * mu.z, m11 / W - mu.y * mu.y, m12 / W - mu.y * mu.z,
                    m22 / W - mu.z * mu.z, nv, l0, tr)) {
            if ((a.view[0] - px) * nv.x + (a.view[1] - py) * nv.y + (a.view[2] - pz) * nv.z < 0.0) nv = {-nv.x, -nv.y, -nv.z};
            curvature = fmax(l0, 0.0) / tr;
            delta = ddot(nv, mu);
            ox = (float)(px + delta * nv.x); oy = (float)(py + delta * nv.y); oz = (float)(pz + delta * nv.z);
            fit = true;
        }
    }
    float *o = a.xyz + (size_t)self * a.xyz_stride;
    o[0] = ox; o[1] = oy; o[2] = oz;
    if (a.nrm) {
        uint32_t *on = reinterpret_cast<uint32_t *>(a.nrm + (size_t)self * a.nrm_stride);
        if (a.keep_nrm) {
            const uint32_t *in = a.keep_nrm + (size_t)self * 6;
            on[0] = in[3]; on[1] = in[4]; on[2] = in[5];
        } else {
            on[0] = __float_as_uint((float)nv.x); on[1] = __float_as_uint((float)nv.y); on[2] = __float_as_uint((float)nv.z);
        }
    }
    if (a.curv) a.curv[self] = (float)curvature;
    a.disp[self] = delta;
    a.count[self] = c;
    a.fitted[self] = fit ? 1 : 0;
    if (a.moments) {
        double *m = a.moments + (size_t)self * 10;
        m[0] = W; m[1] = sx; m[2] = sy; m[3] = sz; m[4] = m00; m[5] = m01; m[6] = m02; m[7] = m11; m[8] = m12; m[9] = m22;
    }
}

// per workgroup: pd[2 b] = the sum of delta^2, pd[2 b + 1] = the max of |delta| over its fitted points; pu[2 b] = their number,
// pu[2 b + 1] = its largest count (the order: fixed_reduce.h; term 0 of each type is a sum, term 1 a maximum)
struct SumMaxD {
    __device__ __forceinline__ double operator()(int k, double a, double b) const { return k == 1 ? fmax(a, b) : a + b; }
};
struct SumMaxU {
    __device__ __forceinline__ uint32_t operator()(int k, uint32_t a, uint32_t b) const { return k == 1 ? max(a, b) : a + b; }
};

__global__ __launch_bounds__(SUM_TPB) void k_smooth_sum(const double *__restrict__ disp, const uint8_t *__restrict__ fitted,
                                                        const uint32_t *__restrict__ count, uint32_t n, double *__restrict__ pd,
                                                        uint32_t *__restrict__ pu) {
    __shared__ double s_d[SUM_TPB / 64][2];
    __shared__ uint32_t s_u[SUM_TPB / 64][2];
    const uint32_t i = blockIdx.x * SUM_TPB + threadIdx.x;
    double d[2] = {0.0, 0.0};        // delta^2, |delta|
    uint32_t u[2] = {0, 0};          // fitted, count
    if (i < n) {
        u[1] = count[i];
        if (fitted[i]) { const double e = disp[i]; d[0] = e * e; d[1] = fabs(e); u[0] = 1; }
    }
    block_reduce<SUM_TPB>(d, s_d, pd, SumMaxD());
    block_reduce<SUM_TPB>(u, s_u, pu, SumMaxU());
}

// rd[0] = rms, rd[1] = max of |delta| over the fitted points (0 when there is none); ru[0] = fitted, ru[1] = the largest count
__global__ __launch_bounds__(64) void k_smooth_final(const double *__restrict__ pd, const uint32_t *__restrict__ pu, uint32_t blocks,
                                                     double *__restrict__ rd, uint32_t *__restrict__ ru) {
    double d[2];
    uint32_t u[2];
    final_reduce(pd, pu, blocks, d, SumMaxD(), u, SumMaxU());
    if (threadIdx.x != 0) return;
    rd[0] = u[0] ? sqrt(d[0] / (double)u[0]) : 0.0;
    rd[1] = d[1];
    ru[0] = u[0]; ru[1] = u[1];
}

}  // namespace

struct SmoothWork {
    TargetGrid grid;
    DBuf<float> in, xyz, nrm, curv;  // the host-pointer entry point's device copies (grow-only)
    DBuf<double> disp, moments, partial_d, res_d;
    DBuf<uint32_t> count, partial_u, res_u;
    DBuf<uint8_t> fitted;
    EventSpans<4> spans;             // grid, fit, reduce
    double h_d[2] = {0.0, 0.0};
    uint32_t h_u[2] = {0, 0};
};

namespace {

void check_params(uint32_t n, uint32_t stride, const plade_smooth_params &p) {
    PLADE_REQUIRE(n >= 1, PLADE_EINVAL, "smooth_cloud: the cloud is empty (n = 0)");
    PLADE_REQUIRE(stride >= 3, PLADE_EINVAL, "smooth_cloud: stride must be >= 3 floats");
    // r2 a normal fp32 number: at 0 no point would be its own neighbour (d = 0 < r2 must hold), a subnormal r2 carries few bits
    PLADE_REQUIRE(radius_ok(p.radius, true), PLADE_EINVAL,
                  "smooth_cloud: radius must be finite and > 0, and its fp32 square finite and not below FLT_MIN");
    PLADE_REQUIRE(p.min_neighbours >= SMOOTH_MIN_NEIGHBOURS, PLADE_EINVAL, "smooth_cloud: min_neighbours must be >= 3");
    PLADE_REQUIRE(std::isfinite(p.viewpoint[0]) && std::isfinite(p.viewpoint[1]) && std::isfinite(p.viewpoint[2]), PLADE_EINVAL,
                  "smooth_cloud: the viewpoint must be finite");
}

// The fit on a device cloud of `stride` floats per point with a known bounding box.  out: where the positions and normals go and
// which optional arrays are wanted (xyz, nrm, keep_nrm, curv, moments; the rest is filled in here).  Leaves delta, count and fitted
// in W, waits, fills the summary and the stats.
void smooth_dev(plade_ctx *ctx, SmoothWork &W, const float *d_rows, uint32_t n, uint32_t stride, const float bbmin[3], const float bbmax[3],
                const plade_smooth_params &p, FitArgs a, plade_smooth_summary *summary) {
    W.spans.mark(ctx, 0);
    TargetGrid &G = W.grid;
    const float r = (float)p.radius;
    G.build(ctx, d_rows, n, stride, radius_cell((double)r, bbmin, bbmax), bbmin, bbmax, true);
    W.spans.mark(ctx, 1);
    a.g = view_of(G, "smooth_cloud");
    a.n = n; a.r2 = r * r;
    a.min_nb = (uint32_t)p.min_neighbours;
    for (int t = 0; t < 3; ++t) a.view[t] = p.viewpoint[t];
    a.disp = W.disp.ensure(n);
    a.count = W.count.ensure(n);
    a.fitted = W.fitted.ensure((size_t)n + 4);
    hipLaunchKernelGGL(k_smooth_fit, dim3(cdiv(n, FIT_TPB)), dim3(FIT_TPB), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    W.spans.mark(ctx, 2);
    const uint32_t blocks = cdiv(n, SUM_TPB);
    double *d_pd = W.partial_d.ensure((size_t)2 * blocks), *d_rd = W.res_d.ensure(2);
    uint32_t *d_pu = W.partial_u.ensure((size_t)2 * blocks), *d_ru = W.res_u.ensure(2);
    hipLaunchKernelGGL(k_smooth_sum, dim3(blocks), dim3(SUM_TPB), 0, ctx->stream, a.disp, a.fitted, a.count, n, d_pd, d_pu);
    hipLaunchKernelGGL(k_smooth_final, dim3(1), dim3(64), 0, ctx->stream, d_pd, d_pu, blocks, d_rd, d_ru);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(W.h_d, d_rd, sizeof(W.h_d), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(W.h_u, d_ru, sizeof(W.h_u), hipMemcpyDeviceToHost, ctx->stream));
    W.spans.mark(ctx, 3);
    ctx->sync();
    if (summary) {
        summary->n = n;
        summary->fitted = W.h_u[0];
        summary->rms = W.h_d[0];
        summary->max = W.h_d[1];
        summary->max_count = W.h_u[1];
        summary->reserved = 0;
    }
    W.spans.collect();
    ctx->stats.clear();
    ctx->stats.add("smooth_grid_s", W.spans.seconds(0));
    ctx->stats.add("smooth_fit_s", W.spans.seconds(1));
    ctx->stats.add("smooth_reduce_s", W.spans.seconds(2));
    ctx->stats.add("smooth_fitted", W.h_u[0]);
    grid_stats(ctx, "smooth", W.grid);
}

}  // namespace
}  // namespace plade

using namespace plade;

// ---- C ABI (include/plade_hip.h) ---------------------------------------------------------------------------------------------
extern "C" void plade_smooth_default_params(plade_smooth_params *p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->radius = 0.0;
    p->min_neighbours = 6;
    p->viewpoint[0] = p->viewpoint[1] = p->viewpoint[2] = 0.f;
}

extern "C" int plade_smooth_cloud(plade_ctx *ctx, const float *rows, uint32_t n, uint32_t stride, const plade_smooth_params *params,
                                  float *out_xyz, float *out_normal, float *curvature_out, double *displacement_out, uint32_t *count_out,
                                  uint8_t *fitted_out, double *moments_out, plade_smooth_summary *summary) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(rows && out_xyz, PLADE_EINVAL, "plade_smooth_cloud: NULL cloud or output");
        const plade_smooth_params p = params_or_default(params, plade_smooth_default_params);
        check_params(n, stride, p);
        SmoothWork &W = work_in<SmoothWork>(ctx->smooth_work);
        float mn[3], mx[3];
        upload_rows(ctx, W.in, rows, n, stride, mn, mx);
        FitArgs a;
        memset(&a, 0, sizeof(a));
        a.xyz = W.xyz.ensure((size_t)n * 3 + 4); a.xyz_stride = 3;
        if (out_normal) { a.nrm = W.nrm.ensure((size_t)n * 3 + 4); a.nrm_stride = 3; }
        if (curvature_out) a.curv = W.curv.ensure(n);
        if (moments_out) a.moments = W.moments.ensure((size_t)n * 10);
        smooth_dev(ctx, W, W.in.p, n, stride, mn, mx, p, a, summary);
        HIP_TRY(hipMemcpyAsync(out_xyz, W.xyz.p, (size_t)n * 12, hipMemcpyDeviceToHost, ctx->stream));
        if (out_normal) HIP_TRY(hipMemcpyAsync(out_normal, W.nrm.p, (size_t)n * 12, hipMemcpyDeviceToHost, ctx->stream));
        if (curvature_out) HIP_TRY(hipMemcpyAsync(curvature_out, W.curv.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (displacement_out) HIP_TRY(hipMemcpyAsync(displacement_out, W.disp.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (count_out) HIP_TRY(hipMemcpyAsync(count_out, W.count.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (fitted_out) HIP_TRY(hipMemcpyAsync(fitted_out, W.fitted.p, n, hipMemcpyDeviceToHost, ctx->stream));
        if (moments_out) HIP_TRY(hipMemcpyAsync(moments_out, W.moments.p, (size_t)n * 80, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        return PLADE_OK;
    });
}

extern "C" int plade_cloud_smooth_dev(plade_ctx *ctx, plade_cloud *cloud, const plade_smooth_params *params, int32_t use_fit_normals,
                                      plade_cloud **out, plade_smooth_summary *summary) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(cloud && out, PLADE_EINVAL, "plade_cloud_smooth_dev: NULL cloud");
        *out = nullptr;
        const plade_smooth_params p = params_or_default(params, plade_smooth_default_params);
        const CloudDev &in = cloud->dev;
        check_params(in.n, 6, p);
        SmoothWork &W = work_in<SmoothWork>(ctx->smooth_work);
        resident_result(ctx, out, [&](CloudDev &c) {
            cloud_shape(c, in.n);
            FitArgs a;
            memset(&a, 0, sizeof(a));
            a.xyz = c.aos.p; a.xyz_stride = 6;
            a.nrm = c.aos.p + 3; a.nrm_stride = 6;
            if (!use_fit_normals) a.keep_nrm = reinterpret_cast<const uint32_t *>(in.aos.p);
            smooth_dev(ctx, W, in.aos.p, in.n, 6, in.bbmin, in.bbmax, p, a, summary);
        });
        return PLADE_OK;
    });
}
