// plade_amd/csrc/k_icp.hip -- point-to-plane ICP refinement on gfx950 (semantics: icp.h).
//
// Layout
//   grids   one dense row index of TargetGrid per stage distance d, cell >= d: the 27 cells around a probe's cell (for_block27,
//           grid_walk.h) hold every target point closer than d, so the argmin over them is the exact one whenever it is below d
//           (and the probe has no correspondence otherwise).  The grids are built up front.
//   mean    k_icp_mean_part / k_icp_mean: the fp64 mean s-bar of the sample, once, in a fixed order (one partial per workgroup:
//           a butterfly across each wave, then the waves in order; one wavefront then sums the partials like k_icp_solve); the
//           second kernel also sets the first centre c_0 = T_0 s-bar.
//   loop    max_iterations pairs (k_icp_corr_lin, k_icp_solve) queued on the context's stream with no host wait in between; the
//           state word lives on the device (IcpState), and once it says done every later kernel returns at once.
//   corr    k_icp_corr_lin: one lane per sample point.  The lane forms p' in fp32, takes the exact (d, j) argmin key over the
//           nine runs of the current stage's grid, and -- with a correspondence -- r and J (about the centre c_k) in fp64; the 29 moments are summed
//           across the wave (butterfly), then the four waves in order, and each workgroup writes one partial to its own slot.
//   solve   k_icp_solve: one wavefront sums the partials in a fixed order (lane l: partials l, l + 64, ..., then a butterfly),
//           and lane 0 runs the Cholesky solve, Rodrigues, the update of T and c and the stage / convergence / failure rules.
#include "icp_core.h"
#include "voxel.h"

namespace plade {

namespace {

// (the state, the mean, the reduction and k_icp_solve are shared with the plane-to-plane ICP: icp_core.h)
struct IcpArgs {
    IcpGridArgs g[ICP_MAX_STAGES];
    const float *tgt;    // n_t x 6: the normals are gathered by the original index
    const float *src;    // sample points, `stride` floats apart
    uint32_t stride, n;
    IcpState *st;
    double *partial;     // gridDim.x x ICP_MOMENTS
    int32_t *corr;       // seam: j or -1 per point (nullptr in the loop)
};

__global__ __launch_bounds__(CORR_TPB) void k_icp_corr_lin(const IcpArgs a) {
    __shared__ double s_red[CORR_TPB / 64][ICP_MOMENTS];
    const IcpState *st = a.st;
    if (st->done) return;                              // (uniform)
    const IcpGridArgs &G = a.g[st->stage];
    const uint32_t i = blockIdx.x * CORR_TPB + threadIdx.x;
    double m[ICP_MOMENTS];
#pragma unroll
    for (int k = 0; k < ICP_MOMENTS; ++k) m[k] = 0.0;
    if (i < a.n) {
        const float *s = a.src + (size_t)i * a.stride;
        const float x = s[0], y = s[1], z = s[2];
        const float *Tf = st->Tf;
        const f3 q(((Tf[0] * x + Tf[1] * y) + Tf[2] * z) + Tf[3], ((Tf[4] * x + Tf[5] * y) + Tf[6] * z) + Tf[7],
                   ((Tf[8] * x + Tf[9] * y) + Tf[10] * z) + Tf[11]);
        const u64 best = nearest_key(G.g, q);
        int32_t jout = -1;
        if (best != EMPTY && key_d(best) < G.d2) {
            const uint32_t j = (uint32_t)best;
            const float *t = a.tgt + (size_t)j * 6;
            const double n0 = t[3], n1 = t[4], n2 = t[5];
            if (isfinite(n0) && isfinite(n1) && isfinite(n2)) {
                jout = (int32_t)j;
                const double *T = st->T;
                const double X = x, Y = y, Z = z;
                const double p0 = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[3];
                const double p1 = ((T[4] * X + T[5] * Y) + T[6] * Z) + T[7];
                const double p2 = ((T[8] * X + T[9] * Y) + T[10] * Z) + T[11];
                const double r = (n0 * (p0 - (double)t[0]) + n1 * (p1 - (double)t[1])) + n2 * (p2 - (double)t[2]);
                const double u0 = p0 - st->c[0], u1 = p1 - st->c[1], u2 = p2 - st->c[2];
                const double J[6] = {u1 * n2 - u2 * n1, u2 * n0 - u0 * n2, u0 * n1 - u1 * n0, n0, n1, n2};
                int k = 0;
#pragma unroll
                for (int u = 0; u < 6; ++u)
#pragma unroll
                    for (int v = u; v < 6; ++v) m[k++] = J[u] * J[v];
#pragma unroll
                for (int u = 0; u < 6; ++u) m[21 + u] = J[u] * r;
                m[27] = r * r;
                m[28] = 1.0;
            }
        }
        if (a.corr) a.corr[i] = jout;
    }
    reduce_moments<ICP_MOMENTS>(m, s_red, a.partial);
}

constexpr auto k_icp_solve29 = k_icp_solve<ICP_MOMENTS, 27, -1>;   // slot 27: sum r^2, slot 28: the count

}  // namespace

struct IcpWork {
    TargetGrid grids[ICP_MAX_STAGES];
    VoxelWork vox;
    DBuf<float> in_t, in_s;        // the host-pointer entry points' device copies (grow-only)
    DBuf<double> partial, out;
    DBuf<IcpState> st;
    DBuf<int32_t> corr;
    EventSpans<4> spans;        // sample, grid, loop
    IcpState h_init, h_st;      // the upload's source and the read-back's destination (never the same memory in flight)
};
IcpWork *icp_work_create() { return new IcpWork; }
void icp_work_destroy(IcpWork *w) { delete w; }

namespace {

// the refinement on device clouds: target n_t x 6, source `s_stride` floats per point, bounding boxes known
int refine_dev(plade_ctx *ctx, IcpWork &W, const float *d_tgt, uint32_t n_t, const float tmn[3], const float tmx[3], const float *d_src,
               uint32_t n_s, uint32_t s_stride, const float smn[3], const float smx[3], const float *T_in16, const plade_icp_params *prm,
               float *T_out16, plade_icp_result *res) {
    const IcpConfig c = resolve(prm, tmn, tmx, "refine_icp");
    float T_in[16];
    memcpy(T_in, T_in16, sizeof(T_in));
    W.spans.mark(ctx, 0);
    // sample: VoxelGrid of the source (waits for its size)
    const uint32_t n = W.vox.run(ctx, d_src, s_stride, nullptr, nullptr, n_s, 1, (float)c.leaf, smn, smx);
    W.spans.mark(ctx, 1);
    IcpArgs a;
    memset(&a, 0, sizeof(a));
    for (int s = 0; s < c.n_stages; ++s) a.g[s] = stage_grid(ctx, W.grids[s], d_tgt, n_t, tmn, tmx, c.dist[s], "refine_icp");
    W.spans.mark(ctx, 2);
    const uint32_t blocks = std::max(1u, cdiv(n, CORR_TPB));
    a.tgt = d_tgt; a.src = W.vox.out_xyz.p; a.stride = 3; a.n = n;
    a.st = W.st.ensure(1);
    a.partial = W.partial.ensure((size_t)blocks * ICP_MOMENTS);
    a.corr = nullptr;
    double T[16];
    for (int k = 0; k < 16; ++k) T[k] = T_in[k];
    init_state(W.h_init, T, nullptr);
    HIP_TRY(hipMemcpyAsync(W.st.p, &W.h_init, sizeof(IcpState), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_icp_mean_part, dim3(blocks), dim3(CORR_TPB), 0, ctx->stream, a.src, 3u, n, a.partial);
    hipLaunchKernelGGL(k_icp_mean, dim3(1), dim3(64), 0, ctx->stream, a.st, (const double *)a.partial, blocks, n);
    IcpSolveArgs sa;
    sa.st = a.st; sa.partial = a.partial; sa.blocks = blocks; sa.n_stages = c.n_stages; sa.max_iter = c.max_iter;
    sa.min_corr = c.min_corr; sa.eps_rot = c.eps_rot; sa.eps_trans = c.eps_trans; sa.moments = nullptr;
    for (int it = 0; it < c.max_iter; ++it) {
        hipLaunchKernelGGL(k_icp_corr_lin, dim3(blocks), dim3(CORR_TPB), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_icp_solve29, dim3(1), dim3(64), 0, ctx->stream, sa);
    }
    HIP_TRY(hipGetLastError());
    W.spans.mark(ctx, 3);
    HIP_TRY(hipMemcpyAsync(&W.h_st, W.st.p, sizeof(IcpState), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    const IcpState &s = W.h_st;
    plade_icp_result r;
    memset(&r, 0, sizeof(r));
    r.iterations = s.iter;
    r.stages = s.lin_stage + 1;
    r.converged = s.converged;
    r.failure = s.failure;
    r.correspondences = s.count;
    r.samples = n;
    r.rmse = s.count ? std::sqrt(s.sum_r2 / (double)s.count) : 0.0;
    r.fitness = n ? (double)s.count / (double)n : 0.0;
    r.final_dist = c.dist[s.lin_stage];
    if (res) *res = r;
    W.spans.collect();
    ctx->stats.clear();
    ctx->stats.add("icp_sample_s", W.spans.seconds(0));
    ctx->stats.add("icp_grid_s", W.spans.seconds(1));
    ctx->stats.add("icp_loop_s", W.spans.seconds(2));
    ctx->stats.add("icp_iterations", s.iter);
    ctx->stats.add("icp_stages", c.n_stages);
    grid_stats(ctx, "icp", W.grids[0]);              // the first (widest) stage
    if (s.failure) {
        memmove(T_out16, T_in, sizeof(T_in));
        ctx->last_error = s.failure == PLADE_ICP_TOO_FEW ? "refine_icp: too few correspondences"
                                                          : "refine_icp: degenerate geometry (the system is singular)";
        return PLADE_EFAIL;
    }
    for (int k = 0; k < 12; ++k) T_out16[k] = (float)s.T[k];
    T_out16[12] = 0.f; T_out16[13] = 0.f; T_out16[14] = 0.f; T_out16[15] = 1.f;
    return PLADE_OK;
}

IcpWork &work_of(plade_ctx *ctx) {
    if (!ctx->icp_work) ctx->icp_work = icp_work_create();
    return *ctx->icp_work;
}

}  // namespace
}  // namespace plade

using namespace plade;

// ---- C ABI (include/plade_hip.h) ---------------------------------------------------------------------------------------------
extern "C" void plade_icp_default_params(plade_icp_params *p) {
    if (!p) return;
    p->source_leaf = 0.0;           // 0.005 D
    p->max_dist = 0.0;              // 0.025 D
    p->min_dist = 0.0;              // 0.0025 D
    p->eps_rotation = 1e-6;
    p->eps_translation = 0.0;       // 1e-6 D
    p->max_iterations = 60;
    p->min_correspondences = 100;
}

extern "C" int plade_refine_icp(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t, const float *src_pos_nrm, uint32_t n_s,
                                const float *T_in16, const plade_icp_params *params, float *T_out16, plade_icp_result *result) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(tgt_pos_nrm && src_pos_nrm && T_in16 && T_out16, PLADE_EINVAL, "plade_refine_icp: bad argument");
        PLADE_REQUIRE(n_t >= 1 && n_s >= 1, PLADE_EINVAL, "plade_refine_icp: empty cloud");
        check_T(T_in16, "refine_icp");
        IcpWork &W = work_of(ctx);
        float tmn[3], tmx[3], smn[3], smx[3];
        upload_rows(ctx, W.in_t, tgt_pos_nrm, n_t, 6, tmn, tmx);
        upload_rows(ctx, W.in_s, src_pos_nrm, n_s, 6, smn, smx);
        return refine_dev(ctx, W, W.in_t.p, n_t, tmn, tmx, W.in_s.p, n_s, 6, smn, smx, T_in16, params, T_out16, result);
    });
}

extern "C" int plade_refine_icp_dev(plade_ctx *ctx, plade_cloud *tgt, plade_cloud *src, const float *T_in16,
                                    const plade_icp_params *params, float *T_out16, plade_icp_result *result) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(tgt && src && T_in16 && T_out16, PLADE_EINVAL, "plade_refine_icp_dev: bad argument");
        PLADE_REQUIRE(tgt->dev.n >= 1 && src->dev.n >= 1, PLADE_EINVAL, "plade_refine_icp_dev: empty cloud");
        check_T(T_in16, "refine_icp");
        IcpWork &W = work_of(ctx);
        const CloudDev &t = tgt->dev, &s = src->dev;
        return refine_dev(ctx, W, t.aos.p, t.n, t.bbmin, t.bbmax, s.aos.p, s.n, 6, s.bbmin, s.bbmax, T_in16, params, T_out16, result);
    });
}

extern "C" int plade_icp_linearize(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t, const float *src_xyz, uint32_t n_s,
                                   uint32_t stride, const double *T16, const double *center, float dist, int32_t *corr_out,
                                   double *moments_out) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(tgt_pos_nrm && src_xyz && T16 && center && moments_out, PLADE_EINVAL, "plade_icp_linearize: bad argument");
        PLADE_REQUIRE(n_t >= 1 && n_s >= 1 && stride >= 3, PLADE_EINVAL, "plade_icp_linearize: empty cloud or stride < 3");
        PLADE_REQUIRE(std::isfinite(dist) && dist > 0.f, PLADE_EINVAL, "plade_icp_linearize: dist must be finite and > 0");
        for (int k = 0; k < 16; ++k) PLADE_REQUIRE(std::isfinite(T16[k]), PLADE_EINVAL, "plade_icp_linearize: T must be finite");
        for (int k = 0; k < 3; ++k) PLADE_REQUIRE(std::isfinite(center[k]), PLADE_EINVAL, "plade_icp_linearize: center must be finite");
        IcpWork &W = work_of(ctx);
        float tmn[3], tmx[3], smn[3], smx[3];
        upload_rows(ctx, W.in_t, tgt_pos_nrm, n_t, 6, tmn, tmx);
        upload_rows(ctx, W.in_s, src_xyz, n_s, stride, smn, smx);
        IcpArgs a;
        memset(&a, 0, sizeof(a));
        a.g[0] = stage_grid(ctx, W.grids[0], W.in_t.p, n_t, tmn, tmx, (double)dist, "refine_icp");
        a.g[0].d2 = dist * dist;
        const uint32_t blocks = cdiv(n_s, CORR_TPB);
        a.tgt = W.in_t.p; a.src = W.in_s.p; a.stride = stride; a.n = n_s;
        a.st = W.st.ensure(1);
        a.partial = W.partial.ensure((size_t)blocks * ICP_MOMENTS);
        a.corr = W.corr.ensure(n_s);
        init_state(W.h_init, T16, center);
        HIP_TRY(hipMemcpyAsync(W.st.p, &W.h_init, sizeof(IcpState), hipMemcpyHostToDevice, ctx->stream));
        IcpSolveArgs sa;
        memset(&sa, 0, sizeof(sa));
        sa.st = a.st; sa.partial = a.partial; sa.blocks = blocks; sa.moments = W.out.ensure(ICP_MOMENTS);
        hipLaunchKernelGGL(k_icp_corr_lin, dim3(blocks), dim3(CORR_TPB), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_icp_solve29, dim3(1), dim3(64), 0, ctx->stream, sa);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(moments_out, sa.moments, ICP_MOMENTS * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (corr_out) HIP_TRY(hipMemcpyAsync(corr_out, a.corr, (size_t)n_s * 4, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        grid_stats(ctx, "icp", W.grids[0]);
        return PLADE_OK;
    });
}
