// plade_amd/csrc/k_gicp.hip -- plane-to-plane (generalized) ICP refinement on gfx950 (semantics: gicp.h).
//
// Layout (what is not named here is the point-to-plane ICP's, shared through icp_core.h: k_icp.hip)
//   sample  merge_fuse_one (merge.h): the source voxel-fused with its normals, n x 6 rows in the context's MergeWork
//   grids   one TargetGrid per stage distance, in the context's GicpWork
//   mean    k_icp_mean_part / k_icp_mean on the sample's x y z (stride 6)
//   loop    max_iterations pairs (k_gicp_corr_lin, k_icp_solve<30>) queued with no host wait in between
//   corr    k_gicp_corr_lin: one lane per sample point, 256 lanes per workgroup.  The match of k_icp_corr_lin; with a correspondence
//           the lane gathers n_j from the target's row and m from its own row, forms Sigma, M = adj(Sigma) / det, M e and M J in
//           fp64 in the written order of gicp.h, and the 30 moments go through the fixed-order reduction (LDS: 4 x 30 doubles)
#include "gicp.h"
#include "icp_core.h"
#include "merge.h"
#include "voxel.h"

namespace plade {

namespace {

struct GicpArgs {
    IcpGridArgs g[ICP_MAX_STAGES];
    const float *tgt;    // n_t x 6: the normals are gathered by the original index
    const float *src;    // n x 6 sample rows: x y z and the normal m
    uint32_t n;
    double k;            // 1 - epsilon
    IcpState *st;
    double *partial;     // gridDim.x x GICP_MOMENTS
    int32_t *corr;       // seam: j or -1 per point (nullptr in the loop)
};

__global__ __launch_bounds__(CORR_TPB) void k_gicp_corr_lin(const GicpArgs a) {
    __shared__ double s_red[CORR_TPB / 64][GICP_MOMENTS];
    const IcpState *st = a.st;
    if (st->done) return;                              // (uniform)
    const IcpGridArgs &G = a.g[st->stage];
    const uint32_t i = blockIdx.x * CORR_TPB + threadIdx.x;
    double m[GICP_MOMENTS];
#pragma unroll
    for (int q = 0; q < GICP_MOMENTS; ++q) m[q] = 0.0;
    if (i < a.n) {
        const float *s = a.src + (size_t)i * 6;
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
            const double m0 = s[3], m1 = s[4], m2 = s[5];
            const double ln2 = (n0 * n0 + n1 * n1) + n2 * n2, lm2 = (m0 * m0 + m1 * m1) + m2 * m2;
            // (a non-finite component makes the sum NaN or +inf: NaN fails > 0, and isfinite catches an infinite one)
            if (isfinite(n0) && isfinite(n1) && isfinite(n2) && ln2 > 0.0 && isfinite(m0) && isfinite(m1) && isfinite(m2) && lm2 > 0.0) {
                jout = (int32_t)j;
                const double *T = st->T;
                const double X = x, Y = y, Z = z;
                double e[3], u[3], nh[3], ah[3];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const double p = ((T[4 * r] * X + T[4 * r + 1] * Y) + T[4 * r + 2] * Z) + T[4 * r + 3];
                    e[r] = p - (double)t[r];
                    u[r] = p - st->c[r];
                    ah[r] = (T[4 * r] * m0 + T[4 * r + 1] * m1) + T[4 * r + 2] * m2;
                }
                const double ln = sqrt(ln2), la = sqrt((ah[0] * ah[0] + ah[1] * ah[1]) + ah[2] * ah[2]);
                nh[0] = n0 / ln; nh[1] = n1 / ln; nh[2] = n2 / ln;
                ah[0] = ah[0] / la; ah[1] = ah[1] / la; ah[2] = ah[2] / la;
                const double k = a.k;
                // Sigma = 2 I - k nh nh^T - k ah ah^T
                const double S00 = (2.0 - k * (nh[0] * nh[0])) - k * (ah[0] * ah[0]);
                const double S01 = (0.0 - k * (nh[0] * nh[1])) - k * (ah[0] * ah[1]);
                const double S02 = (0.0 - k * (nh[0] * nh[2])) - k * (ah[0] * ah[2]);
                const double S11 = (2.0 - k * (nh[1] * nh[1])) - k * (ah[1] * ah[1]);
                const double S12 = (0.0 - k * (nh[1] * nh[2])) - k * (ah[1] * ah[2]);
                const double S22 = (2.0 - k * (nh[2] * nh[2])) - k * (ah[2] * ah[2]);
                // M = adj(Sigma) / det
                const double C00 = S11 * S22 - S12 * S12, C01 = S02 * S12 - S01 * S22, C02 = S01 * S12 - S02 * S11;
                const double C11 = S00 * S22 - S02 * S02, C12 = S01 * S02 - S00 * S12, C22 = S00 * S11 - S01 * S01;
                const double det = (S00 * C00 + S01 * C01) + S02 * C02;
                double M[3][3];
                M[0][0] = C00 / det; M[0][1] = C01 / det; M[0][2] = C02 / det;
                M[1][1] = C11 / det; M[1][2] = C12 / det; M[2][2] = C22 / det;
                M[1][0] = M[0][1]; M[2][0] = M[0][2]; M[2][1] = M[1][2];
                // w = M e, Gm = M J with J = [-[u]x | I]
                double w[3], Gm[3][6];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    w[r] = (M[r][0] * e[0] + M[r][1] * e[1]) + M[r][2] * e[2];
                    Gm[r][0] = M[r][2] * u[1] - M[r][1] * u[2];
                    Gm[r][1] = M[r][0] * u[2] - M[r][2] * u[0];
                    Gm[r][2] = M[r][1] * u[0] - M[r][0] * u[1];
                    Gm[r][3] = M[r][0]; Gm[r][4] = M[r][1]; Gm[r][5] = M[r][2];
                }
                // row a of J^T applied to the 3-vector v
                auto JT = [&](int row, double v0, double v1, double v2) -> double {
                    return row == 0 ? v2 * u[1] - v1 * u[2] : row == 1 ? v0 * u[2] - v2 * u[0] : row == 2 ? v1 * u[0] - v0 * u[1]
                         : row == 3 ? v0 : row == 4 ? v1 : v2;
                };
                int o = 0;
#pragma unroll
                for (int r = 0; r < 6; ++r)
#pragma unroll
                    for (int c = r; c < 6; ++c) m[o++] = JT(r, Gm[0][c], Gm[1][c], Gm[2][c]);
#pragma unroll
                for (int r = 0; r < 6; ++r) m[21 + r] = JT(r, w[0], w[1], w[2]);
                m[27] = (e[0] * w[0] + e[1] * w[1]) + e[2] * w[2];
                m[28] = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
                m[29] = 1.0;
            }
        }
        if (a.corr) a.corr[i] = jout;
    }
    reduce_moments<GICP_MOMENTS>(m, s_red, a.partial);
}

constexpr auto k_gicp_solve = k_icp_solve<GICP_MOMENTS, 28, 27>;   // slot 28: sum |e|^2, 27: sum e^T M e, 29: the count

}  // namespace

struct GicpWork {
    TargetGrid grids[ICP_MAX_STAGES];
    DBuf<float> in_t, in_s;        // the host-pointer entry points' device copies (grow-only)
    DBuf<double> partial, out;
    DBuf<IcpState> st;
    DBuf<int32_t> corr;
    EventSpans<4> spans;        // sample, grid, loop
    IcpState h_init, h_st;      // the upload's source and the read-back's destination (never the same memory in flight)
};
GicpWork *gicp_work_create() { return new GicpWork; }
void gicp_work_destroy(GicpWork *w) { delete w; }

namespace {

// epsilon as given -> the value used (0: 1e-3)
double resolve_epsilon(double eps, const char *who) {
    PLADE_REQUIRE(std::isfinite(eps) && eps >= 0.0 && eps <= 1.0, PLADE_EINVAL,
                  std::string(who) + ": epsilon must be finite, 0 (the default 1e-3) or in (0, 1]");
    return eps > 0.0 ? eps : 1e-3;
}

// the refinement on device clouds: target n_t x 6, source n_s x 6, the target's bounding box known
int refine_dev(plade_ctx *ctx, GicpWork &W, const float *d_tgt, uint32_t n_t, const float tmn[3], const float tmx[3], const float *d_src,
               uint32_t n_s, const float *T_in16, const plade_gicp_params *prm, float *T_out16, plade_gicp_result *res) {
    plade_gicp_params gp;
    if (prm) gp = *prm; else plade_gicp_default_params(&gp);
    plade_icp_params ip;
    ip.source_leaf = gp.source_leaf; ip.max_dist = gp.max_dist; ip.min_dist = gp.min_dist; ip.eps_rotation = gp.eps_rotation;
    ip.eps_translation = gp.eps_translation; ip.max_iterations = gp.max_iterations; ip.min_correspondences = gp.min_correspondences;
    const IcpConfig c = resolve(&ip, tmn, tmx, "refine_gicp");
    const double eps = resolve_epsilon(gp.epsilon, "refine_gicp");
    float T_in[16];
    memcpy(T_in, T_in16, sizeof(T_in));
    W.spans.mark(ctx, 0);
    // sample: the voxel fuse of the source with its normals (waits for its size)
    const float *d_sample = nullptr;
    const uint32_t n = merge_fuse_one(ctx, d_src, n_s, (float)c.leaf, &d_sample, "refine_gicp");
    W.spans.mark(ctx, 1);
    GicpArgs a;
    memset(&a, 0, sizeof(a));
    for (int s = 0; s < c.n_stages; ++s) a.g[s] = stage_grid(ctx, W.grids[s], d_tgt, n_t, tmn, tmx, c.dist[s], "refine_gicp");
    W.spans.mark(ctx, 2);
    const uint32_t blocks = std::max(1u, cdiv(n, CORR_TPB));
    a.tgt = d_tgt; a.src = d_sample; a.n = n; a.k = 1.0 - eps;
    a.st = W.st.ensure(1);
    a.partial = W.partial.ensure((size_t)blocks * GICP_MOMENTS);
    a.corr = nullptr;
    double T[16];
    for (int k = 0; k < 16; ++k) T[k] = T_in[k];
    init_state(W.h_init, T, nullptr);
    HIP_TRY(hipMemcpyAsync(W.st.p, &W.h_init, sizeof(IcpState), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_icp_mean_part, dim3(blocks), dim3(CORR_TPB), 0, ctx->stream, a.src, 6u, n, a.partial);
    hipLaunchKernelGGL(k_icp_mean, dim3(1), dim3(64), 0, ctx->stream, a.st, (const double *)a.partial, blocks, n);
    IcpSolveArgs sa;
    sa.st = a.st; sa.partial = a.partial; sa.blocks = blocks; sa.n_stages = c.n_stages; sa.max_iter = c.max_iter;
    sa.min_corr = c.min_corr; sa.eps_rot = c.eps_rot; sa.eps_trans = c.eps_trans; sa.moments = nullptr;
    for (int it = 0; it < c.max_iter; ++it) {
        hipLaunchKernelGGL(k_gicp_corr_lin, dim3(blocks), dim3(CORR_TPB), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_gicp_solve, dim3(1), dim3(64), 0, ctx->stream, sa);
    }
    HIP_TRY(hipGetLastError());
    W.spans.mark(ctx, 3);
    HIP_TRY(hipMemcpyAsync(&W.h_st, W.st.p, sizeof(IcpState), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    const IcpState &s = W.h_st;
    plade_gicp_result r;
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
    r.cost = s.count ? s.sum_aux / (double)s.count : 0.0;
    if (res) *res = r;
    W.spans.collect();
    ctx->stats.clear();
    ctx->stats.add("gicp_sample_s", W.spans.seconds(0));
    ctx->stats.add("gicp_grid_s", W.spans.seconds(1));
    ctx->stats.add("gicp_loop_s", W.spans.seconds(2));
    ctx->stats.add("gicp_iterations", s.iter);
    ctx->stats.add("gicp_stages", c.n_stages);
    grid_stats(ctx, "gicp", W.grids[0]);             // the first (widest) stage
    if (s.failure) {
        memmove(T_out16, T_in, sizeof(T_in));
        ctx->last_error = s.failure == PLADE_ICP_TOO_FEW ? "refine_gicp: too few correspondences"
                                                          : "refine_gicp: degenerate geometry (the system is singular)";
        return PLADE_EFAIL;
    }
    for (int k = 0; k < 12; ++k) T_out16[k] = (float)s.T[k];
    T_out16[12] = 0.f; T_out16[13] = 0.f; T_out16[14] = 0.f; T_out16[15] = 1.f;
    return PLADE_OK;
}

GicpWork &work_of(plade_ctx *ctx) {
    if (!ctx->gicp_work) ctx->gicp_work = gicp_work_create();
    return *ctx->gicp_work;
}

}  // namespace
}  // namespace plade

using namespace plade;

// ---- C ABI (include/plade_hip.h) ---------------------------------------------------------------------------------------------
extern "C" void plade_gicp_default_params(plade_gicp_params *p) {
    if (!p) return;
    p->source_leaf = 0.0;           // 0.005 D
    p->max_dist = 0.0;              // 0.025 D
    p->min_dist = 0.0;              // 0.0025 D
    p->eps_rotation = 1e-6;
    p->eps_translation = 0.0;       // 1e-6 D
    p->max_iterations = 60;
    p->min_correspondences = 100;
    p->epsilon = 1e-3;
}

extern "C" int plade_refine_gicp(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t, const float *src_pos_nrm, uint32_t n_s,
                                 const float *T_in16, const plade_gicp_params *params, float *T_out16, plade_gicp_result *result) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(tgt_pos_nrm && src_pos_nrm && T_in16 && T_out16, PLADE_EINVAL, "plade_refine_gicp: bad argument");
        PLADE_REQUIRE(n_t >= 1 && n_s >= 1, PLADE_EINVAL, "plade_refine_gicp: empty cloud");
        check_T(T_in16, "refine_gicp");
        GicpWork &W = work_of(ctx);
        float tmn[3], tmx[3], smn[3], smx[3];
        upload_rows(ctx, W.in_t, tgt_pos_nrm, n_t, 6, tmn, tmx);
        upload_rows(ctx, W.in_s, src_pos_nrm, n_s, 6, smn, smx);
        return refine_dev(ctx, W, W.in_t.p, n_t, tmn, tmx, W.in_s.p, n_s, T_in16, params, T_out16, result);
    });
}

extern "C" int plade_refine_gicp_dev(plade_ctx *ctx, plade_cloud *tgt, plade_cloud *src, const float *T_in16,
                                     const plade_gicp_params *params, float *T_out16, plade_gicp_result *result) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(tgt && src && T_in16 && T_out16, PLADE_EINVAL, "plade_refine_gicp_dev: bad argument");
        PLADE_REQUIRE(tgt->dev.n >= 1 && src->dev.n >= 1, PLADE_EINVAL, "plade_refine_gicp_dev: empty cloud");
        check_T(T_in16, "refine_gicp");
        GicpWork &W = work_of(ctx);
        const CloudDev &t = tgt->dev, &s = src->dev;
        return refine_dev(ctx, W, t.aos.p, t.n, t.bbmin, t.bbmax, s.aos.p, s.n, T_in16, params, T_out16, result);
    });
}

extern "C" int plade_gicp_linearize(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t, const float *src_pos_nrm, uint32_t n_s,
                                    const double *T16, const double *center, float dist, double epsilon, int32_t *corr_out,
                                    double *moments_out) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(tgt_pos_nrm && src_pos_nrm && T16 && center && moments_out, PLADE_EINVAL, "plade_gicp_linearize: bad argument");
        PLADE_REQUIRE(n_t >= 1 && n_s >= 1, PLADE_EINVAL, "plade_gicp_linearize: empty cloud");
        PLADE_REQUIRE(std::isfinite(dist) && dist > 0.f, PLADE_EINVAL, "plade_gicp_linearize: dist must be finite and > 0");
        for (int k = 0; k < 16; ++k) PLADE_REQUIRE(std::isfinite(T16[k]), PLADE_EINVAL, "plade_gicp_linearize: T must be finite");
        for (int k = 0; k < 3; ++k) PLADE_REQUIRE(std::isfinite(center[k]), PLADE_EINVAL, "plade_gicp_linearize: center must be finite");
        const double eps = resolve_epsilon(epsilon, "plade_gicp_linearize");
        GicpWork &W = work_of(ctx);
        float tmn[3], tmx[3], smn[3], smx[3];
        upload_rows(ctx, W.in_t, tgt_pos_nrm, n_t, 6, tmn, tmx);
        upload_rows(ctx, W.in_s, src_pos_nrm, n_s, 6, smn, smx);
        GicpArgs a;
        memset(&a, 0, sizeof(a));
        a.g[0] = stage_grid(ctx, W.grids[0], W.in_t.p, n_t, tmn, tmx, (double)dist, "plade_gicp_linearize");
        a.g[0].d2 = dist * dist;
        const uint32_t blocks = cdiv(n_s, CORR_TPB);
        a.tgt = W.in_t.p; a.src = W.in_s.p; a.n = n_s; a.k = 1.0 - eps;
        a.st = W.st.ensure(1);
        a.partial = W.partial.ensure((size_t)blocks * GICP_MOMENTS);
        a.corr = W.corr.ensure(n_s);
        init_state(W.h_init, T16, center);
        HIP_TRY(hipMemcpyAsync(W.st.p, &W.h_init, sizeof(IcpState), hipMemcpyHostToDevice, ctx->stream));
        IcpSolveArgs sa;
        memset(&sa, 0, sizeof(sa));
        sa.st = a.st; sa.partial = a.partial; sa.blocks = blocks; sa.moments = W.out.ensure(GICP_MOMENTS);
        hipLaunchKernelGGL(k_gicp_corr_lin, dim3(blocks), dim3(CORR_TPB), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_gicp_solve, dim3(1), dim3(64), 0, ctx->stream, sa);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(moments_out, sa.moments, GICP_MOMENTS * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (corr_out) HIP_TRY(hipMemcpyAsync(corr_out, a.corr, (size_t)n_s * 4, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        grid_stats(ctx, "gicp", W.grids[0]);
        return PLADE_OK;
    });
}
