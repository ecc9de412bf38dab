// plade_amd/csrc/k_gicp.hip -- plane-to-plane (generalized) ICP refinement on gfx950 (semantics: gicp.h).
//
// Layout (what is not named here is the point-to-plane ICP's, shared through icp_core.h: k_icp.hip)
//   sample  merge_fuse_one (merge.h): the source voxel-fused with its normals, n x 6 rows in the context's MergeWork
//   grids   one TargetGrid per stage distance, in the context's second RefineWork
//   mean    k_icp_mean_part / k_icp_mean on the sample's x y z (stride 6)
//   loop    max_iterations pairs (k_corr_lin<GicpModel>, k_icp_solve<30>) queued with no host wait in between
//   corr    k_corr_lin<GicpModel>: one lane per sample point, 256 lanes per workgroup.  The match is shared; with a correspondence
//           the lane gathers n_j from the target's row and m from its own row, forms Sigma, M = adj(Sigma) / det, M e and M J in
//           fp64 in the written order of gicp.h, and the 30 moments go through the fixed-order reduction (LDS: 4 x 30 doubles)
#include "gicp.h"
#include "icp_core.h"
#include "merge.h"

namespace plade {

namespace {

// epsilon as given -> the value used (0: 1e-3)
double resolve_epsilon(double eps, const char *who) {
    PLADE_REQUIRE(std::isfinite(eps) && eps >= 0.0 && eps <= 1.0, PLADE_EINVAL,
                  std::string(who) + ": epsilon must be finite, 0 (the default 1e-3) or in (0, 1]");
    return eps > 0.0 ? eps : 1e-3;
}

struct GicpModel {
    static constexpr int NM = GICP_MOMENTS, R2 = 28, AUX = 27;    // slot 28: sum |e|^2, 27: sum e^T M e, 29: the count
    static constexpr uint32_t STRIDE = 6;                         // the sample: x y z and the normal m
    static constexpr const char *prefix = "gicp", *who = "refine_gicp", *seam = "plade_gicp_linearize",
                                *seam_grid = "plade_gicp_linearize", *seam_empty = "empty cloud";
    static constexpr WorkSlot plade_ctx::*slot = &plade_ctx::gicp_work;
    using params = plade_gicp_params;
    using result = plade_gicp_result;
    struct Args {
        IcpGridArgs g[ICP_MAX_STAGES];
        const float *tgt;    // n_t x 6: the normals are gathered by the original index
        const float *src;    // n x 6 sample rows: x y z and the normal m
        uint32_t n;
        double k;            // 1 - epsilon
        IcpState *st;
        double *partial;     // gridDim.x x GICP_MOMENTS
        int32_t *corr;       // seam: j or -1 per point (nullptr in the loop)
    };
    static void defaults(params *p) { plade_gicp_default_params(p); }
    static double epsilon_of(const params &p) { return p.epsilon; }
    static void extra(Args &a, double epsilon, const char *who) { a.k = 1.0 - resolve_epsilon(epsilon, who); }
    static void source(Args &a, const float *rows, uint32_t) { a.src = rows; }
    static void finish(result &r, const IcpState &s) { r.cost = s.count ? s.sum_aux / (double)s.count : 0.0; }
    // the voxel fuse of the source with its normals, in the context's MergeWork (the source's bounding box is not needed)
    static uint32_t sample(plade_ctx *ctx, RefineWork &, const float *d_src, uint32_t n_s, float leaf, const float *, const float *,
                           const float **rows) {
        return merge_fuse_one(ctx, d_src, n_s, leaf, rows, "refine_gicp");
    }
    static __device__ __forceinline__ const float *row(const Args &a, uint32_t i) { return a.src + (size_t)i * 6; }
    // Sigma, M = adj(Sigma) / det, M e and M J in fp64, the written expressions of gicp.h
    static __device__ __forceinline__ bool linearise(const Args &a, float x, float y, float z, const float *s, const float *t,
                                                     const IcpState *st, double (&m)[NM]) {
        const double n0 = t[3], n1 = t[4], n2 = t[5];
        const double m0 = s[3], m1 = s[4], m2 = s[5];
        const double ln2 = (n0 * n0 + n1 * n1) + n2 * n2, lm2 = (m0 * m0 + m1 * m1) + m2 * m2;
        // (a non-finite component makes the sum NaN or +inf: NaN fails > 0, and isfinite catches an infinite one)
        // (the arithmetic sits inside this test, not after an early return: the early return costs four SGPRs)
        const bool ok = isfinite(n0) && isfinite(n1) && isfinite(n2) && ln2 > 0.0 && isfinite(m0) && isfinite(m1) && isfinite(m2) && lm2 > 0.0;
        if (ok) {
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
        return ok;
    }
};

}  // namespace
}  // namespace plade

using namespace plade;

// ---- C ABI (include/plade_hip.h) ---------------------------------------------------------------------------------------------
extern "C" void plade_gicp_default_params(plade_gicp_params *p) {
    if (!p) return;
    default_common(p);
    p->epsilon = 1e-3;
}

extern "C" int plade_refine_gicp(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t, const float *src_pos_nrm, uint32_t n_s,
                                 const float *T_in16, const plade_gicp_params *params, float *T_out16, plade_gicp_result *result) {
    return refine_host<GicpModel>(ctx, tgt_pos_nrm, n_t, src_pos_nrm, n_s, T_in16, params, T_out16, result);
}

extern "C" int plade_refine_gicp_dev(plade_ctx *ctx, plade_cloud *tgt, plade_cloud *src, const float *T_in16,
                                     const plade_gicp_params *params, float *T_out16, plade_gicp_result *result) {
    return refine_resident<GicpModel>(ctx, tgt, src, T_in16, params, T_out16, result);
}

extern "C" int plade_gicp_linearize(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t, const float *src_pos_nrm, uint32_t n_s,
                                    const double *T16, const double *center, float dist, double epsilon, int32_t *corr_out,
                                    double *moments_out) {
    return linearize_seam<GicpModel>(ctx, tgt_pos_nrm, n_t, src_pos_nrm, n_s, 6, T16, center, dist, epsilon, corr_out, moments_out);
}
