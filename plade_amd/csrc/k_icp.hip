// plade_amd/csrc/k_icp.hip -- point-to-plane ICP refinement on gfx950 (semantics: icp.h).
//
// Layout
//   grids   one dense row index of TargetGrid per stage distance d, cell >= d: the 27 cells around a probe's cell (for_block27,
//           grid_walk.h) hold every target point closer than d, so the argmin over them is the exact one whenever it is below d
//           (and the probe has no correspondence otherwise).  The grids are built up front.
//   mean    k_icp_mean_part / k_icp_mean: the fp64 mean s-bar of the sample, once, in a fixed order (one partial per workgroup:
//           a butterfly across each wave, then the waves in order; one wavefront then sums the partials like k_icp_solve); the
//           second kernel also sets the first centre c_0 = T_0 s-bar.
//   loop    max_iterations pairs (k_corr_lin<IcpModel>, k_icp_solve) queued on the context's stream with no host wait in between; the
//           state word lives on the device (IcpState), and once it says done every later kernel returns at once.
//   corr    k_corr_lin<IcpModel>: one lane per sample point.  The lane forms p' in fp32, takes the exact (d, j) argmin key over the
//           nine runs of the current stage's grid, and -- with a correspondence -- r and J (about the centre c_k) in fp64; the 29 moments are summed
//           across the wave (butterfly), then the four waves in order, and each workgroup writes one partial to its own slot.
//   solve   k_icp_solve: one wavefront sums the partials in a fixed order (lane l: partials l, l + 64, ..., then a butterfly),
//           and lane 0 runs the Cholesky solve, Rodrigues, the update of T and c and the stage / convergence / failure rules.
#include "icp_core.h"

namespace plade {

namespace {

// (the state, the mean, the match, the reduction, k_icp_solve and the host's loop are shared with the plane-to-plane ICP: icp_core.h)
struct IcpModel {
    static constexpr int NM = ICP_MOMENTS, R2 = 27, AUX = -1;     // slot 27: sum r^2, slot 28: the count
    static constexpr uint32_t STRIDE = 3;                         // the sample: x y z
    static constexpr const char *prefix = "icp", *who = "refine_icp", *seam = "plade_icp_linearize", *seam_grid = "refine_icp",
                                *seam_empty = "empty cloud or stride < 3";
    static constexpr WorkSlot plade_ctx::*slot = &plade_ctx::icp_work;
    using params = plade_icp_params;
    using result = plade_icp_result;
    struct Args {
        IcpGridArgs g[ICP_MAX_STAGES];
        const float *tgt;    // n_t x 6: the normals are gathered by the original index
        const float *src;    // sample points, `stride` floats apart
        uint32_t stride, n;
        IcpState *st;
        double *partial;     // gridDim.x x ICP_MOMENTS
        int32_t *corr;       // seam: j or -1 per point (nullptr in the loop)
    };
    static void defaults(params *p) { plade_icp_default_params(p); }
    static double epsilon_of(const params &) { return 0.0; }
    static void extra(Args &, double, const char *) {}
    static void source(Args &a, const float *rows, uint32_t stride) { a.src = rows; a.stride = stride; }
    static void finish(result &, const IcpState &) {}
    // VoxelGrid of the source's x y z
    static uint32_t sample(plade_ctx *ctx, RefineWork &W, const float *d_src, uint32_t n_s, float leaf, const float smn[3],
                           const float smx[3], const float **rows) {
        const uint32_t n = W.vox.run(ctx, d_src, 6, nullptr, nullptr, n_s, 1, leaf, smn, smx);
        *rows = W.vox.out_xyz.p;
        return n;
    }
    static __device__ __forceinline__ const float *row(const Args &a, uint32_t i) { return a.src + (size_t)i * a.stride; }
    // r and J (about the centre c_k) in fp64, the written expressions of icp.h
    static __device__ __forceinline__ bool linearise(const Args &, float x, float y, float z, const float *, const float *t,
                                                     const IcpState *st, double (&m)[NM]) {
        const double n0 = t[3], n1 = t[4], n2 = t[5];
        if (!(isfinite(n0) && isfinite(n1) && isfinite(n2))) return false;
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
        return true;
    }
};

}  // namespace

}  // namespace plade

using namespace plade;

// ---- C ABI (include/plade_hip.h) ---------------------------------------------------------------------------------------------
extern "C" void plade_icp_default_params(plade_icp_params *p) {
    if (p) default_common(p);
}

extern "C" int plade_refine_icp(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t, const float *src_pos_nrm, uint32_t n_s,
                                const float *T_in16, const plade_icp_params *params, float *T_out16, plade_icp_result *result) {
    return refine_host<IcpModel>(ctx, tgt_pos_nrm, n_t, src_pos_nrm, n_s, T_in16, params, T_out16, result);
}

extern "C" int plade_refine_icp_dev(plade_ctx *ctx, plade_cloud *tgt, plade_cloud *src, const float *T_in16,
                                    const plade_icp_params *params, float *T_out16, plade_icp_result *result) {
    return refine_resident<IcpModel>(ctx, tgt, src, T_in16, params, T_out16, result);
}

extern "C" int plade_icp_linearize(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t, const float *src_xyz, uint32_t n_s,
                                   uint32_t stride, const double *T16, const double *center, float dist, int32_t *corr_out,
                                   double *moments_out) {
    return linearize_seam<IcpModel>(ctx, tgt_pos_nrm, n_t, src_xyz, n_s, stride, T16, center, dist, 0.0, corr_out, moments_out);
}
