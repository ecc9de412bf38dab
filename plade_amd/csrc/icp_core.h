// plade_amd/csrc/icp_core.h -- what the point-to-plane ICP (k_icp.hip, icp.h) and the plane-to-plane ICP (k_gicp.hip, gicp.h) have
// in common: the device state of a refinement, the fp64 mean of the sample, the fixed-order reduction of the moments, the solve /
// update / schedule / failure rules of lane 0, and on the host the resolved parameters and the stage grids.  The two loops differ in
// their match-and-linearise kernel and in the number of moments, which is a template argument here; nothing in this header depends
// on what a moment means beyond the slots named below.
//
// Included by those two .hip files only.  Everything sits in an unnamed namespace: each file gets kernels of its own.
#pragma once
#include "icp.h"
#include "fixed_reduce.h"
#include "grid_walk.h"

namespace plade {
namespace {

constexpr int CORR_TPB = 256;

// the device state of one refinement (one allocation, uploaded once per call)
struct IcpState {
    double T[12];        // the fp64 iterate, rows 0..2 of [R | t]
    double c[3];         // the centre of the linearisation, c_k = T_k s-bar (the seam: given)
    double sbar[3];      // the fp64 mean of the sample
    float Tf[12];        // its fp32 rounding (the match step's transform)
    int32_t done, iter, stage, converged, failure;
    int32_t lin_stage;   // the stage of the last linearisation (stage may have moved on after it: the result reports this one)
    uint32_t count, pad1;
    double sum_r2;       // the moment in slot R2 of the last linearisation
    double sum_aux;      // the moment in slot AUX (plane-to-plane: sum e^T M e; point-to-plane: unused)
};

struct IcpGridArgs {
    GridView g;
    float d2;            // (float)d * (float)d
};

struct IcpSolveArgs {
    IcpState *st;
    const double *partial;
    uint32_t blocks;
    int n_stages, max_iter;
    uint32_t min_corr;
    double eps_rot, eps_trans;
    double *moments;     // seam: the summed moments (nullptr in the loop: solve and update)
};

// the exact (distance, index) argmin key of the probe q over the 27 cells around it: EMPTY when they hold no point
__device__ __forceinline__ u64 nearest_key(const GridView &g, const f3 q) {
    int cx, cy, cz;
    cell_of(g, q, cx, cy, cz);
    u64 best = EMPTY;
    for_block27(g, cx, cy, cz, [&](uint32_t j0, uint32_t j1) {
        for (uint32_t j = j0; j < j1; ++j) {
            const float4 p = g.sorted[j];
            const u64 key = make_key(flann_d2(q, f3(p.x, p.y, p.z)), __float_as_uint(p.w));
            best = key < best ? key : best;
        }
    });
    return best;
}

// a lane's NM moments summed in the fixed order of fixed_reduce.h; the workgroup's sums go to its own slot of `partial`
template <int NM>
__device__ __forceinline__ void reduce_moments(const double (&m)[NM], double (&s_red)[CORR_TPB / 64][NM], double *partial) {
    block_reduce<CORR_TPB>(m, s_red, partial, SumOp());
}

// the fp64 sums of the sample's x y z (`stride` floats apart), one partial per workgroup (the fixed order of reduce_moments)
__global__ __launch_bounds__(CORR_TPB) void k_icp_mean_part(const float *src, uint32_t stride, uint32_t n, double *partial) {
    __shared__ double s_red[CORR_TPB / 64][3];
    const uint32_t i = blockIdx.x * CORR_TPB + threadIdx.x;
    double m[3] = {0.0, 0.0, 0.0};
    if (i < n) { m[0] = src[(size_t)i * stride]; m[1] = src[(size_t)i * stride + 1]; m[2] = src[(size_t)i * stride + 2]; }
    reduce_moments<3>(m, s_red, partial);
}

// T v for the fp64 rows of T (((r0 x + r1 y) + r2 z) + t)
__device__ __forceinline__ void apply_T(const double T[12], const double v[3], double out[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) out[r] = ((T[4 * r] * v[0] + T[4 * r + 1] * v[1]) + T[4 * r + 2] * v[2]) + T[4 * r + 3];
}

// one wavefront: s-bar = the sum of the partials (final_reduce) / n, and c_0 = T_0 s-bar
__global__ __launch_bounds__(64) void k_icp_mean(IcpState *st, const double *partial, uint32_t blocks, uint32_t n) {
    double m[3];
    final_reduce(partial, blocks, m, SumOp());
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) st->sbar[k] = n ? m[k] / (double)n : 0.0;
    double c[3];
    apply_T(st->T, st->sbar, c);
#pragma unroll
    for (int k = 0; k < 3; ++k) st->c[k] = c[k];
}

// fp64 rotation of the axis-angle vector w (Rodrigues); w = 0: the identity
__device__ void rodrigues(const double w[3], double R[9]) {
    const double th = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    R[0] = 1.0; R[1] = 0.0; R[2] = 0.0; R[3] = 0.0; R[4] = 1.0; R[5] = 0.0; R[6] = 0.0; R[7] = 0.0; R[8] = 1.0;
    if (!(th > 0.0)) return;
    const double kx = w[0] / th, ky = w[1] / th, kz = w[2] / th, s = sin(th), c = 1.0 - cos(th);
    // R = I + s K + c K^2, K = [k]x, K^2 = k k^T - I
    R[0] = 1.0 + c * (kx * kx - 1.0); R[1] = -s * kz + c * (kx * ky);   R[2] = s * ky + c * (kx * kz);
    R[3] = s * kz + c * (ky * kx);   R[4] = 1.0 + c * (ky * ky - 1.0);  R[5] = -s * kx + c * (ky * kz);
    R[6] = -s * ky + c * (kz * kx);  R[7] = s * kx + c * (kz * ky);    R[8] = 1.0 + c * (kz * kz - 1.0);
}

// One wavefront sums the partials of NM moments in the fixed order of final_reduce; lane 0 then
// either hands the sums out (the seam) or solves m[0..21) x = -m[21..27), updates T and c and applies the stage / convergence /
// failure rules.  Slots: NM - 1 = the count, R2 -> sum_r2, AUX -> sum_aux (AUX < 0: none).
template <int NM, int R2, int AUX>
__global__ __launch_bounds__(64) void k_icp_solve(const IcpSolveArgs a) {
    IcpState *st = a.st;
    if (!a.moments && st->done) return;                // (uniform)
    double m[NM];
    final_reduce(a.partial, a.blocks, m, SumOp());
    if (threadIdx.x != 0) return;
    if (a.moments) {
#pragma unroll
        for (int k = 0; k < NM; ++k) a.moments[k] = m[k];
        return;
    }
    const uint32_t count = (uint32_t)m[NM - 1];
    st->lin_stage = st->stage;
    st->count = count;
    st->sum_r2 = m[R2];
    if (AUX >= 0) st->sum_aux = m[AUX >= 0 ? AUX : 0];
    if (count < a.min_corr) { st->failure = PLADE_ICP_TOO_FEW; st->done = 1; return; }
    // Cholesky of the 6 x 6 normal matrix (upper triangle in m[0..21))
    double A[6][6], L[6][6];
    {
        int k = 0;
#pragma unroll
        for (int u = 0; u < 6; ++u)
#pragma unroll
            for (int v = u; v < 6; ++v) { A[u][v] = m[k]; A[v][u] = m[k]; ++k; }
    }
    // a pivot is compared with its own diagonal entry: the test does not change when a column is rescaled (units, lever
    // arms), and an exactly zero column (an unconstrained motion) is degenerate
    bool degenerate = false;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double piv = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) piv -= L[j][k] * L[j][k];
        if (!(piv > 1e-12 * A[j][j])) degenerate = true;
        L[j][j] = sqrt(fmax(piv, 1e-300));
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
    if (degenerate) { st->failure = PLADE_ICP_DEGENERATE; st->done = 1; return; }
    double y[6], x[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {                      // L y = -(the gradient)
        double v = -m[21 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {                     // L^T x = y
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) v -= L[k][i] * x[k];
        x[i] = v / L[i][i];
    }
    // T_{k+1} = [R | (c - R c) + x3..5] T_k: a rotation about the centre c = c_k, then x3..5 moves the centre
    double R[9];
    rodrigues(x, R);
    double c[3], tu[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) c[r] = st->c[r];
#pragma unroll
    for (int r = 0; r < 3; ++r) tu[r] = (c[r] - ((R[3 * r] * c[0] + R[3 * r + 1] * c[1]) + R[3 * r + 2] * c[2])) + x[3 + r];
    double Tn[12];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            Tn[4 * r + k] = (R[3 * r] * st->T[k] + R[3 * r + 1] * st->T[4 + k]) + R[3 * r + 2] * st->T[8 + k];
        Tn[4 * r + 3] = ((R[3 * r] * st->T[3] + R[3 * r + 1] * st->T[7]) + R[3 * r + 2] * st->T[11]) + tu[r];
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) { st->T[k] = Tn[k]; st->Tf[k] = (float)Tn[k]; }
    apply_T(Tn, st->sbar, c);
#pragma unroll
    for (int r = 0; r < 3; ++r) st->c[r] = c[r];
    const int iter = st->iter + 1;
    st->iter = iter;
    const double nr = sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]), nt = sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]);
    if (nr < a.eps_rot && nt < a.eps_trans) {
        if (st->stage + 1 < a.n_stages) st->stage = st->stage + 1;
        else { st->converged = 1; st->done = 1; return; }
    }
    if (iter >= a.max_iter) st->done = 1;
}

// ---- host --------------------------------------------------------------------------------------------------------------------
struct IcpConfig {
    double leaf, max_dist, min_dist, eps_rot, eps_trans;
    int max_iter;
    uint32_t min_corr;
    int n_stages;
    double dist[ICP_MAX_STAGES];
};

inline double diag_of(const float mn[3], const float mx[3]) {
    const double ex = (double)mx[0] - mn[0], ey = (double)mx[1] - mn[1], ez = (double)mx[2] - mn[2];
    return std::sqrt(ex * ex + ey * ey + ez * ez);
}

// `who` opens every message ("refine_icp", "refine_gicp")
inline void check_param(double v, const std::string &who, const char *what) {
    PLADE_REQUIRE(std::isfinite(v) && v >= 0.0, PLADE_EINVAL, who + ": " + what + " must be finite and >= 0");
}

// the resolved parameters of the seven common fields (prm NULL: the defaults)
inline IcpConfig resolve(const plade_icp_params *prm, const float tmn[3], const float tmx[3], const std::string &who) {
    plade_icp_params p;
    if (prm) p = *prm; else plade_icp_default_params(&p);
    check_param(p.source_leaf, who, "source_leaf"); check_param(p.max_dist, who, "max_dist"); check_param(p.min_dist, who, "min_dist");
    check_param(p.eps_rotation, who, "eps_rotation"); check_param(p.eps_translation, who, "eps_translation");
    PLADE_REQUIRE(p.max_iterations >= 0 && p.min_correspondences >= 0, PLADE_EINVAL,
                  who + ": max_iterations and min_correspondences must be >= 0");
    const double D = diag_of(tmn, tmx);
    PLADE_REQUIRE(D > 0.0, PLADE_EINVAL, who + ": the target's bounding box is a single point");
    IcpConfig c;
    c.leaf = p.source_leaf > 0.0 ? p.source_leaf : 0.005 * D;
    c.max_dist = p.max_dist > 0.0 ? p.max_dist : 0.025 * D;
    c.min_dist = p.min_dist > 0.0 ? p.min_dist : std::min(0.0025 * D, c.max_dist);
    // the tolerances never fall below what fp32 coordinates of the target's size resolve (4 ulp(1) max|coordinate|): below it
    // a step cannot shrink and the loop would spin to the cap
    const double floor_t = 4.0 * std::ldexp(1.0, -23) * amax_of(tmn, tmx);
    c.eps_rot = std::max(p.eps_rotation > 0.0 ? p.eps_rotation : 1e-6, floor_t / D);
    c.eps_trans = std::max(p.eps_translation > 0.0 ? p.eps_translation : 1e-6 * D, floor_t);
    c.max_iter = p.max_iterations > 0 ? p.max_iterations : 60;
    c.min_corr = p.min_correspondences > 0 ? (uint32_t)p.min_correspondences : 100u;
    PLADE_REQUIRE(c.min_dist <= c.max_dist, PLADE_EINVAL, who + ": min_dist > max_dist");
    c.n_stages = 0;
    for (double d = c.max_dist;; d = std::max(c.min_dist, d / 2)) {
        PLADE_REQUIRE(c.n_stages < ICP_MAX_STAGES, PLADE_EINVAL, who + ": more than 16 stages (max_dist / min_dist > 2^15)");
        c.dist[c.n_stages++] = d;
        if (!(d > c.min_dist)) break;
    }
    return c;
}

// the grid of one stage distance d over the target (n_t x 6 on the device, bounding box known)
inline IcpGridArgs stage_grid(plade_ctx *ctx, TargetGrid &G, const float *d_tgt, uint32_t n_t, const float tmn[3], const float tmx[3],
                              double d, const char *who) {
    // cell >= d with a margin for the fp32 cell assignment: radius_cell with 1 % of d (build() adds 0.1 % and may enlarge the
    // cell further; a larger cell only adds candidates)
    G.build(ctx, d_tgt, n_t, 6, radius_cell(d, tmn, tmx, 1.01), tmn, tmx, true);
    IcpGridArgs g;
    g.g = view_of(G, who);
    const float df = (float)d;
    g.d2 = df * df;
    return g;
}

inline void init_state(IcpState &s, const double T[16], const double *center) {
    memset(&s, 0, sizeof(s));
    for (int k = 0; k < 12; ++k) { s.T[k] = T[k]; s.Tf[k] = (float)T[k]; }
    if (center) for (int k = 0; k < 3; ++k) s.c[k] = center[k];
}

inline void check_T(const float *T16, const std::string &who) {
    for (int k = 0; k < 16; ++k) PLADE_REQUIRE(std::isfinite(T16[k]), PLADE_EINVAL, who + ": T_in must be finite");
}

}  // namespace
}  // namespace plade
