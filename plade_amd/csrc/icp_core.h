// plade_amd/csrc/icp_core.h -- the refinement that the point-to-plane ICP (k_icp.hip, icp.h) and the plane-to-plane ICP (k_gicp.hip,
// gicp.h) are two variants of: the device state, the fp64 mean of the sample, the match kernel around the variant's linearisation,
// the fixed-order reduction of the moments, the solve / update / schedule / failure rules of lane 0, and on the host the resolved
// parameters, the stage grids, the work area, the loop (refine_dev), the test seam (linearize_seam) and the bodies of the entry
// points.  All of it is written once, as templates over a model M that each .hip file defines:
//   NM, R2, AUX          the number of moments and the slots of k_icp_solve (NM - 1 = the count)
//   STRIDE               floats per row of the sample
//   prefix, who, seam, seam_grid, seam_empty   the stats prefix and the names that open the messages
//   slot                 the context's pointer to this variant's work area
//   params, result, defaults()   the public types (include/plade_hip.h)
//   Args                 the match kernel's arguments: g, tgt, src, n, st, partial, corr and what the variant adds
//   source(a, rows, stride)   the rows to match into a;  row(a, i): row i on the device
//   epsilon_of(p), extra(a, epsilon, who)   the variant's own parameter into a, checked after the common ones
//   sample(...)          the source's sample on the device: its size and rows
//   finish(r, s)         the variant's own result field
//   linearise(a, x, y, z, s, t, st, m)   the moments of one correspondence; false when the variant's normal test refuses it
// Nothing here depends on what a moment means beyond the slots named above.
//
// Included by those two .hip files only.  What is not named by ctx.h sits in an unnamed namespace: each file gets kernels of its own.
#pragma once
#include "icp.h"
#include "cloud_tool.h"
#include "fixed_reduce.h"
#include "grid_walk.h"
#include "voxel.h"

namespace plade {

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

// the work area of one variant (plade_ctx holds one per variant, made on first use)
struct RefineWork {
    TargetGrid grids[ICP_MAX_STAGES];
    VoxelWork vox;                 // the point-to-plane sample (grow-only device buffers: a variant that never runs it holds none)
    DBuf<float> in_t, in_s;        // the host-pointer entry points' device copies (grow-only)
    DBuf<double> partial, out;
    DBuf<IcpState> st;
    DBuf<int32_t> corr;
    EventSpans<4> spans;        // sample, grid, loop
    IcpState h_init, h_st;      // the upload's source and the read-back's destination (never the same memory in flight)
};

namespace {

constexpr int CORR_TPB = 256;

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

// match and linearise: one lane per sample point.  The lane forms p' in fp32 with Tf, takes the exact (d, j) argmin key over the
// current stage's grid and -- below the stage distance -- hands the two rows to the variant's linearisation; the moments then go
// through the fixed-order reduction.  Once the state says done, the kernel returns at once.
template <class M>
__global__ __launch_bounds__(CORR_TPB) void k_corr_lin(const typename M::Args a) {
    __shared__ double s_red[CORR_TPB / 64][M::NM];
    const IcpState *st = a.st;
    if (st->done) return;                              // (uniform)
    const IcpGridArgs &G = a.g[st->stage];
    const uint32_t i = blockIdx.x * CORR_TPB + threadIdx.x;
    double m[M::NM];
#pragma unroll
    for (int k = 0; k < M::NM; ++k) m[k] = 0.0;
    if (i < a.n) {
        const float *s = M::row(a, i);
        const float x = s[0], y = s[1], z = s[2];
        const float *Tf = st->Tf;
        const f3 q(((Tf[0] * x + Tf[1] * y) + Tf[2] * z) + Tf[3], ((Tf[4] * x + Tf[5] * y) + Tf[6] * z) + Tf[7],
                   ((Tf[8] * x + Tf[9] * y) + Tf[10] * z) + Tf[11]);
        const u64 best = nearest_key(G.g, q);
        int32_t jout = -1;
        if (best != EMPTY && key_d(best) < G.d2) {
            const uint32_t j = (uint32_t)best;
            if (M::linearise(a, x, y, z, s, a.tgt + (size_t)j * 6, st, m)) jout = (int32_t)j;
        }
        if (a.corr) a.corr[i] = jout;
    }
    reduce_moments<M::NM>(m, s_red, a.partial);
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

// the resolved parameters of the seven common fields, which plade_icp_params and plade_gicp_params name alike
template <class P>
IcpConfig resolve(const P &p, const float tmn[3], const float tmx[3], const std::string &who) {
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

// what the loop and the seam begin alike: the state and the partials for `blocks` workgroups, the state's upload from T (and the
// given centre), and the arguments of k_icp_solve that do not depend on the schedule
template <class M>
IcpSolveArgs begin(plade_ctx *ctx, RefineWork &W, typename M::Args &a, uint32_t blocks, const double T[16], const double *center) {
    a.st = W.st.ensure(1);
    a.partial = W.partial.ensure((size_t)blocks * M::NM);
    init_state(W.h_init, T, center);
    HIP_TRY(hipMemcpyAsync(W.st.p, &W.h_init, sizeof(IcpState), hipMemcpyHostToDevice, ctx->stream));
    IcpSolveArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.st = a.st; sa.partial = a.partial; sa.blocks = blocks;
    return sa;
}

template <class M>
void launch_pair(plade_ctx *ctx, const typename M::Args &a, const IcpSolveArgs &sa) {
    hipLaunchKernelGGL(k_corr_lin<M>, dim3(sa.blocks), dim3(CORR_TPB), 0, ctx->stream, a);
    hipLaunchKernelGGL((k_icp_solve<M::NM, M::R2, M::AUX>), dim3(1), dim3(64), 0, ctx->stream, sa);
}

// the refinement on device clouds: target n_t x 6, source n_s x 6, bounding boxes known
template <class M>
int refine_dev(plade_ctx *ctx, RefineWork &W, const float *d_tgt, uint32_t n_t, const float tmn[3], const float tmx[3], const float *d_src,
               uint32_t n_s, const float smn[3], const float smx[3], const float *T_in16, const typename M::params *prm, float *T_out16,
               typename M::result *res) {
    const typename M::params p = params_or_default(prm, M::defaults);
    const IcpConfig c = resolve(p, tmn, tmx, M::who);
    typename M::Args a;
    memset(&a, 0, sizeof(a));
    M::extra(a, M::epsilon_of(p), M::who);
    float T_in[16];
    memcpy(T_in, T_in16, sizeof(T_in));
    W.spans.mark(ctx, 0);
    // the sample (waits for its size)
    const float *d_sample = nullptr;
    const uint32_t n = M::sample(ctx, W, d_src, n_s, (float)c.leaf, smn, smx, &d_sample);
    W.spans.mark(ctx, 1);
    for (int s = 0; s < c.n_stages; ++s) a.g[s] = stage_grid(ctx, W.grids[s], d_tgt, n_t, tmn, tmx, c.dist[s], M::who);
    W.spans.mark(ctx, 2);
    const uint32_t blocks = std::max(1u, cdiv(n, CORR_TPB));
    a.tgt = d_tgt; a.n = n;
    M::source(a, d_sample, M::STRIDE);
    double T[16];
    for (int k = 0; k < 16; ++k) T[k] = T_in[k];
    IcpSolveArgs sa = begin<M>(ctx, W, a, blocks, T, nullptr);
    hipLaunchKernelGGL(k_icp_mean_part, dim3(blocks), dim3(CORR_TPB), 0, ctx->stream, a.src, (uint32_t)M::STRIDE, n, a.partial);
    hipLaunchKernelGGL(k_icp_mean, dim3(1), dim3(64), 0, ctx->stream, a.st, (const double *)a.partial, blocks, n);
    sa.n_stages = c.n_stages; sa.max_iter = c.max_iter; sa.min_corr = c.min_corr; sa.eps_rot = c.eps_rot; sa.eps_trans = c.eps_trans;
    for (int it = 0; it < c.max_iter; ++it) launch_pair<M>(ctx, a, sa);
    HIP_TRY(hipGetLastError());
    W.spans.mark(ctx, 3);
    HIP_TRY(hipMemcpyAsync(&W.h_st, W.st.p, sizeof(IcpState), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    const IcpState &s = W.h_st;
    typename M::result r;
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
    M::finish(r, s);
    if (res) *res = r;
    W.spans.collect();
    const std::string pre = M::prefix;
    ctx->stats.clear();
    ctx->stats.add(pre + "_sample_s", W.spans.seconds(0));
    ctx->stats.add(pre + "_grid_s", W.spans.seconds(1));
    ctx->stats.add(pre + "_loop_s", W.spans.seconds(2));
    ctx->stats.add(pre + "_iterations", s.iter);
    ctx->stats.add(pre + "_stages", c.n_stages);
    grid_stats(ctx, M::prefix, W.grids[0]);          // the first (widest) stage
    if (s.failure) {
        memmove(T_out16, T_in, sizeof(T_in));
        ctx->last_error = std::string(M::who) + (s.failure == PLADE_ICP_TOO_FEW ? ": too few correspondences"
                                                                                 : ": degenerate geometry (the system is singular)");
        return PLADE_EFAIL;
    }
    for (int k = 0; k < 12; ++k) T_out16[k] = (float)s.T[k];
    T_out16[12] = 0.f; T_out16[13] = 0.f; T_out16[14] = 0.f; T_out16[15] = 1.f;
    return PLADE_OK;
}

// ---- the bodies of the entry points (include/plade_hip.h) ----------------------------------------------------------------------
template <class M>
int refine_host(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t, const float *src_pos_nrm, uint32_t n_s, const float *T_in16,
                const typename M::params *params, float *T_out16, typename M::result *result) {
    return guarded(ctx, [&]() -> int {
        const std::string name = std::string("plade_") + M::who;
        PLADE_REQUIRE(tgt_pos_nrm && src_pos_nrm && T_in16 && T_out16, PLADE_EINVAL, name + ": bad argument");
        PLADE_REQUIRE(n_t >= 1 && n_s >= 1, PLADE_EINVAL, name + ": empty cloud");
        check_T(T_in16, M::who);
        RefineWork &W = work_in<RefineWork>(ctx->*M::slot);
        float tmn[3], tmx[3], smn[3], smx[3];
        upload_rows(ctx, W.in_t, tgt_pos_nrm, n_t, 6, tmn, tmx);
        upload_rows(ctx, W.in_s, src_pos_nrm, n_s, 6, smn, smx);
        return refine_dev<M>(ctx, W, W.in_t.p, n_t, tmn, tmx, W.in_s.p, n_s, smn, smx, T_in16, params, T_out16, result);
    });
}

template <class M>
int refine_resident(plade_ctx *ctx, plade_cloud *tgt, plade_cloud *src, const float *T_in16, const typename M::params *params,
                    float *T_out16, typename M::result *result) {
    return guarded(ctx, [&]() -> int {
        const std::string name = std::string("plade_") + M::who + "_dev";
        PLADE_REQUIRE(tgt && src && T_in16 && T_out16, PLADE_EINVAL, name + ": bad argument");
        PLADE_REQUIRE(tgt->dev.n >= 1 && src->dev.n >= 1, PLADE_EINVAL, name + ": empty cloud");
        check_T(T_in16, M::who);
        const CloudDev &t = tgt->dev, &s = src->dev;
        return refine_dev<M>(ctx, work_in<RefineWork>(ctx->*M::slot), t.aos.p, t.n, t.bbmin, t.bbmax, s.aos.p, s.n, s.bbmin, s.bbmax,
                             T_in16, params, T_out16, result);
    });
}

// the test seam: one match + linearise pass at stage distance `dist` with the fp64 T on every row of the source (no sample), about
// the given centre; the summed moments and, if asked for, j or -1 per row
template <class M>
int linearize_seam(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t, const float *src, uint32_t n_s, uint32_t stride,
                   const double *T16, const double *center, float dist, double epsilon, int32_t *corr_out, double *moments_out) {
    return guarded(ctx, [&]() -> int {
        const std::string name = M::seam;
        PLADE_REQUIRE(tgt_pos_nrm && src && T16 && center && moments_out, PLADE_EINVAL, name + ": bad argument");
        PLADE_REQUIRE(n_t >= 1 && n_s >= 1 && stride >= 3, PLADE_EINVAL, name + ": " + M::seam_empty);
        PLADE_REQUIRE(std::isfinite(dist) && dist > 0.f, PLADE_EINVAL, name + ": dist must be finite and > 0");
        for (int k = 0; k < 16; ++k) PLADE_REQUIRE(std::isfinite(T16[k]), PLADE_EINVAL, name + ": T must be finite");
        for (int k = 0; k < 3; ++k) PLADE_REQUIRE(std::isfinite(center[k]), PLADE_EINVAL, name + ": center must be finite");
        typename M::Args a;
        memset(&a, 0, sizeof(a));
        M::extra(a, epsilon, M::seam);
        RefineWork &W = work_in<RefineWork>(ctx->*M::slot);
        float tmn[3], tmx[3], smn[3], smx[3];
        upload_rows(ctx, W.in_t, tgt_pos_nrm, n_t, 6, tmn, tmx);
        upload_rows(ctx, W.in_s, src, n_s, stride, smn, smx);
        a.g[0] = stage_grid(ctx, W.grids[0], W.in_t.p, n_t, tmn, tmx, (double)dist, M::seam_grid);
        a.g[0].d2 = dist * dist;
        a.tgt = W.in_t.p; a.n = n_s;
        M::source(a, W.in_s.p, stride);
        a.corr = W.corr.ensure(n_s);
        IcpSolveArgs sa = begin<M>(ctx, W, a, cdiv(n_s, CORR_TPB), T16, center);
        sa.moments = W.out.ensure(M::NM);
        launch_pair<M>(ctx, a, sa);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(moments_out, sa.moments, M::NM * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (corr_out) HIP_TRY(hipMemcpyAsync(corr_out, a.corr, (size_t)n_s * 4, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        grid_stats(ctx, M::prefix, W.grids[0]);
        return PLADE_OK;
    });
}

// the seven fields that plade_icp_params and plade_gicp_params name alike (0 = the automatic value of icp.h)
template <class P>
void default_common(P *p) {
    p->source_leaf = 0.0;           // 0.005 D
    p->max_dist = 0.0;              // 0.025 D
    p->min_dist = 0.0;              // 0.0025 D
    p->eps_rotation = 1e-6;
    p->eps_translation = 0.0;       // 1e-6 D
    p->max_iterations = 60;
    p->min_correspondences = 100;
}

}  // namespace
}  // namespace plade
