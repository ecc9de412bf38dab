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
#include "icp.h"
#include "grid_walk.h"
#include "voxel.h"

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
    double sum_r2;
};

struct IcpGridArgs {
    GridView g;
    float d2;            // (float)d * (float)d
};

struct IcpArgs {
    IcpGridArgs g[ICP_MAX_STAGES];
    const float *tgt;    // n_t x 6: the normals are gathered by the original index
    const float *src;    // sample points, `stride` floats apart
    uint32_t stride, n;
    IcpState *st;
    double *partial;     // gridDim.x x ICP_MOMENTS
    int32_t *corr;       // seam: j or -1 per point (nullptr in the loop)
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
        int cx, cy, cz;
        cell_of(G.g, q, cx, cy, cz);
        u64 best = EMPTY;
        for_block27(G.g, cx, cy, cz, [&](uint32_t j0, uint32_t j1) {
            for (uint32_t j = j0; j < j1; ++j) {
                const float4 p = G.g.sorted[j];
                const u64 key = make_key(flann_d2(q, f3(p.x, p.y, p.z)), __float_as_uint(p.w));
                best = key < best ? key : best;
            }
        });
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
    // fixed-order reduction: butterfly across the wave (lane 0's sum), then the waves in order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < ICP_MOMENTS; ++k) {
        double v = m[k];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) s_red[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < ICP_MOMENTS) {
        double v = s_red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < CORR_TPB / 64; ++w) v += s_red[w][threadIdx.x];
        a.partial[(size_t)blockIdx.x * ICP_MOMENTS + threadIdx.x] = v;
    }
}

// the fp64 sums of the sample's x y z, one partial per workgroup (the fixed order of k_icp_corr_lin's reduction)
__global__ __launch_bounds__(CORR_TPB) void k_icp_mean_part(const float *src, uint32_t n, double *partial) {
    __shared__ double s_red[CORR_TPB / 64][3];
    const uint32_t i = blockIdx.x * CORR_TPB + threadIdx.x;
    double m[3] = {0.0, 0.0, 0.0};
    if (i < n) { m[0] = src[(size_t)i * 3]; m[1] = src[(size_t)i * 3 + 1]; m[2] = src[(size_t)i * 3 + 2]; }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double v = m[k];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) s_red[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double v = s_red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < CORR_TPB / 64; ++w) v += s_red[w][threadIdx.x];
        partial[(size_t)blockIdx.x * 3 + threadIdx.x] = v;
    }
}

// T v for the fp64 rows of T (((r0 x + r1 y) + r2 z) + t)
__device__ __forceinline__ void apply_T(const double T[12], const double v[3], double out[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) out[r] = ((T[4 * r] * v[0] + T[4 * r + 1] * v[1]) + T[4 * r + 2] * v[2]) + T[4 * r + 3];
}

// one wavefront: s-bar = the sum of the partials (lane l: l, l + 64, ..., then a butterfly) / n, and c_0 = T_0 s-bar
__global__ __launch_bounds__(64) void k_icp_mean(IcpState *st, const double *partial, uint32_t blocks, uint32_t n) {
    const int lane = threadIdx.x;
    double m[3] = {0.0, 0.0, 0.0};
    for (uint32_t b = (uint32_t)lane; b < blocks; b += 64)
#pragma unroll
        for (int k = 0; k < 3; ++k) m[k] += partial[(size_t)b * 3 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m[k] += __shfl_xor(m[k], o, 64);
    if (lane != 0) return;
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

__global__ __launch_bounds__(64) void k_icp_solve(const IcpSolveArgs a) {
    IcpState *st = a.st;
    if (!a.moments && st->done) return;                // (uniform)
    const int lane = threadIdx.x;
    double m[ICP_MOMENTS];
#pragma unroll
    for (int k = 0; k < ICP_MOMENTS; ++k) m[k] = 0.0;
    for (uint32_t b = (uint32_t)lane; b < a.blocks; b += 64) {
        const double *p = a.partial + (size_t)b * ICP_MOMENTS;
#pragma unroll
        for (int k = 0; k < ICP_MOMENTS; ++k) m[k] += p[k];
    }
#pragma unroll
    for (int k = 0; k < ICP_MOMENTS; ++k)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m[k] += __shfl_xor(m[k], o, 64);
    if (lane != 0) return;
    if (a.moments) {
#pragma unroll
        for (int k = 0; k < ICP_MOMENTS; ++k) a.moments[k] = m[k];
        return;
    }
    const uint32_t count = (uint32_t)m[28];
    st->lin_stage = st->stage;
    st->count = count;
    st->sum_r2 = m[27];
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
    for (int i = 0; i < 6; ++i) {                      // L y = -J^T r
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

}  // namespace

struct IcpWork {
    TargetGrid grids[ICP_MAX_STAGES];
    VoxelWork vox;
    DBuf<float> in_t, in_s;        // the host-pointer entry points' device copies (grow-only)
    DBuf<double> partial, out;
    DBuf<IcpState> st;
    DBuf<int32_t> corr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    IcpState h_init, h_st;      // the upload's source and the read-back's destination (never the same memory in flight)
    ~IcpWork() { for (hipEvent_t &e : ev) if (e) (void)hipEventDestroy(e); }
};
IcpWork *icp_work_create() { return new IcpWork; }
void icp_work_destroy(IcpWork *w) { delete w; }

namespace {

struct IcpConfig {
    double leaf, max_dist, min_dist, eps_rot, eps_trans;
    int max_iter;
    uint32_t min_corr;
    int n_stages;
    double dist[ICP_MAX_STAGES];
};

double diag_of(const float mn[3], const float mx[3]) {
    const double ex = (double)mx[0] - mn[0], ey = (double)mx[1] - mn[1], ez = (double)mx[2] - mn[2];
    return std::sqrt(ex * ex + ey * ey + ez * ez);
}

double amax_of(const float mn[3], const float mx[3]) {
    double a = 0.0;
    for (int t = 0; t < 3; ++t) a = std::max(a, std::max(std::fabs((double)mn[t]), std::fabs((double)mx[t])));
    return a;
}

void check_param(double v, const char *what) {
    PLADE_REQUIRE(std::isfinite(v) && v >= 0.0, PLADE_EINVAL, std::string("refine_icp: ") + what + " must be finite and >= 0");
}

IcpConfig resolve(const plade_icp_params *prm, const float tmn[3], const float tmx[3]) {
    plade_icp_params p;
    if (prm) p = *prm; else plade_icp_default_params(&p);
    check_param(p.source_leaf, "source_leaf"); check_param(p.max_dist, "max_dist"); check_param(p.min_dist, "min_dist");
    check_param(p.eps_rotation, "eps_rotation"); check_param(p.eps_translation, "eps_translation");
    PLADE_REQUIRE(p.max_iterations >= 0 && p.min_correspondences >= 0, PLADE_EINVAL,
                  "refine_icp: max_iterations and min_correspondences must be >= 0");
    const double D = diag_of(tmn, tmx);
    PLADE_REQUIRE(D > 0.0, PLADE_EINVAL, "refine_icp: the target's bounding box is a single point");
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
    PLADE_REQUIRE(c.min_dist <= c.max_dist, PLADE_EINVAL, "refine_icp: min_dist > max_dist");
    c.n_stages = 0;
    for (double d = c.max_dist;; d = std::max(c.min_dist, d / 2)) {
        PLADE_REQUIRE(c.n_stages < ICP_MAX_STAGES, PLADE_EINVAL, "refine_icp: more than 16 stages (max_dist / min_dist > 2^15)");
        c.dist[c.n_stages++] = d;
        if (!(d > c.min_dist)) break;
    }
    return c;
}

// the grid of one stage distance d over the target (n_t x 6 on the device, bounding box known)
IcpGridArgs stage_grid(plade_ctx *ctx, TargetGrid &G, const float *d_tgt, uint32_t n_t, const float tmn[3], const float tmx[3],
                       double d) {
    // cell >= d with a margin for the fp32 cell assignment: 1 % of d and a few ulps of the largest coordinate (build() adds 0.1 %
    // and may enlarge the cell further; a larger cell only adds candidates)
    G.build(ctx, d_tgt, n_t, 6, (float)(1.01 * d + 4e-6 * amax_of(tmn, tmx)), tmn, tmx, true);
    IcpGridArgs g;
    g.g = view_of(G, "refine_icp");
    const float df = (float)d;
    g.d2 = df * df;
    return g;
}

void init_state(IcpState &s, const double T[16], const double *center) {
    memset(&s, 0, sizeof(s));
    for (int k = 0; k < 12; ++k) { s.T[k] = T[k]; s.Tf[k] = (float)T[k]; }
    if (center) for (int k = 0; k < 3; ++k) s.c[k] = center[k];
}

void check_T(const float *T16) {
    for (int k = 0; k < 16; ++k) PLADE_REQUIRE(std::isfinite(T16[k]), PLADE_EINVAL, "refine_icp: T_in must be finite");
}

// the refinement on device clouds: target n_t x 6, source `s_stride` floats per point, bounding boxes known
int refine_dev(plade_ctx *ctx, IcpWork &W, const float *d_tgt, uint32_t n_t, const float tmn[3], const float tmx[3], const float *d_src,
               uint32_t n_s, uint32_t s_stride, const float smn[3], const float smx[3], const float *T_in16, const plade_icp_params *prm,
               float *T_out16, plade_icp_result *res) {
    const IcpConfig c = resolve(prm, tmn, tmx);
    float T_in[16];
    memcpy(T_in, T_in16, sizeof(T_in));
    for (hipEvent_t &e : W.ev) if (!e) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventRecord(W.ev[0], ctx->stream));
    // sample: VoxelGrid of the source (waits for its size)
    const uint32_t n = W.vox.run(ctx, d_src, s_stride, nullptr, nullptr, n_s, 1, (float)c.leaf, smn, smx);
    HIP_TRY(hipEventRecord(W.ev[1], ctx->stream));
    IcpArgs a;
    memset(&a, 0, sizeof(a));
    for (int s = 0; s < c.n_stages; ++s) a.g[s] = stage_grid(ctx, W.grids[s], d_tgt, n_t, tmn, tmx, c.dist[s]);
    HIP_TRY(hipEventRecord(W.ev[2], ctx->stream));
    const uint32_t blocks = std::max(1u, cdiv(n, CORR_TPB));
    a.tgt = d_tgt; a.src = W.vox.out_xyz.p; a.stride = 3; a.n = n;
    a.st = W.st.ensure(1);
    a.partial = W.partial.ensure((size_t)blocks * ICP_MOMENTS);
    a.corr = nullptr;
    double T[16];
    for (int k = 0; k < 16; ++k) T[k] = T_in[k];
    init_state(W.h_init, T, nullptr);
    HIP_TRY(hipMemcpyAsync(W.st.p, &W.h_init, sizeof(IcpState), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_icp_mean_part, dim3(blocks), dim3(CORR_TPB), 0, ctx->stream, a.src, n, a.partial);
    hipLaunchKernelGGL(k_icp_mean, dim3(1), dim3(64), 0, ctx->stream, a.st, (const double *)a.partial, blocks, n);
    IcpSolveArgs sa;
    sa.st = a.st; sa.partial = a.partial; sa.blocks = blocks; sa.n_stages = c.n_stages; sa.max_iter = c.max_iter;
    sa.min_corr = c.min_corr; sa.eps_rot = c.eps_rot; sa.eps_trans = c.eps_trans; sa.moments = nullptr;
    for (int it = 0; it < c.max_iter; ++it) {
        hipLaunchKernelGGL(k_icp_corr_lin, dim3(blocks), dim3(CORR_TPB), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_icp_solve, dim3(1), dim3(64), 0, ctx->stream, sa);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(W.ev[3], ctx->stream));
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
    float ms[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < 3; ++k) HIP_TRY(hipEventElapsedTime(&ms[k], W.ev[k], W.ev[k + 1]));
    ctx->stats.clear();
    ctx->stats.add("icp_sample_s", 1e-3 * ms[0]);
    ctx->stats.add("icp_grid_s", 1e-3 * ms[1]);
    ctx->stats.add("icp_loop_s", 1e-3 * ms[2]);
    ctx->stats.add("icp_iterations", s.iter);
    ctx->stats.add("icp_stages", c.n_stages);
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
        check_T(T_in16);
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
        check_T(T_in16);
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
        a.g[0] = stage_grid(ctx, W.grids[0], W.in_t.p, n_t, tmn, tmx, (double)dist);
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
        hipLaunchKernelGGL(k_icp_solve, dim3(1), dim3(64), 0, ctx->stream, sa);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(moments_out, sa.moments, ICP_MOMENTS * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (corr_out) HIP_TRY(hipMemcpyAsync(corr_out, a.corr, (size_t)n_s * 4, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        return PLADE_OK;
    });
}
