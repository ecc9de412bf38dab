// plade_amd/csrc/k_m3c2.hip -- M3C2 distances between two registered clouds on gfx950 (semantics: m3c2.h).
//
// Layout
//   grids    k_m3c2_transform writes B under T into a scratch xyz array; one dense row index of TargetGrid over A and one over
//            B'.  The cell is radius_cell(R) (grid_walk.h: the smoothing cell of DESIGN.md section 15; build() may enlarge it), so
//            a cylinder is a few cells wide and L / cell cells long.  The walk reads the grid's actual cell, never R.
//   walk     k_m3c2_walk: one wavefront per core point (a cylinder is long: one lane per core point would diverge over its whole
//            length); the core point, the axis and every bound are wave-uniform.  The cover is by grid rows -- a row is a (y, z)
//            pair of cells, a run a stretch of x cells of it.  Lanes take the rows of the cylinder's (y, z) bounding rectangle,
//            clamped to the grid, 64 at a time.  For its row a lane clips the axis parameter t in [-L, L] to the stretch on which
//            the axis passes within R + margin of the row's y and z slabs (a row the axis never comes that near is dropped); the
//            x extent of that stretch, widened by R + margin, is the row's one run.  The runs of the 64 lanes are handed out 64
//            candidates at a time (hand_out_runs of grid_walk.h); each lane applies the exact fp64 predicate and keeps c, S1 and
//            S2 in registers; one xor butterfly closes the wave.  Both clouds in one launch; lane 0 forms the derived values and
//            stores by core index.  No LDS, no atomics.
//            The cover is a superset of the cylinder (every bound is widened by the margin of the fp32 cell assignment), visits
//            every row once with one run (so every grid point at most once), and reads the cells of the clipped stretches only:
//            O(L / cell (R / cell + 1)^2) cells for a generic axis.  What scales with the bounding rectangle is the row test (a
//            few fp64 operations per row, no memory access).
//   summary  k_m3c2_sum / k_m3c2_final, in the fixed order of fixed_reduce.h.
#include "m3c2.h"
#include "fixed_reduce.h"
#include "grid_walk.h"
#include "voxel.h"

namespace plade {

namespace {

constexpr int WALK_WAVES = 4, XF_TPB = 256, SUM_TPB = 256;
// the fp32 cell assignment (x - mn) * inv against the same product in fp64: a relative 3e-7 on the cell coordinate (two fp32
// roundings and the rounding of inv), on top of grid_margin's ulps of the coordinates
constexpr double CELL_LO = 1.0 - 3e-7, CELL_HI = 1.0 + 3e-7;

struct Xf { float m[12]; };

__global__ __launch_bounds__(XF_TPB) void k_m3c2_transform(const float *__restrict__ src, uint32_t n, uint32_t stride, const Xf T,
                                                           float *__restrict__ out) {
    const uint32_t i = blockIdx.x * XF_TPB + threadIdx.x;
    if (i >= n) return;
    const float *s = src + (size_t)i * stride;
    const float x = s[0], y = s[1], z = s[2];
    float *o = out + (size_t)i * 3;
    o[0] = ((T.m[0] * x + T.m[1] * y) + T.m[2] * z) + T.m[3];
    o[1] = ((T.m[4] * x + T.m[5] * y) + T.m[6] * z) + T.m[7];
    o[2] = ((T.m[8] * x + T.m[9] * y) + T.m[10] * z) + T.m[11];
}

struct WalkArgs {
    GridView ga, gb;                 // over A, over B'
    double mga, mgb;                 // grid_margin of each
    const float *core;               // m rows of core_stride floats: x y z nx ny nz
    uint32_t core_stride, m;
    double R, L, R2, reg_error;
    uint32_t min_points;
    double *distance, *lod, *sigma, *moments;   // m, m, m x 2, m x 4
    uint32_t *count;                 // m x 2
    uint8_t *significant;
};

// cells [i0, i1] of one axis (d cells from mn, 1 / inv wide) that can hold a point with a coordinate in [lo, hi]; false: none.
// A point's assigned cell is floorf of the fp32 product, clamped to [0, d - 1]: the fp64 product scaled by CELL_LO / CELL_HI
// brackets it (lo and hi already carry the margin), and no point of the grid lies below cell 0 or at d (1 + 3e-7) and beyond
__device__ __forceinline__ bool cell_range(double lo, double hi, double mn, double inv, int d, int &i0, int &i1) {
    double u0 = (lo - mn) * inv, u1 = (hi - mn) * inv;
    u0 = u0 > 0.0 ? u0 * CELL_LO : u0;
    u1 = u1 > 0.0 ? u1 * CELL_HI : u1;
    if (!(u1 >= 0.0) || !(u0 < (double)d)) return false;
    i0 = (int)floor(fmax(u0, 0.0));
    i1 = (int)floor(fmin(u1, (double)(d - 1)));
    return true;
}

// clips [tlo, thi] to the t with c + t n inside [k0, k1] (one coordinate); false: none
__device__ __forceinline__ bool clip_axis(double c, double n, double k0, double k1, double &tlo, double &thi) {
    if (n == 0.0) return c >= k0 && c <= k1;
    const double ta = (k0 - c) / n, tb = (k1 - c) / n;
    tlo = fmax(tlo, fmin(ta, tb));
    thi = fmin(thi, fmax(ta, tb));
    return tlo <= thi;
}

// the whole wave: count and moments of one cloud inside the cylinder (c, nh, L, R); cnt, s1, s2 are this lane's share
__device__ __forceinline__ void walk_cloud(const GridView &g, double mg, const double (&c)[3], const double (&nh)[3], double L, double R,
                                           double R2, int lane, uint32_t &cnt, double &s1, double &s2) {
    const double reach = R + mg, inv = (double)g.inv, cell = g.cell;
    double lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double a = c[k] - L * nh[k], b = c[k] + L * nh[k];
        lo[k] = fmin(a, b) - reach; hi[k] = fmax(a, b) + reach;
    }
    int x0, x1, y0, y1, z0, z1;
    if (!cell_range(lo[0], hi[0], g.mn[0], inv, g.dx, x0, x1) || !cell_range(lo[1], hi[1], g.mn[1], inv, g.dy, y0, y1) ||
        !cell_range(lo[2], hi[2], g.mn[2], inv, g.dz, z0, z1))
        return;                                                          // (wave-uniform)
    const int ny = y1 - y0 + 1, rows = ny * (z1 - z0 + 1);
    for (int t0 = 0; t0 < rows; t0 += 64) {                              // (wave-uniform)
        const int t = t0 + lane;
        uint32_t a0 = 0, len = 0;
        if (t < rows) {
            const int y = y0 + t % ny, z = z0 + t / ny;
            // the slabs that hold every point assigned to row (y, z), widened by R: open at the grid's edges, where ids are clamped
            const double ya = y == 0 ? -INFINITY : g.mn[1] + (double)y * cell * CELL_LO - reach;
            const double yb = y == g.dy - 1 ? INFINITY : g.mn[1] + (double)(y + 1) * cell * CELL_HI + reach;
            const double za = z == 0 ? -INFINITY : g.mn[2] + (double)z * cell * CELL_LO - reach;
            const double zb = z == g.dz - 1 ? INFINITY : g.mn[2] + (double)(z + 1) * cell * CELL_HI + reach;
            double tlo = -L, thi = L;
            if (clip_axis(c[1], nh[1], ya, yb, tlo, thi) && clip_axis(c[2], nh[2], za, zb, tlo, thi)) {
                const double xa = c[0] + tlo * nh[0], xb = c[0] + thi * nh[0];
                int rx0, rx1;
                if (cell_range(fmin(xa, xb) - reach, fmax(xa, xb) + reach, g.mn[0], inv, g.dx, rx0, rx1)) {
                    const uint32_t row = row_base(g, y, z) + 2u;
                    a0 = g.row_start[row + (uint32_t)rx0];
                    len = g.row_start[row + (uint32_t)rx1 + 1u] - a0;
                }
            }
        }
        hand_out_runs(g, a0, len, lane, [&](bool valid, float4 p) {
            if (!valid) return;
            const double qx = (double)p.x - c[0], qy = (double)p.y - c[1], qz = (double)p.z - c[2];
            const double tt = (qx * nh[0] + qy * nh[1]) + qz * nh[2];
            const double ex = qx - tt * nh[0], ey = qy - tt * nh[1], ez = qz - tt * nh[2];
            const double rho2 = (ex * ex + ey * ey) + ez * ez;
            if (fabs(tt) <= L && rho2 < R2) { ++cnt; s1 += tt; s2 += tt * tt; }
        });
    }
}

__global__ __launch_bounds__(64 * WALK_WAVES) void k_m3c2_walk(const WalkArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * WALK_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (i >= a.m) return;                                                // (wave-uniform)
    const float *row = a.core + (size_t)i * a.core_stride;
    const double c[3] = {(double)row[0], (double)row[1], (double)row[2]};
    const double nx = (double)row[3], ny = (double)row[4], nz = (double)row[5];
    const double len2 = (nx * nx + ny * ny) + nz * nz;
    const bool axis = len2 > 0.0 && len2 < INFINITY;                     // (NaN: false)
    uint32_t ca = 0, cb = 0;
    double s1a = 0.0, s2a = 0.0, s1b = 0.0, s2b = 0.0;
    if (axis) {
        const double len = sqrt(len2);
        const double nh[3] = {nx / len, ny / len, nz / len};
        walk_cloud(a.ga, a.mga, c, nh, a.L, a.R, a.R2, lane, ca, s1a, s2a);
        walk_cloud(a.gb, a.mgb, c, nh, a.L, a.R, a.R2, lane, cb, s1b, s2b);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            ca += __shfl_xor(ca, o, 64); s1a += __shfl_xor(s1a, o, 64); s2a += __shfl_xor(s2a, o, 64);
            cb += __shfl_xor(cb, o, 64); s1b += __shfl_xor(s1b, o, 64); s2b += __shfl_xor(s2b, o, 64);
        }
    }
    if (lane != 0) return;
    double dist = NAN, lod = NAN, sga = NAN, sgb = NAN;
    bool sig = false;
    if (axis && ca >= a.min_points && cb >= a.min_points) {
        const double na = (double)ca, nb = (double)cb;
        const double ma = s1a / na, mb = s1b / nb;
        const double va = fmax(s2a - s1a * ma, 0.0) / (na - 1.0), vb = fmax(s2b - s1b * mb, 0.0) / (nb - 1.0);
        sga = sqrt(va); sgb = sqrt(vb);
        dist = mb - ma;
        lod = 1.96 * (sqrt(va / na + vb / nb) + a.reg_error);
        sig = fabs(dist) > lod;
    }
    a.distance[i] = dist;
    a.lod[i] = lod;
    a.significant[i] = sig ? 1 : 0;
    a.count[2 * (size_t)i] = ca; a.count[2 * (size_t)i + 1] = cb;
    a.sigma[2 * (size_t)i] = sga; a.sigma[2 * (size_t)i + 1] = sgb;
    double *mo = a.moments + 4 * (size_t)i;
    mo[0] = s1a; mo[1] = s2a; mo[2] = s1b; mo[3] = s2b;
}

// per workgroup: pd[3 b] = the sum of distance, pd[3 b + 1] = of distance^2, pd[3 b + 2] = the max of |distance| over its valid core
// points (a valid core point is one whose distance is not NaN); pu[3 b] = their number, pu[3 b + 1] = the significant ones,
// pu[3 b + 2] = its largest count (the order: fixed_reduce.h; terms 0 and 1 of each type are sums, term 2 a maximum)
struct SumMaxD {
    __device__ __forceinline__ double operator()(int k, double a, double b) const { return k == 2 ? fmax(a, b) : a + b; }
};
struct SumMaxU {
    __device__ __forceinline__ uint32_t operator()(int k, uint32_t a, uint32_t b) const { return k == 2 ? max(a, b) : a + b; }
};

__global__ __launch_bounds__(SUM_TPB) void k_m3c2_sum(const double *__restrict__ distance, const uint8_t *__restrict__ significant,
                                                      const uint32_t *__restrict__ count, uint32_t m, double *__restrict__ pd,
                                                      uint32_t *__restrict__ pu) {
    __shared__ double s_d[SUM_TPB / 64][3];
    __shared__ uint32_t s_u[SUM_TPB / 64][3];
    const uint32_t i = blockIdx.x * SUM_TPB + threadIdx.x;
    double d[3] = {0.0, 0.0, 0.0};   // distance, distance^2, |distance|
    uint32_t u[3] = {0, 0, 0};       // valid, significant, count
    if (i < m) {
        u[2] = max(count[2 * (size_t)i], count[2 * (size_t)i + 1]);
        const double e = distance[i];
        if (e == e) { d[0] = e; d[1] = e * e; d[2] = fabs(e); u[0] = 1; u[1] = significant[i]; }
    }
    block_reduce<SUM_TPB>(d, s_d, pd, SumMaxD());
    block_reduce<SUM_TPB>(u, s_u, pu, SumMaxU());
}

// rd[0] = mean, rd[1] = rms of distance, rd[2] = max of |distance| over the valid core points (NaN when there is none);
// ru[0] = valid, ru[1] = significant, ru[2] = the largest count
__global__ __launch_bounds__(64) void k_m3c2_final(const double *__restrict__ pd, const uint32_t *__restrict__ pu, uint32_t blocks,
                                                   double *__restrict__ rd, uint32_t *__restrict__ ru) {
    double d[3];
    uint32_t u[3];
    final_reduce(pd, pu, blocks, d, SumMaxD(), u, SumMaxU());
    if (threadIdx.x != 0) return;
    const uint32_t f = u[0];
    rd[0] = f ? d[0] / (double)f : NAN;
    rd[1] = f ? sqrt(d[1] / (double)f) : NAN;
    rd[2] = f ? d[2] : NAN;
    ru[0] = f; ru[1] = u[1]; ru[2] = u[2];
}

}  // namespace

struct M3c2Work {
    TargetGrid grid_a, grid_b;
    DBuf<float> in_core, in_a, in_b, xyz_b;      // the host-pointer entry point's device copies (grow-only); B under T
    DBuf<double> distance, lod, sigma, moments, partial_d, res_d;
    DBuf<uint32_t> count, partial_u, res_u;
    DBuf<uint8_t> significant;
    EventSpans<4> spans;             // grid, walk, reduce
    double h_d[3] = {0.0, 0.0, 0.0};
    uint32_t h_u[3] = {0, 0, 0};
};

namespace {

const float kIdentity[16] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};

struct Outputs {
    double *distance, *lod;
    uint8_t *significant;
    uint32_t *count;
    double *sigma, *moments;
};

void check_params(const float *T16, const plade_m3c2_params &p) {
    for (int k = 0; k < 16; ++k) PLADE_REQUIRE(std::isfinite(T16[k]), PLADE_EINVAL, "cloud_m3c2: T must be finite");
    PLADE_REQUIRE(std::isfinite(p.radius) && p.radius > 0.0 && std::isfinite(p.radius * p.radius), PLADE_EINVAL,
                  "cloud_m3c2: radius must be finite and > 0, and its square finite");
    PLADE_REQUIRE(std::isfinite(p.depth) && p.depth > 0.0, PLADE_EINVAL, "cloud_m3c2: depth must be finite and > 0");
    PLADE_REQUIRE(std::isfinite(p.reg_error) && p.reg_error >= 0.0, PLADE_EINVAL, "cloud_m3c2: reg_error must be finite and >= 0");
    PLADE_REQUIRE(p.min_points >= M3C2_MIN_POINTS, PLADE_EINVAL, "cloud_m3c2: min_points must be >= 2");
}

// M3C2 on device arrays: core m x core_stride (x y z nx ny nz first), A n_a x stride_a with a known bounding box, B n_b x stride_b.
// Fills the wanted host outputs and the summary, waits, sets the stats.
void m3c2_dev(plade_ctx *ctx, M3c2Work &W, const float *d_core, uint32_t m, uint32_t core_stride, const float *d_a, uint32_t n_a,
              uint32_t stride_a, const float amn[3], const float amx[3], const float *d_b, uint32_t n_b, uint32_t stride_b,
              const float *T16, const plade_m3c2_params &p, const Outputs &out, plade_m3c2_summary *summary) {
    W.spans.mark(ctx, 0);
    Xf T;
    for (int k = 0; k < 12; ++k) T.m[k] = T16[k];
    float *d_bt = W.xyz_b.ensure((size_t)n_b * 3 + 4);
    hipLaunchKernelGGL(k_m3c2_transform, dim3(cdiv(n_b, XF_TPB)), dim3(XF_TPB), 0, ctx->stream, d_b, n_b, stride_b, T, d_bt);
    HIP_TRY(hipGetLastError());
    float bmn[3], bmx[3];
    bbox_host(ctx, d_bt, n_b, 3, bmn, bmx);          // (refuses a B' that left the fp32 range)
    W.grid_a.build(ctx, d_a, n_a, stride_a, radius_cell(p.radius, amn, amx), amn, amx, true);
    W.grid_b.build(ctx, d_bt, n_b, 3, radius_cell(p.radius, bmn, bmx), bmn, bmx, true);
    W.spans.mark(ctx, 1);

    WalkArgs a;
    memset(&a, 0, sizeof(a));
    a.ga = view_of(W.grid_a, "cloud_m3c2");
    a.gb = view_of(W.grid_b, "cloud_m3c2");
    a.mga = grid_margin(a.ga, amn, amx);
    a.mgb = grid_margin(a.gb, bmn, bmx);
    a.core = d_core; a.core_stride = core_stride; a.m = m;
    a.R = p.radius; a.L = p.depth; a.R2 = p.radius * p.radius; a.reg_error = p.reg_error;
    a.min_points = (uint32_t)p.min_points;
    a.distance = W.distance.ensure(m);
    a.lod = W.lod.ensure(m);
    a.sigma = W.sigma.ensure((size_t)m * 2);
    a.moments = W.moments.ensure((size_t)m * 4);
    a.count = W.count.ensure((size_t)m * 2);
    a.significant = W.significant.ensure((size_t)m + 4);
    hipLaunchKernelGGL(k_m3c2_walk, dim3(cdiv(m, WALK_WAVES)), dim3(64 * WALK_WAVES), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    W.spans.mark(ctx, 2);
    const uint32_t blocks = cdiv(m, SUM_TPB);
    double *d_pd = W.partial_d.ensure((size_t)3 * blocks), *d_rd = W.res_d.ensure(4);
    uint32_t *d_pu = W.partial_u.ensure((size_t)3 * blocks), *d_ru = W.res_u.ensure(4);
    hipLaunchKernelGGL(k_m3c2_sum, dim3(blocks), dim3(SUM_TPB), 0, ctx->stream, a.distance, a.significant, a.count, m, d_pd, d_pu);
    hipLaunchKernelGGL(k_m3c2_final, dim3(1), dim3(64), 0, ctx->stream, d_pd, d_pu, blocks, d_rd, d_ru);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(W.h_d, d_rd, sizeof(W.h_d), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(W.h_u, d_ru, sizeof(W.h_u), hipMemcpyDeviceToHost, ctx->stream));
    W.spans.mark(ctx, 3);
    if (out.distance) HIP_TRY(hipMemcpyAsync(out.distance, a.distance, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (out.lod) HIP_TRY(hipMemcpyAsync(out.lod, a.lod, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (out.significant) HIP_TRY(hipMemcpyAsync(out.significant, a.significant, m, hipMemcpyDeviceToHost, ctx->stream));
    if (out.count) HIP_TRY(hipMemcpyAsync(out.count, a.count, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (out.sigma) HIP_TRY(hipMemcpyAsync(out.sigma, a.sigma, (size_t)m * 16, hipMemcpyDeviceToHost, ctx->stream));
    if (out.moments) HIP_TRY(hipMemcpyAsync(out.moments, a.moments, (size_t)m * 32, hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    summary->m = m;
    summary->valid = W.h_u[0];
    summary->significant = W.h_u[1];
    summary->mean = W.h_d[0];
    summary->rms = W.h_d[1];
    summary->max = W.h_d[2];
    summary->max_count = W.h_u[2];
    summary->reserved = 0;
    W.spans.collect();
    ctx->stats.clear();
    ctx->stats.add("m3c2_grid_s", W.spans.seconds(0));
    ctx->stats.add("m3c2_walk_s", W.spans.seconds(1));
    ctx->stats.add("m3c2_reduce_s", W.spans.seconds(2));
    ctx->stats.add("m3c2_valid", W.h_u[0]);
    grid_stats(ctx, "m3c2_a", W.grid_a);
    grid_stats(ctx, "m3c2_b", W.grid_b);
}

}  // namespace
}  // namespace plade

using namespace plade;

// ---- C ABI (include/plade_hip.h) ---------------------------------------------------------------------------------------------
extern "C" void plade_m3c2_default_params(plade_m3c2_params *p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->radius = 0.0;
    p->depth = 0.0;
    p->reg_error = 0.0;
    p->min_points = 4;
}

extern "C" int plade_cloud_m3c2(plade_ctx *ctx, const float *core_pos_nrm, uint32_t m, const float *ref_rows, uint32_t n_a,
                                uint32_t stride_a, const float *cmp_rows, uint32_t n_b, uint32_t stride_b, const float *T16,
                                const plade_m3c2_params *params, double *distance_out, double *lod_out, uint8_t *significant_out,
                                uint32_t *count_out, double *sigma_out, double *moments_out, plade_m3c2_summary *summary) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(core_pos_nrm && ref_rows && cmp_rows && params && summary, PLADE_EINVAL,
                      "plade_cloud_m3c2: NULL cloud, params or summary");
        PLADE_REQUIRE(m >= 1 && n_a >= 1 && n_b >= 1, PLADE_EINVAL, "plade_cloud_m3c2: empty cloud (m = 0 or n = 0)");
        PLADE_REQUIRE(stride_a >= 3 && stride_b >= 3, PLADE_EINVAL, "plade_cloud_m3c2: stride must be >= 3 floats");
        const float *T = T16 ? T16 : kIdentity;
        check_params(T, *params);
        M3c2Work &W = work_in<M3c2Work>(ctx->m3c2_work);
        float cmn[3], cmx[3], amn[3], amx[3], bmn[3], bmx[3];
        upload_rows(ctx, W.in_core, core_pos_nrm, m, 6, cmn, cmx);       // (the bounding boxes check the coordinates)
        upload_rows(ctx, W.in_a, ref_rows, n_a, stride_a, amn, amx);
        upload_rows(ctx, W.in_b, cmp_rows, n_b, stride_b, bmn, bmx);
        const Outputs out = {distance_out, lod_out, significant_out, count_out, sigma_out, moments_out};
        m3c2_dev(ctx, W, W.in_core.p, m, 6, W.in_a.p, n_a, stride_a, amn, amx, W.in_b.p, n_b, stride_b, T, *params, out, summary);
        return PLADE_OK;
    });
}

extern "C" int plade_cloud_m3c2_dev(plade_ctx *ctx, plade_cloud *core, plade_cloud *ref, plade_cloud *cmp, const float *T16,
                                    const plade_m3c2_params *params, double *distance_out, double *lod_out, uint8_t *significant_out,
                                    uint32_t *count_out, double *sigma_out, double *moments_out, plade_m3c2_summary *summary) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(core && ref && cmp && params && summary, PLADE_EINVAL, "plade_cloud_m3c2_dev: NULL cloud, params or summary");
        PLADE_REQUIRE(core->dev.n >= 1 && ref->dev.n >= 1 && cmp->dev.n >= 1, PLADE_EINVAL,
                      "plade_cloud_m3c2_dev: empty cloud (m = 0 or n = 0)");
        const float *T = T16 ? T16 : kIdentity;
        check_params(T, *params);
        M3c2Work &W = work_in<M3c2Work>(ctx->m3c2_work);
        const CloudDev &c = core->dev, &a = ref->dev, &b = cmp->dev;
        const Outputs out = {distance_out, lod_out, significant_out, count_out, sigma_out, moments_out};
        m3c2_dev(ctx, W, c.aos.p, c.n, 6, a.aos.p, a.n, 6, a.bbmin, a.bbmax, b.aos.p, b.n, 6, T, *params, out, summary);
        return PLADE_OK;
    });
}
