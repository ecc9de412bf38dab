// plade_amd/csrc/k_fpfh.hip -- FPFH descriptors and their feature-space match on gfx950 (semantics: fpfh.h).
//
// Layout
//   grid     the dense row index of TargetGrid, built exactly as k_smooth.hip builds it (cell radius_cell(r) of grid_walk.h), so the
//            27-cell block around a point holds everything closer than r.
//   axes     k_fpfh_axes: the fp32 normals gathered into grid order with a has-axis flag in w, so that a walk reads its neighbours'
//            normals from the run it is reading the positions from (not by original index).  They are widened and normalised per
//            pair, as the semantics demand.
//   spfh     k_fpfh_spfh: one lane per point in the grid's sorted order (the 64 queries of a wavefront share their runs).  The 33
//            counters of a lane are indexed by a run-time bin, which in registers would mean scratch: they are lane-private columns
//            hist[bin][lane] of LDS (33 x 256 x 4 B = 33 KiB per workgroup; the word address is bin * 256 + lane, so the 32 lanes
//            a dword access serves together fall on 32 different banks whatever their bins: no conflicts, no atomics, no
//            barrier).  H_i and c_i go out by original index; in grid order the kernel leaves c_i (0 without an axis) and
//            H_i / c_i as fp64 -- the quotient the weighting needs of every neighbour is a function of j alone, so it is divided
//            once per point, not once per pair; the bits are the same.
//   weight   k_fpfh_weight: the second walk, 34 fp64 accumulators per lane in registers (statically indexed: every bin of every
//            neighbour is added, the bin loop is unrolled), rows of 34 doubles read as 17 double2; normalises, stores by original index.
//   summary  k_fpfh_sum / k_fpfh_final, the fixed order of fixed_reduce.h on integers (exact, whatever the order).
//   match    k_feat_match, the pattern of k_match.hip in fp32: one lane owns one query (33 floats in VGPRs), target tiles are staged
//            through LDS (rows padded to 36 floats) and read as wave-wide broadcasts, the two best keys (delta, t) of a lane live in
//            registers (insert<2> of grid_walk.h); the targets are split over blockIdx.y, two keys per (query, chunk);
//            k_feat_merge takes the two smallest over the chunks (a minimum: order-independent, exact); k_feat_keep applies the
//            mutual and ratio tests, the scan of prims.h places the kept pairs, k_feat_compact writes them.
#include "fpfh.h"
#include "cloud_tool.h"
#include "fixed_reduce.h"
#include "grid_walk.h"
#include "prims.h"
#include "voxel.h"

namespace plade {

namespace {

constexpr int SPFH_TPB = 256, WEIGHT_TPB = 256, SUM_TPB = 256, MATCH_TPB = 64;
constexpr int HN_STRIDE = 34;        // doubles per row of the normalised histograms (33, padded to 16-byte rows)
constexpr int TILE_ROW = 36;         // floats per target row in LDS (33, padded to 16-byte rows)

struct dv { double x, y, z; };
__device__ __forceinline__ double dot3(dv a, dv b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ dv cross3(dv a, dv b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
// len2 of fpfh.h; true: the normal gives an axis
__device__ __forceinline__ bool axis_len2(float nx, float ny, float nz, double &len2) {
    const double x = nx, y = ny, z = nz;
    len2 = (x * x + y * y) + z * z;
    return len2 > 0.0 && len2 <= DBL_MAX;        // (false for NaN)
}
__device__ __forceinline__ dv unit_axis(float nx, float ny, float nz, double len2) {
    const double s = sqrt(len2);
    return {(double)nx / s, (double)ny / s, (double)nz / s};
}
__device__ __forceinline__ int bin11(double x) {   // clamp((int)floor(11 x), 0, 10)
    const double t = floor(11.0 * x);
    return !(t >= 0.0) ? 0 : (t > 10.0 ? 10 : (int)t);
}

__global__ __launch_bounds__(256) void k_fpfh_axes(const float4 *__restrict__ sorted, const float *__restrict__ rows, uint32_t stride,
                                                   uint32_t n, float4 *__restrict__ axes) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const uint32_t self = __float_as_uint(sorted[s].w);
    const float *r = rows + (size_t)self * stride;
    const float nx = r[3], ny = r[4], nz = r[5];
    double len2;
    axes[s] = make_float4(nx, ny, nz, axis_len2(nx, ny, nz, len2) ? 1.f : 0.f);
}

struct SpfhArgs {
    GridView g;
    const float4 *axes;              // grid order
    uint32_t n;
    float r2;                        // (float)r * (float)r
    uint32_t min_pairs;
    uint32_t *spfh, *pairs;          // by original index: n x 33, n
    uint8_t *described;
    uint32_t *cs;                    // grid order: c_i, 0 without an axis
    double *hn;                      // grid order: n x HN_STRIDE, H_i[b] / c_i of a described point (else 0)
};

__global__ __launch_bounds__(SPFH_TPB) void k_fpfh_spfh(const SpfhArgs a) {
    __shared__ uint32_t hist[FPFH_DIM * SPFH_TPB];   // lane-private columns: hist[bin * SPFH_TPB + lane]
    const uint32_t lane = threadIdx.x, s = blockIdx.x * SPFH_TPB + lane;
    if (s >= a.n) return;
#pragma unroll
    for (int b = 0; b < FPFH_DIM; ++b) hist[b * SPFH_TPB + lane] = 0u;
    const float4 q4 = a.g.sorted[s];
    const f3 q(q4.x, q4.y, q4.z);
    const uint32_t self = __float_as_uint(q4.w);
    const float4 na = a.axes[s];
    uint32_t c = 0;
    if (na.w != 0.f) {
        double len2;
        axis_len2(na.x, na.y, na.z, len2);
        const dv ni = unit_axis(na.x, na.y, na.z, len2);
        const double px = q.x, py = q.y, pz = q.z;
        int cx, cy, cz;
        cell_of(a.g, q, cx, cy, cz);
        for (int t = 0; t < 9; ++t) {
            const int dy = t % 3 - 1, dz = t / 3 - 1;
            const uint32_t r = (uint32_t)(cx + 1) + row_base(a.g, cy + dy, cz + dz);   // for_block27's runs, as k_smooth_fit
            const uint32_t j1 = a.g.row_start[r + 3];
            for (uint32_t j = a.g.row_start[r]; j < j1; ++j) {
                const float4 p = a.g.sorted[j];
                const float d = flann_d2(q, f3(p.x, p.y, p.z));
                if (!(d > 0.f && d < a.r2)) continue;
                const float4 nb = a.axes[j];
                if (nb.w == 0.f) continue;
                double l2j;
                axis_len2(nb.x, nb.y, nb.z, l2j);
                const dv nj = unit_axis(nb.x, nb.y, nb.z, l2j);
                const dv qv = {(double)p.x - px, (double)p.y - py, (double)p.z - pz};
                const double l = sqrt(dot3(qv, qv));
                const dv e = {qv.x / l, qv.y / l, qv.z / l};
                const double ai = dot3(ni, e), aj = dot3(nj, e);
                const bool swap = fabs(ai) < fabs(aj);
                const dv n1 = swap ? nj : ni, n2 = swap ? ni : nj;
                const dv dp = swap ? dv{-e.x, -e.y, -e.z} : e;
                const double f3v = dot3(n1, dp);
                dv v = cross3(dp, n1);
                const double vl = sqrt(dot3(v, v));
                if (vl == 0.0) continue;
                v = {v.x / vl, v.y / vl, v.z / vl};
                const dv w = cross3(n1, v);
                const double f2v = dot3(v, n2);
                const double f1v = atan2(dot3(w, n2), dot3(n1, n2));
                const int b1 = bin11((f1v + M_PI) / (2.0 * M_PI)), b2 = bin11((f2v + 1.0) * 0.5), b3 = bin11((f3v + 1.0) * 0.5);
                hist[b1 * SPFH_TPB + lane] += 1u;
                hist[(FPFH_BINS + b2) * SPFH_TPB + lane] += 1u;
                hist[(2 * FPFH_BINS + b3) * SPFH_TPB + lane] += 1u;
                ++c;
            }
        }
    }
    const bool desc = na.w != 0.f && c >= a.min_pairs;
    uint32_t *oh = a.spfh + (size_t)self * FPFH_DIM;
    double *on = a.hn + (size_t)s * HN_STRIDE;
    const double cd = (double)c;
#pragma unroll
    for (int b = 0; b < FPFH_DIM; ++b) {
        const uint32_t h = hist[b * SPFH_TPB + lane];
        oh[b] = h;
        on[b] = desc ? (double)h / cd : 0.0;
    }
    on[FPFH_DIM] = 0.0;
    a.pairs[self] = c;
    a.described[self] = desc ? 1 : 0;
    a.cs[s] = c;
}

struct WeightArgs {
    GridView g;
    uint32_t n;
    float r2;
    uint32_t min_pairs;
    const uint32_t *cs;              // grid order
    const double *hn;                // grid order
    const uint32_t *spfh;            // by original index
    float *desc;                     // by original index: n x 33
    double *raw;                     // by original index: n x 34 (or nullptr)
};

__global__ __launch_bounds__(WEIGHT_TPB) void k_fpfh_weight(const WeightArgs a) {
    const uint32_t s = blockIdx.x * WEIGHT_TPB + threadIdx.x;
    if (s >= a.n) return;
    const float4 q4 = a.g.sorted[s];
    const f3 q(q4.x, q4.y, q4.z);
    const uint32_t self = __float_as_uint(q4.w);
    const uint32_t c = a.cs[s];
    float *of = a.desc + (size_t)self * FPFH_DIM;
    double *orw = a.raw ? a.raw + (size_t)self * (FPFH_DIM + 1) : nullptr;
    if (c < a.min_pairs) {           // not described (cs is 0 without an axis, min_pairs >= 1)
#pragma unroll
        for (int b = 0; b < FPFH_DIM; ++b) of[b] = NAN;
        if (orw)
#pragma unroll
            for (int b = 0; b <= FPFH_DIM; ++b) orw[b] = 0.0;
        return;
    }
    double W = 0.0, R[HN_STRIDE];
#pragma unroll
    for (int b = 0; b < HN_STRIDE; ++b) R[b] = 0.0;
    const double r2 = (double)a.r2;
    int cx, cy, cz;
    cell_of(a.g, q, cx, cy, cz);
    for (int t = 0; t < 9; ++t) {
        const int dy = t % 3 - 1, dz = t / 3 - 1;
        const uint32_t r = (uint32_t)(cx + 1) + row_base(a.g, cy + dy, cz + dz);
        const uint32_t j1 = a.g.row_start[r + 3];
        for (uint32_t j = a.g.row_start[r]; j < j1; ++j) {
            const float4 p = a.g.sorted[j];
            const float d = flann_d2(q, f3(p.x, p.y, p.z));
            if (!(d > 0.f && d < a.r2) || a.cs[j] < a.min_pairs) continue;
            const double w = r2 / (double)d;
            W += w;
            const double2 *h = reinterpret_cast<const double2 *>(a.hn + (size_t)j * HN_STRIDE);
#pragma unroll
            for (int k = 0; k < HN_STRIDE / 2; ++k) {
                const double2 v = h[k];
                R[2 * k] += w * v.x;
                R[2 * k + 1] += w * v.y;   // (R[33]: the row's padding, 0)
            }
        }
    }
    const double *own = a.hn + (size_t)s * HN_STRIDE;
    const uint32_t *oh = a.spfh + (size_t)self * FPFH_DIM;
    const double cd = (double)c;
#pragma unroll
    for (int b = 0; b < FPFH_DIM; ++b)
        of[b] = W > 0.0 ? (float)(50.0 * (own[b] + R[b] / W)) : (float)((100.0 * (double)oh[b]) / cd);
    if (orw) {
        orw[0] = W;
#pragma unroll
        for (int b = 0; b < FPFH_DIM; ++b) orw[1 + b] = R[b];
    }
}

// per workgroup: pu[3 b] = its described points, pu[3 b + 1] = the sum of their c, pu[3 b + 2] = the largest c of any of its points
// (the order: fixed_reduce.h; terms 0 and 1 are sums, term 2 a maximum)
struct SumMaxU64 {
    __device__ __forceinline__ u64 operator()(int k, u64 a, u64 b) const { return k == 2 ? (b > a ? b : a) : a + b; }
};

__global__ __launch_bounds__(SUM_TPB) void k_fpfh_sum(const uint8_t *__restrict__ described, const uint32_t *__restrict__ pairs, uint32_t n,
                                                      u64 *__restrict__ pu) {
    __shared__ u64 s_red[SUM_TPB / 64][3];
    const uint32_t i = blockIdx.x * SUM_TPB + threadIdx.x;
    u64 v[3] = {0, 0, 0};            // described, its c, c
    if (i < n) {
        v[2] = pairs[i];
        if (described[i]) { v[0] = 1; v[1] = v[2]; }
    }
    block_reduce<SUM_TPB>(v, s_red, pu, SumMaxU64());
}
__global__ __launch_bounds__(64) void k_fpfh_final(const u64 *__restrict__ pu, uint32_t blocks, u64 *__restrict__ ru) {
    u64 v[3];
    final_reduce(pu, blocks, v, SumMaxU64());
    if (threadIdx.x != 0) return;
    ru[0] = v[0]; ru[1] = v[1]; ru[2] = v[2];
}

// ---- the match ---------------------------------------------------------------------------------------------------------------------
// part[(q * nch + blockIdx.y) * 2 + {0, 1}]: the two smallest keys (delta, t) of query q over the valid targets of chunk blockIdx.y
// (EMPTY: none; both EMPTY for a query that is not valid)
__global__ __launch_bounds__(MATCH_TPB) void k_feat_match(const float *__restrict__ qry, uint32_t nq, const float *__restrict__ tgt,
                                                          uint32_t nt, uint32_t chunk /* a multiple of FEAT_TILE */, uint32_t nch,
                                                          u64 *__restrict__ part) {
    __shared__ float s_t[FEAT_TILE * TILE_ROW];
    const uint32_t q = blockIdx.x * MATCH_TPB + threadIdx.x;
    const bool live = q < nq;
    float qd[FPFH_DIM];
#pragma unroll
    for (int b = 0; b < FPFH_DIM; ++b) qd[b] = live ? qry[(size_t)q * FPFH_DIM + b] : NAN;
    const bool valid = qd[0] == qd[0];
    u64 best[2] = {EMPTY, EMPTY};
    const uint32_t t_begin = blockIdx.y * chunk, t_end = min(nt, t_begin + chunk);
    for (uint32_t t0 = t_begin; t0 < t_end; t0 += FEAT_TILE) {
        const uint32_t tn = min((uint32_t)FEAT_TILE, t_end - t0);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < tn * FPFH_DIM; i += MATCH_TPB) {
            const uint32_t r = i / FPFH_DIM;
            s_t[r * TILE_ROW + (i - r * FPFH_DIM)] = tgt[(size_t)t0 * FPFH_DIM + i];
        }
        __syncthreads();
        if (valid)
            for (uint32_t j = 0; j < tn; ++j) {
                const float *t = s_t + j * TILE_ROW;
                if (t[0] != t[0]) continue;          // (wave-uniform: a broadcast read)
                float d = 0.f;
#pragma unroll
                for (int b = 0; b < FPFH_DIM; ++b) {
                    const float x = qd[b] - t[b];
                    d += x * x;
                }
                if (d == d) insert<2>(best, make_key(d, t0 + j));
            }
    }
    if (live) {
        u64 *o = part + ((size_t)q * nch + blockIdx.y) * 2;
        o[0] = best[0]; o[1] = best[1];
    }
}

__global__ __launch_bounds__(256) void k_feat_merge(const u64 *__restrict__ part, uint32_t nq, uint32_t nch, int32_t *__restrict__ nn,
                                                    float *__restrict__ d2) {
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    u64 best[2] = {EMPTY, EMPTY};
    const u64 *p = part + (size_t)q * nch * 2;
    for (uint32_t c = 0; c < 2 * nch; ++c) insert<2>(best, p[c]);
    nn[q] = best[0] == EMPTY ? -1 : (int32_t)(uint32_t)best[0];
    d2[2 * (size_t)q] = best[0] == EMPTY ? NAN : key_d(best[0]);
    d2[2 * (size_t)q + 1] = best[1] == EMPTY ? NAN : key_d(best[1]);
}

// flags[s] = 1: (s, nn[s]) is a correspondence; flags[ns] = 0 (the scan's extra slot)
__global__ __launch_bounds__(256) void k_feat_keep(const int32_t *__restrict__ nn, const float *__restrict__ d2,
                                                   const int32_t *__restrict__ back /* or nullptr: not mutual */, uint32_t ns,
                                                   float ratio2 /* 0: off */, uint32_t *__restrict__ flags) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s > ns) return;
    uint32_t keep = 0;
    if (s < ns && nn[s] >= 0) {
        keep = 1;
        if (back && back[nn[s]] != (int32_t)s) keep = 0;
        const float d1 = d2[2 * (size_t)s], dd = d2[2 * (size_t)s + 1];
        if (ratio2 != 0.f && dd == dd && !(d1 < ratio2 * dd)) keep = 0;
    }
    flags[s] = keep;
}
__global__ __launch_bounds__(256) void k_feat_compact(const uint32_t *__restrict__ flags, const uint32_t *__restrict__ offs,
                                                      const int32_t *__restrict__ nn, uint32_t ns, int32_t *__restrict__ corr) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= ns || !flags[s]) return;
    corr[2 * (size_t)offs[s]] = (int32_t)s;
    corr[2 * (size_t)offs[s] + 1] = nn[s];
}

}  // namespace

struct FpfhWork {
    TargetGrid grid;
    DBuf<float> in, desc;            // the host-pointer entry point's device copy (grow-only); the descriptors
    DBuf<float4> axes;
    DBuf<double> hn, raw;
    DBuf<uint32_t> cs, spfh, pairs;
    DBuf<uint8_t> described;
    DBuf<u64> partial, res;
    u64 h_u[3] = {0, 0, 0};
    // the match
    DBuf<float> m_src, m_tgt, d2, d2_back;
    DBuf<u64> part;
    DBuf<int32_t> nn, back, corr;
    DBuf<uint32_t> flags, offs;
    EventSpans<6> spans;             // 0..3: grid, spfh, weight; 4..5: the match
};

namespace {

struct Outputs {
    float *desc;
    uint8_t *described;
    uint32_t *pairs, *spfh;
    double *raw;
};

void check_params(uint32_t n, const plade_fpfh_params &p) {
    PLADE_REQUIRE(n >= 1, PLADE_EINVAL, "cloud_fpfh: the cloud is empty (n = 0)");
    PLADE_REQUIRE(radius_ok(p.radius, true), PLADE_EINVAL,
                  "cloud_fpfh: radius must be finite and > 0, and its fp32 square finite and not below FLT_MIN");
    PLADE_REQUIRE(p.min_pairs >= 1, PLADE_EINVAL, "cloud_fpfh: min_pairs must be >= 1");
}

// The descriptors of a device cloud of rows x y z nx ny nz (`stride` floats apart) with a known bounding box: leaves desc, described,
// pairs, spfh (and raw when wanted) in W, copies the wanted ones out, waits, fills the summary and the stats.
void fpfh_dev(plade_ctx *ctx, FpfhWork &W, const float *d_rows, uint32_t n, uint32_t stride, const float bbmin[3], const float bbmax[3],
              const plade_fpfh_params &p, const Outputs &out, plade_fpfh_summary *summary) {
    W.spans.mark(ctx, 0);
    TargetGrid &G = W.grid;
    const float r = (float)p.radius;
    G.build(ctx, d_rows, n, stride, radius_cell((double)r, bbmin, bbmax), bbmin, bbmax, true);
    const GridView g = view_of(G, "cloud_fpfh");
    float4 *d_axes = W.axes.ensure(n);
    hipLaunchKernelGGL(k_fpfh_axes, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, g.sorted, d_rows, stride, n, d_axes);
    HIP_TRY(hipGetLastError());
    W.spans.mark(ctx, 1);
    SpfhArgs a;
    memset(&a, 0, sizeof(a));
    a.g = g; a.axes = d_axes; a.n = n; a.r2 = r * r; a.min_pairs = (uint32_t)p.min_pairs;
    a.spfh = W.spfh.ensure((size_t)n * FPFH_DIM);
    a.pairs = W.pairs.ensure(n);
    a.described = W.described.ensure((size_t)n + 4);
    a.cs = W.cs.ensure(n);
    a.hn = W.hn.ensure((size_t)n * HN_STRIDE);
    hipLaunchKernelGGL(k_fpfh_spfh, dim3(cdiv(n, SPFH_TPB)), dim3(SPFH_TPB), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    W.spans.mark(ctx, 2);
    WeightArgs w;
    memset(&w, 0, sizeof(w));
    w.g = g; w.n = n; w.r2 = a.r2; w.min_pairs = a.min_pairs;
    w.cs = a.cs; w.hn = a.hn; w.spfh = a.spfh;
    w.desc = W.desc.ensure((size_t)n * FPFH_DIM + 4);
    w.raw = out.raw ? W.raw.ensure((size_t)n * (FPFH_DIM + 1)) : nullptr;
    hipLaunchKernelGGL(k_fpfh_weight, dim3(cdiv(n, WEIGHT_TPB)), dim3(WEIGHT_TPB), 0, ctx->stream, w);
    HIP_TRY(hipGetLastError());
    W.spans.mark(ctx, 3);
    const uint32_t blocks = cdiv(n, SUM_TPB);
    u64 *d_pu = W.partial.ensure((size_t)3 * blocks), *d_ru = W.res.ensure(4);
    hipLaunchKernelGGL(k_fpfh_sum, dim3(blocks), dim3(SUM_TPB), 0, ctx->stream, a.described, a.pairs, n, d_pu);
    hipLaunchKernelGGL(k_fpfh_final, dim3(1), dim3(64), 0, ctx->stream, d_pu, blocks, d_ru);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(W.h_u, d_ru, sizeof(W.h_u), hipMemcpyDeviceToHost, ctx->stream));
    if (out.desc) HIP_TRY(hipMemcpyAsync(out.desc, w.desc, (size_t)n * FPFH_DIM * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (out.described) HIP_TRY(hipMemcpyAsync(out.described, a.described, n, hipMemcpyDeviceToHost, ctx->stream));
    if (out.pairs) HIP_TRY(hipMemcpyAsync(out.pairs, a.pairs, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (out.spfh) HIP_TRY(hipMemcpyAsync(out.spfh, a.spfh, (size_t)n * FPFH_DIM * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (out.raw) HIP_TRY(hipMemcpyAsync(out.raw, w.raw, (size_t)n * (FPFH_DIM + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    summary->n = n;
    summary->described = W.h_u[0];
    summary->mean_pairs = W.h_u[0] ? (double)W.h_u[1] / (double)W.h_u[0] : 0.0;
    summary->max_pairs = (uint32_t)W.h_u[2];
    summary->reserved = 0;
    W.spans.collect(3);
    ctx->stats.clear();
    ctx->stats.add("fpfh_grid_s", W.spans.seconds(0));
    ctx->stats.add("fpfh_spfh_s", W.spans.seconds(1));
    ctx->stats.add("fpfh_weight_s", W.spans.seconds(2));
    ctx->stats.add("fpfh_described", (double)W.h_u[0]);
    grid_stats(ctx, "fpfh", W.grid);
}

// nn / d2 of every query over the targets (device tables of 33 floats per row)
void feat_search(plade_ctx *ctx, FpfhWork &W, const float *d_q, uint32_t nq, const float *d_t, uint32_t nt, int32_t *d_nn, float *d_d2) {
    // a workgroup is one wave of 64 queries against one chunk of targets: chunks of FEAT_CHUNK while that gives at most ~8 000
    // workgroups, longer ones for larger tables (two keys per (query, chunk): the table stays small)
    const uint32_t gx = cdiv(nq, MATCH_TPB), nch_max = std::max(1u, 8192u / gx);
    const uint32_t chunk = std::max((uint32_t)FEAT_CHUNK, (uint32_t)cdiv(cdiv(nt, nch_max), FEAT_TILE) * FEAT_TILE);
    const uint32_t nch = cdiv(nt, chunk);
    u64 *d_part = W.part.ensure((size_t)nq * nch * 2);
    hipLaunchKernelGGL(k_feat_match, dim3(gx, nch), dim3(MATCH_TPB), 0, ctx->stream, d_q, nq, d_t, nt, chunk, nch, d_part);
    hipLaunchKernelGGL(k_feat_merge, dim3(cdiv(nq, 256)), dim3(256), 0, ctx->stream, d_part, nq, nch, d_nn, d_d2);
    HIP_TRY(hipGetLastError());
}

int match_dev(plade_ctx *ctx, FpfhWork &W, const float *d_src, uint32_t ns, const float *d_tgt, uint32_t nt,
              const plade_feature_match_params &p, int32_t *nn_out, float *d2_out, int32_t *back_out, int32_t *corr_out, uint64_t cap,
              uint64_t *n_corr) {
    W.spans.mark(ctx, 4);
    int32_t *d_nn = W.nn.ensure(ns), *d_back = nullptr;
    float *d_d2 = W.d2.ensure((size_t)ns * 2);
    feat_search(ctx, W, d_src, ns, d_tgt, nt, d_nn, d_d2);
    if (p.mutual || back_out) {
        d_back = W.back.ensure(nt);
        feat_search(ctx, W, d_tgt, nt, d_src, ns, d_back, W.d2_back.ensure((size_t)nt * 2));
    }
    uint32_t *d_flags = W.flags.ensure((size_t)ns + 1), *d_offs = W.offs.ensure((size_t)ns + 1);
    hipLaunchKernelGGL(k_feat_keep, dim3(cdiv((size_t)ns + 1, 256)), dim3(256), 0, ctx->stream, d_nn, d_d2,
                       p.mutual ? (const int32_t *)d_back : (const int32_t *)nullptr, ns, p.max_ratio * p.max_ratio, d_flags);
    HIP_TRY(hipGetLastError());
    exclusive_scan_u32(ctx, d_flags, d_offs, (size_t)ns + 1);
    int32_t *d_corr = W.corr.ensure((size_t)ns * 2);
    hipLaunchKernelGGL(k_feat_compact, dim3(cdiv(ns, 256)), dim3(256), 0, ctx->stream, d_flags, d_offs, d_nn, ns, d_corr);
    HIP_TRY(hipGetLastError());
    W.spans.mark(ctx, 5);
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, d_offs + ns, 4, hipMemcpyDeviceToHost, ctx->stream));
    if (nn_out) HIP_TRY(hipMemcpyAsync(nn_out, d_nn, (size_t)ns * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (d2_out) HIP_TRY(hipMemcpyAsync(d2_out, d_d2, (size_t)ns * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (back_out) HIP_TRY(hipMemcpyAsync(back_out, d_back, (size_t)nt * 4, hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    *n_corr = total;
    const uint64_t w = std::min<uint64_t>(total, cap);
    if (corr_out && w) {
        HIP_TRY(hipMemcpyAsync(corr_out, d_corr, (size_t)w * 8, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
    }
    W.spans.collect(5, 4);
    ctx->stats.clear();
    ctx->stats.add("feat_match_s", W.spans.seconds(4));
    ctx->stats.add("feat_corr", (double)total);
    return (corr_out && total > cap) ? PLADE_ECAP : PLADE_OK;
}

void check_match(const plade_feature_match_params &p, uint32_t ns, uint32_t nt) {
    PLADE_REQUIRE(ns >= 1 && nt >= 1, PLADE_EINVAL, "match_features: an empty table (ns = 0 or nt = 0)");
    PLADE_REQUIRE(std::isfinite(p.max_ratio) && p.max_ratio >= 0.f && std::isfinite(p.max_ratio * p.max_ratio), PLADE_EINVAL,
                  "match_features: max_ratio must be finite and >= 0");
}

}  // namespace

// ---- the two steps as plade_register_features chains them (k_corr_pose.hip): nothing leaves the device but the summaries -------
void fpfh_table_dev(plade_ctx *ctx, const float *d_rows, uint32_t n, const float bbmin[3], const float bbmax[3],
                    const plade_fpfh_params &p, plade_features &out, plade_fpfh_summary *summary) {
    check_params(n, p);
    FpfhWork &W = work_in<FpfhWork>(ctx->fpfh_work);
    const Outputs none = {nullptr, nullptr, nullptr, nullptr, nullptr};
    fpfh_dev(ctx, W, d_rows, n, 6, bbmin, bbmax, p, none, summary);
    out.n = n;
    out.desc.ensure((size_t)n * FPFH_DIM + 4);
    HIP_TRY(hipMemcpyAsync(out.desc.p, W.desc.p, (size_t)n * FPFH_DIM * 4, hipMemcpyDeviceToDevice, ctx->stream));
}
const int32_t *feature_corr_dev(plade_ctx *ctx, const plade_features &src, const plade_features &tgt, const plade_feature_match_params &p,
                                uint64_t *n_corr) {
    check_match(p, src.n, tgt.n);
    FpfhWork &W = work_in<FpfhWork>(ctx->fpfh_work);
    match_dev(ctx, W, src.desc.p, src.n, tgt.desc.p, tgt.n, p, nullptr, nullptr, nullptr, nullptr, 0, n_corr);
    return W.corr.p;
}

}  // namespace plade

using namespace plade;

// ---- C ABI (include/plade_hip.h) ---------------------------------------------------------------------------------------------
extern "C" void plade_fpfh_default_params(plade_fpfh_params *p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->radius = 0.0;
    p->min_pairs = 5;
}

extern "C" void plade_feature_match_default_params(plade_feature_match_params *p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->mutual = 1;
    p->max_ratio = 0.f;
}

extern "C" int plade_cloud_fpfh(plade_ctx *ctx, const float *pos_nrm, uint32_t n, const plade_fpfh_params *params, float *desc_out,
                                uint8_t *described_out, uint32_t *pairs_out, uint32_t *spfh_out, double *raw_out,
                                plade_fpfh_summary *summary) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(pos_nrm && params && summary, PLADE_EINVAL, "plade_cloud_fpfh: NULL cloud, params or summary");
        check_params(n, *params);
        FpfhWork &W = work_in<FpfhWork>(ctx->fpfh_work);
        float mn[3], mx[3];
        upload_rows(ctx, W.in, pos_nrm, n, 6, mn, mx);                   // (the bounding box checks the coordinates)
        const Outputs out = {desc_out, described_out, pairs_out, spfh_out, raw_out};
        fpfh_dev(ctx, W, W.in.p, n, 6, mn, mx, *params, out, summary);
        return PLADE_OK;
    });
}

extern "C" int plade_cloud_fpfh_dev(plade_ctx *ctx, plade_cloud *cloud, const plade_fpfh_params *params, float *desc_out,
                                    uint8_t *described_out, uint32_t *pairs_out, uint32_t *spfh_out, double *raw_out,
                                    plade_features **features_out, plade_fpfh_summary *summary) {
    return guarded(ctx, [&]() -> int {
        if (features_out) *features_out = nullptr;
        PLADE_REQUIRE(cloud && params && summary, PLADE_EINVAL, "plade_cloud_fpfh_dev: NULL cloud, params or summary");
        const CloudDev &c = cloud->dev;
        check_params(c.n, *params);
        FpfhWork &W = work_in<FpfhWork>(ctx->fpfh_work);
        const Outputs out = {desc_out, described_out, pairs_out, spfh_out, raw_out};
        fpfh_dev(ctx, W, c.aos.p, c.n, 6, c.bbmin, c.bbmax, *params, out, summary);
        if (features_out) {
            plade_features *f = new plade_features;
            try {
                f->n = c.n;
                f->desc.ensure((size_t)c.n * FPFH_DIM + 4);
                HIP_TRY(hipMemcpyAsync(f->desc.p, W.desc.p, (size_t)c.n * FPFH_DIM * 4, hipMemcpyDeviceToDevice, ctx->stream));
                ctx->sync();
            } catch (...) { delete f; throw; }
            *features_out = f;
        }
        return PLADE_OK;
    });
}

extern "C" void plade_features_free(plade_features *f) { delete f; }

extern "C" int plade_match_features(plade_ctx *ctx, const float *src, uint32_t ns, const float *tgt, uint32_t nt,
                                    const plade_feature_match_params *params, int32_t *nn_out, float *d2_out, int32_t *back_out,
                                    int32_t *corr_out, uint64_t cap, uint64_t *n_corr) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(src && tgt && n_corr, PLADE_EINVAL, "plade_match_features: NULL table or n_corr");
        const plade_feature_match_params p = params_or_default(params, plade_feature_match_default_params);
        check_match(p, ns, nt);
        FpfhWork &W = work_in<FpfhWork>(ctx->fpfh_work);
        float *d_s = W.m_src.ensure((size_t)ns * FPFH_DIM + 4), *d_t = W.m_tgt.ensure((size_t)nt * FPFH_DIM + 4);
        HIP_TRY(hipMemcpyAsync(d_s, src, (size_t)ns * FPFH_DIM * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d_t, tgt, (size_t)nt * FPFH_DIM * 4, hipMemcpyHostToDevice, ctx->stream));
        return match_dev(ctx, W, d_s, ns, d_t, nt, p, nn_out, d2_out, back_out, corr_out, cap, n_corr);
    });
}

extern "C" int plade_match_features_dev(plade_ctx *ctx, plade_features *src, plade_features *tgt, const plade_feature_match_params *params,
                                        int32_t *nn_out, float *d2_out, int32_t *back_out, int32_t *corr_out, uint64_t cap,
                                        uint64_t *n_corr) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(src && tgt && n_corr, PLADE_EINVAL, "plade_match_features_dev: NULL table or n_corr");
        const plade_feature_match_params p = params_or_default(params, plade_feature_match_default_params);
        check_match(p, src->n, tgt->n);
        return match_dev(ctx, work_in<FpfhWork>(ctx->fpfh_work), src->desc.p, src->n, tgt->desc.p, tgt->n, p, nn_out, d2_out, back_out,
                         corr_out, cap, n_corr);
    });
}
