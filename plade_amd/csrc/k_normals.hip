// plade_amd/csrc/k_normals.hip -- exact k-nearest-neighbour PCA normals on gfx950 (semantics: normals.h).
//
// Layout
//   grid    the dense row index of TargetGrid, walked with the pieces of grid_walk.h.  The cell is adapted to the cloud
//           (build_knn_grid) so that an occupied cell holds about 0.7 k points: the k-th neighbour of a surface point then
//           usually lies well inside the 27-cell block around its cell, and no cell is large.
//   search  k_normals_grid: one lane per point, lanes in the grid's sorted order (the 64 queries of a wavefront share their
//           candidate runs: L1 / L2 hits).  Each lane keeps its K best (d, j) keys -- 64-bit words d_bits << 32 | j, ordered
//           exactly like (d, j) because d >= 0 -- as a sorted list in registers (statically indexed: no scratch).  A point
//           whose k-th key is closer than the outside of its 27-cell block (less a margin for the fp32 cell assignment) is
//           finished; the others are appended to a compacted list.
//   rings   k_normals_ring: one wavefront per listed point.  The wave keeps the exact 64 best keys of what it has scanned as one
//           key per lane (wave_merge: two registers per lane whatever k is) and scans blocks of growing radius (ring_step); it
//           ends when the k-th key is closer than the outside of the block or the block covers the grid.  Sparse regions and
//           isolated outliers come out exact.
//   PCA     in the same kernels, by the one function pca_store (identical fp64 arithmetic on both paths): two passes over the
//           neighbour list (staged in LDS) in its order, then pca_eig (pca_eig.h, shared with k_smooth.hip): the closed-form
//           eigen-solve of the 3 x 3 symmetric covariance, the eigenvector of the smallest eigenvalue as well as its conditioning
//           allows (the contract stands there); orientation toward the viewpoint.
#include "normals.h"
#include "cloud_tool.h"
#include "grid_walk.h"
#include "pca_eig.h"
#include "voxel.h"

namespace plade {

struct NormalsWork {
    TargetGrid grid;
    DBuf<uint32_t> fail, count;
    DBuf<float> in, out, curv;       // the host-pointer entry points' device copies (grow-only)
    DBuf<int32_t> nbr;
    EventSpans<3> spans;             // grid, search
    int builds = 0;
    uint32_t h_count = 0;
};

namespace {

struct NrmArgs {
    GridView g;
    const float *xyz;
    uint32_t stride, n;
    int m, k;                        // k_eff = min(k, n); k = the requested count (row length of nbr)
    double margin;                   // grid_margin
    double view[3];
    float *out;
    float *curv;
    int32_t *nbr;
    uint32_t *fail, *fail_count;
};

// candidates [j0, j1) of the sorted points
template <int K>
__device__ __forceinline__ void scan_run(const NrmArgs &a, u64 (&best)[K], f3 q, uint32_t j0, uint32_t j1) {
    for (uint32_t j = j0; j < j1; ++j) {
        const float4 p = a.g.sorted[j];
        insert<K>(best, make_key(flann_d2(q, f3(p.x, p.y, p.z)), __float_as_uint(p.w)));
    }
}

// neighbour list -> outputs of point `orig` (p: its coordinates).  The list is staged in LDS: original index of neighbour b
// = list[b * ld], b < a.m (plain loops: unrolled over K, the gathers of all neighbours would be hoisted into registers)
__device__ void pca_store(const NrmArgs &a, const uint32_t *list, int ld, f3 p, uint32_t orig) {
    const int m = a.m;
    if (a.nbr) {
        int32_t *row = a.nbr + (size_t)orig * (uint32_t)a.k;
        for (int b = 0; b < a.k; ++b) row[b] = b < m ? (int32_t)list[b * ld] : -1;
    }
    const double px = p.x, py = p.y, pz = p.z;
    double nx = NAN, ny = NAN, nz = NAN, curvature = NAN;
    if (m >= 3) {
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (int b = 0; b < m; ++b) {
            const float *r = a.xyz + (size_t)list[b * ld] * a.stride;
            sx += (double)r[0] - px; sy += (double)r[1] - py; sz += (double)r[2] - pz;
        }
        const double mx = sx / m, my = sy / m, mz = sz / m;
        double c00 = 0.0, c01 = 0.0, c02 = 0.0, c11 = 0.0, c12 = 0.0, c22 = 0.0;
        for (int b = 0; b < m; ++b) {
            const float *r = a.xyz + (size_t)list[b * ld] * a.stride;
            const double ex = ((double)r[0] - px) - mx, ey = ((double)r[1] - py) - my, ez = ((double)r[2] - pz) - mz;
            c00 += ex * ex; c01 += ex * ey; c02 += ex * ez;
            c11 += ey * ey; c12 += ey * ez; c22 += ez * ez;
        }
        c00 /= m; c01 /= m; c02 /= m; c11 /= m; c12 /= m; c22 /= m;
        d3 nv;
        double l0, tr;
        if (pca_eig(c00, c01, c02, c11, c12, c22, nv, l0, tr)) {   // closed-form eigen-solve (pca_eig.h)
            nx = nv.x; ny = nv.y; nz = nv.z;
            if ((a.view[0] - px) * nx + (a.view[1] - py) * ny + (a.view[2] - pz) * nz < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
            curvature = fmax(l0, 0.0) / tr;
        }
    }
    float *o = a.out + (size_t)orig * 6;
    o[0] = p.x; o[1] = p.y; o[2] = p.z;
    o[3] = (float)nx; o[4] = (float)ny; o[5] = (float)nz;
    if (a.curv) a.curv[orig] = (float)curvature;
}

constexpr int GRID_TPB = 128;

template <int K>
__global__ __launch_bounds__(GRID_TPB) void k_normals_grid(const NrmArgs a) {
    __shared__ uint32_t s_idx[K][GRID_TPB];   // the finished lists, column per lane (K = 64: 32 KB)
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    bool fail = false;
    if (s < a.n) {
        const float4 q4 = a.g.sorted[s];
        const f3 q(q4.x, q4.y, q4.z);
        int cx, cy, cz;
        cell_of(a.g, q, cx, cy, cz);
        u64 best[K];
#pragma unroll
        for (int b = 0; b < K; ++b) best[b] = EMPTY;
        // for_block27's runs, written out: handed to a lambda by reference, the register list is allocated differently for K = 32, 64
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy) {
                const uint32_t r = (uint32_t)(cx + 1) + row_base(a.g, cy + dy, cz + dz);
                scan_run<K>(a, best, q, a.g.row_start[r], a.g.row_start[r + 3]);
            }
        u64 kth = EMPTY;
#pragma unroll
        for (int b = 0; b < K; ++b) if (b == a.m - 1) kth = best[b];
        if (kth != EMPTY && inside_reach(key_d(kth), block_reach(a.g, q, cx, cy, cz, 1, a.margin))) {
#pragma unroll
            for (int b = 0; b < K; ++b) if (b < a.m) s_idx[b][threadIdx.x] = (uint32_t)best[b];
            pca_store(a, &s_idx[0][threadIdx.x], GRID_TPB, q, __float_as_uint(q4.w));
        } else
            fail = true;
    }
    fail_append(fail, s, a.fail, a.fail_count);   // to the list of the ring path
}

constexpr int RING_WAVES = 4;

// One wavefront per point the grid kernel could not finish.  The wave keeps the exact top 64 of everything it has scanned as
// one key per lane (wave_merge) and scans blocks of growing radius (ring_step); a batch is merged only when one of its keys is
// below the current k-th.  The point is finished when the k-th key is closer than the outside of the block, or the block covers
// the grid.
__global__ __launch_bounds__(64 * RING_WAVES) void k_normals_ring(const NrmArgs a) {
    __shared__ uint32_t s_list[RING_WAVES][64];
    const int lane = (int)(threadIdx.x & 63u), wv = (int)(threadIdx.x >> 6);
    const uint32_t total = *a.fail_count, stride_w = gridDim.x * RING_WAVES;
    for (uint32_t i = blockIdx.x * RING_WAVES + (uint32_t)wv; i < total; i += stride_w) {
        const uint32_t s = a.fail[i];
        const float4 q4 = a.g.sorted[s];
        const f3 q(q4.x, q4.y, q4.z);
        int cx, cy, cz;
        cell_of(a.g, q, cx, cy, cz);
        u64 list = EMPTY;
        for (int rin = -1, rout = 1;; rin = rout, rout += max(1, rout / 2)) {
            ring_step(a.g, cx, cy, cz, rin, rout, lane, [&](bool valid, float4 p) {
                const u64 key = valid ? make_key(flann_d2(q, f3(p.x, p.y, p.z)), __float_as_uint(p.w)) : EMPTY;
                const u64 kth = __shfl(list, a.m - 1, 64);
                if (__ballot(key < kth)) list = wave_merge(list, key, lane);
            });
            const double reach = block_reach(a.g, q, cx, cy, cz, rout, a.margin);
            if (reach == INFINITY) break;
            if (inside_reach(key_d(__shfl(list, a.m - 1, 64)), reach)) break;   // (EMPTY: NaN, not inside)
        }
        if (lane < a.m) s_list[wv][lane] = (uint32_t)list;
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) pca_store(a, &s_list[wv][0], 1, q, __float_as_uint(q4.w));
        __builtin_amdgcn_wave_barrier();
    }
}

template <int K>
void launch_search(plade_ctx *ctx, const NrmArgs &a) {
    hipLaunchKernelGGL(k_normals_grid<K>, dim3(cdiv(a.n, GRID_TPB)), dim3(GRID_TPB), 0, ctx->stream, a);
    // persistent: the list's length stays on the device (no host round trip)
    hipLaunchKernelGGL(k_normals_ring, dim3(std::min(cdiv(a.n, RING_WAVES), 2048u)), dim3(64 * RING_WAVES), 0, ctx->stream, a);
}

}  // namespace

void normals_check_args(uint32_t n, uint32_t stride, int k, const float *view) {
    PLADE_REQUIRE(n >= 1, PLADE_EINVAL, "estimate_normals: the cloud is empty (n = 0)");
    PLADE_REQUIRE(stride >= 3, PLADE_EINVAL, "estimate_normals: stride must be >= 3 floats");
    PLADE_REQUIRE(k >= NORMALS_K_MIN && k <= NORMALS_K_MAX, PLADE_EINVAL, "estimate_normals: k must be in [3, 64]");
    PLADE_REQUIRE(view && std::isfinite(view[0]) && std::isfinite(view[1]) && std::isfinite(view[2]), PLADE_EINVAL,
                  "estimate_normals: the viewpoint must be finite");
}

void estimate_normals_dev(plade_ctx *ctx, NormalsWork &W, const float *d_xyz, uint32_t n, uint32_t stride, const float bbmin[3],
                          const float bbmax[3], int k, const float view[3], float *d_out, float *d_curv, int32_t *d_nbr) {
    W.spans.mark(ctx, 0);
    TargetGrid &G = W.grid;
    const int m = (int)std::min<uint32_t>((uint32_t)k, n);
    uint32_t *d_occ = W.count.ensure(4);   // [0]: the ring list's length, [1]: occupied cells
    W.builds = build_knn_grid(ctx, G, d_xyz, n, stride, bbmin, bbmax, k, d_occ + 1, "estimate_normals");
    W.spans.mark(ctx, 1);
    NrmArgs a;
    a.g = view_of(G, "estimate_normals");
    a.xyz = d_xyz; a.stride = stride; a.n = n; a.m = m; a.k = k;
    a.margin = grid_margin(a.g, bbmin, bbmax);
    for (int t = 0; t < 3; ++t) a.view[t] = view[t];
    a.out = d_out; a.curv = d_curv; a.nbr = d_nbr;
    a.fail = W.fail.ensure(n); a.fail_count = d_occ;
    ctx->fill_async(d_occ, 0, 4);
    if (k <= 8) launch_search<8>(ctx, a);
    else if (k <= 16) launch_search<16>(ctx, a);
    else if (k <= 32) launch_search<32>(ctx, a);
    else launch_search<64>(ctx, a);
    HIP_TRY(hipGetLastError());
    W.spans.mark(ctx, 2);
    ctx->d2h(&W.h_count, d_occ, 4);
}

void normals_stats(plade_ctx *ctx, NormalsWork &W) {
    W.spans.collect();
    ctx->stats.clear();
    ctx->stats.add("normals_grid_s", W.spans.seconds(0));
    ctx->stats.add("normals_search_s", W.spans.seconds(1));
    ctx->stats.add("normals_grid_builds", W.builds);
    ctx->stats.add("normals_ring_queries", W.h_count);
    grid_stats(ctx, "normals", W.grid);
}

}  // namespace plade

using namespace plade;

// ---- C ABI (include/plade_hip.h) ---------------------------------------------------------------------------------------------
namespace {
const float kOrigin[3] = {0.f, 0.f, 0.f};
}  // namespace

extern "C" int plade_estimate_normals(plade_ctx *ctx, const float *xyz, uint32_t n, uint32_t stride, int32_t k,
                                      const float *viewpoint, float *pos_nrm_out, float *curvature_out, int32_t *nbr_out) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(xyz && pos_nrm_out, PLADE_EINVAL, "plade_estimate_normals: bad argument");
        const float *view = viewpoint ? viewpoint : kOrigin;
        normals_check_args(n, stride, k, view);
        NormalsWork &W = work_in<NormalsWork>(ctx->normals_work);
        float mn[3], mx[3];
        upload_rows(ctx, W.in, xyz, n, stride, mn, mx);
        W.out.ensure((size_t)n * 6);
        if (curvature_out) W.curv.ensure(n);
        if (nbr_out) W.nbr.ensure((size_t)n * k);
        estimate_normals_dev(ctx, W, W.in.p, n, stride, mn, mx, k, view, W.out.p, curvature_out ? W.curv.p : nullptr,
                             nbr_out ? W.nbr.p : nullptr);
        HIP_TRY(hipMemcpyAsync(pos_nrm_out, W.out.p, (size_t)n * 24, hipMemcpyDeviceToHost, ctx->stream));
        if (curvature_out) HIP_TRY(hipMemcpyAsync(curvature_out, W.curv.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (nbr_out) HIP_TRY(hipMemcpyAsync(nbr_out, W.nbr.p, (size_t)n * k * 4, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        normals_stats(ctx, W);
        return PLADE_OK;
    });
}

extern "C" int plade_cloud_upload_xyz(plade_ctx *ctx, const float *xyz, uint32_t n, uint32_t stride, int32_t k,
                                      const float *viewpoint, plade_cloud **out) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(xyz && out, PLADE_EINVAL, "plade_cloud_upload_xyz: bad argument");
        *out = nullptr;
        const float *view = viewpoint ? viewpoint : kOrigin;
        normals_check_args(n, stride, k, view);
        NormalsWork &W = work_in<NormalsWork>(ctx->normals_work);
        float mn[3], mx[3];
        upload_rows(ctx, W.in, xyz, n, stride, mn, mx);
        resident_result(ctx, out, [&](CloudDev &c) {
            cloud_shape(c, n);
            estimate_normals_dev(ctx, W, W.in.p, n, stride, mn, mx, k, view, c.aos.p, nullptr, nullptr);
            ctx->sync();
            normals_stats(ctx, W);
        });
        return PLADE_OK;
    });
}
