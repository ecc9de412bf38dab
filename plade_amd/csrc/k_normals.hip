// plade_amd/csrc/k_normals.hip -- exact k-nearest-neighbour PCA normals on gfx950 (semantics: normals.h).
//
// Layout
//   grid    the dense row index of TargetGrid (overlap.h: points sorted by padded linear cell id, float4 with the original index
//           in w; the 27 cells around a cell are nine contiguous runs of `sorted`).  The cell is adapted to the cloud so that
//           an occupied cell holds about 0.7 k points: the k-th neighbour of a surface point then usually lies well inside
//           the 27-cell block around its cell, and no cell is large.
//   search  k_normals_grid: one lane per point, lanes in the grid's sorted order (the 64 queries of a wavefront share their
//           candidate runs: L1 / L2 hits).  Each lane keeps its K best (d, j) keys -- 64-bit words d_bits << 32 | j, ordered
//           exactly like (d, j) because d >= 0 -- as a sorted list in registers (statically indexed: no scratch).  A point
//           whose k-th key is closer than the outside of its 27-cell block (less a margin for the fp32 cell assignment) is
//           finished; the others are appended to a compacted list.
//   rings   k_normals_ring: one wavefront per listed point.  The wave keeps the exact 64 best keys of what it has scanned as one
//           key per lane (bitonic merges across the lanes: two registers per lane whatever k is) and scans blocks of growing
//           radius, each step reading only the runs its previous block did not hold (O(R^2) row look-ups for radius R); it ends
//           when the k-th key is closer than the outside of the block or the block covers the grid.  Sparse regions and
//           isolated outliers come out exact.
//   PCA     in the same kernels, by the one function pca_store (identical fp64 arithmetic on both paths): two passes over the
//           neighbour list (staged in LDS) in its order, closed-form eigenvalues of the 3 x 3 symmetric covariance, the eigenvector of the
//           smallest from the cross products of the rows of C - l0 I, orientation toward the viewpoint.
#include "normals.h"
#include "overlap.h"
#include "voxel.h"

namespace plade {

struct NormalsWork {
    TargetGrid grid;
    DBuf<uint32_t> fail, count;
    DBuf<float> in, out, curv;       // the host-pointer entry points' device copies (grow-only)
    DBuf<int32_t> nbr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    int builds = 0;
    uint32_t h_count = 0;
    ~NormalsWork() { for (hipEvent_t &e : ev) if (e) (void)hipEventDestroy(e); }
};
NormalsWork *normals_work_create() { return new NormalsWork; }
void normals_work_destroy(NormalsWork *w) { delete w; }

namespace {

struct NrmArgs {
    const float4 *sorted;
    const uint32_t *row_start;
    const float *xyz;
    uint32_t stride, n;
    int m, k;                        // k_eff = min(k, n); k = the requested count (row length of nbr)
    float mnx, mny, mnz, inv;        // the grid's cell assignment (k_cell_ids)
    int dx, dy, dz, DX, DY;          // cells, padded row pitch
    double mn[3], cell, margin;
    double view[3];
    float *out;
    float *curv;
    int32_t *nbr;
    uint32_t *fail, *fail_count;
};

typedef unsigned long long u64;
constexpr u64 EMPTY = ~0ull;

__device__ __forceinline__ u64 make_key(float d, uint32_t j) { return ((u64)__float_as_uint(d) << 32) | (u64)j; }
__device__ __forceinline__ float key_d(u64 key) { return __uint_as_float((uint32_t)(key >> 32)); }   // EMPTY: NaN

template <int K>
__device__ __forceinline__ void insert(u64 (&best)[K], u64 key) {
    if (key < best[K - 1]) {
        // top down, in place: the new entry b depends only on the old entries b - 1 and b (no second copy of the list)
#pragma unroll
        for (int b = K - 1; b > 0; --b) best[b] = key < best[b - 1] ? best[b - 1] : (key < best[b] ? key : best[b]);
        best[0] = key < best[0] ? key : best[0];
    }
}

// candidates [j0, j1) of the sorted points
template <int K>
__device__ __forceinline__ void scan_run(const NrmArgs &a, u64 (&best)[K], f3 q, uint32_t j0, uint32_t j1) {
    for (uint32_t j = j0; j < j1; ++j) {
        const float4 p = a.sorted[j];
        insert<K>(best, make_key(flann_d2(q, f3(p.x, p.y, p.z)), __float_as_uint(p.w)));
    }
}

// distance from q to the outside of the block of cells [c - R, c + R]^3 (infinite where the block reaches the grid's edge:
// cell ids are clamped there, nothing lies beyond), less the margin; +inf: the block covers the grid
__device__ __forceinline__ double block_reach(const NrmArgs &a, f3 q, int cx, int cy, int cz, int R) {
    double b = INFINITY;
    const double qv[3] = {q.x, q.y, q.z};
    const int c[3] = {cx, cy, cz}, d[3] = {a.dx, a.dy, a.dz};
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        if (c[t] - R > 0) b = fmin(b, qv[t] - (a.mn[t] + (double)(c[t] - R) * a.cell));
        if (c[t] + R < d[t] - 1) b = fmin(b, (a.mn[t] + (double)(c[t] + R + 1) * a.cell) - qv[t]);
    }
    return b == INFINITY ? b : b - a.margin;
}
// true: every point outside the block is farther than d (squared distance)
__device__ __forceinline__ bool inside_reach(float d, double reach) {
    if (reach == INFINITY) return true;
    return reach > 0.0 && d < (float)(reach * reach);
}

__device__ __forceinline__ void cell_of(const NrmArgs &a, f3 q, int &cx, int &cy, int &cz) {   // = k_cell_ids
    cx = min(max((int)floorf((q.x - a.mnx) * a.inv), 0), a.dx - 1);
    cy = min(max((int)floorf((q.y - a.mny) * a.inv), 0), a.dy - 1);
    cz = min(max((int)floorf((q.z - a.mnz) * a.inv), 0), a.dz - 1);
}

// fp64 3-vector helpers of the eigen-solve
struct d3 { double x, y, z; };
__device__ __forceinline__ d3 dcross(d3 u, d3 v) { return {u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x}; }
__device__ __forceinline__ double ddot(d3 u, d3 v) { return u.x * v.x + u.y * v.y + u.z * v.z; }

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
        if (!(c00 == 0.0 && c01 == 0.0 && c02 == 0.0 && c11 == 0.0 && c12 == 0.0 && c22 == 0.0)) {
            // eigenvalues: trigonometric solution of det(C - l I) = 0 on the shifted, scaled matrix
            const double tr = c00 + c11 + c22, q = tr / 3.0;
            const double b00 = c00 - q, b11 = c11 - q, b22 = c22 - q;
            const double p2 = b00 * b00 + b11 * b11 + b22 * b22 + 2.0 * (c01 * c01 + c02 * c02 + c12 * c12);
            double l0 = q;
            if (p2 > 0.0) {
                const double pp = sqrt(p2 / 6.0);
                const double i00 = b00 / pp, i11 = b11 / pp, i22 = b22 / pp, i01 = c01 / pp, i02 = c02 / pp, i12 = c12 / pp;
                double r = 0.5 * (i00 * (i11 * i22 - i12 * i12) - i01 * (i01 * i22 - i12 * i02) + i02 * (i01 * i12 - i11 * i02));
                r = fmin(1.0, fmax(-1.0, r));
                const double phi = acos(r) / 3.0;
                l0 = q + 2.0 * pp * cos(phi + 2.0943951023931954923);   // the smallest root (2 pi / 3)
            }
            // eigenvector of l0: the largest cross product of two rows of C - l0 I; when all of them vanish (a line: the
            // eigenspace of l0 is a plane) any vector orthogonal to the largest row
            const d3 r0 = {c00 - l0, c01, c02}, r1 = {c01, c11 - l0, c12}, r2 = {c02, c12, c22 - l0};
            const d3 x01 = dcross(r0, r1), x02 = dcross(r0, r2), x12 = dcross(r1, r2);
            const double n01 = ddot(x01, x01), n02 = ddot(x02, x02), n12 = ddot(x12, x12);
            d3 v = x01;
            double vn = n01;
            if (n02 > vn) { v = x02; vn = n02; }
            if (n12 > vn) { v = x12; vn = n12; }
            const double q0 = ddot(r0, r0), q1 = ddot(r1, r1), q2 = ddot(r2, r2);
            double rmax = q0;
            d3 rr = r0;
            if (q1 > rmax) { rr = r1; rmax = q1; }
            if (q2 > rmax) { rr = r2; rmax = q2; }
            if (!(vn > 1e-20 * rmax * rmax)) {
                if (rmax > 0.0) {
                    const double ax = fabs(rr.x), ay = fabs(rr.y), az = fabs(rr.z);
                    const d3 e = ax <= ay && ax <= az ? d3{1.0, 0.0, 0.0} : ay <= az ? d3{0.0, 1.0, 0.0} : d3{0.0, 0.0, 1.0};
                    v = dcross(rr, e);
                } else {
                    v = {0.0, 0.0, 1.0};   // isotropic: every direction is an eigenvector
                }
                vn = ddot(v, v);
            }
            const double s = 1.0 / sqrt(vn);
            nx = v.x * s; ny = v.y * s; nz = v.z * s;
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
        const float4 q4 = a.sorted[s];
        const f3 q(q4.x, q4.y, q4.z);
        int cx, cy, cz;
        cell_of(a, q, cx, cy, cz);
        u64 best[K];
#pragma unroll
        for (int b = 0; b < K; ++b) best[b] = EMPTY;
        // nine runs of three cells; the padding of the row index makes every row of the block valid
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy) {
                const uint32_t r = (uint32_t)(cx + 1) + (uint32_t)a.DX * ((uint32_t)(cy + dy + 2) + (uint32_t)a.DY * (uint32_t)(cz + dz + 2));
                scan_run<K>(a, best, q, a.row_start[r], a.row_start[r + 3]);
            }
        u64 kth = EMPTY;
#pragma unroll
        for (int b = 0; b < K; ++b) if (b == a.m - 1) kth = best[b];
        if (kth != EMPTY && inside_reach(key_d(kth), block_reach(a, q, cx, cy, cz, 1))) {
#pragma unroll
            for (int b = 0; b < K; ++b) if (b < a.m) s_idx[b][threadIdx.x] = (uint32_t)best[b];
            pca_store(a, &s_idx[0][threadIdx.x], GRID_TPB, q, __float_as_uint(q4.w));
        } else
            fail = true;
    }
    // wave-aggregated append to the list of the ring path
    const u64 mask = __ballot(fail);
    if (mask) {
        const uint32_t lane = threadIdx.x & 63u, leader = (uint32_t)__ffsll((long long)mask) - 1u;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(a.fail_count, (uint32_t)__popcll(mask));
        base = __shfl(base, (int)leader, 64);
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        if (fail) a.fail[base + rank] = s;
    }
}

constexpr int RING_WAVES = 4;

// The wave's 64 smallest keys: lane r holds the r-th.  merged with one key per lane (EMPTY: none): the new keys are sorted across
// the wave (bitonic, 21 steps), reversed and merged with the list (the element-wise minimum of an ascending and a descending
// sequence is a bitonic sequence that holds the 64 smallest of both, 6 more steps).  Two u64 registers per lane, whatever k is.
__device__ __forceinline__ u64 wave_merge(u64 list, u64 key, int lane) {
    u64 v = key;
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1)
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const u64 o = __shfl_xor(v, stride, 64);
            const bool keep_min = ((lane & stride) == 0) == ((lane & size) == 0);
            v = keep_min ? (o < v ? o : v) : (o < v ? v : o);
        }
    const u64 r = __shfl(v, 63 - lane, 64);
    u64 t = list < r ? list : r;
#pragma unroll
    for (int stride = 32; stride > 0; stride >>= 1) {
        const u64 o = __shfl_xor(t, stride, 64);
        t = (lane & stride) == 0 ? (o < t ? o : t) : (o < t ? t : o);
    }
    return t;
}

// One wavefront per point the grid kernel could not finish.  The wave keeps the exact top 64 of everything it has scanned as
// one key per lane (wave_merge) and scans the block [c - rout, c + rout]^3 in growing steps: a step reads only what the previous
// block [c - rin, c + rin]^3 did not hold -- whole x runs of the rows outside the old block's y-z square, the two x runs left and
// right of it in the rows inside --, so each step costs one or two row look-ups per in-grid row of the new block (its y-z square,
// not its volume), and the radius grows by half per step (rout = rout + max(1, rout / 2)): an isolated point's search costs
// O(rows of the final block), i.e. O(R^2) look-ups, not the O(R^3) of ring-by-ring cells.  The candidates of all lanes' runs are
// handed out 64 at a time (a wave-wide prefix sum over the run lengths, each lane finding its run by binary search over the
// lanes), and a batch is merged only when one of its keys is below the current k-th.  The point is finished when the k-th key
// is closer than the outside of the block, or the block covers the grid.
__global__ __launch_bounds__(64 * RING_WAVES) void k_normals_ring(const NrmArgs a) {
    __shared__ uint32_t s_list[RING_WAVES][64];
    const int lane = (int)(threadIdx.x & 63u), wv = (int)(threadIdx.x >> 6);
    const uint32_t total = *a.fail_count, stride_w = gridDim.x * RING_WAVES;
    for (uint32_t i = blockIdx.x * RING_WAVES + (uint32_t)wv; i < total; i += stride_w) {
        const uint32_t s = a.fail[i];
        const float4 q4 = a.sorted[s];
        const f3 q(q4.x, q4.y, q4.z);
        int cx, cy, cz;
        cell_of(a, q, cx, cy, cz);
        u64 list = EMPTY;
        for (int rin = -1, rout = 1;; rin = rout, rout += max(1, rout / 2)) {
            const int y0 = max(cy - rout, 0), y1 = min(cy + rout, a.dy - 1), z0 = max(cz - rout, 0), z1 = min(cz + rout, a.dz - 1);
            const int ny = y1 - y0 + 1, rows = ny * (z1 - z0 + 1);
            const int xo0 = max(cx - rout, 0), xo1 = min(cx + rout, a.dx - 1);   // x range of the new block
            for (int t0 = 0; t0 < rows; t0 += 64) {                              // (wave-uniform)
                const int t = t0 + lane;
                uint32_t a0 = 0, la = 0, b0 = 0, lb = 0;                         // up to two runs of this lane's row
                if (t < rows) {
                    const int y = y0 + t % ny, z = z0 + t / ny;
                    const uint32_t row = (uint32_t)a.DX * ((uint32_t)(y + 2) + (uint32_t)a.DY * (uint32_t)(z + 2)) + 2u;
                    if (abs(y - cy) > rin || abs(z - cz) > rin) {                // outside the old block's y-z square: the whole run
                        a0 = a.row_start[row + (uint32_t)xo0];
                        la = a.row_start[row + (uint32_t)xo1 + 1u] - a0;
                    } else {                                                     // inside: left and right of the old block
                        if (cx - rin - 1 >= xo0) {
                            a0 = a.row_start[row + (uint32_t)xo0];
                            la = a.row_start[row + (uint32_t)(cx - rin)] - a0;
                        }
                        if (cx + rin + 1 <= xo1) {
                            b0 = a.row_start[row + (uint32_t)(cx + rin + 1)];
                            lb = a.row_start[row + (uint32_t)xo1 + 1u] - b0;
                        }
                    }
                }
                const uint32_t len = la + lb;
                uint32_t incl = len;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(incl, d, 64); if (lane >= d) incl += o; }
                const uint32_t pre = incl - len, cand_total = __shfl(incl, 63, 64);
                for (uint32_t c0 = 0; c0 < cand_total; c0 += 64) {               // (wave-uniform)
                    const uint32_t idx = c0 + (uint32_t)lane;
                    int o = 0;                                                   // the last lane whose run starts at or before idx
#pragma unroll
                    for (int st = 32; st >= 1; st >>= 1) if (__shfl(pre, o + st, 64) <= idx) o += st;
                    const uint32_t off = idx - __shfl(pre, o, 64), la_o = __shfl(la, o, 64);
                    const uint32_t a0_o = __shfl(a0, o, 64), b0_o = __shfl(b0, o, 64);
                    u64 key = EMPTY;
                    if (idx < cand_total) {
                        const float4 p = a.sorted[off < la_o ? a0_o + off : b0_o + (off - la_o)];
                        key = make_key(flann_d2(q, f3(p.x, p.y, p.z)), __float_as_uint(p.w));
                    }
                    const u64 kth = __shfl(list, a.m - 1, 64);
                    if (__ballot(key < kth)) list = wave_merge(list, key, lane);
                }
            }
            const double reach = block_reach(a, q, cx, cy, cz, rout);
            if (reach == INFINITY) break;
            if (inside_reach(key_d(__shfl(list, a.m - 1, 64)), reach)) break;   // (EMPTY: NaN, not inside)
        }
        if (lane < a.m) s_list[wv][lane] = (uint32_t)list;
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) pca_store(a, &s_list[wv][0], 1, q, __float_as_uint(q4.w));
        __builtin_amdgcn_wave_barrier();
    }
}

// occ[0] += occupied cells (distinct sorted keys)
__global__ __launch_bounds__(256) void k_count_cells(const uint32_t *__restrict__ keys, uint32_t n, uint32_t *__restrict__ occ) {
    uint32_t c = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        c += (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(occ, c);
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
    for (hipEvent_t &e : W.ev) if (!e) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventRecord(W.ev[0], ctx->stream));
    TargetGrid &G = W.grid;
    const int m = (int)std::min<uint32_t>((uint32_t)k, n);
    // cell: a surface-like cloud spread over the faces of its box has r_k = sqrt(k A / (pi n)) (A = the box's area); the cell
    // is 1.5 r_k, so that an occupied cell holds ~0.7 k points, then adapted to the measured mean occupancy (clouds that are
    // lines, slabs or clumps)
    const double ex = std::max(1e-9, (double)bbmax[0] - bbmin[0]), ey = std::max(1e-9, (double)bbmax[1] - bbmin[1]),
                 ez = std::max(1e-9, (double)bbmax[2] - bbmin[2]);
    const double area = 2 * (ex * ey + ey * ez + ex * ez), target = 0.7 * k;
    float cell = (float)(1.5 * std::sqrt((double)k * area / (M_PI * (double)n)));
    if (!(cell > 0.f) || !std::isfinite(cell)) cell = 1.f;
    uint32_t *d_occ = W.count.ensure(4);   // [0]: the ring list's length, [1]: occupied cells
    W.builds = 0;
    for (int attempt = 0;; ++attempt) {
        G.build(ctx, d_xyz, n, stride, cell, bbmin, bbmax, true);
        ++W.builds;
        PLADE_REQUIRE(G.dense, PLADE_EINVAL, "estimate_normals: needs the dense row index (unset PLADE_OVERLAP_INDEX_COMPACT)");
        if (attempt == 3 || n <= (uint32_t)(4 * k)) break;
        ctx->fill_async(d_occ + 1, 0, 4);
        hipLaunchKernelGGL(k_count_cells, dim3(std::min(cdiv(n, 1024), 512u)), dim3(256), 0, ctx->stream, G.keys2.p, n, d_occ + 1);
        HIP_TRY(hipGetLastError());
        uint32_t occ = 0;
        ctx->d2h(&occ, d_occ + 1, 4);
        ctx->sync();
        const double mean = (double)n / std::max(occ, 1u);
        const float built = 1.f / G.gp.inv;          // build() enlarges the cell when the cell budget is hit
        if (mean > 2.0 * target && built <= cell * 1.01f) cell = built * (float)std::max(0.25, std::sqrt(target / mean));   // too coarse
        else if (mean < 0.5 * target && occ < n) cell = built * (float)std::min(4.0, std::sqrt(target / mean));          // too fine
        else break;
    }
    HIP_TRY(hipEventRecord(W.ev[1], ctx->stream));
    NrmArgs a;
    a.sorted = G.sorted.p; a.row_start = G.row_start.p; a.xyz = d_xyz; a.stride = stride; a.n = n; a.m = m; a.k = k;
    a.mnx = G.gp.mnx; a.mny = G.gp.mny; a.mnz = G.gp.mnz; a.inv = G.gp.inv;
    a.dx = G.gp.dx; a.dy = G.gp.dy; a.dz = G.gp.dz; a.DX = G.DX; a.DY = G.DY;
    a.mn[0] = G.gp.mnx; a.mn[1] = G.gp.mny; a.mn[2] = G.gp.mnz;
    a.cell = 1.0 / (double)G.gp.inv;
    // fp32 cell assignment: (x - mn) * inv is off by a few ulps of the coordinates; 1 % of a cell on top
    double amax = 0.0;
    for (int t = 0; t < 3; ++t) amax = std::max(amax, std::max(std::fabs((double)bbmin[t]), std::fabs((double)bbmax[t])));
    a.margin = 0.01 * a.cell + 1e-6 * amax;
    for (int t = 0; t < 3; ++t) a.view[t] = view[t];
    a.out = d_out; a.curv = d_curv; a.nbr = d_nbr;
    a.fail = W.fail.ensure(n); a.fail_count = d_occ;
    ctx->fill_async(d_occ, 0, 4);
    if (k <= 8) launch_search<8>(ctx, a);
    else if (k <= 16) launch_search<16>(ctx, a);
    else if (k <= 32) launch_search<32>(ctx, a);
    else launch_search<64>(ctx, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(W.ev[2], ctx->stream));
    ctx->d2h(&W.h_count, d_occ, 4);
}

void normals_stats(plade_ctx *ctx, NormalsWork &W) {
    float t01 = 0.f, t12 = 0.f;
    HIP_TRY(hipEventElapsedTime(&t01, W.ev[0], W.ev[1]));
    HIP_TRY(hipEventElapsedTime(&t12, W.ev[1], W.ev[2]));
    ctx->stats.clear();
    ctx->stats.add("normals_grid_s", 1e-3 * t01);
    ctx->stats.add("normals_search_s", 1e-3 * t12);
    ctx->stats.add("normals_grid_builds", W.builds);
    ctx->stats.add("normals_ring_queries", W.h_count);
}

}  // namespace plade

using namespace plade;

// ---- C ABI (include/plade_hip.h) ---------------------------------------------------------------------------------------------
namespace {
const float kOrigin[3] = {0.f, 0.f, 0.f};
// upload + bounding box (refuses non-finite coordinates) of a host xyz array into W.in
void normals_upload(plade_ctx *ctx, NormalsWork &W, const float *xyz, uint32_t n, uint32_t stride, float mn[3], float mx[3]) {
    W.in.ensure((size_t)n * stride + 4);
    HIP_TRY(hipMemcpyAsync(W.in.p, xyz, (size_t)n * stride * 4, hipMemcpyHostToDevice, ctx->stream));
    bbox_host(ctx, W.in.p, n, stride, mn, mx);
}
}  // namespace

extern "C" int plade_estimate_normals(plade_ctx *ctx, const float *xyz, uint32_t n, uint32_t stride, int32_t k,
                                      const float *viewpoint, float *pos_nrm_out, float *curvature_out, int32_t *nbr_out) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(xyz && pos_nrm_out, PLADE_EINVAL, "plade_estimate_normals: bad argument");
        const float *view = viewpoint ? viewpoint : kOrigin;
        normals_check_args(n, stride, k, view);
        if (!ctx->normals_work) ctx->normals_work = normals_work_create();
        NormalsWork &W = *ctx->normals_work;
        float mn[3], mx[3];
        normals_upload(ctx, W, xyz, n, stride, mn, mx);
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
        if (!ctx->normals_work) ctx->normals_work = normals_work_create();
        NormalsWork &W = *ctx->normals_work;
        float mn[3], mx[3];
        normals_upload(ctx, W, xyz, n, stride, mn, mx);
        plade_cloud *c = new plade_cloud;
        try {
            cloud_shape(c->dev, n);
            estimate_normals_dev(ctx, W, W.in.p, n, stride, mn, mx, k, view, c->dev.aos.p, nullptr, nullptr);
            ctx->sync();
            normals_stats(ctx, W);
            cloud_finish_device(ctx, c->dev);   // SoA planes + bounding box of the resident cloud, as plade_cloud_upload
        } catch (...) { delete c; throw; }
        *out = c;
        return PLADE_OK;
    });
}
