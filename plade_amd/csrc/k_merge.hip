// plade_amd/csrc/k_merge.hip -- merge registered clouds into one voxel-fused cloud (merge.h).
//
// (a) k_merge_transform  all k clouds in one pass: row (p, n) of cloud c -> (p', n') at its place in the concatenation, and the
//                        bounding box of all p' (which also refuses non-finite coordinates)
// (b) k_merge_keys       packed (k | j | i) voxel keys of p' -- 32 bits when they fit, 64 otherwise, as VoxelWork -- and the stable
//                        radix sort of (key, item)
// (c) k_merge_runs       ONE launch: run heads by a decoupled look-back scan (the scan of k_voxel_runs) and the gather of the six
//                        channels plus the item's cloud bit into sorted order.  The sort is stable, so sorted position = ascending
//                        (cloud, index) inside a voxel
// (d) k_merge_fuse       one lane per voxel adds its run in that order in fp64 from LDS-staged, coalesced chunks
// No floating-point atomics anywhere: the bits do not depend on the launch shape or the run.
#include "merge.h"
#include "cloud_tool.h"
#include "prims.h"
#include "voxel.h"

namespace plade {

struct MergeArgs {
    const float *rows[MERGE_MAX_CLOUDS];    // cloud c on the device: n_c x 6
    float T[MERGE_MAX_CLOUDS][12];          // rows 0..2 of its 4 x 4
    uint32_t start[MERGE_MAX_CLOUDS + 1];   // first item of cloud c in the concatenation; the entries behind k hold the total
    uint32_t total;
};

// the cloud of item v: its position among the <= 17 offsets
__device__ __forceinline__ uint32_t mg_cloud(const uint32_t *start, uint32_t v) {
    uint32_t c = 0;
#pragma unroll
    for (int q = 1; q < MERGE_MAX_CLOUDS; ++q) c += v >= start[q] ? 1u : 0u;
    return c;
}

// ---- (a) -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_merge_transform(const MergeArgs A, float *__restrict__ cat, int *__restrict__ out8) {
    // matrices, offsets and row pointers are looked up per lane: staged in LDS once per workgroup
    __shared__ float s_T[MERGE_MAX_CLOUDS][12];
    __shared__ uint32_t s_start[MERGE_MAX_CLOUDS + 1];
    __shared__ const float *s_rows[MERGE_MAX_CLOUDS];
    __shared__ float s_lds[6][8];
    for (int q = threadIdx.x; q < MERGE_MAX_CLOUDS * 12; q += blockDim.x) s_T[q / 12][q % 12] = A.T[q / 12][q % 12];
    if (threadIdx.x <= MERGE_MAX_CLOUDS) s_start[threadIdx.x] = A.start[threadIdx.x];
    if (threadIdx.x < MERGE_MAX_CLOUDS) s_rows[threadIdx.x] = A.rows[threadIdx.x];
    __syncthreads();
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool bad = false;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < A.total; i += gridDim.x * blockDim.x) {
        const uint32_t c = mg_cloud(s_start, i);
        const float2 *r = reinterpret_cast<const float2 *>(s_rows[c] + 6 * (size_t)(i - s_start[c]));
        const float2 a = r[0], b = r[1], d = r[2];
        const float x = a.x, y = a.y, z = b.x, nx = b.y, ny = d.x, nz = d.y;
        const float *T = s_T[c];
        float p[3], n[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p[k] = ((T[4 * k] * x + T[4 * k + 1] * y) + T[4 * k + 2] * z) + T[4 * k + 3];
            n[k] = (T[4 * k] * nx + T[4 * k + 1] * ny) + T[4 * k + 2] * nz;
            mn[k] = fminf(mn[k], p[k]);
            mx[k] = fmaxf(mx[k], p[k]);
        }
        // NaN or infinity, before or after the transform (fminf / fmaxf would hide a NaN)
        bad = bad || !(fabsf(x) <= FLT_MAX) || !(fabsf(y) <= FLT_MAX) || !(fabsf(z) <= FLT_MAX) || !(fabsf(p[0]) <= FLT_MAX) ||
              !(fabsf(p[1]) <= FLT_MAX) || !(fabsf(p[2]) <= FLT_MAX);
        float2 *o = reinterpret_cast<float2 *>(cat + 6 * (size_t)i);
        o[0] = make_float2(p[0], p[1]); o[1] = make_float2(p[2], n[0]); o[2] = make_float2(n[1], n[2]);
    }
    if (bad) out8[6] = 1;
    block_minmax_commit<3>(mn, mx, out8, s_lds);
}

// ---- (b) -----------------------------------------------------------------------------------------------------------------------
template <class K>
__global__ __launch_bounds__(256) void k_merge_keys(const float *__restrict__ cat, uint32_t n, float inv, int lminx, int lminy, int lminz,
                                                    int bx, int by, K *__restrict__ keys, uint32_t *__restrict__ vals) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float2 *r = reinterpret_cast<const float2 *>(cat + 6 * (size_t)i);
    const float2 a = r[0];
    const float z = cat[6 * (size_t)i + 2];
    // the key of k_voxel_keys: floor(x * inverse_leaf_size) in fp32, then the integer offset
    const uint64_t lx = (uint64_t)((int)floorf(a.x * inv) - lminx);
    const uint64_t ly = (uint64_t)((int)floorf(a.y * inv) - lminy);
    const uint64_t lz = (uint64_t)((int)floorf(z * inv) - lminz);
    keys[i] = (K)((lz << (bx + by)) | (ly << bx) | lx);
    vals[i] = i;
}

// ---- (c) -----------------------------------------------------------------------------------------------------------------------
// Tiles of 4096 sorted positions.  heads[s] = first sorted position of voxel s, *n_seg = their number; sorted[0..6) = the planes
// x | y | z | nx | ny | nz (pitch n) in sorted order, sbit = 1 << cloud of the item.
constexpr int MR_T = 256, MR_I = 16, MR_TILE = MR_T * MR_I;
constexpr uint64_t MR_AGG = 1ull << 32, MR_PREFIX = 2ull << 32, MR_STATUS = 3ull << 32;
template <class K>
__global__ __launch_bounds__(MR_T) void k_merge_runs(const K *__restrict__ keys, const uint32_t *__restrict__ vals, uint32_t n,
                                                      const float *__restrict__ cat, const MergeArgs A, uint64_t *__restrict__ state,
                                                      uint32_t *__restrict__ ticket, uint32_t base, uint32_t gen,
                                                      uint32_t *__restrict__ heads, uint32_t *__restrict__ n_seg,
                                                      float *__restrict__ sorted, uint32_t *__restrict__ sbit) {
    __shared__ uint32_t s_tile, s_w[MR_T / 64], s_excl, s_start[MERGE_MAX_CLOUDS + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_tile = atomicAdd(ticket, 1u) - base;
    if (tid <= MERGE_MAX_CLOUDS) s_start[tid] = A.start[tid];
    __syncthreads();
    const uint32_t tile = s_tile;
    const uint32_t first = tile * MR_TILE + tid * MR_I;
    K k[MR_I + 1];
    k[0] = (first > 0 && first <= n) ? keys[first - 1] : (K)~(K)0;
#pragma unroll
    for (int q = 0; q < MR_I; ++q) k[q + 1] = first + q < n ? keys[first + q] : (K)~(K)0;
    uint32_t fl = 0, sum = 0;
#pragma unroll
    for (int q = 0; q < MR_I; ++q) {
        const bool head = first + q < n && (first + q == 0 || k[q + 1] != k[q]);
        fl |= (head ? 1u : 0u) << q;
        sum += head;
    }
    uint32_t incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t agg = 0, woff = 0;
    for (int w = 0; w < MR_T / 64; ++w) { if (w < wave) woff += s_w[w]; agg += s_w[w]; }
    const uint64_t tag = (uint64_t)gen << 34;
    if (wave == 0) {
        if (lane == 0)
            __hip_atomic_store(state + tile, tag | (tile == 0 ? MR_PREFIX : MR_AGG) | agg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint32_t excl = 0;
        if (tile > 0) {
            int t = (int)tile - 1;
            for (;;) {
                const int idx = t - lane;
                uint64_t st = tag | MR_PREFIX;
                if (idx >= 0) st = __hip_atomic_load(state + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const bool ready = (st >> 34) == gen && (st & MR_STATUS) != 0ull;
                const unsigned long long not_ready = __ballot(!ready), is_prefix = __ballot(ready && (st & MR_PREFIX));
                const int first_bad = not_ready ? __ffsll((long long)not_ready) - 1 : 64;
                const int first_pre = is_prefix ? __ffsll((long long)is_prefix) - 1 : 64;
                const int take = first_pre < first_bad ? first_pre + 1 : first_bad;
                uint32_t part = lane < take ? (uint32_t)st : 0u;
                for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d, 64);
                excl += part;
                if (first_pre < first_bad) break;
                t -= take;
            }
            if (lane == 0)
                __hip_atomic_store(state + tile, tag | MR_PREFIX | (uint64_t)(excl + agg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (lane == 0) s_excl = excl;
    }
    __syncthreads();
    uint32_t rank = s_excl + woff + incl - sum;
#pragma unroll
    for (int q = 0; q < MR_I; ++q)
        if (fl & (1u << q)) heads[rank++] = first + q;
    if ((uint64_t)tile * MR_TILE + MR_TILE >= n && tid == MR_T - 1) *n_seg = s_excl + agg;   // the last tile
    // the gather: 24 B rows in, seven coalesced streams out
#pragma unroll 4
    for (int q = 0; q < MR_I; ++q) {
        const uint32_t j = tile * MR_TILE + q * MR_T + tid;
        if (j < n) {
            const uint32_t it = vals[j];
            const float2 *r = reinterpret_cast<const float2 *>(cat + 6 * (size_t)it);
            const float2 a = r[0], b = r[1], d = r[2];
            sorted[j] = a.x; sorted[(size_t)n + j] = a.y; sorted[2 * (size_t)n + j] = b.x;
            sorted[3 * (size_t)n + j] = b.y; sorted[4 * (size_t)n + j] = d.x; sorted[5 * (size_t)n + j] = d.y;
            sbit[j] = 1u << mg_cloud(s_start, it);
        }
    }
}

// ---- (d) -----------------------------------------------------------------------------------------------------------------------
// The 128 voxels of a workgroup own one contiguous span of the sorted points.  The span goes through LDS in chunks of 1024
// positions (7 x 4 KB = 28 KB per workgroup: five workgroups, ten wavefronts, per CU) with coalesced loads, and every lane adds,
// in ascending position, the part of its run that lies in the chunk -- a lane walking its run in global memory would touch 64
// lines per wavefront load.  summary[0] += rows seen by two or more clouds, summary[1] = max(count): integer atomics.
constexpr uint32_t MF_T = 128, MF_CH = 1024;
__global__ __launch_bounds__(MF_T) void k_merge_fuse(const float *__restrict__ sorted, const uint32_t *__restrict__ sbit,
                                                     const uint32_t *__restrict__ heads, const uint32_t *__restrict__ n_seg_p,
                                                     uint32_t n_items, float *__restrict__ out_rows, uint32_t *__restrict__ out_count,
                                                     uint32_t *__restrict__ out_mask, uint32_t *__restrict__ summary) {
    __shared__ float s_c[6][MF_CH];
    __shared__ uint32_t s_b[MF_CH];
    __shared__ uint32_t s_span[2];
    const uint32_t n_seg = *n_seg_p;
    const uint32_t s0 = blockIdx.x * MF_T;
    if (s0 >= n_seg) return;
    const uint32_t s = s0 + threadIdx.x;
    const bool live = s < n_seg;
    const uint32_t b = live ? heads[s] : 0u, e = live ? ((s + 1 < n_seg) ? heads[s + 1] : n_items) : 0u;
    if (threadIdx.x == 0) s_span[0] = b;
    if (s == min(n_seg, s0 + MF_T) - 1) s_span[1] = e;
    __syncthreads();
    const uint32_t span_b = s_span[0], span_e = s_span[1];
    double ap[3] = {0.0, 0.0, 0.0}, an[3] = {0.0, 0.0, 0.0};
    uint32_t n_fin = 0, mask = 0;
    for (uint32_t c0 = span_b; c0 < span_e; c0 += MF_CH) {
        const uint32_t c1 = min(span_e, c0 + MF_CH);
        for (uint32_t j = c0 + threadIdx.x; j < c1; j += MF_T) {
#pragma unroll
            for (int ch = 0; ch < 6; ++ch) s_c[ch][j - c0] = sorted[(size_t)ch * n_items + j];
            s_b[j - c0] = sbit[j];
        }
        __syncthreads();
        const uint32_t jb = max(b, c0), je = min(e, c1);
        for (uint32_t j = jb; j < je; ++j) {
            const uint32_t o = j - c0;
            ap[0] += (double)s_c[0][o]; ap[1] += (double)s_c[1][o]; ap[2] += (double)s_c[2][o];
            const float nx = s_c[3][o], ny = s_c[4][o], nz = s_c[5][o];
            if (fabsf(nx) <= FLT_MAX && fabsf(ny) <= FLT_MAX && fabsf(nz) <= FLT_MAX) {
                an[0] += (double)nx; an[1] += (double)ny; an[2] += (double)nz;
                ++n_fin;
            }
            mask |= s_b[o];
        }
        __syncthreads();
    }
    const uint32_t cnt = e - b;
    uint32_t shared = live && __popc(mask) >= 2 ? 1u : 0u, mx = cnt;
    for (int d = 32; d >= 1; d >>= 1) { shared += __shfl_xor(shared, d, 64); mx = max(mx, (uint32_t)__shfl_xor(mx, d, 64)); }
    if ((threadIdx.x & 63) == 0) {
        if (shared) atomicAdd(&summary[0], shared);
        if (mx > summary[1]) atomicMax(&summary[1], mx);
    }
    if (!live) return;
    const double dc = (double)cnt;
    const float px = (float)(ap[0] / dc), py = (float)(ap[1] / dc), pz = (float)(ap[2] / dc);
    const double q = (an[0] * an[0] + an[1] * an[1]) + an[2] * an[2];
    float nx = __int_as_float(0x7fc00000), ny = nx, nz = nx;
    if (n_fin != 0 && q != 0.0) {
        const double r = sqrt(q);
        nx = (float)(an[0] / r); ny = (float)(an[1] / r); nz = (float)(an[2] / r);
    }
    float2 *o = reinterpret_cast<float2 *>(out_rows + 6 * (size_t)s);
    o[0] = make_float2(px, py); o[1] = make_float2(pz, nx); o[2] = make_float2(ny, nz);
    out_count[s] = cnt;
    out_mask[s] = mask;
}

// --------------------------------------------------------------------------------------------------------------------------------
struct MergeWork {
    DBuf<float> in;                  // the host clouds, one behind the other
    DBuf<float> cat;                 // the transformed concatenation (total x 6)
    DBuf<uint64_t> keys, keys2;
    DBuf<uint32_t> vals, vals2, heads, count, sbit;   // count: [0] voxels, [1] n_shared, [2] max_count
    DBuf<float> sorted;              // six planes in voxel order
    DBuf<float> out_rows;
    DBuf<uint32_t> out_count, out_mask;
    EventSpans<5> spans;             // transform; with a leaf: sort, runs, fuse
    uint32_t h_count[4] = {0, 0, 0, 0};
};

namespace {

const float kIdentity[16] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};

// what can be refused before anything is queued; returns sum n_c
uint32_t check_args(uint32_t k, const void *const clouds[], const uint32_t n[], const float *const *T, float leaf) {
    PLADE_REQUIRE(k >= 1 && k <= (uint32_t)MERGE_MAX_CLOUDS, PLADE_EINVAL, "merge_clouds: 1 to 16 clouds");
    PLADE_REQUIRE(clouds && n, PLADE_EINVAL, "merge_clouds: NULL cloud table");
    PLADE_REQUIRE(std::isfinite(leaf) && leaf >= 0.f, PLADE_EINVAL, "merge_clouds: leaf must be finite and >= 0");
    uint64_t total = 0;
    for (uint32_t c = 0; c < k; ++c) {
        PLADE_REQUIRE(clouds[c], PLADE_EINVAL, "merge_clouds: NULL cloud");
        PLADE_REQUIRE(n[c] >= 1, PLADE_EINVAL, "merge_clouds: an empty cloud (n = 0)");
        total += n[c];
        if (T && T[c])
            for (int q = 0; q < 16; ++q) PLADE_REQUIRE(std::isfinite(T[c][q]), PLADE_EINVAL, "merge_clouds: non-finite transform");
    }
    PLADE_REQUIRE(total < (1ull << 31), PLADE_ELIMIT, "merge_clouds: 2^31 points or more");
    return (uint32_t)total;
}

// The merge of k device clouds (n_c x 6 rows each).  d_cat receives the transformed concatenation (total x 6): with leaf = 0 that
// is the result.  With leaf > 0 the fused rows, counts and masks are left in W.out_*; returns the number of output rows (waits).
uint32_t merge_dev(plade_ctx *ctx, MergeWork &W, uint32_t k, const float *const d_rows[], const uint32_t n[], const float *const *T,
                   float leaf, uint32_t total, float *d_cat, plade_merge_summary *summary) {
    MergeArgs A;
    memset(&A, 0, sizeof(A));
    for (uint32_t c = 0; c < (uint32_t)MERGE_MAX_CLOUDS; ++c) {
        const bool in = c < k;
        A.rows[c] = d_rows[in ? c : 0];
        memcpy(A.T[c], in && T && T[c] ? T[c] : kIdentity, sizeof(A.T[c]));
        A.start[c + 1] = in ? A.start[c] + n[c] : total;
    }
    A.total = total;
    int init[8], box[8];
    bbox_init_pattern(init);
    int *d_slot = reinterpret_cast<int *>(ctx->scratch[3].ensure(64));
    W.spans.mark(ctx, 0);
    ctx->h2d(d_slot, init, 32);
    hipLaunchKernelGGL(k_merge_transform, dim3(std::min(cdiv(total, 1024), 1024u)), dim3(256), 0, ctx->stream, A, d_cat, d_slot);
    HIP_TRY(hipGetLastError());
    ctx->d2h(box, d_slot, 32);
    W.spans.mark(ctx, 1);
    ctx->sync();
    float mn[3], mx[3];
    bbox_decode(box, mn, mx);   // (refuses non-finite coordinates)
    uint32_t n_out = total, n_shared = 0, max_count = 1;
    const bool fuse = leaf > 0.f;
    if (fuse) {
        const float inv = 1.f / leaf;
        int lmin[3], bits[3];
        for (int a = 0; a < 3; ++a) {
            const float lo = floorf(mn[a] * inv), hi = floorf(mx[a] * inv);
            PLADE_REQUIRE(std::isfinite(lo) && std::isfinite(hi) && fabsf(lo) < 1073741824.f && fabsf(hi) < 1073741824.f &&
                              (int64_t)hi - (int64_t)lo < (1 << 18),
                          PLADE_ELIMIT, "merge_clouds: more than 2^18 leaves along one axis");
            lmin[a] = (int)lo;
            int bb = 1;
            while (((int64_t)1 << bb) <= (int64_t)hi - (int64_t)lo) ++bb;
            bits[a] = bb;
        }
        const int key_bits = bits[0] + bits[1] + bits[2];
        const bool narrow = key_bits <= 31;   // (31: the all-ones padding key of k_merge_runs must not be a real key)
        W.keys.ensure(total); W.keys2.ensure(total); W.vals.ensure(total); W.vals2.ensure(total);
        W.heads.ensure((size_t)total + 1);
        W.count.ensure(4);
        W.sorted.ensure(6 * (size_t)total + 4);
        W.sbit.ensure(total);
        W.out_rows.ensure(6 * (size_t)total + 4);
        W.out_count.ensure(total);
        W.out_mask.ensure(total);
        uint32_t *k32 = reinterpret_cast<uint32_t *>(W.keys.p), *k32b = reinterpret_cast<uint32_t *>(W.keys2.p);
        ctx->fill_async(W.count.p, 0, 16);
        if (narrow) {
            hipLaunchKernelGGL(k_merge_keys<uint32_t>, dim3(cdiv(total, 256)), dim3(256), 0, ctx->stream, d_cat, total, inv, lmin[0], lmin[1],
                               lmin[2], bits[0], bits[1], k32, W.vals.p);
            sort_pairs_u32(ctx, k32, k32b, W.vals.p, W.vals2.p, total, key_bits);
        } else {
            hipLaunchKernelGGL(k_merge_keys<uint64_t>, dim3(cdiv(total, 256)), dim3(256), 0, ctx->stream, d_cat, total, inv, lmin[0], lmin[1],
                               lmin[2], bits[0], bits[1], W.keys.p, W.vals.p);
            sort_pairs_u64(ctx, W.keys.p, W.keys2.p, W.vals.p, W.vals2.p, total, key_bits);
        }
        W.spans.mark(ctx, 2);
        const ScanTicket t = scan_ticket(ctx, total, MR_TILE);
        if (narrow)
            hipLaunchKernelGGL(k_merge_runs<uint32_t>, dim3(t.tiles), dim3(MR_T), 0, ctx->stream, k32b, W.vals2.p, total, d_cat, A, t.state,
                               t.ticket, t.base, t.gen, W.heads.p, W.count.p, W.sorted.p, W.sbit.p);
        else
            hipLaunchKernelGGL(k_merge_runs<uint64_t>, dim3(t.tiles), dim3(MR_T), 0, ctx->stream, W.keys2.p, W.vals2.p, total, d_cat, A,
                               t.state, t.ticket, t.base, t.gen, W.heads.p, W.count.p, W.sorted.p, W.sbit.p);
        W.spans.mark(ctx, 3);
        hipLaunchKernelGGL(k_merge_fuse, dim3(cdiv(total, MF_T)), dim3(MF_T), 0, ctx->stream, W.sorted.p, W.sbit.p, W.heads.p, W.count.p,
                           total, W.out_rows.p, W.out_count.p, W.out_mask.p, W.count.p + 1);
        HIP_TRY(hipGetLastError());
        W.spans.mark(ctx, 4);
        ctx->d2h(W.h_count, W.count.p, 16);
        ctx->sync();
        n_out = W.h_count[0]; n_shared = W.h_count[1]; max_count = W.h_count[2];
    }
    if (summary) {
        summary->n_in = total;
        summary->n_out = n_out;
        summary->n_shared = n_shared;
        summary->max_count = max_count;
        summary->reserved = 0;
    }
    W.spans.collect(fuse ? 4 : 1);
    ctx->stats.clear();
    ctx->stats.add("merge_transform_s", W.spans.seconds(0));
    ctx->stats.add("merge_sort_s", W.spans.seconds(1));
    ctx->stats.add("merge_runs_s", W.spans.seconds(2));
    ctx->stats.add("merge_fuse_s", W.spans.seconds(3));
    ctx->stats.add("merge_rows", n_out);
    return n_out;
}

// count and mask of the unfused form: 1 and 1 << c
void fill_unfused(uint32_t k, const uint32_t n[], uint32_t *out_count, uint32_t *out_mask) {
    size_t o = 0;
    for (uint32_t c = 0; c < k; ++c)
        for (uint32_t i = 0; i < n[c]; ++i, ++o) {
            if (out_count) out_count[o] = 1u;
            if (out_mask) out_mask[o] = 1u << c;
        }
}

}  // namespace

uint32_t merge_fuse_one(plade_ctx *ctx, const float *d_rows, uint32_t n, float leaf, const float **d_out, const char *who) {
    const void *const clouds[1] = {d_rows};
    const uint32_t ns[1] = {n};
    const float *const rows[1] = {d_rows};
    try {
        // (a leaf that rounds to 0 in fp32 would select the concatenation: there would be no fused rows to hand out)
        PLADE_REQUIRE(leaf > 0.f, PLADE_EINVAL, "merge_clouds: the leaf is 0 in fp32");
        const uint32_t total = check_args(1, clouds, ns, nullptr, leaf);
        MergeWork &W = work_in<MergeWork>(ctx->merge_work);
        const uint32_t m = merge_dev(ctx, W, 1, rows, ns, nullptr, leaf, total, W.cat.ensure(6 * (size_t)total + 8), nullptr);
        *d_out = W.out_rows.p;
        return m;
    } catch (Err &e) {   // the merge's refusals, under the caller's name
        const std::string own = "merge_clouds: ";
        e.msg = std::string(who) + ": the sample: " + (e.msg.compare(0, own.size(), own) == 0 ? e.msg.substr(own.size()) : e.msg);
        throw;
    }
}

}  // namespace plade

using namespace plade;

// ---- C ABI (include/plade_hip.h) -----------------------------------------------------------------------------------------------
extern "C" int plade_merge_clouds(plade_ctx *ctx, uint32_t k, const float *const *clouds, const uint32_t *n, const float *T, float leaf,
                                  float *out_rows, uint32_t *out_count, uint32_t *out_mask, plade_merge_summary *summary) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(out_rows, PLADE_EINVAL, "plade_merge_clouds: NULL output");
        const float *Tc[MERGE_MAX_CLOUDS] = {};
        for (uint32_t c = 0; c < k && c < (uint32_t)MERGE_MAX_CLOUDS; ++c) Tc[c] = T ? T + 16 * (size_t)c : nullptr;
        const uint32_t total = check_args(k, reinterpret_cast<const void *const *>(clouds), n, Tc, leaf);
        MergeWork &W = work_in<MergeWork>(ctx->merge_work);
        W.in.ensure(6 * (size_t)total + 8);
        W.cat.ensure(6 * (size_t)total + 8);
        const float *d_rows[MERGE_MAX_CLOUDS];
        size_t o = 0;
        for (uint32_t c = 0; c < k; ++c) {   // the copies first, the host waits, then the kernels (cloud.hip)
            d_rows[c] = W.in.p + 6 * o;
            HIP_TRY(hipMemcpyAsync(W.in.p + 6 * o, clouds[c], (size_t)n[c] * 24, hipMemcpyHostToDevice, ctx->stream));
            o += n[c];
        }
        ctx->sync();
        const uint32_t m = merge_dev(ctx, W, k, d_rows, n, Tc, leaf, total, W.cat.p, summary);
        if (leaf > 0.f) {
            HIP_TRY(hipMemcpyAsync(out_rows, W.out_rows.p, (size_t)m * 24, hipMemcpyDeviceToHost, ctx->stream));
            if (out_count) HIP_TRY(hipMemcpyAsync(out_count, W.out_count.p, (size_t)m * 4, hipMemcpyDeviceToHost, ctx->stream));
            if (out_mask) HIP_TRY(hipMemcpyAsync(out_mask, W.out_mask.p, (size_t)m * 4, hipMemcpyDeviceToHost, ctx->stream));
        } else {
            HIP_TRY(hipMemcpyAsync(out_rows, W.cat.p, (size_t)m * 24, hipMemcpyDeviceToHost, ctx->stream));
            fill_unfused(k, n, out_count, out_mask);
        }
        ctx->sync();
        return PLADE_OK;
    });
}

extern "C" int plade_merge_clouds_dev(plade_ctx *ctx, uint32_t k, plade_cloud *const *clouds, const float *T, float leaf, plade_cloud **out,
                                      uint32_t *out_count, uint32_t *out_mask, plade_merge_summary *summary) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(out, PLADE_EINVAL, "plade_merge_clouds_dev: NULL output");
        *out = nullptr;
        const float *Tc[MERGE_MAX_CLOUDS] = {};
        uint32_t n[MERGE_MAX_CLOUDS] = {};
        const float *d_rows[MERGE_MAX_CLOUDS] = {};
        for (uint32_t c = 0; c < k && c < (uint32_t)MERGE_MAX_CLOUDS; ++c) {
            Tc[c] = T ? T + 16 * (size_t)c : nullptr;
            if (clouds && clouds[c]) { n[c] = clouds[c]->dev.n; d_rows[c] = clouds[c]->dev.aos.p; }
        }
        const uint32_t total = check_args(k, reinterpret_cast<const void *const *>(clouds), n, Tc, leaf);
        MergeWork &W = work_in<MergeWork>(ctx->merge_work);
        resident_result(ctx, out, [&](CloudDev &r) {
            const bool fuse = leaf > 0.f;
            float *d_cat;
            if (fuse) d_cat = W.cat.ensure(6 * (size_t)total + 8);
            else { cloud_shape(r, total); d_cat = r.aos.p; }
            const uint32_t m = merge_dev(ctx, W, k, d_rows, n, Tc, leaf, total, d_cat, summary);
            if (fuse) {
                cloud_shape(r, m);
                ctx->copy_dd_async(r.aos.p, W.out_rows.p, (size_t)m * 24);
                if (out_count) HIP_TRY(hipMemcpyAsync(out_count, W.out_count.p, (size_t)m * 4, hipMemcpyDeviceToHost, ctx->stream));
                if (out_mask) HIP_TRY(hipMemcpyAsync(out_mask, W.out_mask.p, (size_t)m * 4, hipMemcpyDeviceToHost, ctx->stream));
                ctx->sync();
            } else fill_unfused(k, n, out_count, out_mask);
        });
        return PLADE_OK;
    });
}

extern "C" int plade_cloud_download(plade_ctx *ctx, const plade_cloud *cloud, float *rows, uint32_t capacity_rows, uint32_t *n_out) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(cloud && n_out, PLADE_EINVAL, "plade_cloud_download: NULL argument");
        *n_out = cloud->dev.n;
        if (!rows) return PLADE_OK;
        PLADE_REQUIRE(capacity_rows >= cloud->dev.n, PLADE_ECAP, "plade_cloud_download: the buffer holds fewer rows than the cloud");
        if (cloud->dev.n) HIP_TRY(hipMemcpyAsync(rows, cloud->dev.aos.p, (size_t)cloud->dev.n * 24, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        return PLADE_OK;
    });
}
