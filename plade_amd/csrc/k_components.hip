// plade_amd/csrc/k_components.hip -- connected components of the radius graph on gfx950 (semantics: components.h).
//
// Layout
//   grid     the dense row index of TargetGrid with the radius filter's cell, radius_cell(r) of grid_walk.h (the rule of DESIGN.md
//            section 10): the 27-cell block around a point holds everything closer than r.
//   link     k_cc_link: one lane per point in the grid's sorted order walks the nine runs of its block and tests only the
//            candidates at a smaller sorted position, so every undirected edge is tested once.  An edge unites the two original
//            indices in parent[] by the lock-free min-hooking of cluster_tail.h (unite): no lane waits for another, and at the end
//            every root is the smallest original index of its component -- whatever the order of the unions.
// The tail (cluster_label_select of cluster_tail.h, which k_dbscan.hip runs too; its kernels are here, once):
//   flatten  k_cc_flatten (next launch): root[i] by walking up, flags[i] = (root[i] == i).  compact_flags over the flags gives C and,
//            by its exclusive positions, the id of every root: ascending root = ascending smallest index.
//   label    k_cc_label_size: label[i] = id[root[i]]; the sizes by integer atomics, one per distinct id of a wavefront.
//   select   k_cc_pass; with keep_largest the keys ~size << 32 | id (all ones in the high word: does not pass) through the stable
//            sort_pairs_u64 and k_cc_mark_first; k_cc_summary (largest, kept components); k_cc_keep, compact_flags, gather_rows (prims.h).
// For DBSCAN a point may have no root (noise: NO_POINT, label -1); the components never meet that case.
#include "components.h"
#include "cluster_tail.h"
#include "grid_walk.h"
#include "voxel.h"

namespace plade {

namespace {

constexpr int LINK_TPB = 256, ROW_TPB = 256;
constexpr uint32_t NO_PASS = 0xffffffffu;   // high word of a sort key: the component does not pass

struct LinkArgs {
    GridView g;
    uint32_t n;
    float r2;                        // (float)r * (float)r
    uint32_t *parent;                // by original index
};

__global__ __launch_bounds__(ROW_TPB) void k_cc_init(uint32_t *__restrict__ parent, uint32_t n) {
    const uint32_t i = blockIdx.x * ROW_TPB + threadIdx.x;
    if (i < n) parent[i] = i;
}

__global__ __launch_bounds__(LINK_TPB) void k_cc_link(const LinkArgs a) {
    const uint32_t s = blockIdx.x * LINK_TPB + threadIdx.x;
    if (s >= a.n) return;
    const float4 q4 = a.g.sorted[s];
    const f3 q(q4.x, q4.y, q4.z);
    const uint32_t self = __float_as_uint(q4.w);
    int cx, cy, cz;
    cell_of(a.g, q, cx, cy, cz);
    for_block27(a.g, cx, cy, cz, [&](uint32_t j0, uint32_t j1) {
        j1 = min(j1, s);             // the sorted positions below this lane's own (runs of later rows are empty)
        for (uint32_t j = j0; j < j1; ++j) {
            const float4 p = a.g.sorted[j];
            if (flann_d2(q, f3(p.x, p.y, p.z)) < a.r2) {
                const uint32_t other = __float_as_uint(p.w);
                const uint32_t pa = parent_of(a.parent, self), pb = parent_of(a.parent, other);
                if (pa != pb) unite(a.parent, pa, pb);   // (the same parent: already in one tree)
            }
        }
    });
}

// root[i] by walking up from i, or from attach[i] where that is given (NO_POINT: no root); flags[i] = i is a root
__global__ __launch_bounds__(ROW_TPB) void k_cc_flatten(const uint32_t *__restrict__ parent, const uint32_t *__restrict__ attach, uint32_t n,
                                                        uint32_t *__restrict__ root, uint32_t *__restrict__ flags) {
    const uint32_t i = blockIdx.x * ROW_TPB + threadIdx.x;
    if (i >= n) return;
    uint32_t x = attach ? attach[i] : i;
    if (x != NO_POINT)
        for (uint32_t p = parent[x]; p != x; p = parent[x]) x = p;
    root[i] = x;
    flags[i] = x == i ? 1u : 0u;
}

// label[i] = id[root[i]]; size[id] += 1, one atomic per distinct id of the wavefront (a room-sized component would otherwise put
// every point's atomic on one address).  Integer sums: the same in any order.  A point without a root: label -1, in no size
__global__ __launch_bounds__(ROW_TPB) void k_cc_label_size(const uint32_t *__restrict__ root, const uint32_t *__restrict__ id, uint32_t n,
                                                           int32_t *__restrict__ label, uint32_t *__restrict__ size) {
    const uint32_t i = blockIdx.x * ROW_TPB + threadIdx.x, lane = threadIdx.x & 63u;
    bool valid = i < n;
    uint32_t c = 0;
    if (valid) {
        const uint32_t r = root[i];
        valid = r != NO_POINT;
        c = valid ? id[r] : NO_POINT;
        label[i] = (int32_t)c;
    }
    u64 todo = __ballot(valid);
    while (todo) {                   // (wave-uniform)
        const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
        const uint32_t lc = (uint32_t)__builtin_amdgcn_readlane((int)c, (int)leader);
        const u64 same = __ballot(valid && c == lc);
        if (lane == leader) atomicAdd(size + lc, (uint32_t)__popcll(same));
        todo &= ~same;
    }
}

// kept[c] = passes (keep_largest = 0), or the sort key of c: ~size << 32 | c when it passes, NO_PASS << 32 | c when not
__global__ __launch_bounds__(ROW_TPB) void k_cc_pass(const uint32_t *__restrict__ size, uint32_t C, uint32_t min_size, uint32_t max_size,
                                                     uint8_t *__restrict__ kept, u64 *__restrict__ key, uint32_t *__restrict__ val) {
    const uint32_t c = blockIdx.x * ROW_TPB + threadIdx.x;
    if (c >= C) return;
    const uint32_t sz = size[c];
    const bool pass = sz >= min_size && (max_size == 0u || sz <= max_size);
    if (key) {
        key[c] = ((u64)(pass ? ~sz : NO_PASS) << 32) | (u64)c;   // (sz >= 1: ~sz < NO_PASS)
        val[c] = c;
        kept[c] = 0;
    } else
        kept[c] = pass ? 1 : 0;
}

// the first m entries of the sorted keys that pass
__global__ __launch_bounds__(ROW_TPB) void k_cc_mark_first(const u64 *__restrict__ key, const uint32_t *__restrict__ val, uint32_t C, uint32_t m,
                                                           uint8_t *__restrict__ kept) {
    const uint32_t t = blockIdx.x * ROW_TPB + threadIdx.x;
    if (t >= C || t >= m) return;
    if ((uint32_t)(key[t] >> 32) != NO_PASS) kept[val[t]] = 1;
}

// out[0] = the largest size, out[1] = the number of kept components (integer atomics, one pair per wavefront)
__global__ __launch_bounds__(ROW_TPB) void k_cc_summary(const uint32_t *__restrict__ size, const uint8_t *__restrict__ kept, uint32_t C,
                                                        uint32_t *__restrict__ out) {
    const uint32_t c = blockIdx.x * ROW_TPB + threadIdx.x;
    uint32_t big = c < C ? size[c] : 0u;
    const u64 k = __ballot(c < C && kept[c]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) big = max(big, (uint32_t)__shfl_xor((int)big, o, 64));
    if ((threadIdx.x & 63u) == 0) {
        atomicMax(out, big);
        if (k) atomicAdd(out + 1, (uint32_t)__popcll(k));
    }
}

__global__ __launch_bounds__(ROW_TPB) void k_cc_keep(const int32_t *__restrict__ label, const uint8_t *__restrict__ kept, uint32_t n,
                                                     uint8_t *__restrict__ keep, uint32_t *__restrict__ flags) {
    const uint32_t i = blockIdx.x * ROW_TPB + threadIdx.x;
    if (i >= n) return;
    const int32_t c = label[i];
    const uint32_t k = c >= 0 && kept[c] ? 1u : 0u;
    keep[i] = (uint8_t)k;
    flags[i] = k;
}

}  // namespace

struct ComponentWork : ClusterWork {
    TargetGrid grid;
    DBuf<uint32_t> parent;
    EventSpans<5> spans;             // grid, link, label, compact
};

void cluster_init_parents(plade_ctx *ctx, uint32_t *d_parent, uint32_t n) {
    hipLaunchKernelGGL(k_cc_init, dim3(cdiv(n, ROW_TPB)), dim3(ROW_TPB), 0, ctx->stream, d_parent, n);
}

void cluster_label_select(plade_ctx *ctx, ClusterWork &W, uint32_t n, const uint32_t *d_parent, const uint32_t *d_attach, uint32_t min_size,
                          uint32_t max_size, uint32_t keep_largest) {
    uint32_t *d_root = W.root.ensure(n), *d_size = W.size.ensure(n), *d_cnt = W.count.ensure(4);
    int32_t *d_label = W.label.ensure(n);
    uint8_t *d_keep = W.keep.ensure((size_t)n + 4), *d_ckept = W.cluster_kept.ensure((size_t)n + 4);
    uint32_t *d_flags = keep_flags(ctx, W, n);   // first the roots' flags, then the kept points'
    ctx->fill_async(d_size, 0, (size_t)n * 4);
    ctx->fill_async(d_cnt, 0, 16);
    hipLaunchKernelGGL(k_cc_flatten, dim3(cdiv(n, ROW_TPB)), dim3(ROW_TPB), 0, ctx->stream, d_parent, d_attach, n, d_root, d_flags);
    HIP_TRY(hipGetLastError());
    const uint32_t C = compact_flags(ctx, d_flags, n, W.root_pos, W.root_list);   // (waits for the count)
    W.clusters = C;
    hipLaunchKernelGGL(k_cc_label_size, dim3(cdiv(n, ROW_TPB)), dim3(ROW_TPB), 0, ctx->stream, d_root, W.root_pos.p, n, d_label, d_size);
    const dim3 cgrid(cdiv(C, ROW_TPB));
    if (C == 0) {
        // (DBSCAN with every point noise: nothing to select, d_cnt stays 0)
    } else if (keep_largest > 0) {
        unsigned long long *d_key = W.sort_key.ensure(C), *d_key2 = W.sort_key2.ensure(C);
        uint32_t *d_val = W.sort_val.ensure(C), *d_val2 = W.sort_val2.ensure(C);
        hipLaunchKernelGGL(k_cc_pass, cgrid, dim3(ROW_TPB), 0, ctx->stream, d_size, C, min_size, max_size, d_ckept, d_key, d_val);
        HIP_TRY(hipGetLastError());
        sort_pairs_u64(ctx, reinterpret_cast<const uint64_t *>(d_key), reinterpret_cast<uint64_t *>(d_key2), d_val, d_val2, C, 64);
        hipLaunchKernelGGL(k_cc_mark_first, cgrid, dim3(ROW_TPB), 0, ctx->stream, d_key2, d_val2, C, keep_largest, d_ckept);
    } else
        hipLaunchKernelGGL(k_cc_pass, cgrid, dim3(ROW_TPB), 0, ctx->stream, d_size, C, min_size, max_size, d_ckept, (u64 *)nullptr,
                           (uint32_t *)nullptr);
    if (C) hipLaunchKernelGGL(k_cc_summary, cgrid, dim3(ROW_TPB), 0, ctx->stream, d_size, d_ckept, C, d_cnt);
    hipLaunchKernelGGL(k_cc_keep, dim3(cdiv(n, ROW_TPB)), dim3(ROW_TPB), 0, ctx->stream, d_label, d_ckept, n, d_keep, d_flags);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(W.h_count, d_cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
}

namespace {

void check_params(uint32_t n, uint32_t stride, const plade_component_params &p) {
    PLADE_REQUIRE(n >= 1, PLADE_EINVAL, "label_components: the cloud is empty (n = 0)");
    PLADE_REQUIRE(stride >= 3, PLADE_EINVAL, "label_components: stride must be >= 3 floats");
    PLADE_REQUIRE(radius_ok(p.radius, false), PLADE_EINVAL, "label_components: radius must be finite and > 0");
    PLADE_REQUIRE(p.min_size >= 1, PLADE_EINVAL, "label_components: min_size must be >= 1");
    PLADE_REQUIRE(p.max_size == 0 || p.max_size >= p.min_size, PLADE_EINVAL, "label_components: max_size must be 0 (no bound) or >= min_size");
    PLADE_REQUIRE(p.keep_largest >= 0, PLADE_EINVAL, "label_components: keep_largest must be >= 0");
}

// The components of a device cloud of `stride` floats per point with a known bounding box.  Leaves label, size, keep and the kept
// list in W, gathers the kept rows into dst(kept) -- not called when nothing is kept --, waits, fills the summary and the stats.
// Returns the number of kept points.
uint32_t components_dev(plade_ctx *ctx, ComponentWork &W, const float *d_rows, uint32_t n, uint32_t stride, const float bbmin[3],
                        const float bbmax[3], const plade_component_params &p, const KeepRows &dst,
                        plade_component_summary *summary) {
    W.spans.mark(ctx, 0);
    TargetGrid &G = W.grid;
    const float r = (float)p.radius;
    G.build(ctx, d_rows, n, stride, radius_cell((double)r, bbmin, bbmax), bbmin, bbmax, true);
    W.spans.mark(ctx, 1);

    LinkArgs a;
    memset(&a, 0, sizeof(a));
    a.g = view_of(G, "label_components");
    a.n = n; a.r2 = r * r;
    a.parent = W.parent.ensure(n);
    cluster_init_parents(ctx, a.parent, n);
    hipLaunchKernelGGL(k_cc_link, dim3(cdiv(n, LINK_TPB)), dim3(LINK_TPB), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    W.spans.mark(ctx, 2);

    cluster_label_select(ctx, W, n, a.parent, nullptr, (uint32_t)p.min_size, (uint32_t)p.max_size, (uint32_t)p.keep_largest);
    const uint32_t C = W.clusters;
    W.spans.mark(ctx, 3);

    const uint32_t total = keep_compact_gather(ctx, W, d_rows, n, stride, dst);
    W.spans.mark(ctx, 4);
    ctx->sync();
    if (summary) {
        summary->n = n;
        summary->components = C;
        summary->kept_components = W.h_count[1];
        summary->kept = total;
        summary->largest = W.h_count[0];
        summary->reserved = 0;
    }
    W.spans.collect();
    ctx->stats.clear();
    ctx->stats.add("components_grid_s", W.spans.seconds(0));
    ctx->stats.add("components_link_s", W.spans.seconds(1));
    ctx->stats.add("components_label_s", W.spans.seconds(2));
    ctx->stats.add("components_compact_s", W.spans.seconds(3));
    ctx->stats.add("components_count", C);
    ctx->stats.add("components_kept", total);
    grid_stats(ctx, "components", W.grid);
    return total;
}

}  // namespace
}  // namespace plade

using namespace plade;

// ---- C ABI (include/plade_hip.h) ---------------------------------------------------------------------------------------------
extern "C" void plade_component_default_params(plade_component_params *p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->radius = 0.0;
    p->min_size = 1;
    p->max_size = 0;
    p->keep_largest = 0;
}

extern "C" int plade_label_components(plade_ctx *ctx, const float *rows, uint32_t n, uint32_t stride, const plade_component_params *params,
                                      int32_t *label_out, uint32_t *size_out, uint8_t *keep_out, uint32_t *kept_index_out,
                                      float *rows_out, plade_component_summary *summary) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(rows, PLADE_EINVAL, "plade_label_components: NULL cloud");
        const plade_component_params p = params_or_default(params, plade_component_default_params);
        check_params(n, stride, p);
        ComponentWork &W = work_in<ComponentWork>(ctx->component_work);
        float mn[3], mx[3];
        upload_rows(ctx, W.in, rows, n, stride, mn, mx);
        const uint32_t total = components_dev(ctx, W, W.in.p, n, stride, mn, mx, p, keep_rows_host(W, stride), summary);
        if (label_out) HIP_TRY(hipMemcpyAsync(label_out, W.label.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (size_out) HIP_TRY(hipMemcpyAsync(size_out, W.size.p, (size_t)W.clusters * 4, hipMemcpyDeviceToHost, ctx->stream));
        keep_copy_out(ctx, W, n, total, stride, keep_out, kept_index_out, rows_out);
        ctx->sync();
        return PLADE_OK;
    });
}

extern "C" int plade_cloud_filter_components_dev(plade_ctx *ctx, plade_cloud *cloud, const plade_component_params *params, plade_cloud **out,
                                                 int32_t *label_out, uint32_t *kept_index_out, plade_component_summary *summary) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(cloud && out, PLADE_EINVAL, "plade_cloud_filter_components_dev: NULL cloud");
        *out = nullptr;
        const plade_component_params p = params_or_default(params, plade_component_default_params);
        const CloudDev &in = cloud->dev;
        check_params(in.n, 6, p);
        ComponentWork &W = work_in<ComponentWork>(ctx->component_work);
        resident_result(ctx, out, [&](CloudDev &c) {
            const uint32_t total = components_dev(ctx, W, in.aos.p, in.n, 6, in.bbmin, in.bbmax, p, keep_rows_cloud(c), summary);
            if (label_out) HIP_TRY(hipMemcpyAsync(label_out, W.label.p, (size_t)in.n * 4, hipMemcpyDeviceToHost, ctx->stream));
            keep_copy_out(ctx, W, in.n, total, 6, nullptr, kept_index_out, nullptr);
            ctx->sync();
            require_kept(total, "plade_cloud_filter_components_dev: the selection");
        });
        return PLADE_OK;
    });
}
