// plade_amd/csrc/k_dbscan.hip -- DBSCAN on gfx950 (semantics: dbscan.h).
//
// Layout
//   grid     the dense row index of TargetGrid at radius_cell(r) of grid_walk.h, as for the components: the 27-cell block around
//            a point holds everything closer than r.  Built once, walked twice.
//   core     k_db_core: one lane per point in the grid's sorted order counts the candidates of its block with d < r2 (itself
//            among them), the whole block.  The core flags go out BY SORTED POSITION, one __ballot word per
//            wavefront: the second walk reads one bit per candidate next to the float4 it loads anyway, not a byte gathered by
//            original index.  kind[] (0 / 2) by original index; the core points counted, one atomic per wavefront.
//   link     k_db_link: a core lane tests only the core candidates at a smaller sorted position -- every core-core edge once -- and
//            unites the two original indices (unite of cluster_tail.h).  A non-core lane walks its whole block, keeps the smallest
//            make_key(d, j) over its core candidates in one u64 register and writes attach[i] = that j (NO_POINT: noise),
//            kind[i] = 1.  A core point is attached to itself.  No LDS; nobody waits for anybody.
//   tail     cluster_label_select of cluster_tail.h (the components' kernels, with attach[]): flatten, ids, labels, sizes, the
//            selection; then the keep tail of cloud_tool.h.
#include "dbscan.h"
#include "cluster_tail.h"
#include "grid_walk.h"
#include "voxel.h"

namespace plade {

namespace {

constexpr int WALK_TPB = 256;

struct WalkArgs {
    GridView g;
    uint32_t n;
    float r2;                        // (float)r * (float)r
    uint32_t min_points;
    u64 *core_bits;                  // bit s & 63 of word s >> 6: the point at sorted position s is core (cdiv(n, 64) words)
    uint8_t *kind;                   // by original index
    uint32_t *parent, *attach;       // by original index
    uint32_t *counts;                // [0] core points, [1] border points
};

__global__ __launch_bounds__(WALK_TPB) void k_db_core(const WalkArgs a) {
    const uint32_t s = blockIdx.x * WALK_TPB + threadIdx.x;
    bool core = false;
    if (s < a.n) {
        const float4 q4 = a.g.sorted[s];
        const f3 q(q4.x, q4.y, q4.z);
        int cx, cy, cz;
        cell_of(a.g, q, cx, cy, cz);
        uint32_t count = 0;
        // (no exit at min_points: measured, the spans cannot tell the two forms apart -- DESIGN.md section 30)
        for_block27(a.g, cx, cy, cz, [&](uint32_t j0, uint32_t j1) {
            for (uint32_t j = j0; j < j1; ++j) {
                const float4 p = a.g.sorted[j];
                count += flann_d2(q, f3(p.x, p.y, p.z)) < a.r2 ? 1u : 0u;
            }
        });
        core = count >= a.min_points;
        a.kind[__float_as_uint(q4.w)] = core ? 2 : 0;
    }
    // (all 64 lanes: the lanes past n of the last wavefront vote 0)
    const u64 word = __ballot(core);
    if ((threadIdx.x & 63u) == 0 && s < a.n) {
        a.core_bits[s >> 6] = word;
        if (word) atomicAdd(a.counts, (uint32_t)__popcll(word));
    }
}

// the core bit of sorted position j; w / wi: the word read last and its index
__device__ __forceinline__ bool core_at(const u64 *__restrict__ bits, uint32_t j, u64 &w, uint32_t &wi) {
    if ((j >> 6) != wi) {
        wi = j >> 6;
        w = bits[wi];
    }
    return (w >> (j & 63u)) & 1ull;
}

__global__ __launch_bounds__(WALK_TPB) void k_db_link(const WalkArgs a) {
    const uint32_t s = blockIdx.x * WALK_TPB + threadIdx.x;
    bool border = false;
    if (s < a.n) {
        const float4 q4 = a.g.sorted[s];
        const f3 q(q4.x, q4.y, q4.z);
        const uint32_t self = __float_as_uint(q4.w);
        int cx, cy, cz;
        cell_of(a.g, q, cx, cy, cz);
        u64 w = a.core_bits[s >> 6];
        uint32_t wi = s >> 6;
        if ((w >> (s & 63u)) & 1ull) {
            for_block27(a.g, cx, cy, cz, [&](uint32_t j0, uint32_t j1) {
                j1 = min(j1, s);     // the sorted positions below this lane's own (runs of later rows are empty)
                for (uint32_t j = j0; j < j1; ++j) {
                    if (!core_at(a.core_bits, j, w, wi)) continue;
                    const float4 p = a.g.sorted[j];
                    if (flann_d2(q, f3(p.x, p.y, p.z)) < a.r2) {
                        const uint32_t other = __float_as_uint(p.w);
                        const uint32_t pa = parent_of(a.parent, self), pb = parent_of(a.parent, other);
                        if (pa != pb) unite(a.parent, pa, pb);   // (the same parent: already in one tree)
                    }
                }
            });
            a.attach[self] = self;
        } else {
            u64 best = EMPTY;
            for_block27(a.g, cx, cy, cz, [&](uint32_t j0, uint32_t j1) {
                for (uint32_t j = j0; j < j1; ++j) {
                    if (!core_at(a.core_bits, j, w, wi)) continue;
                    const float4 p = a.g.sorted[j];
                    const float d = flann_d2(q, f3(p.x, p.y, p.z));
                    if (d < a.r2) {
                        const u64 key = make_key(d, __float_as_uint(p.w));
                        best = key < best ? key : best;
                    }
                }
            });
            border = best != EMPTY;
            a.attach[self] = border ? (uint32_t)best : NO_POINT;
            if (border) a.kind[self] = 1;
        }
    }
    const u64 word = __ballot(border);
    if ((threadIdx.x & 63u) == 0 && word) atomicAdd(a.counts + 1, (uint32_t)__popcll(word));
}

}  // namespace

struct DbscanWork : ClusterWork {
    TargetGrid grid;
    DBuf<uint32_t> parent, attach, counts;
    DBuf<unsigned long long> core_bits;
    DBuf<uint8_t> kind;
    EventSpans<6> spans;             // grid, core, link, label, compact
    uint32_t h_counts[2] = {0, 0};   // core, border
};

namespace {

void check_params(uint32_t n, uint32_t stride, const plade_dbscan_params &p) {
    PLADE_REQUIRE(n >= 1, PLADE_EINVAL, "cluster_dbscan: the cloud is empty (n = 0)");
    PLADE_REQUIRE(stride >= 3, PLADE_EINVAL, "cluster_dbscan: stride must be >= 3 floats");
    PLADE_REQUIRE(radius_ok(p.radius, true), PLADE_EINVAL,
                  "cluster_dbscan: radius must be finite and > 0, its fp32 square finite and not below FLT_MIN");
    PLADE_REQUIRE(p.min_points >= 1, PLADE_EINVAL, "cluster_dbscan: min_points must be >= 1");
    PLADE_REQUIRE(p.min_size >= 1, PLADE_EINVAL, "cluster_dbscan: min_size must be >= 1");
    PLADE_REQUIRE(p.max_size == 0 || p.max_size >= p.min_size, PLADE_EINVAL, "cluster_dbscan: max_size must be 0 (no bound) or >= min_size");
    PLADE_REQUIRE(p.keep_largest >= 0, PLADE_EINVAL, "cluster_dbscan: keep_largest must be >= 0");
}

// The clusters of a device cloud of `stride` floats per point with a known bounding box.  Leaves label, kind, size, keep and the
// kept list in W, gathers the kept rows into dst(kept) -- not called when nothing is kept --, waits, fills the summary and the
// stats.  Returns the number of kept points.
uint32_t dbscan_dev(plade_ctx *ctx, DbscanWork &W, const float *d_rows, uint32_t n, uint32_t stride, const float bbmin[3], const float bbmax[3],
                    const plade_dbscan_params &p, const KeepRows &dst, plade_dbscan_summary *summary) {
    W.spans.mark(ctx, 0);
    TargetGrid &G = W.grid;
    const float r = (float)p.radius;
    G.build(ctx, d_rows, n, stride, radius_cell((double)r, bbmin, bbmax), bbmin, bbmax, true);
    W.spans.mark(ctx, 1);

    WalkArgs a;
    memset(&a, 0, sizeof(a));
    a.g = view_of(G, "cluster_dbscan");
    a.n = n; a.r2 = r * r;
    a.min_points = (uint32_t)p.min_points;
    a.core_bits = W.core_bits.ensure(cdiv(n, 64));
    a.kind = W.kind.ensure((size_t)n + 4);
    a.parent = W.parent.ensure(n);
    a.attach = W.attach.ensure(n);
    a.counts = W.counts.ensure(4);
    ctx->fill_async(a.counts, 0, 16);
    const dim3 wgrid(cdiv(n, WALK_TPB));
    hipLaunchKernelGGL(k_db_core, wgrid, dim3(WALK_TPB), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    W.spans.mark(ctx, 2);

    cluster_init_parents(ctx, a.parent, n);
    hipLaunchKernelGGL(k_db_link, wgrid, dim3(WALK_TPB), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(W.h_counts, a.counts, 8, hipMemcpyDeviceToHost, ctx->stream));
    W.spans.mark(ctx, 3);

    cluster_label_select(ctx, W, n, a.parent, a.attach, (uint32_t)p.min_size, (uint32_t)p.max_size, (uint32_t)p.keep_largest);
    const uint32_t C = W.clusters;
    W.spans.mark(ctx, 4);

    const uint32_t total = keep_compact_gather(ctx, W, d_rows, n, stride, dst);
    W.spans.mark(ctx, 5);
    ctx->sync();
    if (summary) {
        summary->n = n;
        summary->clusters = C;
        summary->core = W.h_counts[0];
        summary->border = W.h_counts[1];
        summary->noise = (uint64_t)n - W.h_counts[0] - W.h_counts[1];
        summary->kept_clusters = W.h_count[1];
        summary->kept = total;
        summary->largest = W.h_count[0];
        summary->reserved = 0;
    }
    W.spans.collect();
    ctx->stats.clear();
    ctx->stats.add("dbscan_grid_s", W.spans.seconds(0));
    ctx->stats.add("dbscan_core_s", W.spans.seconds(1));
    ctx->stats.add("dbscan_link_s", W.spans.seconds(2));
    ctx->stats.add("dbscan_label_s", W.spans.seconds(3));
    ctx->stats.add("dbscan_compact_s", W.spans.seconds(4));
    ctx->stats.add("dbscan_clusters", C);
    ctx->stats.add("dbscan_kept", total);
    grid_stats(ctx, "dbscan", W.grid);
    return total;
}

}  // namespace
}  // namespace plade

using namespace plade;

// ---- C ABI (include/plade_hip.h) ---------------------------------------------------------------------------------------------
extern "C" void plade_dbscan_default_params(plade_dbscan_params *p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->radius = 0.0;
    p->min_points = 4;
    p->min_size = 1;
    p->max_size = 0;
    p->keep_largest = 0;
}

extern "C" int plade_cluster_dbscan(plade_ctx *ctx, const float *rows, uint32_t n, uint32_t stride, const plade_dbscan_params *params,
                                    int32_t *label_out, uint8_t *kind_out, uint32_t *size_out, uint8_t *keep_out, uint32_t *kept_index_out,
                                    float *rows_out, plade_dbscan_summary *summary) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(rows, PLADE_EINVAL, "plade_cluster_dbscan: NULL cloud");
        const plade_dbscan_params p = params_or_default(params, plade_dbscan_default_params);
        check_params(n, stride, p);
        DbscanWork &W = work_in<DbscanWork>(ctx->dbscan_work);
        float mn[3], mx[3];
        upload_rows(ctx, W.in, rows, n, stride, mn, mx);
        const uint32_t total = dbscan_dev(ctx, W, W.in.p, n, stride, mn, mx, p, keep_rows_host(W, stride), summary);
        if (label_out) HIP_TRY(hipMemcpyAsync(label_out, W.label.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (kind_out) HIP_TRY(hipMemcpyAsync(kind_out, W.kind.p, n, hipMemcpyDeviceToHost, ctx->stream));
        if (size_out && W.clusters) HIP_TRY(hipMemcpyAsync(size_out, W.size.p, (size_t)W.clusters * 4, hipMemcpyDeviceToHost, ctx->stream));
        keep_copy_out(ctx, W, n, total, stride, keep_out, kept_index_out, rows_out);
        ctx->sync();
        return PLADE_OK;
    });
}

extern "C" int plade_cloud_cluster_dbscan_dev(plade_ctx *ctx, plade_cloud *cloud, const plade_dbscan_params *params, plade_cloud **out,
                                              int32_t *label_out, uint8_t *kind_out, uint32_t *kept_index_out, plade_dbscan_summary *summary) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(cloud && out, PLADE_EINVAL, "plade_cloud_cluster_dbscan_dev: NULL cloud");
        *out = nullptr;
        const plade_dbscan_params p = params_or_default(params, plade_dbscan_default_params);
        const CloudDev &in = cloud->dev;
        check_params(in.n, 6, p);
        DbscanWork &W = work_in<DbscanWork>(ctx->dbscan_work);
        resident_result(ctx, out, [&](CloudDev &c) {
            const uint32_t total = dbscan_dev(ctx, W, in.aos.p, in.n, 6, in.bbmin, in.bbmax, p, keep_rows_cloud(c), summary);
            if (label_out) HIP_TRY(hipMemcpyAsync(label_out, W.label.p, (size_t)in.n * 4, hipMemcpyDeviceToHost, ctx->stream));
            if (kind_out) HIP_TRY(hipMemcpyAsync(kind_out, W.kind.p, in.n, hipMemcpyDeviceToHost, ctx->stream));
            keep_copy_out(ctx, W, in.n, total, 6, nullptr, kept_index_out, nullptr);
            ctx->sync();
            require_kept(total, "plade_cloud_cluster_dbscan_dev: the selection");
        });
        return PLADE_OK;
    });
}
