// plade_amd/csrc/k_subsample.hip -- a cloud's own points at a minimum spacing on gfx950 (semantics: subsample.h).
//
// Layout
//   grid     the dense row index of TargetGrid with the radius filter's cell, radius_cell(spacing) of grid_walk.h (the rule of
//            DESIGN.md section 10): the 27-cell block around a point holds everything closer than spacing.  Where the grid caps its
//            cell count the cell grows and the block holds more: the walk stays exact.
//   state    one uint32 per point in the grid's SORTED order, read alongside sorted[s]: 0 = undecided, otherwise round << 1 | kept.
//            A reader in round t treats an entry whose round field equals t as undecided.  One buffer then gives the synchronous
//            rounds of subsample.h however the hardware interleaves the lanes: a read that races with this round's store sees 0
//            or a word written this round (an aligned 32-bit store is a single write), and both mean "undecided"; a word of an
//            earlier round was complete before this launch began.  So what a lane decides is a function of the state at the end
//            of the previous round alone.
//   round    k_sub_round, one launch per round, one lane per active sorted position (round 1: all n).  The lane walks the nine
//            runs of its block; for each j != i with d < r2 it reads state[j]: kept in an earlier round (then key_j < key_i): i is
//            dropped and leaves the walk; undecided in the sense above and key_j < key_i -- the neighbour's key is recomputed from
//            the original index in sorted[j].w, there is no key array --: i is blocked.  Neither dropped nor blocked: i is kept.  A lane
//            makes ONE pass per launch and waits on nobody: no spin on a state word, no grid barrier, no persistent kernel.  The
//            lanes still undecided go to the next round's active list through fail_append, whose counter is the number of
//            undecided points.  The list's order varies from run to run; no result depends on it: a lane's decision reads the
//            state words alone, and the list only says which positions get a lane.
//   host     after each round the undecided count comes back through the context's page-locked read-back (d2h + sync); the loop
//            stops at 0.  The undecided point with the smallest key is decided in every round: at most n rounds.
//   output   k_sub_scatter: keep, flags and round in the original order; compact_flags (one scan) gives the ascending kept list;
//            gather_rows (prims.h) copies the kept rows word for word.
#include "subsample.h"
#include "cloud_tool.h"
#include "grid_walk.h"
#include "voxel.h"

namespace plade {

namespace {

constexpr int ROUND_TPB = 256, ROW_TPB = 256;

struct RoundArgs {
    GridView g;
    uint32_t n_active;               // lanes of this launch
    const uint32_t *active;          // their sorted positions; nullptr: 0 .. n_active - 1 (round 1)
    uint32_t round;                  // t >= 1
    float r2;                        // (float)spacing * (float)spacing
    uint64_t base;                   // mix64(seed)
    uint32_t *state;                 // by sorted position
    uint32_t *next, *count;          // the next round's active list and its length = the points still undecided
};

__global__ __launch_bounds__(ROUND_TPB) void k_sub_round(const RoundArgs a) {
    const uint32_t t = blockIdx.x * ROUND_TPB + threadIdx.x;
    uint32_t s = 0;
    bool waits = false;
    if (t < a.n_active) {
        s = a.active ? a.active[t] : t;
        const float4 q4 = a.g.sorted[s];
        const f3 q(q4.x, q4.y, q4.z);
        const uint32_t self = __float_as_uint(q4.w);
        const uint64_t key = mix64(a.base ^ (uint64_t)self);
        int cx, cy, cz;
        cell_of(a.g, q, cx, cy, cz);
        // A neighbour that was kept in an earlier round always has the smaller key: it was kept when every neighbour of ITS with a
        // smaller key had been dropped, and this point is a neighbour that has not been.  So the state word is read first and only
        // the undecided neighbours cost a key.  In round 1 nothing has been kept yet: the first undecided neighbour with a smaller
        // key settles that the point waits.
        uint32_t verdict = 0;        // bit 0: blocked, bit 1: dropped
        const uint32_t leave = a.round == 1u ? 3u : 2u;
        for_block27(a.g, cx, cy, cz, [&](uint32_t j0, uint32_t j1) {
            for (uint32_t j = j0; j < j1 && !(verdict & leave); ++j) {
                if (j == s) continue;
                const float4 p = a.g.sorted[j];
                if (!(flann_d2(q, f3(p.x, p.y, p.z)) < a.r2)) continue;
                const uint32_t st = __hip_atomic_load(a.state + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (st == 0u || (st >> 1) == a.round) {                // undecided at the end of the previous round
                    const uint32_t other = __float_as_uint(p.w);
                    const uint64_t okey = mix64(a.base ^ (uint64_t)other);
                    if (okey < key || (okey == key && other < self)) verdict |= 1u;
                } else verdict |= (st & 1u) << 1;                      // kept in an earlier round: dropped, leaves the walk
            }
        });
        if (verdict & 2u) __hip_atomic_store(a.state + s, a.round << 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if (!verdict) __hip_atomic_store(a.state + s, (a.round << 1) | 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else waits = true;
    }
    fail_append(waits, s, a.next, a.count);   // (all lanes)
}

// keep, flags and round by original index from the state words by sorted position (every point is decided)
__global__ __launch_bounds__(ROW_TPB) void k_sub_scatter(const float4 *__restrict__ sorted, const uint32_t *__restrict__ state, uint32_t n,
                                                         uint8_t *__restrict__ keep, uint32_t *__restrict__ flags,
                                                         uint32_t *__restrict__ round) {
    const uint32_t s = blockIdx.x * ROW_TPB + threadIdx.x;
    if (s >= n) return;
    const uint32_t i = __float_as_uint(sorted[s].w), st = state[s];
    keep[i] = (uint8_t)(st & 1u);
    flags[i] = st & 1u;
    round[i] = st >> 1;
}

}  // namespace

struct SubsampleWork : KeepWork {
    TargetGrid grid;
    DBuf<uint32_t> state, list[2], count, round;
    EventSpans<4> spans;             // grid, rounds, compact + gather
};

namespace {

void check_params(uint32_t n, uint32_t stride, const plade_subsample_params &p) {
    PLADE_REQUIRE(n >= 1, PLADE_EINVAL, "subsample_spacing: the cloud is empty (n = 0)");
    PLADE_REQUIRE(n < 0x80000000u, PLADE_EINVAL, "subsample_spacing: more than 2^31 - 1 points");   // (round << 1 | kept in 32 bits)
    PLADE_REQUIRE(stride >= 3, PLADE_EINVAL, "subsample_spacing: stride must be >= 3 floats");
    PLADE_REQUIRE(radius_ok(p.spacing, true), PLADE_EINVAL,
                  "subsample_spacing: spacing must be finite and > 0, its fp32 square finite and not below FLT_MIN");
}

// The subsample of a device cloud of `stride` floats per point with a known bounding box.  Leaves keep, round and the kept list in
// W, gathers the kept rows into dst(kept), waits, fills the summary and the stats.  Returns the number of kept points (>= 1).
uint32_t subsample_dev(plade_ctx *ctx, SubsampleWork &W, const float *d_rows, uint32_t n, uint32_t stride, const float bbmin[3],
                       const float bbmax[3], const plade_subsample_params &p, const KeepRows &dst,
                       plade_subsample_summary *summary) {
    W.spans.mark(ctx, 0);
    TargetGrid &G = W.grid;
    const float r = (float)p.spacing;
    G.build(ctx, d_rows, n, stride, radius_cell((double)r, bbmin, bbmax), bbmin, bbmax, true);
    W.spans.mark(ctx, 1);

    RoundArgs a;
    memset(&a, 0, sizeof(a));
    a.g = view_of(G, "subsample_spacing");
    a.r2 = r * r;
    a.base = mix64(p.seed);
    a.state = W.state.ensure(n);
    uint32_t *d_cnt = W.count.ensure(4);
    W.list[0].ensure(n); W.list[1].ensure(n);
    ctx->fill_async(a.state, 0, (size_t)n * 4);
    uint32_t active = n, rounds = 0;
    while (active) {
        // (cannot happen: the undecided point with the smallest key is decided in every round)
        PLADE_REQUIRE(rounds <= n, PLADE_EFAIL, "subsample_spacing: the rounds did not end");
        ++rounds;
        a.n_active = active;
        a.active = rounds == 1 ? nullptr : W.list[rounds & 1].p;
        a.round = rounds;
        a.next = W.list[(rounds + 1) & 1].p; a.count = d_cnt;
        ctx->fill_async(d_cnt, 0, 4);
        hipLaunchKernelGGL(k_sub_round, dim3(cdiv(active, ROUND_TPB)), dim3(ROUND_TPB), 0, ctx->stream, a);
        HIP_TRY(hipGetLastError());
        ctx->d2h(&active, d_cnt, 4);
        ctx->sync();
    }
    W.spans.mark(ctx, 2);

    uint8_t *d_keep = W.keep.ensure((size_t)n + 4);
    uint32_t *d_round = W.round.ensure(n), *d_flags = keep_flags(ctx, W, n);
    hipLaunchKernelGGL(k_sub_scatter, dim3(cdiv(n, ROW_TPB)), dim3(ROW_TPB), 0, ctx->stream, a.g.sorted, a.state, n, d_keep, d_flags, d_round);
    HIP_TRY(hipGetLastError());
    const uint32_t total = keep_compact_gather(ctx, W, d_rows, n, stride, dst);
    PLADE_REQUIRE(total >= 1, PLADE_EFAIL, "subsample_spacing: no point was kept");   // (cannot happen: the smallest key is kept)
    W.spans.mark(ctx, 3);
    ctx->sync();
    if (summary) {
        summary->n = n;
        summary->kept = total;
        summary->rounds = rounds;
    }
    W.spans.collect();
    ctx->stats.clear();
    ctx->stats.add("subsample_grid_s", W.spans.seconds(0));
    ctx->stats.add("subsample_rounds_s", W.spans.seconds(1));
    ctx->stats.add("subsample_compact_s", W.spans.seconds(2));
    ctx->stats.add("subsample_rounds", rounds);
    ctx->stats.add("subsample_kept", total);
    grid_stats(ctx, "subsample", W.grid);
    return total;
}

}  // namespace
}  // namespace plade

using namespace plade;

// ---- C ABI (include/plade_hip.h) ---------------------------------------------------------------------------------------------
extern "C" void plade_subsample_default_params(plade_subsample_params *p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->spacing = 0.0;
    p->seed = 0;
}

extern "C" int plade_subsample_spacing(plade_ctx *ctx, const float *rows, uint32_t n, uint32_t stride, const plade_subsample_params *params,
                                       uint8_t *keep_out, uint32_t *kept_index_out, float *rows_out, uint32_t *round_out,
                                       plade_subsample_summary *summary) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(rows, PLADE_EINVAL, "plade_subsample_spacing: NULL cloud");
        const plade_subsample_params p = params_or_default(params, plade_subsample_default_params);
        check_params(n, stride, p);
        SubsampleWork &W = work_in<SubsampleWork>(ctx->subsample_work);
        float mn[3], mx[3];
        upload_rows(ctx, W.in, rows, n, stride, mn, mx);
        const uint32_t total = subsample_dev(ctx, W, W.in.p, n, stride, mn, mx, p, keep_rows_host(W, stride), summary);
        keep_copy_out(ctx, W, n, total, stride, keep_out, kept_index_out, rows_out);
        if (round_out) HIP_TRY(hipMemcpyAsync(round_out, W.round.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        return PLADE_OK;
    });
}

extern "C" int plade_cloud_subsample_dev(plade_ctx *ctx, plade_cloud *cloud, const plade_subsample_params *params, plade_cloud **out,
                                         uint8_t *keep_out, uint32_t *kept_index_out, plade_subsample_summary *summary) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(cloud && out, PLADE_EINVAL, "plade_cloud_subsample_dev: NULL cloud");
        *out = nullptr;
        const plade_subsample_params p = params_or_default(params, plade_subsample_default_params);
        const CloudDev &in = cloud->dev;
        check_params(in.n, 6, p);
        SubsampleWork &W = work_in<SubsampleWork>(ctx->subsample_work);
        resident_result(ctx, out, [&](CloudDev &c) {
            const uint32_t total = subsample_dev(ctx, W, in.aos.p, in.n, 6, in.bbmin, in.bbmax, p, keep_rows_cloud(c), summary);
            keep_copy_out(ctx, W, in.n, total, 6, keep_out, kept_index_out, nullptr);
            ctx->sync();
        });
        return PLADE_OK;
    });
}
