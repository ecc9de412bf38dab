// plade_amd/csrc/registration.hip -- the registration() overloads of code/PLADE/plade.h behind the
// C ABI: auto-tuned plane extraction (plade.cpp:602-662) + the planes-given pipeline, device-resident
// cloud handles, and the S1b seam entry point.
#include "pipeline.h"
#include "prims.h"
#include "ransac.h"
#include <algorithm>
#include <numeric>
#include <thread>

using namespace plade;

namespace {

RansacParams ransac_params(plade_ctx *ctx, uint32_t min_support, bool host_indices = true) {
    RansacParams rp;
    rp.host_indices = host_indices;
    rp.min_support = min_support;
    rp.orient_normals = ctx->params.orient_normals;
    rp.seed = ctx->params.ransac_seed;
    return rp;  // 0.005f, 0.02f, 0.8f, 0.001f: plade.cpp:607,627
}

// extract() (code/PLADE/plade.cpp:602-635) of ALL clouds of a call -- the two scans of a registration, or the four of a
// group of registrations: the reference runs it once per cloud; here pass p of the halving loops is one merged launch
// sequence (ransac_detect_prepared) in which every cloud that still needs a detect call takes part with its own
// min_support.  Cloud g's statistics (the trace of its auto-tuning loop: plane count of every detect call, the min_support
// it ends at; tests compare it with the reference loop over libransac, g2_extract.npz) go to stat_ctx[g], under tags[g].
void extract_clouds(plade_ctx *ctx, int n_clouds, const CloudDev *const clouds[], const int init_min_support[], bool auto_tune,
                    PlaneSetOut *const planes[], plade_ctx *const stat_ctx[], const char *const tags[], bool host_indices) {
    const uint32_t min_num = (uint32_t)ctx->params.min_planes, max_num = (uint32_t)ctx->params.max_planes;
    const int min_allowed_support = 200, max_trials = 10;
    if (!ctx->ransac_work) ctx->ransac_work = ransac_work_create();
    RansacWork &W = *ctx->ransac_work;
    ransac_prepare(ctx, W, clouds, n_clouds);
    {   // average_spacing(source, k = 6) of plade.cpp:41 for every pair's source cloud, see ransac.hip
        int src_slots[PLADE_GROUP_MAX], ns = 0;
        for (int g = 1; g < n_clouds; g += 2) src_slots[ns++] = g;
        if (ns) ransac_spacing_enqueue(ctx, W, src_slots, ns, 6, 10000);
    }
    int ms[RANSAC_SLOTS], trials[RANSAC_SLOTS];
    bool finished[RANSAC_SLOTS];
    for (int g = 0; g < RANSAC_SLOTS; ++g) { ms[g] = g < n_clouds ? init_min_support[g] : 0; trials[g] = 0; finished[g] = g >= n_clouds; }
    for (;;) {
        RansacJob jobs[RANSAC_SLOTS];
        bool any = false;
        for (int g = 0; g < n_clouds; ++g) {
            jobs[g].active = !finished[g];
            jobs[g].rp = ransac_params(ctx, (uint32_t)ms[g], host_indices);
            jobs[g].out = planes[g];
            jobs[g].stats = &stat_ctx[g]->stats;
            any = any || jobs[g].active;
        }
        if (!any) break;
        ransac_detect_prepared(ctx, W, jobs);
        for (int g = 0; g < n_clouds; ++g) {
            if (finished[g]) continue;
            PlaneSetOut &pl = *planes[g];
            Stats &st = stat_ctx[g]->stats;
            const std::string tag = tags[g];
            ++trials[g];
            st.add("n_detect_calls", 1);
            st.add("n_score_passes", pl.n_score_passes);
            st.add("bytes_ransac", pl.score_bytes);
            st.add("extract_planes_trial" + std::to_string(trials[g]) + tag, pl.P());
            st.add("extract_final_min_support" + tag, ms[g] - ctx_stat(stat_ctx[g], ("extract_final_min_support" + tag).c_str()));
            if (!auto_tune) { finished[g] = true; continue; }   // plade.cpp:583-599: one call with the caller's min_support
            if (trials[g] == 1 && pl.P() > max_num) {
                // top max_num by support.  The reference sorts with a `>=` comparator (plade.cpp:612-615,
                // undefined behaviour on ties); a stable descending sort is used here.
                const uint32_t P = pl.P();
                pl.fetch_indices(ctx->stream);
                std::vector<uint32_t> order(P);
                std::iota(order.begin(), order.end(), 0u);
                std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
                    return pl.offsets[a + 1] - pl.offsets[a] > pl.offsets[b + 1] - pl.offsets[b];
                });
                PlaneSetOut r;
                r.offsets.assign(1, 0);
                for (uint32_t k = 0; k < max_num; ++k) {
                    const uint32_t i = order[k];
                    r.coef.insert(r.coef.end(), pl.coef.begin() + 4 * i, pl.coef.begin() + 4 * i + 4);
                    r.idx.insert(r.idx.end(), pl.idx.begin() + pl.offsets[i], pl.idx.begin() + pl.offsets[i + 1]);
                    r.offsets.push_back((int32_t)r.idx.size());
                }
                r.n_score_passes = pl.n_score_passes;
                r.trace = std::move(pl.trace);   // (of the untrimmed call: its plane indices are those before the sort)
                pl = std::move(r);   // d_idx is null now: the next stage uploads the reordered host lists
                finished[g] = true;
                continue;
            }
            // plade.cpp:620-633: fewer than min_num planes -> halve min_support, at most 10 detect calls, never below 200
            const int next = ms[g] / 2;
            if (pl.P() >= min_num || trials[g] >= max_trials || next < min_allowed_support) finished[g] = true;
            else ms[g] = next;
        }
    }
}

// Everything of registration(T, target, source) (plade.cpp:638-662) behind the plane extraction, for ONE pair, on the streams
// and work areas of `pc` (the pair's context: the calling context, or its peer for the second pair of a group); the planes'
// device lists and the spacing query live in the work area of `owner`, slots `slot_t` and `slot_t + 1`.
int register_tail(plade_ctx *pc, plade_ctx *owner, int slot_t, const CloudDev &tgt, const CloudDev &src, PlaneSetOut &tp, PlaneSetOut &sp,
                  bool auto_tune, bool have_spacing, float spacing, float *T16, Clock::time_point t0) {
    plade_ctx *ctx = pc;
    (void)slot_t;
    if (!have_spacing) { spacing = source_spacing(ctx, *ctx->reg_work, src); have_spacing = true; }   // clumped cloud
    if (auto_tune) {
        if (tp.P() < (uint32_t)owner->params.min_planes) {  // plade.cpp:646-650
            ctx->last_error = "too few planes extracted from the target point cloud";
            return PLADE_EFAIL;
        }
        if (sp.P() < (uint32_t)owner->params.min_planes) {  // plade.cpp:653-657
            ctx->last_error = "too few planes extracted from the source point cloud";
            return PLADE_EFAIL;
        }
    }
    // the device index lists live in the slots of the owner's work area and stay valid for the next stage
    if (ctx->params.dump) {
        ctx->put("tgt_planes", tp.coef.data(), tp.coef.size());
        ctx->put("tgt_plane_offsets", tp.offsets.data(), tp.offsets.size());
        ctx->put("tgt_plane_idx", tp.idx.data(), tp.idx.size());
        ctx->put("src_planes", sp.coef.data(), sp.coef.size());
        ctx->put("src_plane_offsets", sp.offsets.data(), sp.offsets.size());
        ctx->put("src_plane_idx", sp.idx.data(), sp.idx.size());
        tp.trace.put(ctx, "tgt_");
        sp.trace.put(ctx, "src_");
    }
    ctx->stats.add("n_planes_tgt", tp.P());
    ctx->stats.add("n_planes_src", sp.P());
    PlaneSetView tv, sv;
    tv.coef = tp.coef.data(); tv.offsets = tp.offsets.data(); tv.idx = tp.idx.data(); tv.P = tp.P();
    sv.coef = sp.coef.data(); sv.offsets = sp.offsets.data(); sv.idx = sp.idx.data(); sv.P = sp.P(); sv.d_idx = sp.d_idx;
    tv.d_idx = tp.d_idx;
    if (tp.d_idx) { tv.d_pos = tp.d_pos; tv.m_x = tp.m_x; tv.m_y = tp.m_y; tv.m_z = tp.m_z; }
    if (sp.d_idx) { sv.d_pos = sp.d_pos; sv.m_x = sp.m_x; sv.m_y = sp.m_y; sv.m_z = sp.m_z; }
    MirroredPlanes mirror;
    if (ctx->params.unoriented_normals) {   // README.md:109-110, see MirroredPlanes (pipeline.h)
        mirror.build(tp.coef.data(), tp.offsets.data(), tp.idx.size() == (size_t)tp.offsets.back() ? tp.idx.data() : nullptr, tp.P());
        tv.coef = mirror.coef.data(); tv.offsets = mirror.offsets.data(); tv.P = 2 * tp.P(); tv.mirrored = true;
        tv.idx = mirror.idx.empty() ? nullptr : mirror.idx.data();
        if (!tv.d_idx && !tv.idx && tv.offsets[tv.P]) { tv.mirrored = false; }   // cannot happen: one of the two lists always exists
    }
    const bool ok = run_registration(ctx, *ctx->reg_work, tgt, src, tv, sv, T16, have_spacing ? &spacing : nullptr);
    ctx->stats.add("t_registration", secs_since(t0));
    // roofline bookkeeping; bytes_ransac was summed per scan launch and cloud by extract_clouds
    ctx->stats.add("bytes_voxel", 12.0 * ((double)tgt.n + src.n));
    ctx->ev_collect();
    if (!ok) { if (ctx->last_error.empty()) ctx->last_error = "registration failed: no matched result found"; return PLADE_EFAIL; }
    return PLADE_OK;
}

void ensure_pair_areas(plade_ctx *ctx) {
    if (!ctx->aux) {
        plade_ctx *a = nullptr;
        PLADE_REQUIRE(plade_ctx_create(ctx->device, &a) == PLADE_OK, PLADE_EDEVICE, "cannot create the auxiliary stream");
        ctx->aux = a;
    }
    if (!ctx->reg_work) ctx->reg_work = registration_work_create();
}

plade_ctx *peer_ctx(plade_ctx *ctx, int i) {   // the context of pair i >= 1 of a group
    plade_ctx *&p = ctx->peers[i - 1];
    if (!p) {
        plade_ctx *a = nullptr;
        PLADE_REQUIRE(plade_ctx_create(ctx->device, &a) == PLADE_OK, PLADE_EDEVICE, "cannot create the context of a further pair of the group");
        p = a;
    }
    return p;
}

// `count` (1 .. PLADE_GROUP_MAX) registrations as ONE group: the plane extraction of all their clouds is one launch sequence on
// the calling context's stream (count pairs = 2 x count clouds per kernel: the extraction is a chain of ~150 short, mostly
// latency-bound kernels whose duration grows slowly with more workgroups, so a group divides its commands, host waits and
// GPU time per registration); behind it every pair runs the rest of its registration on its own context (pair 0: the calling
// one on the calling thread, pair i: peer context i on a helper thread), concurrently.  status[i]: PLADE_OK / PLADE_EFAIL /
// an error code.
// `first`: the pairs are numbers first .. first + count - 1 of the caller's group (register_group_parts): pair number j runs on
// peer context j (number 0 on ctx itself), whichever part of the group it is registered with.
void register_group(plade_ctx *ctx, int first, int count, const CloudDev *const tgt[], const CloudDev *const src[], const int ms_t[],
                    const int ms_s[], bool auto_tune, float *T16, int32_t *status) {
    PLADE_REQUIRE(count >= 1 && first >= 0 && first + count <= PLADE_GROUP_MAX, PLADE_EINVAL, "a group holds one to PLADE_GROUP_MAX pairs");
    Clock::time_point t0 = Clock::now();
    plade_ctx *pcs[PLADE_GROUP_MAX] = {};
    struct ShardOff {      // pair 0 of a group of several runs on ctx itself: its shard is set aside for the call
        plade_ctx *c; plade_ctx::CandidateShard saved; bool off;
        ShardOff(plade_ctx *c_, bool off_) : c(c_), saved(c_->shard), off(off_) { if (off) c->shard = plade_ctx::CandidateShard{}; }
        ~ShardOff() { if (off) c->shard = saved; }
    } shard_off(ctx, count > 1);
    // whatever way this call ends, no pair context keeps a grid marked "queued by the group" (a later single-pair call on it
    // would adopt a stale one)
    struct ReadyGuard {
        plade_ctx **pcs; int count;
        ~ReadyGuard() {
            for (int i = 0; i < count; ++i) {
                if (!pcs[i] || !pcs[i]->reg_work) continue;
                for (int side = 0; side < 2; ++side) {
                    const WholeVoxelSlot sl = whole_voxel_slot(*pcs[i]->reg_work, side == 0, 0);
                    *sl.ready = false; *sl.planes_ready = false; *sl.obb_ready = false;
                }
            }
        }
    } ready_guard{pcs, count};
    for (int i = 0; i < count; ++i) {
        if (first + i == 0) { pcs[i] = ctx; continue; }
        pcs[i] = peer_ctx(ctx, first + i);
        pcs[i]->params = ctx->params;
        // the candidate shard is an axis of ONE pair (include/plade_hip.h): the pairs of a group run their tails on concurrent
        // threads, and a collective entered from several threads in an order that differs between the ranks would mismatch
        // or hang (advisor r4) -- a batch shards whole pairs over the ranks instead
        pcs[i]->shard = count > 1 ? plade_ctx::CandidateShard{} : ctx->shard;
        pcs[i]->stats.clear();
        pcs[i]->dump.clear();
        pcs[i]->last_error.clear();
        pcs[i]->drop_reads();
    }
    for (int i = 0; i < count; ++i) {
        pcs[i]->in_group = count > 1;
        if (pcs[i]->reg_work)
            for (int side = 0; side < 2; ++side) {
                const WholeVoxelSlot sl = whole_voxel_slot(*pcs[i]->reg_work, side == 0, 0);
                *sl.ready = false; *sl.planes_ready = false; *sl.obb_ready = false;
            }
        ensure_pair_areas(pcs[i]);
        for (int k = 0; k < 16; ++k) T16[16 * i + k] = (k % 5 == 0) ? 1.f : 0.f;
        status[i] = PLADE_OK;
    }
    PlaneSetOut planes[2 * PLADE_GROUP_MAX];
    float spacing[PLADE_GROUP_MAX] = {};
    bool have_spacing[PLADE_GROUP_MAX] = {};
    {
        StageTimer t(ctx, "t_extract");
        const CloudDev *clouds[2 * PLADE_GROUP_MAX];
        int init[2 * PLADE_GROUP_MAX];
        PlaneSetOut *outs[2 * PLADE_GROUP_MAX];
        plade_ctx *stat_ctx[2 * PLADE_GROUP_MAX];
        const char *tags[2 * PLADE_GROUP_MAX];
        for (int i = 0; i < count; ++i) {
            clouds[2 * i] = tgt[i]; clouds[2 * i + 1] = src[i];
            init[2 * i] = auto_tune ? ctx->params.init_min_support : ms_t[i];
            init[2 * i + 1] = auto_tune ? ctx->params.init_min_support : ms_s[i];
            outs[2 * i] = &planes[2 * i]; outs[2 * i + 1] = &planes[2 * i + 1];
            stat_ctx[2 * i] = stat_ctx[2 * i + 1] = pcs[i];
            tags[2 * i] = "_tgt"; tags[2 * i + 1] = "_src";
        }
        // the next stage reads the index lists from the device; the host copy is only for dumps.  The point spacing
        // (plade.cpp:41) only needs the source cloud: its two kernels are queued right behind the Morton order of the
        // extraction and run ahead of the RANSAC iterations on the same stream -- no helper thread
        extract_clouds(ctx, 2 * count, clouds, init, auto_tune, outs, stat_ctx, tags, ctx->params.dump != 0);
        StageTimer ts(ctx, "t_spacing");
        for (int i = 0; i < count; ++i) have_spacing[i] = ransac_spacing_finish(ctx, *ctx->ransac_work, 2 * i + 1, &spacing[i]);
    }
    // The whole-cloud voxel grids of all clouds of the group (DownSamplePointCloud, plade.cpp:77-79 / :292-294: leaf = 4 x the
    // pair's point spacing) in ONE launch sequence on this stream -- 7 launches instead of 7 per cloud; doubling the per-cloud grids
    // was measured to cost the batch 8 % -- written where every pair's preparation expects its own (pipeline.hip: prepare_side).
    if (count > 1 && ctx->params.prepare_sides != 1) {
        bool all = true;
        for (int i = 0; i < count; ++i) all = all && have_spacing[i] && planes[2 * i].P() && planes[2 * i + 1].P();
        if (all) {
            StageTimer tv(ctx, "t_group_voxel");
            VoxBatchItem items[2 * PLADE_GROUP_MAX];
            bool *ready[2 * PLADE_GROUP_MAX];
            for (int i = 0; i < count; ++i)
                for (int side = 0; side < 2; ++side) {
                    const CloudDev &c = side ? *src[i] : *tgt[i];
                    const WholeVoxelSlot slot = whole_voxel_slot(*pcs[i]->reg_work, side == 0, c.n);
                    VoxBatchItem &it = items[2 * i + side];
                    it.aos = c.aos.p; it.sx = c.x(); it.sy = c.y(); it.sz = c.z(); it.n = c.n;
                    it.leaf = spacing[i] * 4;   // pipeline.hip: downSampleDistance
                    for (int k = 0; k < 3; ++k) { it.bbmin[k] = c.bbmin[k]; it.bbmax[k] = c.bbmax[k]; }
                    it.work = slot.work; it.out_soa = slot.out_soa;
                    ready[2 * i + side] = slot.ready;
                }
            if (voxel_whole_batch(ctx, ctx->vox_batch, 2 * count, items))
                for (int q = 0; q < 2 * count; ++q) *ready[q] = true;
            // ... and the per-plane grids (plade.cpp:93-105 / :308-319): the planes' supports as the extraction left them on the
            // device (positions in its Morton-ordered copy), one group per plane
            bool lists = !ctx->params.unoriented_normals;
            for (int q = 0; q < 2 * count; ++q) lists = lists && planes[q].d_pos && planes[q].m_x && planes[q].P() <= 1024;
            if (lists) {
                for (int i = 0; i < count; ++i)
                    for (int side = 0; side < 2; ++side) {
                        const PlaneSetOut &pl = planes[2 * i + side];
                        const WholeVoxelSlot slot = whole_voxel_slot(*pcs[i]->reg_work, side == 0, 0);
                        VoxBatchItem &it = items[2 * i + side];
                        it.aos = nullptr; it.sx = pl.m_x; it.sy = pl.m_y; it.sz = pl.m_z;
                        it.items = pl.d_pos; it.offsets_host = pl.offsets.data(); it.P = pl.P();
                        it.n = (uint32_t)pl.offsets[pl.P()];
                        it.work = slot.planes; it.out_soa = nullptr;
                        ready[2 * i + side] = slot.planes_ready;
                    }
                if (voxel_whole_batch(ctx, ctx->vox_batch, 2 * count, items)) {
                    for (int q = 0; q < 2 * count; ++q) *ready[q] = true;
                    // ... and, both grids of every cloud being queued, the boxes of all of them (ComputeBoundingBox, plade.cpp:81-84,
                    // :106-117): one launch of latency-chain workgroups instead of one per cloud
                    ObbBatchItem ob[2 * PLADE_GROUP_MAX];
                    for (int i = 0; i < count; ++i)
                        for (int side = 0; side < 2; ++side) {
                            const PlaneSetOut &pl = planes[2 * i + side];
                            const WholeVoxelSlot slot = whole_voxel_slot(*pcs[i]->reg_work, side == 0, 0);
                            ob[2 * i + side] = ObbBatchItem{slot.work->out_xyz.p, slot.work->count.p, slot.planes->out_xyz.p, slot.planes->group_offsets.p,
                                                            pl.P(), pl.coef.data(), slot.obb};
                            ready[2 * i + side] = slot.obb_ready;
                        }
                    if (obb_units_batch(ctx, 2 * count, ob, ctx->vox_batch.obb_coef))
                        for (int q = 0; q < 2 * count; ++q) *ready[q] = true;
                }
            }
        }
    }
    if (count == 1 && pcs[0] == ctx) {
        status[0] = register_tail(ctx, ctx, 0, *tgt[0], *src[0], planes[0], planes[1], auto_tune, have_spacing[0], spacing[0], T16, t0);
        return;
    }
    // The other pairs' streams read what the extraction wrote on this context's stream (support lists, the Morton-ordered
    // copy), and the extraction's host loop returns as soon as the device reports through host-mapped memory, with the last
    // kernels possibly still running: the peers' streams wait for this one.
    if (!ctx->ev_group) HIP_TRY(hipEventCreateWithFlags(&ctx->ev_group, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(ctx->ev_group, ctx->stream));
    Err errs[PLADE_GROUP_MAX];
    for (Err &e : errs) e = Err{0, ""};
    // Lock step (launch.h): what the pairs launch behind this point is collected per pair and issued, merged, on THIS context's
    // stream whenever all of them have reached their next host wait.  Not with the profiled modes (HIP events around single
    // launches), nor under PLADE_DEBUG_READS (eager copies on the pair's own stream); PLADE_NO_LOCKSTEP=1 is the A/B switch.
    static const bool no_lockstep = getenv("PLADE_NO_LOCKSTEP") != nullptr;
    Combiner comb;
    comb.lead = ctx;
    const bool lockstep = !no_lockstep && !ctx->profiling() && !ctx->debug_reads;
    struct CombGuard {      // no context keeps a pointer to the combiner of a call that has ended
        plade_ctx **pcs; int count;
        ~CombGuard() { for (int i = 0; i < count; ++i) if (pcs[i]) { pcs[i]->comb = nullptr; pcs[i]->comb_slot = -1; } }
    } comb_guard{pcs, count};
    if (lockstep) for (int i = 0; i < count; ++i) comb.join(pcs[i]);
    auto tail = [&](int i) {
        std::vector<void *> graveyard;     // allocations replaced while launches that may name them were still queued (common.h)
        struct Leave {
            Combiner &cb; plade_ctx *pc; bool on; std::vector<void *> &gy;
            ~Leave() {
                tl_deferred_free = nullptr;
                if (on) { try { cb.leave(pc); } catch (...) {} cb.bury(gy); }   // (what the pair still had queued may name them: freed with the call)
                for (void *p : gy) dev_free(p);
            }
        } leave{comb, pcs[i], lockstep, graveyard};
        if (lockstep) tl_deferred_free = &graveyard;
        try {
            status[i] = register_tail(pcs[i], ctx, 2 * i, *tgt[i], *src[i], planes[2 * i], planes[2 * i + 1], auto_tune, have_spacing[i], spacing[i],
                                      T16 + 16 * i, t0);
        } catch (const Err &e) { errs[i] = e; }
        catch (const std::exception &e) { errs[i] = Err{PLADE_EDEVICE, e.what()}; }
    };
    struct Joiner {       // an exception between the first helper's start and the joins must not destroy a joinable thread
        std::thread t[PLADE_GROUP_MAX];
        ~Joiner() { for (std::thread &x : t) if (x.joinable()) x.join(); }
    } joiner;
    std::thread *ths = joiner.t;
    for (int i = 0; i < count; ++i)
        if (pcs[i] != ctx) HIP_TRY(hipStreamWaitEvent(pcs[i]->stream, ctx->ev_group, 0));
    for (int i = 0; i < count; ++i) {
        if (i == 0) continue;   // the first pair of the part runs on the calling thread
        ths[i] = std::thread([&, i]() {
            const double cpu0 = thread_cpu_seconds();
            (void)hipSetDevice(ctx->device);
            tail(i);
            pcs[i]->stats.add("cpu_pair_thread", thread_cpu_seconds() - cpu0);
        });
    }
    tail(0);
    for (int i = 1; i < count; ++i) ths[i].join();
    if (lockstep) {
        uint64_t asked = 0;
        for (int i = 0; i < count; ++i) asked += comb.asked[i];
        ctx->stats.add("lockstep_operations_asked", (double)asked);
        ctx->stats.add("lockstep_commands_issued", (double)comb.launches_issued);
        ctx->stats.add("lockstep_group_waits", (double)comb.waits);
    }
    for (int i = 0; i < count; ++i)
        if (errs[i].code) { pcs[i]->drop_reads(); pcs[i]->last_error = errs[i].msg; status[i] = errs[i].code; }
}

// A group whose clouds together hold more than plade_params.group_max_points points is registered in consecutive PARTS, each
// within that budget (or a single pair): the extraction's work area takes ~0.9 KB of HBM per point of the clouds it serves at
// once -- sixteen 1M-point clouds are 14 GB, sixteen 10M-point clouds would be 144 GB per context -- and is reused from part to
// part.  Results do not depend on the partition (every pair is the pair alone, bit for bit).
void register_group_parts(plade_ctx *ctx, int count, const CloudDev *const tgt[], const CloudDev *const src[], const int ms_t[],
                          const int ms_s[], bool auto_tune, float *T16, int32_t *status) {
    PLADE_REQUIRE(count >= 1 && count <= PLADE_GROUP_MAX, PLADE_EINVAL, "a group holds one to PLADE_GROUP_MAX pairs");
    const uint64_t budget = ctx->params.group_max_points ? ctx->params.group_max_points : 48000000u;
    int parts = 0;
    for (int b = 0; b < count;) {
        int e = b + 1;
        uint64_t pts = (uint64_t)tgt[b]->n + src[b]->n;
        while (e < count && pts + tgt[e]->n + src[e]->n <= budget) { pts += (uint64_t)tgt[e]->n + src[e]->n; ++e; }
        register_group(ctx, b, e - b, tgt + b, src + b, ms_t + b, ms_s + b, auto_tune, T16 + 16 * b, status + b);
        b = e;
        ++parts;
    }
    ctx->stats.add("group_parts", parts);
}

int register_clouds(plade_ctx *ctx, const CloudDev &tgt, const CloudDev &src, int ms_t, int ms_s, bool auto_tune, float *T16) {
    const CloudDev *t[1] = {&tgt}, *s[1] = {&src};
    int32_t status[1] = {PLADE_OK};
    register_group(ctx, 0, 1, t, s, &ms_t, &ms_s, auto_tune, T16, status);
    return status[0];
}

}  // namespace

namespace plade {
double ctx_stat(plade_ctx *ctx, const char *name) {
    for (size_t i = 0; i < ctx->stats.names.size(); ++i) if (ctx->stats.names[i] == name) return ctx->stats.values[i];
    return 0.0;
}
}  // namespace plade

// ---- C ABI ---------------------------------------------------------------------------------
// ---- C ABI: seam S1a -------------------------------------------------------------------------
// Runs on the RANSAC loop's own kernels (ransac.hip: score_planes_seam / score_subset_seam).
extern "C" int plade_score_planes(plade_ctx *ctx, const float *pos_nrm, const int32_t *shape_index, uint32_t n,
                                  const float *planes, uint32_t h, float eps, float cos_thresh, uint32_t *counts,
                                  uint32_t *idx_out, uint32_t cap) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(planes && counts && (pos_nrm || !n), PLADE_EINVAL, "plade_score_planes: null argument");
        for (uint32_t j = 0; j < h; ++j) counts[j] = 0;
        if (n == 0 || h == 0) return PLADE_OK;
        CloudDev cloud;
        cloud_upload(ctx, pos_nrm, n, cloud);
        DBuf<int32_t> d_assigned;
        if (shape_index) {
            d_assigned.ensure((size_t)n + 8);
            ctx->h2d(d_assigned.p, shape_index, (size_t)n * 4);
        }
        if (!ctx->ransac_work) ctx->ransac_work = ransac_work_create();
        score_planes_seam(ctx, *ctx->ransac_work, cloud, shape_index ? d_assigned.p : nullptr, planes, h, eps, cos_thresh, counts,
                          idx_out, cap);
        return PLADE_OK;
    });
}

extern "C" int plade_score_planes_subset(plade_ctx *ctx, const float *pos_nrm, const int32_t *shape_index, uint32_t n,
                                         const uint32_t *sub_index, uint32_t m, const float *planes, uint32_t h, float eps,
                                         float cos_thresh, uint32_t *counts, uint32_t *n_unassigned) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(planes && counts && (pos_nrm || !n) && (sub_index || !m), PLADE_EINVAL, "plade_score_planes_subset: null argument");
        for (uint32_t j = 0; j < h; ++j) counts[j] = 0;
        if (n_unassigned) *n_unassigned = 0;
        for (uint32_t i = 0; i < m; ++i) PLADE_REQUIRE(sub_index[i] < n, PLADE_EINVAL, "plade_score_planes_subset: subset index outside the cloud");
        if (n == 0 || h == 0 || m == 0) return PLADE_OK;
        CloudDev cloud;
        cloud_upload(ctx, pos_nrm, n, cloud);
        DBuf<int32_t> d_assigned;
        if (shape_index) {
            d_assigned.ensure((size_t)n + 8);
            ctx->h2d(d_assigned.p, shape_index, (size_t)n * 4);
        }
        if (!ctx->ransac_work) ctx->ransac_work = ransac_work_create();
        score_subset_seam(ctx, *ctx->ransac_work, cloud, shape_index ? d_assigned.p : nullptr, sub_index, m, planes, h, eps, cos_thresh,
                          counts, n_unassigned);
        return PLADE_OK;
    });
}

extern "C" int plade_extract_planes(plade_ctx *ctx, const float *pos_nrm, uint32_t n, uint32_t min_support, float dist_rel,
                                    float bitmap_rel, float cos_thresh, float overlook_p, float *planes_out,
                                    int32_t *offsets_out, int32_t *idx_out, uint32_t max_planes, uint32_t *n_planes_out) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(pos_nrm && planes_out && offsets_out && idx_out && n_planes_out, PLADE_EINVAL, "plade_extract_planes: null argument");
        *n_planes_out = 0;
        offsets_out[0] = 0;
        if (n < 3) return PLADE_OK;  // plane_extraction.cpp:181-184
        CloudDev cloud;
        cloud_upload(ctx, pos_nrm, n, cloud);
        if (!ctx->ransac_work) ctx->ransac_work = ransac_work_create();
        RansacParams rp = ransac_params(ctx, min_support);
        rp.dist_rel = dist_rel; rp.bitmap_rel = bitmap_rel; rp.cos_thresh = cos_thresh; rp.overlook_p = overlook_p;
        PlaneSetOut out;
        ransac_detect(ctx, *ctx->ransac_work, cloud, rp, out);
        out.trace.put(ctx, "");
        const uint32_t P = out.P();
        PLADE_REQUIRE(P <= max_planes, PLADE_ECAP, "plade_extract_planes: more planes than max_planes");
        memcpy(planes_out, out.coef.data(), 16 * (size_t)P);
        memcpy(offsets_out, out.offsets.data(), 4 * ((size_t)P + 1));
        memcpy(idx_out, out.idx.data(), 4 * out.idx.size());
        *n_planes_out = P;
        return PLADE_OK;
    });
}

extern "C" int plade_cloud_upload(plade_ctx *ctx, const float *pos_nrm, uint32_t n, plade_cloud **out) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(pos_nrm && out && n, PLADE_EINVAL, "plade_cloud_upload: bad argument");
        plade_cloud *c = new plade_cloud;
        try {
            cloud_upload(ctx, pos_nrm, n, c->dev);
            ctx->sync();
        } catch (...) { delete c; throw; }
        *out = c;
        return PLADE_OK;
    });
}

// Page-locking of caller-owned host buffers: with it the 24 B/point upload of plade_registration* is an asynchronous DMA
// transfer (the calling thread goes on queueing work, uploads of one context overlap the kernels of the others);
// from pageable memory the HIP runtime stages the data through its own pinned buffer and the call blocks meanwhile.
extern "C" int plade_host_pin(plade_ctx *ctx, const void *ptr, size_t bytes) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(ptr && bytes, PLADE_EINVAL, "plade_host_pin: bad argument");
        HIP_TRY(hipHostRegister(const_cast<void *>(ptr), bytes, hipHostRegisterDefault));
        return PLADE_OK;
    });
}
extern "C" int plade_host_unpin(plade_ctx *ctx, const void *ptr) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(ptr, PLADE_EINVAL, "plade_host_unpin: bad argument");
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        HIP_TRY(hipHostUnregister(const_cast<void *>(ptr)));
        return PLADE_OK;
    });
}

extern "C" void plade_cloud_free(plade_ctx *ctx, plade_cloud *c) {
    if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); }
    delete c;
}

extern "C" int plade_registration_dev(plade_ctx *ctx, plade_cloud *tgt, plade_cloud *src, float *T16) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(tgt && src && T16, PLADE_EINVAL, "plade_registration_dev: null argument");
        ctx->stats.clear();
        ctx->dump.clear();
        ctx->last_error.clear();
        cloud_drop_prefetch(ctx);
        return register_clouds(ctx, tgt->dev, src->dev, 0, 0, true, T16);
    });
}

extern "C" int plade_registration(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t, const float *src_pos_nrm,
                                  uint32_t n_s, float *T16) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(tgt_pos_nrm && src_pos_nrm && T16 && n_t && n_s, PLADE_EINVAL, "plade_registration: bad argument");
        ctx->stats.clear();
        ctx->dump.clear();
        ctx->last_error.clear();
        cloud_drop_prefetch(ctx);
        CloudDev &tgt = ctx->up_tgt, &src = ctx->up_src;
        {
            StageTimer t(ctx, "t_upload");
            cloud_upload_pair(ctx, tgt_pos_nrm, n_t, tgt, src_pos_nrm, n_s, src);
        }
        return register_clouds(ctx, tgt, src, 0, 0, true, T16);
    });
}

namespace {
// The fallback of a group that raised as a whole: pair i alone (on peer context i, as in the group), `prepare(i)` first (the
// host-pointer path uploads the pair's clouds again: the failed group upload stopped at the first refused cloud).
template <class Prepare>
void register_pairs_one_by_one(plade_ctx *ctx, int count, const CloudDev *const ct[], const CloudDev *const cs[], float *T16, int32_t *status,
                               Prepare prepare) {
    ctx->stats.add("group_fallback_pair_by_pair", 1);
    for (int i = 0; i < count; ++i) {
        plade_ctx *pc = i ? peer_ctx(ctx, i) : ctx;
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipStreamSynchronize(pc->stream);
        ctx->drop_reads();
        for (int k = 0; k < 16; ++k) T16[16 * i + k] = (k % 5 == 0) ? 1.f : 0.f;
        const int zero = 0;
        try {
            prepare(i);
            register_group(ctx, i, 1, ct + i, cs + i, &zero, &zero, true, T16 + 16 * i, status + i);
        } catch (const Err &e) {
            ctx->drop_reads();
            if (i) { pc->stats.clear(); pc->dump.clear(); }
            pc->last_error = e.msg;
            status[i] = e.code;
        }
    }
}

// Batch mode: the clouds of THIS call (taken over from the prefetch of the previous call when they are the announced ones),
// then the upload of the NEXT call's clouds started on the prefetch stream; then the group is registered.
int registration_batch(plade_ctx *ctx, uint32_t count, const float *const *tgt, const uint32_t *n_t, const float *const *src,
                       const uint32_t *n_s, uint32_t next_count, const float *const *next_tgt, const uint32_t *next_n_t,
                       const float *const *next_src, const uint32_t *next_n_s, float *T16, int32_t *status) {
    ctx->stats.clear();
    ctx->dump.clear();
    ctx->last_error.clear();
    const float *ptr[2 * PLADE_GROUP_MAX], *nptr[2 * PLADE_GROUP_MAX];
    uint32_t n[2 * PLADE_GROUP_MAX], nn[2 * PLADE_GROUP_MAX];
    CloudDev *out[2 * PLADE_GROUP_MAX];
    const CloudDev *ct[PLADE_GROUP_MAX], *cs[PLADE_GROUP_MAX];
    for (uint32_t i = 0; i < count; ++i) {
        plade_ctx *pc = i ? peer_ctx(ctx, (int)i) : ctx;
        out[2 * i] = &pc->up_tgt; out[2 * i + 1] = &pc->up_src;
        ct[i] = &pc->up_tgt; cs[i] = &pc->up_src;
    }
    for (uint32_t i = 0; i < count; ++i) { ptr[2 * i] = tgt[i]; ptr[2 * i + 1] = src[i]; n[2 * i] = n_t[i]; n[2 * i + 1] = n_s[i]; }
    for (uint32_t i = 0; i < next_count; ++i) { nptr[2 * i] = next_tgt[i]; nptr[2 * i + 1] = next_src[i]; nn[2 * i] = next_n_t[i]; nn[2 * i + 1] = next_n_s[i]; }
    // A cloud the path cannot digest (non-finite coordinates, a bounding box without extent, ...) fails the upload or the
    // extraction of the WHOLE launch sequence; the reference's loop (main.cpp:122-148) fails that pair only.  So a group that
    // raises is registered again pair by pair, each under its own guard: the healthy pairs return what they return alone,
    // the offending one its error code in status[i] and its message in plade_last_error(plade_pair_ctx(ctx, i)).
    bool group_ok = true;
    {
        StageTimer t(ctx, "t_upload");
        Clock::time_point t0 = Clock::now();
        try {
            if (!cloud_take_prefetched(ctx, 2 * (int)count, ptr, n, out)) cloud_upload_many(ctx, 2 * (int)count, ptr, n, out);
            else ctx->stats.add("upload_prefetched", 1);
        } catch (const Err &) { if (count == 1) throw; group_ok = false; }
        ctx->stats.add("t_upload_take", secs_since(t0));
        t0 = Clock::now();
        if (next_count) cloud_prefetch(ctx, 2 * (int)next_count, nptr, nn);
        ctx->stats.add("t_upload_submit", secs_since(t0));
    }
    const int zero[PLADE_GROUP_MAX] = {};
    if (group_ok) {
        try { register_group_parts(ctx, (int)count, ct, cs, zero, zero, true, T16, status); return PLADE_OK; }
        catch (const Err &) { if (count == 1) throw; }
    }
    register_pairs_one_by_one(ctx, (int)count, ct, cs, T16, status, [&](int i) {
        CloudDev *o[2] = {out[2 * i], out[2 * i + 1]};
        cloud_upload_many(ctx, 2, ptr + 2 * i, n + 2 * i, o);
    });
    return PLADE_OK;
}
}  // namespace

// Batch mode (code/PLADE/main.cpp:97-158 is a loop over pairs): plade_registration of THIS pair, with the upload of the
// NEXT pair started first on the prefetch stream, so that its PCIe transfer runs under this pair's kernels.
extern "C" int plade_registration_next(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t, const float *src_pos_nrm,
                                       uint32_t n_s, const float *next_tgt_pos_nrm, uint32_t next_n_t,
                                       const float *next_src_pos_nrm, uint32_t next_n_s, float *T16) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(tgt_pos_nrm && src_pos_nrm && T16 && n_t && n_s, PLADE_EINVAL, "plade_registration_next: bad argument");
        const bool have_next = next_tgt_pos_nrm && next_src_pos_nrm && next_n_t && next_n_s;
        int32_t status = PLADE_OK;
        registration_batch(ctx, 1, &tgt_pos_nrm, &n_t, &src_pos_nrm, &n_s, have_next ? 1u : 0u, &next_tgt_pos_nrm, &next_n_t,
                           &next_src_pos_nrm, &next_n_s, T16, &status);
        return status;
    });
}

// Batch mode, `count` (<= PLADE_GROUP_MAX) pairs of the list per call: see include/plade_hip.h.
extern "C" int plade_registration_pairs(plade_ctx *ctx, uint32_t count, const float *const *tgt_pos_nrm, const uint32_t *n_t,
                                        const float *const *src_pos_nrm, const uint32_t *n_s, uint32_t next_count,
                                        const float *const *next_tgt_pos_nrm, const uint32_t *next_n_t,
                                        const float *const *next_src_pos_nrm, const uint32_t *next_n_s, float *T16, int32_t *status) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(count >= 1 && count <= PLADE_GROUP_MAX && tgt_pos_nrm && src_pos_nrm && n_t && n_s && T16 && status, PLADE_EINVAL,
                      "plade_registration_pairs: bad argument");
        for (uint32_t i = 0; i < count; ++i)
            PLADE_REQUIRE(tgt_pos_nrm[i] && src_pos_nrm[i] && n_t[i] && n_s[i], PLADE_EINVAL, "plade_registration_pairs: empty cloud");
        if (next_count > PLADE_GROUP_MAX || !next_tgt_pos_nrm || !next_src_pos_nrm || !next_n_t || !next_n_s) next_count = 0;
        for (uint32_t i = 0; i < next_count; ++i)
            if (!next_tgt_pos_nrm[i] || !next_src_pos_nrm[i] || !next_n_t[i] || !next_n_s[i]) next_count = 0;
        return registration_batch(ctx, count, tgt_pos_nrm, n_t, src_pos_nrm, n_s, next_count, next_tgt_pos_nrm, next_n_t, next_src_pos_nrm,
                                  next_n_s, T16, status);
    });
}

extern "C" int plade_registration_pairs_dev(plade_ctx *ctx, uint32_t count, plade_cloud *const *tgt, plade_cloud *const *src, float *T16,
                                            int32_t *status) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(count >= 1 && count <= PLADE_GROUP_MAX && tgt && src && T16 && status, PLADE_EINVAL, "plade_registration_pairs_dev: bad argument");
        const CloudDev *ct[PLADE_GROUP_MAX] = {}, *cs[PLADE_GROUP_MAX] = {};
        for (uint32_t i = 0; i < count; ++i) {
            PLADE_REQUIRE(tgt[i] && src[i], PLADE_EINVAL, "plade_registration_pairs_dev: null cloud");
            ct[i] = &tgt[i]->dev; cs[i] = &src[i]->dev;
        }
        ctx->stats.clear();
        ctx->dump.clear();
        ctx->last_error.clear();
        cloud_drop_prefetch(ctx);
        const int zero[PLADE_GROUP_MAX] = {};
        try { register_group_parts(ctx, (int)count, ct, cs, zero, zero, true, T16, status); }
        catch (const Err &) {
            if (count == 1) throw;
            register_pairs_one_by_one(ctx, (int)count, ct, cs, T16, status, [](int) {});   // see registration_batch
        }
        return PLADE_OK;
    });
}

extern "C" int plade_sort_segments(plade_ctx *ctx, const uint32_t *keys, const uint32_t *vals, const uint32_t *seg_off, uint32_t nseg, int bits,
                                   uint32_t *keys_out, uint32_t *vals_out) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(seg_off && nseg >= 1 && nseg <= 16 && bits >= 1 && bits <= 32 && seg_off[0] == 0, PLADE_EINVAL,
                      "plade_sort_segments: 1..16 segments starting at 0, 1 <= bits <= 32");
        for (uint32_t q = 0; q < nseg; ++q) PLADE_REQUIRE(seg_off[q] <= seg_off[q + 1], PLADE_EINVAL, "plade_sort_segments: offsets must ascend");
        const uint32_t n = seg_off[nseg];
        PLADE_REQUIRE(!n || (keys && vals && keys_out && vals_out), PLADE_EINVAL, "plade_sort_segments: null argument");
        if (!n) return PLADE_OK;
        HIP_TRY(hipSetDevice(ctx->device));
        DBuf<uint32_t> ki, ko, vi, vo;
        ki.ensure(n); ko.ensure(n); vi.ensure(n); vo.ensure(n);
        ctx->h2d(ki.p, keys, (size_t)n * 4);
        ctx->h2d(vi.p, vals, (size_t)n * 4);
        radix_sort_segments_u32(ctx, ki.p, ko.p, vi.p, vo.p, seg_off, (int)nseg, bits);
        ctx->d2h(keys_out, ko.p, (size_t)n * 4);
        ctx->d2h(vals_out, vo.p, (size_t)n * 4);
        ctx->sync();
        return PLADE_OK;
    });
}

// The context that carried pair `index` of the last group call (0: ctx itself): its stats, dump and last error are read with
// the ordinary entry points.  Borrowed: it lives and dies with ctx.
extern "C" plade_ctx *plade_pair_ctx(plade_ctx *ctx, uint32_t index) {
    if (!ctx) return nullptr;
    return index == 0 ? ctx : (index < PLADE_GROUP_MAX ? ctx->peers[index - 1] : nullptr);
}

extern "C" int plade_registration_minsupport(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t,
                                             const float *src_pos_nrm, uint32_t n_s, int32_t min_support_t,
                                             int32_t min_support_s, float *T16) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(tgt_pos_nrm && src_pos_nrm && T16 && n_t && n_s && min_support_t > 0 && min_support_s > 0, PLADE_EINVAL,
                      "plade_registration_minsupport: bad argument");
        ctx->stats.clear();
        ctx->dump.clear();
        ctx->last_error.clear();
        cloud_drop_prefetch(ctx);
        CloudDev &tgt = ctx->up_tgt, &src = ctx->up_src;
        cloud_upload_pair(ctx, tgt_pos_nrm, n_t, tgt, src_pos_nrm, n_s, src);
        return register_clouds(ctx, tgt, src, min_support_t, min_support_s, false, T16);
    });
}

extern "C" int plade_plane_component(plade_ctx *ctx, const float *pos_nrm, uint32_t n, const float *normal, const float *point,
                                     const int32_t *idx, uint32_t m, float bitmap_eps, int closing_filter, float w_eps,
                                     int32_t *kept_out, uint32_t *n_kept, float *fit_out, double *wscore_out) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(pos_nrm && normal && point && (idx || !m) && n_kept && (kept_out || !m), PLADE_EINVAL,
                      "plade_plane_component: null argument");
        {
            std::vector<uint8_t> seen(n, 0);
            for (uint32_t i = 0; i < m; ++i) {
                PLADE_REQUIRE(idx[i] >= 0 && (uint32_t)idx[i] < n && !seen[idx[i]], PLADE_EINVAL,
                              "plade_plane_component: indices must be distinct and inside the cloud");
                seen[idx[i]] = 1;
            }
        }
        CloudDev cloud;
        cloud_upload(ctx, pos_nrm, n, cloud);
        if (!ctx->ransac_work) ctx->ransac_work = ransac_work_create();
        ComponentOut out;
        plane_component(ctx, *ctx->ransac_work, cloud, normal, point, idx, m, bitmap_eps, closing_filter != 0, w_eps, out);
        PLADE_REQUIRE(out.err == 0, PLADE_ELIMIT, "plane component: bitmap too large");
        *n_kept = (uint32_t)out.kept.size();
        if (!out.kept.empty()) memcpy(kept_out, out.kept.data(), 4 * out.kept.size());
        if (fit_out) memcpy(fit_out, out.fit, sizeof(out.fit));
        if (wscore_out) *wscore_out = out.wscore;
        return PLADE_OK;
    });
}

extern "C" int plade_sort_pairs(plade_ctx *ctx, const void *keys, const uint32_t *vals, uint32_t n, int key_bytes, int bits,
                                void *keys_out, uint32_t *vals_out) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE((key_bytes == 4 || key_bytes == 8) && bits >= 1 && bits <= 8 * key_bytes, PLADE_EINVAL,
                      "plade_sort_pairs: key_bytes must be 4 or 8 and 1 <= bits <= 8 * key_bytes");
        PLADE_REQUIRE(!n || (keys && vals && keys_out && vals_out), PLADE_EINVAL, "plade_sort_pairs: null argument");
        if (!n) return PLADE_OK;
        HIP_TRY(hipSetDevice(ctx->device));
        DBuf<char> ki, ko;
        DBuf<uint32_t> vi, vo;
        ki.ensure((size_t)n * key_bytes); ko.ensure((size_t)n * key_bytes); vi.ensure(n); vo.ensure(n);
        ctx->h2d(ki.p, keys, (size_t)n * key_bytes);
        ctx->h2d(vi.p, vals, (size_t)n * 4);
        if (key_bytes == 4) sort_pairs_u32(ctx, (const uint32_t *)ki.p, (uint32_t *)ko.p, vi.p, vo.p, n, bits);
        else sort_pairs_u64(ctx, (const uint64_t *)ki.p, (uint64_t *)ko.p, vi.p, vo.p, n, bits);
        ctx->d2h(keys_out, ko.p, (size_t)n * key_bytes);
        ctx->d2h(vals_out, vo.p, (size_t)n * 4);
        ctx->sync();
        return PLADE_OK;
    });
}

// Test seam of the device -> host hand-over (ctx.h: d2h / sync): `n_ranges` device arrays of `words` 32-bit words each,
// filled with a pattern, are read back through ONE sync(); *mismatches = words that did not arrive as written.
extern "C" int plade_selftest_readback(plade_ctx *ctx, uint32_t n_ranges, uint32_t words, uint32_t *mismatches) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(mismatches && n_ranges >= 1 && n_ranges <= 64 && words >= 1 && words <= (1u << 18), PLADE_EINVAL,
                      "plade_selftest_readback: 1..64 ranges of 1..2^18 words");
        HIP_TRY(hipSetDevice(ctx->device));
        std::vector<DBuf<uint32_t>> dev(n_ranges);
        std::vector<std::vector<uint32_t>> want(n_ranges), got(n_ranges);
        for (uint32_t r = 0; r < n_ranges; ++r) {
            const uint32_t w = words - (r % 3);            // ragged sizes
            want[r].resize(std::max(w, 1u));
            for (uint32_t i = 0; i < want[r].size(); ++i) want[r][i] = 0x9E3779B9u * (i + 1) + 0x7F4A7C15u * (r + 1);
            got[r].assign(want[r].size(), 0xdeadbeefu);
            dev[r].ensure(want[r].size() + 4);
            HIP_TRY(hipMemcpyAsync(dev[r].p, want[r].data(), 4 * want[r].size(), hipMemcpyHostToDevice, ctx->stream));
        }
        HIP_TRY(hipStreamSynchronize(ctx->stream));        // the pageable sources are done with
        for (uint32_t r = 0; r < n_ranges; ++r) ctx->d2h(got[r].data(), dev[r].p, 4 * got[r].size());
        ctx->sync();
        uint32_t bad = 0;
        for (uint32_t r = 0; r < n_ranges; ++r)
            for (size_t i = 0; i < want[r].size(); ++i) bad += got[r][i] != want[r][i];
        *mismatches = bad;
        return PLADE_OK;
    });
}

extern "C" int plade_kernel_time(plade_ctx *ctx, const char *which, int iters, double *avg_seconds,
                                 double *algorithmic_bytes_per_launch) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(which && avg_seconds && algorithmic_bytes_per_launch && iters > 0, PLADE_EINVAL, "plade_kernel_time: bad argument");
        // per-kernel figures of the LAST registration run with params.dump & 2 (HIP events recorded on
        // the ctx stream around every launch of the named kernel)
        const std::string base = std::string("k_") + which;
        const double s = ctx_stat(ctx, (base + "_seconds").c_str()), nl = ctx_stat(ctx, (base + "_launches").c_str()),
                     b = ctx_stat(ctx, (base + "_bytes").c_str());
        PLADE_REQUIRE(nl > 0, PLADE_EINVAL, "plade_kernel_time: no profiled launches of that kernel (run a registration with dump & 2)");
        *avg_seconds = s / nl;
        *algorithmic_bytes_per_launch = b / nl;
        return PLADE_OK;
    });
}
