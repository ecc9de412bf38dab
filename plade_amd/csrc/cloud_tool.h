// plade_amd/csrc/cloud_tool.h -- the host frame the cloud tools share (host code only, no kernel): the parameter intake, the tail
// of the tools that end in a keep mask, and the resident result.  The work slots are in work_slot.h, the radius test (radius_ok)
// next to radius_cell in grid_walk.h.
#pragma once
#include "ctx.h"
#include "prims.h"
#include "stages.h"
#include <functional>
#include <memory>

namespace plade {

// the caller's parameters, or the tool's defaults where it passed none
template <class P, class D>
P params_or_default(const P *params, D defaults) {
    P p;
    if (params) p = *params; else defaults(&p);
    return p;
}

// ---- the keep tail (k_outliers, k_components, k_subsample) ------------------------------------------------------------------------
// What a tool that ends in a keep mask holds for it.  Its own kernel writes keep (n bytes, 0 / 1) and flags (the same as words); the
// tail gives the ascending kept list and the kept rows.
struct KeepWork {
    DBuf<uint32_t> flags, pos, kept;
    DBuf<uint8_t> keep;
    DBuf<float> in, out;             // the host-pointer entry point's device copies (grow-only)
};
using KeepRows = std::function<float *(uint32_t)>;   // where `kept` rows go (not asked when nothing is kept)

// The flags of n points, the zero behind them queued: compact_flags scans n + 1 entries.  Called where the tool sizes its buffers,
// before its kernels; they write flags[0 .. n) only, so the zero also serves a second compaction of the same call (k_components).
inline uint32_t *keep_flags(plade_ctx *ctx, KeepWork &K, uint32_t n) {
    uint32_t *d_flags = K.flags.ensure((size_t)n + 1);
    ctx->fill_async(d_flags + n, 0, 4);
    return d_flags;
}
// compact + gather: the kept list of the flags (waits for the count), the kept rows of d_rows into dst(total).  Returns the count.
inline uint32_t keep_compact_gather(plade_ctx *ctx, KeepWork &K, const float *d_rows, uint32_t n, uint32_t stride, const KeepRows &dst) {
    const uint32_t total = compact_flags(ctx, K.flags.p, n, K.pos, K.kept);
    if (total) gather_rows(ctx, d_rows, stride, K.kept.p, total, dst(total));
    return total;
}
// the two destinations: the host form's K.out, and the rows of a resident cloud shaped for what is kept
inline KeepRows keep_rows_host(KeepWork &K, uint32_t stride) {
    return [&K, stride](uint32_t kept) { return K.out.ensure((size_t)kept * stride + 4); };
}
inline KeepRows keep_rows_cloud(CloudDev &c) {
    return [&c](uint32_t kept) { cloud_shape(c, kept); return c.aos.p; };
}
// the copies out, each where its pointer is given (rows_out: the host form's alone); queued, the caller waits
inline void keep_copy_out(plade_ctx *ctx, const KeepWork &K, uint32_t n, uint32_t total, uint32_t stride, uint8_t *keep_out,
                          uint32_t *kept_index_out, float *rows_out) {
    if (keep_out) HIP_TRY(hipMemcpyAsync(keep_out, K.keep.p, n, hipMemcpyDeviceToHost, ctx->stream));
    if (kept_index_out && total) HIP_TRY(hipMemcpyAsync(kept_index_out, K.kept.p, (size_t)total * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (rows_out && total) HIP_TRY(hipMemcpyAsync(rows_out, K.out.p, (size_t)total * stride * 4, hipMemcpyDeviceToHost, ctx->stream));
}

// ---- a resident result ------------------------------------------------------------------------------------------------------------
// body(c) fills the rows of a fresh cloud (cloud_shape, its kernels, its copies out and its waits); then the SoA planes and the
// bounding box of the resident cloud, as plade_cloud_upload, and the cloud goes to *out.  Whatever is thrown on the way deletes the
// cloud and leaves *out as the entry point set it before its parameter checks: NULL.
template <class F>
void resident_result(plade_ctx *ctx, plade_cloud **out, F body) {
    std::unique_ptr<plade_cloud> c(new plade_cloud);
    body(c->dev);
    cloud_finish_device(ctx, c->dev);
    *out = c.release();
}
// what: the entry point and its subject, "plade_x_dev: the filter"
inline void require_kept(uint32_t total, const char *what) {
    PLADE_REQUIRE(total >= 1, PLADE_EFAIL, std::string(what) + " keeps no point (a resident cloud cannot be empty)");
}

}  // namespace plade
