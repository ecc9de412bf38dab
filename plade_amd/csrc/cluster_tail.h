// plade_amd/csrc/cluster_tail.h -- what the two clustering tools share (k_components.hip: every point is a vertex; k_dbscan.hip:
// only the core points are): the lock-free union-find their link kernels hook into, and the tail from the parents to the labels,
// the sizes, the selection by size and the keep flags.  The device functions are here; the tail's kernels and its host sequence
// exist once, in k_components.hip.
#pragma once
#include "cloud_tool.h"

namespace plade {

constexpr uint32_t NO_POINT = 0xffffffffu;   // attach[i] / root[i] of a point that belongs to no cluster (n <= 2^32 - 1: no index)

// ---- the union-find: parent[] is uint32 by original index, parent[i] = i at the start (cluster_init_parents) ----
// An edge unites its two ends by min-hooking: find both roots, atomicMin(&parent[hi], lo) at agent scope with hi > lo; a returned
// value other than hi means somebody hooked hi first, and the union goes on with (that value, lo).  Parents only ever decrease:
// every loop ends, no lane waits for another, and at the end every root is the smallest original index of its tree -- whatever the
// order of the unions.  parent[] is read with relaxed agent-scope atomic loads; a stale value costs a round, never a link, because
// the atomicMin's return value decides.
__device__ __forceinline__ uint32_t parent_of(const uint32_t *parent, uint32_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a, b: any two ancestors (or the points themselves) of the two ends
__device__ __forceinline__ void unite(uint32_t *parent, uint32_t a, uint32_t b) {
    for (;;) {
        for (uint32_t p = parent_of(parent, a); p != a; p = parent_of(parent, a)) a = p;
        for (uint32_t p = parent_of(parent, b); p != b; p = parent_of(parent, b)) b = p;
        if (a == b) return;
        const uint32_t hi = max(a, b), lo = min(a, b);
        const uint32_t old = __hip_atomic_fetch_min(parent + hi, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == hi) return;
        a = old; b = lo;             // hi had been hooked to `old` already (parent[hi] is now min(old, lo)): old and lo remain to be united
    }
}

// ---- the tail ----
// What it holds on top of the keep tail's: label (n int32, -1 = in no cluster), size (`clusters` words, room for n), keep and flags.
struct ClusterWork : KeepWork {
    DBuf<uint32_t> root, root_pos, root_list, size, count, sort_val, sort_val2;
    DBuf<unsigned long long> sort_key, sort_key2;
    DBuf<int32_t> label;
    DBuf<uint8_t> cluster_kept;
    uint32_t h_count[2] = {0, 0};    // the largest size, the kept clusters (valid after the caller's next wait)
    uint32_t clusters = 0;
};

// parent[i] = i, queued
void cluster_init_parents(plade_ctx *ctx, uint32_t *d_parent, uint32_t n);

// From the parents of a finished link kernel to label, size, keep and the kept points' flags in W, and W.clusters (waits for that
// count once); the copy of h_count is queued.  d_attach = nullptr: every point is a vertex of the forest (the components).
// Otherwise point i starts its walk at attach[i] -- itself for a vertex, the vertex a border point hangs on -- and NO_POINT means
// "in no cluster": label -1, counted in no size, never kept.  The ids run in ascending order of a cluster's smallest vertex.
// Selection: cluster c passes when min_size <= size[c] and (max_size = 0 or size[c] <= max_size); keep_largest = m > 0 keeps only
// the m passing ones that come first in the order (size descending, id ascending).  The caller goes on with keep_compact_gather.
void cluster_label_select(plade_ctx *ctx, ClusterWork &W, uint32_t n, const uint32_t *d_parent, const uint32_t *d_attach, uint32_t min_size,
                          uint32_t max_size, uint32_t keep_largest);

}  // namespace plade
