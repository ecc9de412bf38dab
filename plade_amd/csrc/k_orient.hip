// plade_amd/csrc/k_orient.hip -- consistent normal orientation by a minimum spanning forest on gfx950 (semantics: orient.h).
//
// Layout
//   grid     the dense row index of TargetGrid with the radius filter's cell, radius_cell(radius) of grid_walk.h (the rule of
//            DESIGN.md section 10): the 27-cell block around a point holds everything closer than radius.  Where the grid caps its
//            cell count the cell grows and the block holds more: the walk stays exact.
//   state    everything per point lives in the grid's SORTED order, read alongside sorted[s]; a component is named by the sorted
//            position of its root.  snap[s] = root << 1 | parity: the flattened snapshot at the end of the previous round (the root
//            IS a root, the parity is that of s relative to it; INVALID for a point that is no vertex).  link[r] = the hook word of
//            a position that is or was a root: itself << 1 while it is one, other_root << 1 | parity once it has been hooked.
//   round    Boruvka, four launches, none of which waits on another workgroup (no spin on a word, no grid barrier, no persistent
//            kernel):
//            k_or_pick    one lane per active position (round 1: all n) walks the nine runs of its block and keeps the smallest
//                         (key32, min(i,j), max(i,j)) among its neighbours whose snapshot names another root; it records the
//                         triple with the neighbour's position and s_ij, and joins a wave-aggregated 64-bit atomicMin of
//                         key32 << 32 | min(i,j) on best[root].  A lane that saw a foreign root goes to the next round's active
//                         list through fail_append (a lane that saw none never will: components only grow).  The list says who
//                         gets a lane; no result depends on it or on its order.
//            k_or_pick_hi the lanes whose record matches best[root]: 32-bit atomicMin of max(i,j) on best_hi[root].
//            k_or_hook    the one lane whose whole triple matches its root's (the edge has one end in the component, and that end's
//                         own minimum is the edge) hooks the root: if the other root picked the same edge and this root is the
//                         smaller position, it stays root; otherwise link[root] = other_root << 1 | (parity_i ^ parity_j ^ s_ij).
//                         A hook reads the snapshot, the records and best / best_hi -- all complete before the launch -- and
//                         writes one link word that no lane of the launch reads.  Under a total order the picked edges form no
//                         cycle but that mutual pair.  The hooks and the sum of their key32 are counted by integer atomics.
//            k_or_flatten every point starts at its snapshot's root and follows link[] to a root, composing the parities, and
//                         writes its new snapshot.  A position hooked in this round then replaces its own link word by the
//                         flattened one (one writer per word: position s alone writes link[s]); a lane that meets either the old
//                         or the new word reads a true (ancestor, parity) pair, so the walk ends at the same root with the same
//                         parity and waits for nobody.  The walk is bounded by n steps; the bound raises the error word.
//            The atomic minima and integer sums are order-free: every round's result is a function of the previous snapshot.
//   host     after each round the hooks, the next active count and the error word come back through the context's page-locked
//            read-back (d2h + sync); the loop stops at 0 hooks.  Each round at least halves the components that still have a
//            neighbour: at most floor(log2 n) + 1 rounds; the guard stops at 40.
//   anchor   k_or_tally (per component, wave-aggregated: the smallest original index; VOTE: the two counts; EXTREME: atomicMax of
//            the ordered fp64 bits of e), k_or_extreme_index (EXTREME: atomicMin of the index among the equals), k_or_anchor (the
//            anchor's lane writes the component's toggle; flags[i] = i is its component's smallest index), compact_flags (the ids,
//            the rule of k_components.hip: the exclusive position of a component's smallest index), k_or_scatter (rows, flip and
//            label in the original order; the flipped and the unoriented by ballots).
#include "orient.h"
#include "cloud_tool.h"
#include "grid_walk.h"
#include "prims.h"
#include "stages.h"
#include "voxel.h"

namespace plade {

namespace {

constexpr int PICK_TPB = 256, ROW_TPB = 256;
constexpr uint32_t INVALID = 0xffffffffu, NONE = 0xffffffffu;
constexpr uint32_t KEY_TOP = 0x7F800000u;
constexpr uint32_t MAX_ROUNDS = 40;
constexpr float NORMAL_MAX = 1e18f;
// the counter words: the next active count and the hooks (zeroed before every round), then the error word, the unoriented and the
// flipped points; behind them (8-byte aligned) the sum of key32 over the hooks
enum { C_ACTIVE = 0, C_HOOKS = 1, C_ERROR = 2, C_UNORIENTED = 3, C_FLIPPED = 4, C_KEYSUM = 6, C_WORDS = 8 };

struct RoundArgs {
    GridView g;
    uint32_t n, n_active;            // points; lanes of this launch
    const uint32_t *active;          // their sorted positions; nullptr: 0 .. n_active - 1 (round 1)
    float r2;                        // (float)radius * (float)radius
    const float4 *nrm;               // the normals by sorted position
    uint32_t *snap, *link;           // by sorted position
    u64 *best;                       // by root: min key32 << 32 | min(i,j)
    uint32_t *best_hi;               // by root: min max(i,j) among the lanes that matched best
    u64 *rec_key;                    // by sorted position: the lane's own pick, EMPTY: none
    uint32_t *rec_hi, *rec_js;       // max(i,j); neighbour's sorted position << 1 | s_ij
    uint32_t *next, *cnt;            // the next round's active list; the counter words
};

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

// The lanes of a wave with `valid` in groups of equal `r`: f(member, leader) once per group, called by ALL lanes (wave-uniform)
template <class F>
__device__ __forceinline__ void by_root(bool valid, uint32_t r, F &&f) {
    u64 todo = __ballot(valid);
    while (todo) {                   // (wave-uniform)
        const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
        const uint32_t lr = (uint32_t)__builtin_amdgcn_readlane((int)r, (int)leader);
        const u64 same = __ballot(valid && r == lr);
        f(valid && r == lr, lane_id() == leader, same);
        todo &= ~same;
    }
}

__device__ __forceinline__ u64 wave_max(u64 v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const u64 w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}
__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ bool normal_valid(float x, float y, float z) {
    return fabsf(x) <= NORMAL_MAX && fabsf(y) <= NORMAL_MAX && fabsf(z) <= NORMAL_MAX;   // (false for NaN and inf)
}

// the normals into sorted order, the first snapshot (every valid point its own root), the hook words and the empty minima
__global__ __launch_bounds__(ROW_TPB) void k_or_init(const float4 *__restrict__ sorted, const float *__restrict__ rows, uint32_t n,
                                                     float4 *__restrict__ nrm, uint32_t *__restrict__ snap, uint32_t *__restrict__ link,
                                                     u64 *__restrict__ best, uint32_t *__restrict__ best_hi) {
    const uint32_t s = blockIdx.x * ROW_TPB + threadIdx.x;
    if (s >= n) return;
    const float *row = rows + (size_t)__float_as_uint(sorted[s].w) * 6;
    const float x = row[3], y = row[4], z = row[5];
    nrm[s] = make_float4(x, y, z, 0.f);
    snap[s] = normal_valid(x, y, z) ? s << 1 : INVALID;
    link[s] = s << 1;
    best[s] = EMPTY;
    best_hi[s] = NONE;
}

__global__ __launch_bounds__(PICK_TPB) void k_or_pick(const RoundArgs a) {
    const uint32_t t = blockIdx.x * PICK_TPB + threadIdx.x;
    uint32_t s = 0, root = 0;
    u64 mine = EMPTY;
    if (t < a.n_active) {
        s = a.active ? a.active[t] : t;
        const uint32_t w = a.snap[s];
        if (w != INVALID) {
            root = w >> 1;
            const float4 q4 = a.g.sorted[s], nq = a.nrm[s];
            const f3 q(q4.x, q4.y, q4.z);
            const uint32_t self = __float_as_uint(q4.w);
            int cx, cy, cz;
            cell_of(a.g, q, cx, cy, cz);
            uint32_t mine_hi = NONE, mine_js = 0;
            for_block27(a.g, cx, cy, cz, [&](uint32_t j0, uint32_t j1) {
                for (uint32_t j = j0; j < j1; ++j) {
                    if (j == s) continue;
                    const float4 p = a.g.sorted[j];
                    if (!(flann_d2(q, f3(p.x, p.y, p.z)) < a.r2)) continue;
                    const uint32_t wj = a.snap[j];
                    if (wj == INVALID || (wj >> 1) == root) continue;
                    const float4 np = a.nrm[j];
                    const float dot = (nq.x * np.x + nq.y * np.y) + nq.z * np.z;
                    const uint32_t key32 = KEY_TOP - __float_as_uint(fabsf(dot));
                    const uint32_t other = __float_as_uint(p.w);
                    const u64 k = ((u64)key32 << 32) | (u64)min(self, other);
                    const uint32_t hi = max(self, other);
                    if (k < mine || (k == mine && hi < mine_hi)) {
                        mine = k; mine_hi = hi;
                        mine_js = (j << 1) | (dot < 0.0f ? 1u : 0u);
                    }
                }
            });
            a.rec_key[s] = mine;
            a.rec_hi[s] = mine_hi;
            a.rec_js[s] = mine_js;
        } else
            a.rec_key[s] = EMPTY;
    }
    const bool has = mine != EMPTY;
    fail_append(has, s, a.next, a.cnt + C_ACTIVE);   // (all lanes)
    by_root(has, root, [&](bool member, bool leader, u64) {
        const u64 m = wave_min(member ? mine : EMPTY);
        if (leader) __hip_atomic_fetch_min(a.best + root, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    });
}

__global__ __launch_bounds__(PICK_TPB) void k_or_pick_hi(const RoundArgs a) {
    const uint32_t t = blockIdx.x * PICK_TPB + threadIdx.x;
    if (t >= a.n_active) return;
    const uint32_t s = a.active ? a.active[t] : t;
    const u64 mine = a.rec_key[s];
    if (mine == EMPTY) return;
    const uint32_t root = a.snap[s] >> 1;
    if (a.best[root] == mine) __hip_atomic_fetch_min(a.best_hi + root, a.rec_hi[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(PICK_TPB) void k_or_hook(const RoundArgs a) {
    const uint32_t t = blockIdx.x * PICK_TPB + threadIdx.x;
    bool hooked = false;
    u64 key = 0;
    if (t < a.n_active) {
        const uint32_t s = a.active ? a.active[t] : t;
        const u64 mine = a.rec_key[s];
        if (mine != EMPTY) {
            const uint32_t w = a.snap[s], root = w >> 1, hi = a.rec_hi[s];
            if (a.best[root] == mine && a.best_hi[root] == hi) {          // this lane owns its root's pick
                const uint32_t js = a.rec_js[s], wj = a.snap[js >> 1], other = wj >> 1;
                const bool mutual = a.best[other] == mine && a.best_hi[other] == hi;
                if (!(mutual && root < other)) {
                    __hip_atomic_store(a.link + root, (other << 1) | ((w ^ wj ^ js) & 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    hooked = true;
                    key = mine >> 32;
                }
            }
        }
    }
    const u64 mask = __ballot(hooked);
    if (mask) {                      // (wave-uniform)
        const u64 sum = wave_sum(key);
        if (lane_id() == 0) {
            atomicAdd(a.cnt + C_HOOKS, (uint32_t)__popcll(mask));
            atomicAdd(reinterpret_cast<u64 *>(a.cnt + C_KEYSUM), sum);
        }
    }
}

__global__ __launch_bounds__(ROW_TPB) void k_or_flatten(const RoundArgs a) {
    const uint32_t s = blockIdx.x * ROW_TPB + threadIdx.x;
    if (s >= a.n) return;
    a.best[s] = EMPTY;               // (the minima of the next round)
    a.best_hi[s] = NONE;
    const uint32_t w = a.snap[s];
    if (w == INVALID) return;
    uint32_t r = w >> 1, p = w & 1u;
    uint32_t x = __hip_atomic_load(a.link + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), steps = 0;
    while ((x >> 1) != r) {
        if (++steps > a.n) {         // (cannot happen: the hooks form no cycle)
            atomicOr(a.cnt + C_ERROR, 1u);
            return;
        }
        p ^= x & 1u;
        r = x >> 1;
        x = __hip_atomic_load(a.link + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    a.snap[s] = (r << 1) | p;
    if ((w >> 1) == s && r != s) __hip_atomic_store(a.link + s, (r << 1) | p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct FinishArgs {
    const float4 *sorted, *nrm;
    const float *rows;               // the input, n x 6
    const uint32_t *snap;
    uint32_t n;
    int mode, inward;
    double v[3];                     // the viewpoint (VOTE) or the direction (EXTREME)
    uint32_t *min_idx;               // by root: the component's smallest original index
    uint32_t *votes;                 // by root: 2 r = towards, 2 r + 1 = away, in the root's frame (VOTE)
    u64 *e_max;                      // by root: the largest ordered e (EXTREME)
    uint32_t *e_idx;                 // by root: the smallest original index among the points with that e (EXTREME)
    uint32_t *toggle;                // by root
    uint32_t *flags;                 // by original index: the point is its component's smallest index
    const uint32_t *id;              // by original index: compact_flags' exclusive positions
    float *out;                      // n x 6
    uint8_t *flip;
    int32_t *label;
    uint32_t *cnt;
};

// ((double)a0 * v0 + (double)a1 * v1) + (double)a2 * v2
__device__ __forceinline__ double along(const double v[3], float a0, float a1, float a2) {
    return ((double)a0 * v[0] + (double)a1 * v[1]) + (double)a2 * v[2];
}
// the bits of a finite double in an order that unsigned comparison follows; -0 counts as +0
__device__ __forceinline__ u64 ordered_bits(double e) {
    if (e == 0.0) e = 0.0;
    const u64 b = (u64)__double_as_longlong(e);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ u64 extreme_of(const FinishArgs &a, uint32_t s) {
    const float4 q = a.sorted[s];
    return ordered_bits(along(a.v, q.x, q.y, q.z));
}

__global__ __launch_bounds__(ROW_TPB) void k_or_tally(const FinishArgs a) {
    const uint32_t s = blockIdx.x * ROW_TPB + threadIdx.x;
    uint32_t w = INVALID;
    if (s < a.n) w = a.snap[s];
    const bool valid = w != INVALID;
    const uint32_t root = w >> 1;
    uint32_t orig = NONE;
    bool towards = false, away = false;
    u64 e = 0;
    if (valid) {
        const float4 q = a.sorted[s], m = a.nrm[s];
        orig = __float_as_uint(q.w);
        if (a.mode == PLADE_ORIENT_VOTE) {
            const double sg = (w & 1u) ? -1.0 : 1.0;     // the normal as the root's frame has it (a sign change is exact)
            const double nx = sg * (double)m.x, ny = sg * (double)m.y, nz = sg * (double)m.z;
            const double tt = (a.v[0] - (double)q.x) * nx + (a.v[1] - (double)q.y) * ny + (a.v[2] - (double)q.z) * nz;
            towards = tt > 0.0; away = tt < 0.0;
        } else
            e = extreme_of(a, s);
    }
    by_root(valid, root, [&](bool member, bool leader, u64) {
        const uint32_t lo = (uint32_t)wave_min(member ? (u64)orig : EMPTY);
        const u64 tw = __ballot(member && towards), aw = __ballot(member && away);
        const u64 em = wave_max(member ? e : 0ull);
        if (leader) {
            atomicMin(a.min_idx + root, lo);
            if (a.mode == PLADE_ORIENT_VOTE) {
                if (tw) atomicAdd(a.votes + 2 * (size_t)root, (uint32_t)__popcll(tw));
                if (aw) atomicAdd(a.votes + 2 * (size_t)root + 1, (uint32_t)__popcll(aw));
            } else
                __hip_atomic_fetch_max(a.e_max + root, em, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    });
}

__global__ __launch_bounds__(ROW_TPB) void k_or_extreme_index(const FinishArgs a) {
    const uint32_t s = blockIdx.x * ROW_TPB + threadIdx.x;
    if (s >= a.n) return;
    const uint32_t w = a.snap[s];
    if (w == INVALID) return;
    if (extreme_of(a, s) == a.e_max[w >> 1]) atomicMin(a.e_idx + (w >> 1), __float_as_uint(a.sorted[s].w));
}

__global__ __launch_bounds__(ROW_TPB) void k_or_anchor(const FinishArgs a) {
    const uint32_t s = blockIdx.x * ROW_TPB + threadIdx.x;
    if (s >= a.n) return;
    const uint32_t w = a.snap[s], orig = __float_as_uint(a.sorted[s].w);
    if (w == INVALID) { a.flags[orig] = 0u; return; }
    const uint32_t root = w >> 1, p = w & 1u;
    a.flags[orig] = orig == a.min_idx[root] ? 1u : 0u;
    if (a.mode == PLADE_ORIENT_VOTE) {
        if (orig != a.min_idx[root]) return;
        // the counts are in the root's frame; anchored at this point (flip 0) they swap when its parity is 1
        const uint32_t t0 = a.votes[2 * (size_t)root], t1 = a.votes[2 * (size_t)root + 1];
        const uint32_t towards = p ? t1 : t0, away = p ? t0 : t1;
        a.toggle[root] = p ^ (away > towards ? 1u : 0u) ^ (uint32_t)a.inward;
    } else {
        if (orig != a.e_idx[root]) return;
        const float4 m = a.nrm[s];
        a.toggle[root] = p ^ (along(a.v, m.x, m.y, m.z) < 0.0 ? 1u : 0u) ^ (uint32_t)a.inward;
    }
}

__global__ __launch_bounds__(ROW_TPB) void k_or_scatter(const FinishArgs a) {
    const uint32_t s = blockIdx.x * ROW_TPB + threadIdx.x;
    bool flipped = false, unoriented = false;
    if (s < a.n) {
        const uint32_t w = a.snap[s], orig = __float_as_uint(a.sorted[s].w);
        uint32_t f = 0;
        int32_t label = -1;
        if (w != INVALID) {
            f = (w & 1u) ^ a.toggle[w >> 1];
            label = (int32_t)a.id[a.min_idx[w >> 1]];
        }
        flipped = f != 0; unoriented = w == INVALID;
        const uint32_t *in = reinterpret_cast<const uint32_t *>(a.rows) + (size_t)orig * 6;
        uint32_t *o = reinterpret_cast<uint32_t *>(a.out) + (size_t)orig * 6;
        const uint32_t sign = f << 31;
        o[0] = in[0]; o[1] = in[1]; o[2] = in[2];
        o[3] = in[3] ^ sign; o[4] = in[4] ^ sign; o[5] = in[5] ^ sign;
        a.flip[orig] = (uint8_t)f;
        a.label[orig] = label;
    }
    const u64 fm = __ballot(flipped), um = __ballot(unoriented);
    if (lane_id() == 0) {
        if (fm) atomicAdd(a.cnt + C_FLIPPED, (uint32_t)__popcll(fm));
        if (um) atomicAdd(a.cnt + C_UNORIENTED, (uint32_t)__popcll(um));
    }
}

}  // namespace

struct OrientWork {
    TargetGrid grid;
    DBuf<float4> nrm;
    DBuf<uint32_t> snap, link, best_hi, rec_hi, rec_js, list[2], cnt, min_idx, votes, e_idx, toggle, flags, pos, firsts;
    DBuf<unsigned long long> best, rec_key, e_max;
    DBuf<uint8_t> flip;
    DBuf<int32_t> label;
    DBuf<float> in, out;             // the host-pointer entry point's device copies (grow-only)
    EventSpans<4> spans;             // grid, rounds, finish
};

namespace {

void check_params(uint32_t n, const plade_orient_params &p) {
    PLADE_REQUIRE(n >= 1, PLADE_EINVAL, "orient_normals: the cloud is empty (n = 0)");
    PLADE_REQUIRE(n < 0x80000000u, PLADE_EINVAL, "orient_normals: more than 2^31 - 1 points");   // (root << 1 | parity in 32 bits)
    PLADE_REQUIRE(radius_ok(p.radius, true), PLADE_EINVAL,
                  "orient_normals: radius must be finite and > 0, its fp32 square finite and not below FLT_MIN");
    PLADE_REQUIRE(p.mode == PLADE_ORIENT_VOTE || p.mode == PLADE_ORIENT_EXTREME, PLADE_EINVAL,
                  "orient_normals: mode must be 0 (vote) or 1 (extreme point)");
    PLADE_REQUIRE(p.inward == 0 || p.inward == 1, PLADE_EINVAL, "orient_normals: inward must be 0 or 1");
    PLADE_REQUIRE(std::isfinite(p.viewpoint[0]) && std::isfinite(p.viewpoint[1]) && std::isfinite(p.viewpoint[2]), PLADE_EINVAL,
                  "orient_normals: the viewpoint must be finite");
    PLADE_REQUIRE(std::isfinite(p.direction[0]) && std::isfinite(p.direction[1]) && std::isfinite(p.direction[2]), PLADE_EINVAL,
                  "orient_normals: the direction must be finite");
    PLADE_REQUIRE(p.direction[0] != 0.f || p.direction[1] != 0.f || p.direction[2] != 0.f, PLADE_EINVAL,
                  "orient_normals: the direction must not be zero");
}

// The orientation of a device cloud of n rows x y z nx ny nz with a known bounding box.  Writes the n rows to d_out, leaves flip
// and label in W, waits, fills the summary and the stats.
void orient_dev(plade_ctx *ctx, OrientWork &W, const float *d_rows, uint32_t n, const float bbmin[3], const float bbmax[3],
                const plade_orient_params &p, float *d_out, plade_orient_summary *summary) {
    W.spans.mark(ctx, 0);
    TargetGrid &G = W.grid;
    const float r = (float)p.radius;
    G.build(ctx, d_rows, n, 6, radius_cell((double)r, bbmin, bbmax), bbmin, bbmax, true);
    W.spans.mark(ctx, 1);

    RoundArgs a;
    memset(&a, 0, sizeof(a));
    a.g = view_of(G, "orient_normals");
    a.n = n; a.r2 = r * r;
    float4 *d_nrm = W.nrm.ensure(n);
    a.nrm = d_nrm;
    a.snap = W.snap.ensure(n); a.link = W.link.ensure(n);
    a.best = W.best.ensure(n); a.best_hi = W.best_hi.ensure(n);
    a.rec_key = W.rec_key.ensure(n); a.rec_hi = W.rec_hi.ensure(n); a.rec_js = W.rec_js.ensure(n);
    a.cnt = W.cnt.ensure(C_WORDS);
    W.list[0].ensure(n); W.list[1].ensure(n);
    const dim3 rows_grid(cdiv(n, ROW_TPB));
    ctx->fill_async(a.cnt, 0, C_WORDS * 4);
    hipLaunchKernelGGL(k_or_init, rows_grid, dim3(ROW_TPB), 0, ctx->stream, a.g.sorted, d_rows, n, d_nrm, a.snap, a.link, a.best, a.best_hi);
    HIP_TRY(hipGetLastError());
    uint32_t active = n, rounds = 0, tree_edges = 0;
    for (;;) {
        // (cannot happen below 2^31 points: every round at least halves the components that still have a neighbour)
        PLADE_REQUIRE(rounds < MAX_ROUNDS, PLADE_EFAIL, "orient_normals: the rounds did not end");
        ++rounds;
        a.n_active = active;
        a.active = rounds == 1 ? nullptr : W.list[rounds & 1].p;
        a.next = W.list[(rounds + 1) & 1].p;
        ctx->fill_async(a.cnt, 0, 8);                    // C_ACTIVE, C_HOOKS
        const dim3 pick_grid(cdiv(active, PICK_TPB));
        hipLaunchKernelGGL(k_or_pick, pick_grid, dim3(PICK_TPB), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_or_pick_hi, pick_grid, dim3(PICK_TPB), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_or_hook, pick_grid, dim3(PICK_TPB), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_or_flatten, rows_grid, dim3(ROW_TPB), 0, ctx->stream, a);
        HIP_TRY(hipGetLastError());
        uint32_t back[3] = {0, 0, 0};
        ctx->d2h(back, a.cnt, 12);
        ctx->sync();
        PLADE_REQUIRE(back[C_ERROR] == 0, PLADE_EFAIL, "orient_normals: a chain of hooks did not end at a root");   // (cannot happen)
        tree_edges += back[C_HOOKS];
        if (!back[C_HOOKS]) break;
        active = back[C_ACTIVE];
    }
    W.spans.mark(ctx, 2);

    FinishArgs f;
    memset(&f, 0, sizeof(f));
    f.sorted = a.g.sorted; f.nrm = d_nrm; f.rows = d_rows; f.snap = a.snap; f.n = n;
    f.mode = p.mode; f.inward = p.inward;
    for (int t = 0; t < 3; ++t) f.v[t] = p.mode == PLADE_ORIENT_VOTE ? (double)p.viewpoint[t] : (double)p.direction[t];
    f.min_idx = W.min_idx.ensure(n); f.toggle = W.toggle.ensure(n);
    f.flags = W.flags.ensure((size_t)n + 1);
    f.out = d_out; f.flip = W.flip.ensure((size_t)n + 4); f.label = W.label.ensure(n);
    f.cnt = a.cnt;
    ctx->fill_async(f.min_idx, 0xff, (size_t)n * 4);
    ctx->fill_async(f.flags + n, 0, 4);    // compact_flags scans n + 1 entries
    if (p.mode == PLADE_ORIENT_VOTE) {
        f.votes = W.votes.ensure((size_t)n * 2);
        ctx->fill_async(f.votes, 0, (size_t)n * 8);
    } else {
        f.e_max = W.e_max.ensure(n); f.e_idx = W.e_idx.ensure(n);
        ctx->fill_async(f.e_max, 0, (size_t)n * 8);
        ctx->fill_async(f.e_idx, 0xff, (size_t)n * 4);
    }
    hipLaunchKernelGGL(k_or_tally, rows_grid, dim3(ROW_TPB), 0, ctx->stream, f);
    if (p.mode == PLADE_ORIENT_EXTREME) hipLaunchKernelGGL(k_or_extreme_index, rows_grid, dim3(ROW_TPB), 0, ctx->stream, f);
    hipLaunchKernelGGL(k_or_anchor, rows_grid, dim3(ROW_TPB), 0, ctx->stream, f);
    HIP_TRY(hipGetLastError());
    const uint32_t C = compact_flags(ctx, f.flags, n, W.pos, W.firsts);   // (waits for the count)
    f.id = W.pos.p;
    hipLaunchKernelGGL(k_or_scatter, rows_grid, dim3(ROW_TPB), 0, ctx->stream, f);
    HIP_TRY(hipGetLastError());
    uint32_t back[C_WORDS] = {};
    ctx->d2h(back, a.cnt, C_WORDS * 4);
    W.spans.mark(ctx, 3);
    ctx->sync();
    // (cannot happen: every hook joins two components)
    PLADE_REQUIRE(n - back[C_UNORIENTED] == C + tree_edges, PLADE_EFAIL, "orient_normals: the forest does not span the components");
    uint64_t key_sum;
    memcpy(&key_sum, back + C_KEYSUM, 8);
    if (summary) {
        summary->n = n;
        summary->unoriented = back[C_UNORIENTED];
        summary->components = C;
        summary->flipped = back[C_FLIPPED];
        summary->tree_edges = tree_edges;
        summary->rounds = rounds;
        summary->tree_key_sum = key_sum;
    }
    W.spans.collect();
    ctx->stats.clear();
    ctx->stats.add("orient_grid_s", W.spans.seconds(0));
    ctx->stats.add("orient_rounds_s", W.spans.seconds(1));
    ctx->stats.add("orient_finish_s", W.spans.seconds(2));
    ctx->stats.add("orient_rounds", rounds);
    ctx->stats.add("orient_components", C);
    ctx->stats.add("orient_flipped", back[C_FLIPPED]);
    grid_stats(ctx, "orient", W.grid);
}

}  // namespace
}  // namespace plade

using namespace plade;

// ---- C ABI (include/plade_hip.h) ---------------------------------------------------------------------------------------------
extern "C" void plade_orient_default_params(plade_orient_params *p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->radius = 0.0;
    p->mode = PLADE_ORIENT_VOTE;
    p->inward = 0;
    p->direction[2] = 1.f;
}

extern "C" int plade_orient_normals(plade_ctx *ctx, const float *pos_nrm, uint32_t n, const plade_orient_params *params, float *rows_out,
                                    uint8_t *flip_out, int32_t *label_out, plade_orient_summary *summary) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(pos_nrm, PLADE_EINVAL, "plade_orient_normals: NULL cloud");
        const plade_orient_params p = params_or_default(params, plade_orient_default_params);
        check_params(n, p);
        OrientWork &W = work_in<OrientWork>(ctx->orient_work);
        float mn[3], mx[3];
        upload_rows(ctx, W.in, pos_nrm, n, 6, mn, mx);
        orient_dev(ctx, W, W.in.p, n, mn, mx, p, W.out.ensure((size_t)n * 6 + 4), summary);
        if (rows_out) HIP_TRY(hipMemcpyAsync(rows_out, W.out.p, (size_t)n * 24, hipMemcpyDeviceToHost, ctx->stream));
        if (flip_out) HIP_TRY(hipMemcpyAsync(flip_out, W.flip.p, n, hipMemcpyDeviceToHost, ctx->stream));
        if (label_out) HIP_TRY(hipMemcpyAsync(label_out, W.label.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        return PLADE_OK;
    });
}

extern "C" int plade_cloud_orient_normals_dev(plade_ctx *ctx, plade_cloud *cloud, const plade_orient_params *params, plade_cloud **out,
                                              uint8_t *flip_out, int32_t *label_out, plade_orient_summary *summary) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(cloud && out, PLADE_EINVAL, "plade_cloud_orient_normals_dev: NULL cloud");
        *out = nullptr;
        const plade_orient_params p = params_or_default(params, plade_orient_default_params);
        const CloudDev &in = cloud->dev;
        check_params(in.n, p);
        OrientWork &W = work_in<OrientWork>(ctx->orient_work);
        resident_result(ctx, out, [&](CloudDev &c) {
            cloud_shape(c, in.n);
            orient_dev(ctx, W, in.aos.p, in.n, in.bbmin, in.bbmax, p, c.aos.p, summary);
            if (flip_out) HIP_TRY(hipMemcpyAsync(flip_out, W.flip.p, in.n, hipMemcpyDeviceToHost, ctx->stream));
            if (label_out) HIP_TRY(hipMemcpyAsync(label_out, W.label.p, (size_t)in.n * 4, hipMemcpyDeviceToHost, ctx->stream));
            ctx->sync();
        });
        return PLADE_OK;
    });
}
