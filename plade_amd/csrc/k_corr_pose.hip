// plade_amd/csrc/k_corr_pose.hip -- RANSAC pose estimation from correspondences on gfx950 (semantics: corr_pose.h).
//
// Layout
//   gather   k_corr_gather: S and Q of every correspondence as one packed row of six doubles, so that the points are read once
//            instead of through two index hops per (hypothesis, correspondence).
//   build    k_hyp_build: one lane per hypothesis -- the three draws, the prerejection, the two triangle frames; writes the triple,
//            the status, a 0 / 1 flag for the scan and, for status 0, the 12 coefficients [R | t].
//   compact  exclusive_scan_u32 (prims.h) over the flags and k_hyp_compact: the ascending list of the scored hypotheses.  A few
//            percent of the hypotheses survive the prerejection; scoring runs over this list, so every lane of a wavefront works.
//   score    k_hyp_score, the hot kernel: one lane owns one scored hypothesis with its 12 fp64 coefficients in registers;
//            correspondences are staged through LDS in tiles of 64 rows and read as wave-wide broadcasts (the pattern of
//            k_feat_match); M is split over blockIdx.y and a lane adds its chunk's count to count[h] with one integer atomicAdd
//            (exact, whatever the order).
//   best     k_hyp_best_part / k_hyp_best: the maximum of count << 32 | ~h in the order of fixed_reduce.h; lane 0 opens the state.
//   refine   per iteration k_corr_sum1, k_corr_mean, k_corr_sum2, k_corr_solve (one wavefront: the final sums, then Horn's
//            quaternion on lane 0), k_corr_flags under the new T and k_corr_accept -- all queued without a host wait; the state
//            (CorrState) lives on the device and once it says done every later kernel of the loop returns at once.
#include "corr_pose.h"
#include "cloud_tool.h"
#include "fpfh.h"
#include "keypoints.h"
#include "fixed_reduce.h"
#include "prims.h"
#include "voxel.h"

namespace plade {

namespace {

using u64 = unsigned long long;

constexpr int GATHER_TPB = 256, BUILD_TPB = 256, SCORE_TPB = 64, FLAGS_TPB = 256;
constexpr int ROW = 6;                 // doubles per packed correspondence: S, Q

struct dv { double x, y, z; };
__device__ __forceinline__ dv sub3(dv a, dv b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot3(dv a, dv b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ dv cross3(dv a, dv b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ dv div3(dv a, double s) { return {a.x / s, a.y / s, a.z / s}; }

// the state of one estimate (device memory; read back once at the end)
struct CorrState {
    double T[12], Tn[12];              // the current iterate; the refit under test
    double n, sm[3], qm[3], sum_d2;    // of the current pass: inliers, means, sum of d2
    double C[9];
    u64 best_key;
    uint32_t count, count_new, changed;   // inliers of T; of Tn; correspondences whose flag differs between the two
    uint32_t best_h, best_count;
    int32_t done, refinements, failure, cur;   // cur: which of the two flag buffers holds T's flags
};

__global__ __launch_bounds__(GATHER_TPB) void k_corr_gather(const float *__restrict__ src, uint32_t sstride, const float *__restrict__ tgt,
                                                            uint32_t tstride, const int32_t *__restrict__ corr, uint32_t m,
                                                            double *__restrict__ sq) {
    const uint32_t i = blockIdx.x * GATHER_TPB + threadIdx.x;
    if (i >= m) return;
    const float *s = src + (size_t)corr[2 * (size_t)i] * sstride, *t = tgt + (size_t)corr[2 * (size_t)i + 1] * tstride;
    double *o = sq + (size_t)i * ROW;
    o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
    o[3] = t[0]; o[4] = t[1]; o[5] = t[2];
}

// e1, e2, e3 of the triangle (pa, pb, pc); false: sqrt(w.w) is 0 or not finite
__device__ __forceinline__ bool frame(dv pa, dv pb, dv pc, dv &e1, dv &e2, dv &e3) {
    const dv u = sub3(pb, pa), v = sub3(pc, pa);
    e1 = div3(u, sqrt(dot3(u, u)));
    const dv w = cross3(u, v);
    const double wl = sqrt(dot3(w, w));
    e3 = div3(w, wl);
    e2 = cross3(e3, e1);
    return wl > 0.0 && wl <= DBL_MAX;        // (false for NaN)
}
// fmin(ls, lt) < sim * fmax(ls, lt) on the edge (i, j)
__device__ __forceinline__ bool edge_fails(dv si, dv sj, dv qi, dv qj, double sim) {
    const dv ds = sub3(si, sj), dq = sub3(qi, qj);
    const double ls = sqrt(dot3(ds, ds)), lt = sqrt(dot3(dq, dq));
    return fmin(ls, lt) < sim * fmax(ls, lt);
}

struct BuildArgs {
    const double *sq;
    uint32_t m, H;
    uint64_t base;                   // mix64(seed)
    double sim;
    int32_t *triple;                 // H x 3
    uint8_t *status;                 // H
    uint32_t *flags;                 // H + 1: 1 = scored; flags[H] = 0 (the scan's extra slot)
    double *T;                       // H x 12
    int zero_T;                      // the T seam is wanted: rows of the hypotheses that are not scored are zeroed
};

__global__ __launch_bounds__(BUILD_TPB) void k_hyp_build(const BuildArgs a) {
    const uint32_t h = blockIdx.x * BUILD_TPB + threadIdx.x;
    if (h > a.H) return;
    if (h == a.H) { a.flags[h] = 0u; return; }
    uint32_t idx[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint64_t z = mix64(a.base ^ (4ull * h + (uint64_t)k));
        idx[k] = (uint32_t)(((z >> 32) * (uint64_t)a.m) >> 32);      // < m
    }
    a.triple[3 * (size_t)h] = (int32_t)idx[0];
    a.triple[3 * (size_t)h + 1] = (int32_t)idx[1];
    a.triple[3 * (size_t)h + 2] = (int32_t)idx[2];
    int status = 0;
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = 0.0;
    if (idx[0] == idx[1] || idx[1] == idx[2] || idx[0] == idx[2]) status = 1;
    else {
        dv S[3], Q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double *r = a.sq + (size_t)idx[k] * ROW;
            S[k] = {r[0], r[1], r[2]};
            Q[k] = {r[3], r[4], r[5]};
        }
        if (edge_fails(S[0], S[1], Q[0], Q[1], a.sim) || edge_fails(S[1], S[2], Q[1], Q[2], a.sim) ||
            edge_fails(S[2], S[0], Q[2], Q[0], a.sim)) status = 2;
        else {
            dv s1, s2, s3, t1, t2, t3;
            const bool oks = frame(S[0], S[1], S[2], s1, s2, s3), okt = frame(Q[0], Q[1], Q[2], t1, t2, t3);
            if (!oks || !okt) status = 3;
            else {
                const double e1t[3] = {t1.x, t1.y, t1.z}, e2t[3] = {t2.x, t2.y, t2.z}, e3t[3] = {t3.x, t3.y, t3.z};
                const double e1s[3] = {s1.x, s1.y, s1.z}, e2s[3] = {s2.x, s2.y, s2.z}, e3s[3] = {s3.x, s3.y, s3.z};
                const double cs[3] = {((S[0].x + S[1].x) + S[2].x) / 3.0, ((S[0].y + S[1].y) + S[2].y) / 3.0, ((S[0].z + S[1].z) + S[2].z) / 3.0};
                const double ct[3] = {((Q[0].x + Q[1].x) + Q[2].x) / 3.0, ((Q[0].y + Q[1].y) + Q[2].y) / 3.0, ((Q[0].z + Q[1].z) + Q[2].z) / 3.0};
#pragma unroll
                for (int i = 0; i < 3; ++i) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) T[4 * i + j] = (e1t[i] * e1s[j] + e2t[i] * e2s[j]) + e3t[i] * e3s[j];
                    T[4 * i + 3] = ct[i] - ((T[4 * i] * cs[0] + T[4 * i + 1] * cs[1]) + T[4 * i + 2] * cs[2]);
                }
            }
        }
    }
    a.status[h] = (uint8_t)status;
    a.flags[h] = status == 0 ? 1u : 0u;
    if (status == 0 || a.zero_T) {
        double2 *o = reinterpret_cast<double2 *>(a.T + 12 * (size_t)h);      // (rows of 96 bytes: 16-byte aligned)
#pragma unroll
        for (int k = 0; k < 6; ++k) o[k] = make_double2(T[2 * k], T[2 * k + 1]);
    }
}

__global__ __launch_bounds__(256) void k_hyp_compact(const uint32_t *__restrict__ flags, const uint32_t *__restrict__ offs, uint32_t H,
                                                     uint32_t *__restrict__ list) {
    const uint32_t h = blockIdx.x * 256 + threadIdx.x;
    if (h >= H || !flags[h]) return;
    list[offs[h]] = h;
}

// d2 of one packed row under T
__device__ __forceinline__ double row_d2(const double (&T)[12], double s0, double s1, double s2, double q0, double q1, double q2) {
    const double dx = (((T[0] * s0 + T[1] * s1) + T[2] * s2) + T[3]) - q0;
    const double dy = (((T[4] * s0 + T[5] * s1) + T[6] * s2) + T[7]) - q1;
    const double dz = (((T[8] * s0 + T[9] * s1) + T[10] * s2) + T[11]) - q2;
    return (dx * dx + dy * dy) + dz * dz;
}

__global__ __launch_bounds__(SCORE_TPB) void k_hyp_score(const double *__restrict__ sq, uint32_t m, uint32_t chunk /* a multiple of the tile */,
                                                         const uint32_t *__restrict__ list, uint32_t ns, const double *__restrict__ Tall,
                                                         double thr2, uint32_t *__restrict__ count) {
    __shared__ __align__(16) double s_p[CORR_SCORE_TILE * ROW];      // rows of 48 bytes: read as three double2
    const uint32_t i = blockIdx.x * SCORE_TPB + threadIdx.x;
    const bool live = i < ns;
    const uint32_t h = live ? list[i] : 0u;
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = 0.0;
    if (live) {
        const double2 *p = reinterpret_cast<const double2 *>(Tall + 12 * (size_t)h);
#pragma unroll
        for (int k = 0; k < 6; ++k) { const double2 v = p[k]; T[2 * k] = v.x; T[2 * k + 1] = v.y; }
    }
    uint32_t cnt = 0;
    const uint32_t m_begin = blockIdx.y * chunk, m_end = min(m, m_begin + chunk);
    for (uint32_t m0 = m_begin; m0 < m_end; m0 += CORR_SCORE_TILE) {
        const uint32_t tn = min((uint32_t)CORR_SCORE_TILE, m_end - m0);
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < tn * ROW; k += SCORE_TPB) s_p[k] = sq[(size_t)m0 * ROW + k];
        __syncthreads();
        for (uint32_t j = 0; j < tn; ++j) {
            const double2 *r = reinterpret_cast<const double2 *>(s_p + j * ROW);      // (wave-uniform: broadcast reads)
            const double2 r0 = r[0], r1 = r[1], r2 = r[2];
            cnt += row_d2(T, r0.x, r0.y, r1.x, r1.y, r2.x, r2.y) < thr2 ? 1u : 0u;
        }
    }
    if (live && cnt) atomicAdd(&count[h], cnt);
}

struct MaxU64 {
    __device__ __forceinline__ u64 operator()(int, u64 a, u64 b) const { return b > a ? b : a; }
};

// the key of scored hypothesis h: count << 32 | ~h (0 for the lanes past the list: below every real key, h < 2^24)
__global__ __launch_bounds__(256) void k_hyp_best_part(const uint32_t *__restrict__ list, uint32_t ns, const uint32_t *__restrict__ count,
                                                       u64 *__restrict__ partial) {
    __shared__ u64 s_red[256 / 64][1];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    u64 v[1] = {0};
    if (i < ns) {
        const uint32_t h = list[i];
        v[0] = ((u64)count[h] << 32) | (u64)(uint32_t)~h;
    }
    block_reduce<256>(v, s_red, partial, MaxU64());
}
__global__ __launch_bounds__(64) void k_hyp_best(const u64 *__restrict__ partial, uint32_t blocks, const double *__restrict__ Tall,
                                                 uint32_t min_inliers, CorrState *st) {
    u64 v[1];
    final_reduce(partial, blocks, v, MaxU64());
    if (threadIdx.x != 0) return;
    const uint32_t h = ~(uint32_t)v[0], c = (uint32_t)(v[0] >> 32);
    st->best_key = v[0];
    st->best_h = h;
    st->best_count = c;
    for (int k = 0; k < 12; ++k) { st->T[k] = Tall[12 * (size_t)h + k]; st->Tn[k] = 0.0; }
    st->count = c;
    st->count_new = 0; st->changed = 0;
    st->refinements = 0;
    st->cur = 0;
    st->failure = c < min_inliers ? PLADE_CORR_POSE_FEW_INLIERS : 0;
    st->done = st->failure != 0;
}

// flags under st->T into the current buffer (use_new = 0), or under st->Tn into the other one, with the counts the accept rule needs
__global__ __launch_bounds__(FLAGS_TPB) void k_corr_flags(const double *__restrict__ sq, uint32_t m, CorrState *st, int use_new, double thr2,
                                                          uint8_t *f0, uint8_t *f1) {
    if (use_new && st->done) return;                 // (uniform)
    const uint32_t i = blockIdx.x * FLAGS_TPB + threadIdx.x;
    const int cur = st->cur;
    uint8_t *fc = cur ? f1 : f0, *fo = cur ? f0 : f1;
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = use_new ? st->Tn[k] : st->T[k];
    bool in = false, diff = false;
    if (i < m) {
        const double *r = sq + (size_t)i * ROW;
        in = row_d2(T, r[0], r[1], r[2], r[3], r[4], r[5]) < thr2;
        if (use_new) { fo[i] = in ? 1 : 0; diff = (fc[i] != 0) != in; }
        else fc[i] = in ? 1 : 0;
    }
    if (!use_new) return;
    const uint32_t n_in = (uint32_t)__popcll(__ballot(in)), n_diff = (uint32_t)__popcll(__ballot(diff));
    if ((threadIdx.x & 63) == 0) {
        if (n_in) atomicAdd(&st->count_new, n_in);
        if (n_diff) atomicAdd(&st->changed, n_diff);
    }
}

__global__ void k_corr_accept(CorrState *st) {
    if (threadIdx.x != 0 || st->done) return;
    if (st->count_new >= st->count) {
        for (int k = 0; k < 12; ++k) st->T[k] = st->Tn[k];
        st->count = st->count_new;
        st->refinements += 1;
        st->cur ^= 1;
        if (st->changed == 0) st->done = 1;
    } else st->done = 1;
    st->count_new = 0;
    st->changed = 0;
}

// n, sum S, sum Q, sum d2 over the flagged correspondences under st->T: partial[b * 8 + k]
__global__ __launch_bounds__(CORR_SUM_TPB) void k_corr_sum1(const double *__restrict__ sq, uint32_t m, const CorrState *st, int gated,
                                                            const uint8_t *f0, const uint8_t *f1, double *__restrict__ partial) {
    __shared__ double s_red[CORR_SUM_TPB / 64][8];
    if (gated && st->done) return;                   // (uniform)
    const uint32_t i = blockIdx.x * CORR_SUM_TPB + threadIdx.x;
    const uint8_t *fc = st->cur ? f1 : f0;
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = 0.0;
    if (i < m && fc[i]) {
        double T[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = st->T[k];
        const double *r = sq + (size_t)i * ROW;
        v[0] = 1.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) v[1 + k] = r[k];
        v[7] = row_d2(T, r[0], r[1], r[2], r[3], r[4], r[5]);
    }
    block_reduce<CORR_SUM_TPB>(v, s_red, partial, SumOp());
}
__global__ __launch_bounds__(64) void k_corr_mean(const double *__restrict__ partial, uint32_t blocks, CorrState *st, int gated) {
    if (gated && st->done) return;
    double v[8];
    final_reduce(partial, blocks, v, SumOp());
    if (threadIdx.x != 0) return;
    st->n = v[0];
    for (int k = 0; k < 3; ++k) { st->sm[k] = v[1 + k] / v[0]; st->qm[k] = v[4 + k] / v[0]; }
    st->sum_d2 = v[7];
}
// C_ij = sum (Q - q)_i (S - s)_j: partial[b * 9 + 3 i + j]
__global__ __launch_bounds__(CORR_SUM_TPB) void k_corr_sum2(const double *__restrict__ sq, uint32_t m, const CorrState *st, int gated,
                                                            const uint8_t *f0, const uint8_t *f1, double *__restrict__ partial) {
    __shared__ double s_red[CORR_SUM_TPB / 64][9];
    if (gated && st->done) return;
    const uint32_t i = blockIdx.x * CORR_SUM_TPB + threadIdx.x;
    const uint8_t *fc = st->cur ? f1 : f0;
    double v[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) v[k] = 0.0;
    if (i < m && fc[i]) {
        const double *r = sq + (size_t)i * ROW;
        const double s[3] = {r[0] - st->sm[0], r[1] - st->sm[1], r[2] - st->sm[2]};
        const double q[3] = {r[3] - st->qm[0], r[4] - st->qm[1], r[5] - st->qm[2]};
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) v[3 * a + b] = q[a] * s[b];
    }
    block_reduce<CORR_SUM_TPB>(v, s_red, partial, SumOp());
}

// one Jacobi rotation that zeroes A[P][Q] of the symmetric A (A <- J^T A J, V <- V J); the indices are compile-time constants, so
// A and V stay in registers
template <int P, int Q>
__device__ __forceinline__ void jacobi_rot(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 4; ++k) { const double x = A[k][P], y = A[k][Q]; A[k][P] = c * x - s * y; A[k][Q] = s * x + c * y; }
#pragma unroll
    for (int k = 0; k < 4; ++k) { const double x = A[P][k], y = A[Q][k]; A[P][k] = c * x - s * y; A[Q][k] = s * x + c * y; }
#pragma unroll
    for (int k = 0; k < 4; ++k) { const double x = V[k][P], y = V[k][Q]; V[k][P] = c * x - s * y; V[k][Q] = s * x + c * y; }
}

// Horn 1987: the rotation R that maximises sum (Q - q).R (S - s), from C_ij = sum (Q - q)_i (S - s)_j
__device__ __forceinline__ void horn_rotation(const double (&C)[9], double (&R)[9]) {
    // Horn's S_ab = sum s_a q_b = C[b][a]
    const double Sxx = C[0], Sxy = C[3], Sxz = C[6], Syx = C[1], Syy = C[4], Syz = C[7], Szx = C[2], Szy = C[5], Szz = C[8];
    double A[4][4] = {{(Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, (Syy - Sxx) - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, (Szz - Sxx) - Syy}};
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < CORR_JACOBI_SWEEPS; ++sweep) {
        jacobi_rot<0, 1>(A, V); jacobi_rot<0, 2>(A, V); jacobi_rot<0, 3>(A, V);
        jacobi_rot<1, 2>(A, V); jacobi_rot<1, 3>(A, V); jacobi_rot<2, 3>(A, V);
    }
    // the column of the largest eigenvalue (ties: the first)
    // picked with 0 / 1 weights, not by a run-time column index, which would send V to scratch
    double best = A[0][0];
    int col = 0;
    if (A[1][1] > best) { best = A[1][1]; col = 1; }
    if (A[2][2] > best) { best = A[2][2]; col = 2; }
    if (A[3][3] > best) { best = A[3][3]; col = 3; }
    const double m0 = col == 0 ? 1.0 : 0.0, m1 = col == 1 ? 1.0 : 0.0, m2 = col == 2 ? 1.0 : 0.0, m3 = col == 3 ? 1.0 : 0.0;
    const double q0 = (V[0][0] * m0 + V[0][1] * m1) + (V[0][2] * m2 + V[0][3] * m3);
    const double q1 = (V[1][0] * m0 + V[1][1] * m1) + (V[1][2] * m2 + V[1][3] * m3);
    const double q2 = (V[2][0] * m0 + V[2][1] * m1) + (V[2][2] * m2 + V[2][3] * m3);
    const double q3 = (V[3][0] * m0 + V[3][1] * m1) + (V[3][2] * m2 + V[3][3] * m3);
    const double l = sqrt((q0 * q0 + q1 * q1) + (q2 * q2 + q3 * q3));
    const double w = q0 / l, x = q1 / l, y = q2 / l, z = q3 / l;
    R[0] = ((w * w + x * x) - y * y) - z * z; R[1] = 2.0 * (x * y - w * z);             R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);             R[4] = ((w * w - x * x) + y * y) - z * z; R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);             R[7] = 2.0 * (y * z + w * x);             R[8] = ((w * w - x * x) - y * y) + z * z;
}

__global__ __launch_bounds__(64) void k_corr_solve(const double *__restrict__ partial, uint32_t blocks, CorrState *st, int solve) {
    if (solve && st->done) return;
    double C[9];
    final_reduce(partial, blocks, C, SumOp());
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int k = 0; k < 9; ++k) st->C[k] = C[k];
    if (!solve) return;
    double R[9];
    horn_rotation(C, R);
    const double s0 = st->sm[0], s1 = st->sm[1], s2 = st->sm[2];
    const double t0 = st->qm[0] - ((R[0] * s0 + R[1] * s1) + R[2] * s2);
    const double t1 = st->qm[1] - ((R[3] * s0 + R[4] * s1) + R[5] * s2);
    const double t2 = st->qm[2] - ((R[6] * s0 + R[7] * s1) + R[8] * s2);
    st->Tn[0] = R[0]; st->Tn[1] = R[1]; st->Tn[2] = R[2]; st->Tn[3] = t0;
    st->Tn[4] = R[3]; st->Tn[5] = R[4]; st->Tn[6] = R[5]; st->Tn[7] = t1;
    st->Tn[8] = R[6]; st->Tn[9] = R[7]; st->Tn[10] = R[8]; st->Tn[11] = t2;
    // a unit quaternion's entries are finite or all NaN: one sum tells
    const double probe = ((R[0] + R[4]) + R[8]) + ((t0 + t1) + t2);
    if (!(fabs(probe) <= DBL_MAX)) st->done = 1;     // the old T stays
}

// the current flags as the caller's inlier array
__global__ __launch_bounds__(256) void k_corr_finish(const CorrState *st, const uint8_t *f0, const uint8_t *f1, uint32_t m,
                                                     uint8_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < m) out[i] = (st->cur ? f1 : f0)[i];
}

}  // namespace

struct CorrPoseWork {
    DBuf<float> in_s, in_t;          // the host-pointer entry points' device copies (grow-only)
    DBuf<int32_t> corr, triple;
    DBuf<double> sq, T, partial;
    DBuf<uint8_t> status, f0, f1, inlier;
    DBuf<uint32_t> flags, offs, list, count;
    DBuf<u64> best_partial;
    DBuf<CorrState> st;
    plade_features feat_s, feat_t;   // plade_register_features: the two descriptor tables (grow-only)
    plade_features feat_k;           // plade_register_keypoints: the source rows at the keypoints
    CorrState h_st;
    EventSpans<4> spans;             // build, score, refine
};

namespace {

void check_params(const plade_corr_pose_params &p) {
    PLADE_REQUIRE(std::isfinite(p.inlier_dist) && p.inlier_dist > 0.0 && std::isfinite(p.inlier_dist * p.inlier_dist) &&
                      p.inlier_dist * p.inlier_dist > 0.0,
                  PLADE_EINVAL, "estimate_pose_corr: inlier_dist must be finite and > 0 (and so must its square)");
    PLADE_REQUIRE(p.hypotheses >= 1 && p.hypotheses <= (1 << 24), PLADE_EINVAL, "estimate_pose_corr: hypotheses must be 1 .. 2^24");
    PLADE_REQUIRE(p.edge_similarity >= 0.0 && p.edge_similarity <= 1.0, PLADE_EINVAL, "estimate_pose_corr: edge_similarity must be in [0, 1]");
    PLADE_REQUIRE(p.min_inliers >= 3, PLADE_EINVAL, "estimate_pose_corr: min_inliers must be >= 3");
    PLADE_REQUIRE(p.refine_iterations >= 0, PLADE_EINVAL, "estimate_pose_corr: refine_iterations must be >= 0");
}

void check_list(const int32_t *corr, uint64_t m, uint32_t ns, uint32_t nt, const char *who) {
    PLADE_REQUIRE(ns >= 1 && nt >= 1, PLADE_EINVAL, std::string(who) + ": an empty cloud (ns = 0 or nt = 0)");
    PLADE_REQUIRE(m >= 1, PLADE_EINVAL, std::string(who) + ": the correspondence list is empty (m = 0)");
    PLADE_REQUIRE(m <= 0x7fffffffull, PLADE_EINVAL, std::string(who) + ": more than 2^31 - 1 correspondences");
    for (uint64_t i = 0; i < m; ++i) {
        const int32_t s = corr[2 * i], t = corr[2 * i + 1];
        PLADE_REQUIRE(s >= 0 && (uint32_t)s < ns && t >= 0 && (uint32_t)t < nt, PLADE_EINVAL,
                      std::string(who) + ": correspondence " + std::to_string(i) + " names a point that does not exist");
    }
}

// the packed rows of the list (device)
const double *gather(plade_ctx *ctx, CorrPoseWork &W, const float *d_src, uint32_t sstride, const float *d_tgt, uint32_t tstride,
                     const int32_t *corr, uint32_t m, bool corr_on_device = false) {
    const int32_t *d_corr = corr;
    if (!corr_on_device) {
        HIP_TRY(hipMemcpyAsync(W.corr.ensure((size_t)m * 2), corr, (size_t)m * 8, hipMemcpyHostToDevice, ctx->stream));
        d_corr = W.corr.p;
    }
    double *d_sq = W.sq.ensure((size_t)m * ROW + 2);
    hipLaunchKernelGGL(k_corr_gather, dim3(cdiv(m, GATHER_TPB)), dim3(GATHER_TPB), 0, ctx->stream, d_src, sstride, d_tgt, tstride,
                       d_corr, m, d_sq);
    HIP_TRY(hipGetLastError());
    return d_sq;
}

void identity16(float *T16) {
    for (int k = 0; k < 16; ++k) T16[k] = (k % 5 == 0) ? 1.f : 0.f;
}

struct Seams {
    uint8_t *inlier;
    int32_t *triple;
    uint8_t *status;
    uint32_t *count;
    double *T;
};

// n, means and sum d2 of the current flags under st->T (into the state)
void queue_sum1(plade_ctx *ctx, CorrPoseWork &W, const double *d_sq, uint32_t m, int gated) {
    const uint32_t blocks = cdiv(m, CORR_SUM_TPB);
    double *d_part = W.partial.ensure((size_t)9 * blocks);
    hipLaunchKernelGGL(k_corr_sum1, dim3(blocks), dim3(CORR_SUM_TPB), 0, ctx->stream, d_sq, m, (const CorrState *)W.st.p, gated,
                       (const uint8_t *)W.f0.p, (const uint8_t *)W.f1.p, d_part);
    hipLaunchKernelGGL(k_corr_mean, dim3(1), dim3(64), 0, ctx->stream, (const double *)d_part, blocks, W.st.p, gated);
}
// C (and, with solve, the refit Tn)
void queue_sum2(plade_ctx *ctx, CorrPoseWork &W, const double *d_sq, uint32_t m, int gated, int solve) {
    const uint32_t blocks = cdiv(m, CORR_SUM_TPB);
    double *d_part = W.partial.ensure((size_t)9 * blocks);
    hipLaunchKernelGGL(k_corr_sum2, dim3(blocks), dim3(CORR_SUM_TPB), 0, ctx->stream, d_sq, m, (const CorrState *)W.st.p, gated,
                       (const uint8_t *)W.f0.p, (const uint8_t *)W.f1.p, d_part);
    hipLaunchKernelGGL(k_corr_solve, dim3(1), dim3(64), 0, ctx->stream, (const double *)d_part, blocks, W.st.p, solve);
}

int pose_dev(plade_ctx *ctx, CorrPoseWork &W, const float *d_src, uint32_t sstride, const float *d_tgt, uint32_t tstride,
             const int32_t *corr, uint32_t m, const plade_corr_pose_params &p, float *T16, const Seams &out,
             plade_corr_pose_result *res, bool corr_on_device = false) {
    const uint32_t H = (uint32_t)p.hypotheses;
    const double thr2 = p.inlier_dist * p.inlier_dist;
    memset(res, 0, sizeof(*res));
    res->hypotheses = H;
    identity16(T16);
    res->T[0] = res->T[5] = res->T[10] = 1.0;
    ctx->stats.clear();
    if (m < 3) {                                     // no triple exists: nothing is drawn, the seams are not written
        res->failure = PLADE_CORR_POSE_TOO_FEW;
        ctx->last_error = "estimate_pose_corr: fewer than 3 correspondences";
        return PLADE_EFAIL;
    }
    W.spans.mark(ctx, 0);
    const double *d_sq = gather(ctx, W, d_src, sstride, d_tgt, tstride, corr, m, corr_on_device);
    BuildArgs b;
    memset(&b, 0, sizeof(b));
    b.sq = d_sq; b.m = m; b.H = H; b.base = mix64(p.seed); b.sim = p.edge_similarity;
    b.triple = W.triple.ensure((size_t)H * 3);
    b.status = W.status.ensure((size_t)H + 4);
    b.flags = W.flags.ensure((size_t)H + 1);
    b.T = W.T.ensure((size_t)H * 12);
    b.zero_T = out.T ? 1 : 0;
    hipLaunchKernelGGL(k_hyp_build, dim3(cdiv((size_t)H + 1, BUILD_TPB)), dim3(BUILD_TPB), 0, ctx->stream, b);
    HIP_TRY(hipGetLastError());
    uint32_t *d_offs = W.offs.ensure((size_t)H + 1), *d_list = W.list.ensure(H), *d_count = W.count.ensure(H);
    exclusive_scan_u32(ctx, b.flags, d_offs, (size_t)H + 1);
    hipLaunchKernelGGL(k_hyp_compact, dim3(cdiv(H, 256)), dim3(256), 0, ctx->stream, (const uint32_t *)b.flags, (const uint32_t *)d_offs, H,
                       d_list);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(d_count, 0, (size_t)H * 4, ctx->stream));
    uint32_t scored = 0;
    HIP_TRY(hipMemcpyAsync(&scored, d_offs + H, 4, hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();                                     // the one wait inside: the list's length sizes the scoring grid
    res->scored = scored;
    W.spans.mark(ctx, 1);
    CorrState *d_st = W.st.ensure(1);
    uint8_t *d_f0 = W.f0.ensure((size_t)m + 4), *d_f1 = W.f1.ensure((size_t)m + 4), *d_in = W.inlier.ensure((size_t)m + 4);
    if (scored) {
        // a workgroup is one wave of 64 hypotheses against one chunk of correspondences: chunks of CORR_SCORE_CHUNK while that gives
        // at most ~16 000 workgroups, longer ones above
        const uint32_t gx = cdiv(scored, SCORE_TPB), nch_max = std::max(1u, 16384u / gx);
        const uint32_t chunk = std::max((uint32_t)CORR_SCORE_CHUNK, (uint32_t)cdiv(cdiv(m, nch_max), CORR_SCORE_TILE) * CORR_SCORE_TILE);
        const uint32_t nch = cdiv(m, chunk);
        hipLaunchKernelGGL(k_hyp_score, dim3(gx, nch), dim3(SCORE_TPB), 0, ctx->stream, d_sq, m, chunk, (const uint32_t *)d_list, scored,
                           (const double *)b.T, thr2, d_count);
        const uint32_t bb = cdiv(scored, 256);
        u64 *d_bp = W.best_partial.ensure(bb);
        hipLaunchKernelGGL(k_hyp_best_part, dim3(bb), dim3(256), 0, ctx->stream, (const uint32_t *)d_list, scored, (const uint32_t *)d_count, d_bp);
        hipLaunchKernelGGL(k_hyp_best, dim3(1), dim3(64), 0, ctx->stream, (const u64 *)d_bp, bb, (const double *)b.T,
                           (uint32_t)p.min_inliers, d_st);
        HIP_TRY(hipGetLastError());
    }
    W.spans.mark(ctx, 2);
    if (scored) {
        const uint32_t fb = cdiv(m, FLAGS_TPB);
        hipLaunchKernelGGL(k_corr_flags, dim3(fb), dim3(FLAGS_TPB), 0, ctx->stream, d_sq, m, d_st, 0, thr2, d_f0, d_f1);
        for (int it = 0; it < p.refine_iterations; ++it) {      // queued without a host wait: `done` on the device ends it
            queue_sum1(ctx, W, d_sq, m, 1);
            queue_sum2(ctx, W, d_sq, m, 1, 1);
            hipLaunchKernelGGL(k_corr_flags, dim3(fb), dim3(FLAGS_TPB), 0, ctx->stream, d_sq, m, d_st, 1, thr2, d_f0, d_f1);
            hipLaunchKernelGGL(k_corr_accept, dim3(1), dim3(64), 0, ctx->stream, d_st);
        }
        queue_sum1(ctx, W, d_sq, m, 0);              // inliers and sum d2 under the final T
        hipLaunchKernelGGL(k_corr_finish, dim3(cdiv(m, 256)), dim3(256), 0, ctx->stream, (const CorrState *)d_st, (const uint8_t *)d_f0,
                           (const uint8_t *)d_f1, m, d_in);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&W.h_st, d_st, sizeof(CorrState), hipMemcpyDeviceToHost, ctx->stream));
        if (out.inlier) HIP_TRY(hipMemcpyAsync(out.inlier, d_in, m, hipMemcpyDeviceToHost, ctx->stream));
    }
    W.spans.mark(ctx, 3);
    if (out.triple) HIP_TRY(hipMemcpyAsync(out.triple, b.triple, (size_t)H * 12, hipMemcpyDeviceToHost, ctx->stream));
    if (out.status) HIP_TRY(hipMemcpyAsync(out.status, b.status, H, hipMemcpyDeviceToHost, ctx->stream));
    if (out.count) HIP_TRY(hipMemcpyAsync(out.count, d_count, (size_t)H * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (out.T) HIP_TRY(hipMemcpyAsync(out.T, b.T, (size_t)H * 96, hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    W.spans.collect();
    ctx->stats.add("corr_pose_build_s", W.spans.seconds(0));
    ctx->stats.add("corr_pose_score_s", W.spans.seconds(1));
    ctx->stats.add("corr_pose_refine_s", W.spans.seconds(2));
    ctx->stats.add("corr_pose_scored", (double)scored);
    if (!scored) {
        if (out.inlier) memset(out.inlier, 0, m);
        res->failure = PLADE_CORR_POSE_NONE_SCORED;
        ctx->stats.add("corr_pose_inliers", 0.0);
        ctx->last_error = "estimate_pose_corr: no hypothesis passed the prerejection";
        return PLADE_EFAIL;
    }
    const CorrState &s = W.h_st;
    res->best_hypothesis = s.best_h;
    res->best_count = s.best_count;
    if (s.failure) {
        if (out.inlier) memset(out.inlier, 0, m);
        res->failure = s.failure;
        ctx->stats.add("corr_pose_inliers", 0.0);
        ctx->last_error = "estimate_pose_corr: the best hypothesis has fewer than min_inliers inliers";
        return PLADE_EFAIL;
    }
    res->inliers = (uint32_t)s.n;
    res->refinements = s.refinements;
    res->rmse = std::sqrt(s.sum_d2 / s.n);
    res->fitness = s.n / (double)m;
    for (int k = 0; k < 12; ++k) { res->T[k] = s.T[k]; T16[k] = (float)s.T[k]; }
    ctx->stats.add("corr_pose_inliers", s.n);
    return PLADE_OK;
}

// FPFH of both clouds, the match, the pose: device rows x y z nx ny nz with their bounding boxes in, only summaries (and the list,
// when wanted) out.
int register_dev(plade_ctx *ctx, CorrPoseWork &W, const float *d_tgt, uint32_t nt, const float tmn[3], const float tmx[3],
                 const float *d_src, uint32_t ns, const float smn[3], const float smx[3], const plade_fpfh_params &fp,
                 const plade_feature_match_params &mp, const plade_corr_pose_params &pp, float *T16, plade_fpfh_summary *sum_src,
                 plade_fpfh_summary *sum_tgt, plade_corr_pose_result *res, int32_t *corr_out, uint64_t cap, uint64_t *n_corr) {
    check_params(pp);
    fpfh_table_dev(ctx, d_src, ns, smn, smx, fp, W.feat_s, sum_src);
    fpfh_table_dev(ctx, d_tgt, nt, tmn, tmx, fp, W.feat_t, sum_tgt);
    uint64_t total = 0;
    const int32_t *d_corr = feature_corr_dev(ctx, W.feat_s, W.feat_t, mp, &total);
    if (n_corr) *n_corr = total;
    if (corr_out && std::min(total, cap))
        HIP_TRY(hipMemcpyAsync(corr_out, d_corr, (size_t)std::min(total, cap) * 8, hipMemcpyDeviceToHost, ctx->stream));
    const Seams none = {nullptr, nullptr, nullptr, nullptr, nullptr};
    const int rc = pose_dev(ctx, W, d_src, 6, d_tgt, 6, d_corr, (uint32_t)total, pp, T16, none, res, true);
    if (total < 3) ctx->sync();                      // (pose_dev returned before its wait: the list's copy is still in flight)
    return rc;
}

// The same with the detector in front of the match: ISS on the source, FPFH of both clouds, the source rows at the keypoints against
// the whole target table, the list's source column mapped back to original indices, the pose.
int register_keypoints_dev(plade_ctx *ctx, CorrPoseWork &W, const float *d_tgt, uint32_t nt, const float tmn[3], const float tmx[3],
                           const float *d_src, uint32_t ns, const float smn[3], const float smx[3], const plade_iss_params &ip,
                           const plade_fpfh_params &fp, const plade_feature_match_params &mp, const plade_corr_pose_params &pp, float *T16,
                           plade_iss_summary *sum_iss, plade_fpfh_summary *sum_src, plade_fpfh_summary *sum_tgt,
                           plade_corr_pose_result *res, int32_t *corr_out, uint64_t cap, uint64_t *n_corr) {
    check_params(pp);
    uint32_t k = 0;
    const uint32_t *d_key = iss_list_dev(ctx, d_src, ns, 6, smn, smx, ip, sum_iss, &k);
    fpfh_table_dev(ctx, d_src, ns, smn, smx, fp, W.feat_s, sum_src);
    fpfh_table_dev(ctx, d_tgt, nt, tmn, tmx, fp, W.feat_t, sum_tgt);
    uint64_t total = 0;
    const int32_t *d_corr = nullptr;
    if (k) {                                         // (no keypoint: no match, and the pose fails with too few correspondences)
        features_select_dev(ctx, W.feat_s, d_key, k, W.feat_k);
        const int32_t *d_sel = feature_corr_dev(ctx, W.feat_k, W.feat_t, mp, &total);
        d_corr = corr_map_source_dev(ctx, d_sel, total, d_key);
    }
    if (n_corr) *n_corr = total;
    if (corr_out && std::min(total, cap))
        HIP_TRY(hipMemcpyAsync(corr_out, d_corr, (size_t)std::min(total, cap) * 8, hipMemcpyDeviceToHost, ctx->stream));
    const Seams none = {nullptr, nullptr, nullptr, nullptr, nullptr};
    const int rc = pose_dev(ctx, W, d_src, 6, d_tgt, 6, d_corr, (uint32_t)total, pp, T16, none, res, true);
    if (total < 3) ctx->sync();                      // (as register_dev)
    return rc;
}

}  // namespace
}  // namespace plade

using namespace plade;

// ---- C ABI (include/plade_hip.h) ---------------------------------------------------------------------------------------------
extern "C" void plade_corr_pose_default_params(plade_corr_pose_params *p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->inlier_dist = 0.0;
    p->edge_similarity = 0.9;
    p->seed = 0;
    p->hypotheses = 65536;
    p->min_inliers = 3;
    p->refine_iterations = 5;
}

extern "C" int plade_estimate_pose_corr(plade_ctx *ctx, const float *src, uint32_t ns, uint32_t src_stride, const float *tgt, uint32_t nt,
                                        uint32_t tgt_stride, const int32_t *corr, uint64_t m, const plade_corr_pose_params *params,
                                        float *T16, uint8_t *inlier_out, int32_t *triple_out, uint8_t *status_out, uint32_t *count_out,
                                        double *T_out, plade_corr_pose_result *result) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(src && tgt && corr && params && T16 && result, PLADE_EINVAL,
                      "plade_estimate_pose_corr: NULL points, list, params, T16 or result");
        PLADE_REQUIRE(src_stride >= 3 && tgt_stride >= 3, PLADE_EINVAL, "plade_estimate_pose_corr: a stride below 3 floats");
        check_params(*params);
        check_list(corr, m, ns, nt, "plade_estimate_pose_corr");
        CorrPoseWork &W = work_in<CorrPoseWork>(ctx->corr_pose_work);
        float mn[3], mx[3];
        upload_rows(ctx, W.in_s, src, ns, src_stride, mn, mx);           // (the bounding box checks the coordinates)
        upload_rows(ctx, W.in_t, tgt, nt, tgt_stride, mn, mx);
        const Seams out = {inlier_out, triple_out, status_out, count_out, T_out};
        return pose_dev(ctx, W, W.in_s.p, src_stride, W.in_t.p, tgt_stride, corr, (uint32_t)m, *params, T16, out, result);
    });
}

extern "C" int plade_estimate_pose_corr_dev(plade_ctx *ctx, plade_cloud *src, plade_cloud *tgt, const int32_t *corr, uint64_t m,
                                            const plade_corr_pose_params *params, float *T16, uint8_t *inlier_out, int32_t *triple_out,
                                            uint8_t *status_out, uint32_t *count_out, double *T_out, plade_corr_pose_result *result) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(src && tgt && corr && params && T16 && result, PLADE_EINVAL,
                      "plade_estimate_pose_corr_dev: NULL cloud, list, params, T16 or result");
        check_params(*params);
        check_list(corr, m, src->dev.n, tgt->dev.n, "plade_estimate_pose_corr_dev");
        const Seams out = {inlier_out, triple_out, status_out, count_out, T_out};
        return pose_dev(ctx, work_in<CorrPoseWork>(ctx->corr_pose_work), src->dev.aos.p, 6, tgt->dev.aos.p, 6, corr, (uint32_t)m, *params,
                        T16, out, result);
    });
}

extern "C" int plade_corr_pose_moments(plade_ctx *ctx, const float *src, uint32_t ns, uint32_t src_stride, const float *tgt, uint32_t nt,
                                       uint32_t tgt_stride, const int32_t *corr, uint64_t m, const double *T12, double inlier_dist,
                                       uint8_t *flags_out, double *moments_out) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(src && tgt && corr && T12 && moments_out, PLADE_EINVAL, "plade_corr_pose_moments: NULL points, list, T12 or moments_out");
        PLADE_REQUIRE(src_stride >= 3 && tgt_stride >= 3, PLADE_EINVAL, "plade_corr_pose_moments: a stride below 3 floats");
        PLADE_REQUIRE(std::isfinite(inlier_dist) && inlier_dist > 0.0 && std::isfinite(inlier_dist * inlier_dist) && inlier_dist * inlier_dist > 0.0,
                      PLADE_EINVAL, "plade_corr_pose_moments: inlier_dist must be finite and > 0");
        for (int k = 0; k < 12; ++k) PLADE_REQUIRE(std::isfinite(T12[k]), PLADE_EINVAL, "plade_corr_pose_moments: T12 is not finite");
        check_list(corr, m, ns, nt, "plade_corr_pose_moments");
        CorrPoseWork &W = work_in<CorrPoseWork>(ctx->corr_pose_work);
        float mn[3], mx[3];
        upload_rows(ctx, W.in_s, src, ns, src_stride, mn, mx);
        upload_rows(ctx, W.in_t, tgt, nt, tgt_stride, mn, mx);
        const uint32_t M = (uint32_t)m;
        const double *d_sq = gather(ctx, W, W.in_s.p, src_stride, W.in_t.p, tgt_stride, corr, M);
        CorrState *d_st = W.st.ensure(1);
        memset(&W.h_st, 0, sizeof(W.h_st));
        for (int k = 0; k < 12; ++k) W.h_st.T[k] = T12[k];
        HIP_TRY(hipMemcpyAsync(d_st, &W.h_st, sizeof(CorrState), hipMemcpyHostToDevice, ctx->stream));
        uint8_t *d_f0 = W.f0.ensure((size_t)M + 4), *d_f1 = W.f1.ensure((size_t)M + 4);
        hipLaunchKernelGGL(k_corr_flags, dim3(cdiv(M, FLAGS_TPB)), dim3(FLAGS_TPB), 0, ctx->stream, d_sq, M, d_st, 0,
                           inlier_dist * inlier_dist, d_f0, d_f1);
        queue_sum1(ctx, W, d_sq, M, 0);
        queue_sum2(ctx, W, d_sq, M, 0, 0);
        HIP_TRY(hipGetLastError());
        ctx->sync();                                 // (the upload of the state read W.h_st)
        HIP_TRY(hipMemcpyAsync(&W.h_st, d_st, sizeof(CorrState), hipMemcpyDeviceToHost, ctx->stream));
        if (flags_out) HIP_TRY(hipMemcpyAsync(flags_out, d_f0, M, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        const CorrState &s = W.h_st;
        moments_out[0] = s.n;
        for (int k = 0; k < 3; ++k) { moments_out[1 + k] = s.sm[k]; moments_out[4 + k] = s.qm[k]; }
        for (int k = 0; k < 9; ++k) moments_out[7 + k] = s.C[k];
        moments_out[16] = s.sum_d2;
        return PLADE_OK;
    });
}

extern "C" int plade_register_features(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t, const float *src_pos_nrm, uint32_t n_s,
                                       const plade_fpfh_params *fpfh, const plade_feature_match_params *match,
                                       const plade_corr_pose_params *pose, float *T16, plade_fpfh_summary *src_summary,
                                       plade_fpfh_summary *tgt_summary, plade_corr_pose_result *result, int32_t *corr_out, uint64_t cap,
                                       uint64_t *n_corr) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(tgt_pos_nrm && src_pos_nrm && fpfh && pose && T16 && src_summary && tgt_summary && result, PLADE_EINVAL,
                      "plade_register_features: NULL cloud, params, T16, summary or result");
        PLADE_REQUIRE(n_t >= 1 && n_s >= 1, PLADE_EINVAL, "plade_register_features: an empty cloud (n = 0)");
        const plade_feature_match_params mp = params_or_default(match, plade_feature_match_default_params);
        CorrPoseWork &W = work_in<CorrPoseWork>(ctx->corr_pose_work);
        float tmn[3], tmx[3], smn[3], smx[3];
        upload_rows(ctx, W.in_t, tgt_pos_nrm, n_t, 6, tmn, tmx);         // (the bounding box checks the coordinates)
        upload_rows(ctx, W.in_s, src_pos_nrm, n_s, 6, smn, smx);
        return register_dev(ctx, W, W.in_t.p, n_t, tmn, tmx, W.in_s.p, n_s, smn, smx, *fpfh, mp, *pose, T16, src_summary, tgt_summary,
                            result, corr_out, cap, n_corr);
    });
}

extern "C" int plade_register_features_dev(plade_ctx *ctx, plade_cloud *tgt, plade_cloud *src, const plade_fpfh_params *fpfh,
                                           const plade_feature_match_params *match, const plade_corr_pose_params *pose, float *T16,
                                           plade_fpfh_summary *src_summary, plade_fpfh_summary *tgt_summary,
                                           plade_corr_pose_result *result, int32_t *corr_out, uint64_t cap, uint64_t *n_corr) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(tgt && src && fpfh && pose && T16 && src_summary && tgt_summary && result, PLADE_EINVAL,
                      "plade_register_features_dev: NULL cloud, params, T16, summary or result");
        const plade_feature_match_params mp = params_or_default(match, plade_feature_match_default_params);
        const CloudDev &t = tgt->dev, &s = src->dev;
        return register_dev(ctx, work_in<CorrPoseWork>(ctx->corr_pose_work), t.aos.p, t.n, t.bbmin, t.bbmax, s.aos.p, s.n, s.bbmin, s.bbmax,
                            *fpfh, mp, *pose, T16, src_summary, tgt_summary, result, corr_out, cap, n_corr);
    });
}

extern "C" int plade_register_keypoints(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t, const float *src_pos_nrm, uint32_t n_s,
                                        const plade_iss_params *iss, const plade_fpfh_params *fpfh, const plade_feature_match_params *match,
                                        const plade_corr_pose_params *pose, float *T16, plade_iss_summary *iss_summary,
                                        plade_fpfh_summary *src_summary, plade_fpfh_summary *tgt_summary, plade_corr_pose_result *result,
                                        int32_t *corr_out, uint64_t cap, uint64_t *n_corr) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(tgt_pos_nrm && src_pos_nrm && iss && fpfh && pose && T16 && iss_summary && src_summary && tgt_summary && result,
                      PLADE_EINVAL, "plade_register_keypoints: NULL cloud, params, T16, summary or result");
        PLADE_REQUIRE(n_t >= 1 && n_s >= 1, PLADE_EINVAL, "plade_register_keypoints: an empty cloud (n = 0)");
        const plade_feature_match_params mp = params_or_default(match, plade_feature_match_default_params);
        CorrPoseWork &W = work_in<CorrPoseWork>(ctx->corr_pose_work);
        float tmn[3], tmx[3], smn[3], smx[3];
        upload_rows(ctx, W.in_t, tgt_pos_nrm, n_t, 6, tmn, tmx);         // (the bounding box checks the coordinates)
        upload_rows(ctx, W.in_s, src_pos_nrm, n_s, 6, smn, smx);
        return register_keypoints_dev(ctx, W, W.in_t.p, n_t, tmn, tmx, W.in_s.p, n_s, smn, smx, *iss, *fpfh, mp, *pose, T16, iss_summary,
                                      src_summary, tgt_summary, result, corr_out, cap, n_corr);
    });
}

extern "C" int plade_register_keypoints_dev(plade_ctx *ctx, plade_cloud *tgt, plade_cloud *src, const plade_iss_params *iss,
                                            const plade_fpfh_params *fpfh, const plade_feature_match_params *match,
                                            const plade_corr_pose_params *pose, float *T16, plade_iss_summary *iss_summary,
                                            plade_fpfh_summary *src_summary, plade_fpfh_summary *tgt_summary,
                                            plade_corr_pose_result *result, int32_t *corr_out, uint64_t cap, uint64_t *n_corr) {
    return guarded(ctx, [&]() -> int {
        PLADE_REQUIRE(tgt && src && iss && fpfh && pose && T16 && iss_summary && src_summary && tgt_summary && result, PLADE_EINVAL,
                      "plade_register_keypoints_dev: NULL cloud, params, T16, summary or result");
        const plade_feature_match_params mp = params_or_default(match, plade_feature_match_default_params);
        const CloudDev &t = tgt->dev, &s = src->dev;
        return register_keypoints_dev(ctx, work_in<CorrPoseWork>(ctx->corr_pose_work), t.aos.p, t.n, t.bbmin, t.bbmax, s.aos.p, s.n,
                                      s.bbmin, s.bbmax, *iss, *fpfh, mp, *pose, T16, iss_summary, src_summary, tgt_summary, result,
                                      corr_out, cap, n_corr);
    });
}
