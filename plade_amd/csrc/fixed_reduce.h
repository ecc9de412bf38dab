// plade_amd/csrc/fixed_reduce.h -- the fixed-order reduction behind every summary of the cloud tools (k_outliers, k_distances,
// k_smooth, k_m3c2, k_fpfh, the moments of icp_core.h).  The order, which is what makes a summary the same bits from run to run
// and lets tests/fixed_order.py replay it:
//   wave       the xor butterfly over offsets 32 .. 1: v = op(v, v of lane ^ o); afterwards every lane holds the wave's value
//   workgroup  lane 0 of each wave writes s_red[wave][k]; after the barrier thread k combines the waves in ascending order and
//              writes partial[blockIdx.x * N + k]
//   final      one wavefront: lane l combines partial[b * N + k] for b = l, l + 64, ... in ascending b, then the butterfly;
//              lane 0 holds the result
// No atomics.  A tool keeps what is its own: the per-point terms in front of block_reduce, the scalar lines of lane 0 behind
// final_reduce.  The N terms of one call share a type; a tool with two types calls block_reduce twice (terms are independent)
// and the two-type final_reduce.
//
// op(k, a, b) combines two values of term k -- a sum, or the tool's own maximum (fmax, max, a > b ? a : b: what a NaN does rides
// on it).  In the unrolled loops k is a constant, so `k == 3 ? fmax(a, b) : a + b` costs nothing there.
#pragma once
#include <hip/hip_runtime.h>

namespace plade {

struct SumOp {
    template <class T> __device__ __forceinline__ T operator()(int, T a, T b) const { return a + b; }
};

template <class T, class Op>
__device__ __forceinline__ T wave_reduce(int k, T v, Op op) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = op(k, v, __shfl_xor(v, o, 64));
    return v;
}

// called by all TPB threads of the workgroup (one barrier).  A term goes to LDS as soon as its butterfly is done: the 29 and 30
// moments of the ICP kernels are never all live at once
template <int TPB, int N, class T, class Op>
__device__ __forceinline__ void block_reduce(const T (&term)[N], T (&s_red)[TPB / 64][N], T *partial, Op op) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const T v = wave_reduce(k, term[k], op);
        if (lane == 0) s_red[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const int k = threadIdx.x;
        T t = s_red[0][k];
#pragma unroll
        for (int w = 1; w < TPB / 64; ++w) t = op(k, t, s_red[w][k]);
        partial[(size_t)blockIdx.x * N + k] = t;
    }
}

// the pieces of final_reduce: v starts from 0 (every tool's sums and maxima of non-negative terms do), takes workgroup b's partials ...
template <int N, class T>
__device__ __forceinline__ void final_zero(T (&v)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = T(0);
}
template <int N, class T, class Op>
__device__ __forceinline__ void final_take(const T *partial, uint32_t b, T (&v)[N], Op op) {
    const T *p = partial + (size_t)b * N;
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = op(k, v[k], p[k]);
}
// ... and is closed by the butterfly
template <int N, class T, class Op>
__device__ __forceinline__ void final_close(T (&v)[N], Op op) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = wave_reduce(k, v[k], op);
}

// called by the 64 lanes of a one-wavefront kernel
template <int N, class T, class Op>
__device__ __forceinline__ void final_reduce(const T *partial, uint32_t blocks, T (&v)[N], Op op) {
    final_zero(v);
    for (uint32_t b = threadIdx.x; b < blocks; b += 64) final_take(partial, b, v, op);
    final_close(v, op);
}
// The same for a tool with two types, in ONE walk over the workgroups: the walk is a chain of dependent waits for memory (61
// rounds at 1M points), and two walks one after the other took 6 us longer than one in k_smooth_final
template <int NA, class A, class OpA, int NB, class B, class OpB>
__device__ __forceinline__ void final_reduce(const A *pa, const B *pb, uint32_t blocks, A (&a)[NA], OpA opa, B (&b)[NB], OpB opb) {
    final_zero(a);
    final_zero(b);
    for (uint32_t i = threadIdx.x; i < blocks; i += 64) { final_take(pa, i, a, opa); final_take(pb, i, b, opb); }
    final_close(a, opa);
    final_close(b, opb);
}

}  // namespace plade
