// plade_amd/csrc/grid_walk.hip -- the host side of grid_walk.h: the grid of a k-nearest-neighbour search.
#include "grid_walk.h"

namespace plade {

namespace {
// occ[0] += occupied cells (distinct sorted keys)
__global__ __launch_bounds__(256) void k_count_cells(const uint32_t *__restrict__ keys, uint32_t n, uint32_t *__restrict__ occ) {
    uint32_t c = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        c += (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(occ, c);
}
}  // namespace

int build_knn_grid(plade_ctx *ctx, TargetGrid &G, const float *d_rows, uint32_t n, uint32_t stride, const float bbmin[3],
                   const float bbmax[3], int k, uint32_t *d_occ, const char *who) {
    const double ex = std::max(1e-9, (double)bbmax[0] - bbmin[0]), ey = std::max(1e-9, (double)bbmax[1] - bbmin[1]),
                 ez = std::max(1e-9, (double)bbmax[2] - bbmin[2]);
    const double area = 2 * (ex * ey + ey * ez + ex * ez), target = 0.7 * k;
    float cell = (float)(1.5 * std::sqrt((double)k * area / (M_PI * (double)n)));
    if (!(cell > 0.f) || !std::isfinite(cell)) cell = 1.f;
    for (int attempt = 0;; ++attempt) {
        G.build(ctx, d_rows, n, stride, cell, bbmin, bbmax, true);
        require_dense(G, who);
        if (attempt == 3 || n <= (uint32_t)(4 * k)) return attempt + 1;
        ctx->fill_async(d_occ, 0, 4);
        hipLaunchKernelGGL(k_count_cells, dim3(std::min(cdiv(n, 1024), 512u)), dim3(256), 0, ctx->stream, G.keys2.p, n, d_occ);
        HIP_TRY(hipGetLastError());
        uint32_t occ = 0;
        ctx->d2h(&occ, d_occ, 4);
        ctx->sync();
        const double mean = (double)n / std::max(occ, 1u);
        const float built = 1.f / G.gp.inv;          // build() enlarges the cell when the cell budget is hit
        if (mean > 2.0 * target && built <= cell * 1.01f) cell = built * (float)std::max(0.25, std::sqrt(target / mean));   // too coarse
        else if (mean < 0.5 * target && occ < n) cell = built * (float)std::min(4.0, std::sqrt(target / mean));          // too fine
        else return attempt + 1;
    }
}

}  // namespace plade
