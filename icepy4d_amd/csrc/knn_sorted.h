// What the kernels over the cell-sorted cloud share (knn.hip: the k nearest neighbours; ballfeat.hip: the sums over a ball): the cloud in
// cell order and the kernel that gathers it into the context's scratch (stage_scratch.h: KnnSortedScratch), the contiguous range of a row
// of cells, the step budget that bounds a query's work whatever the grid, and what the entry points refuse about a grid.
#pragma once
#include <cmath>

#include "common.h"
#include "knn_point.h"

namespace im {
namespace {

constexpr long long KNN_MAX_CELLS = 1LL << 24;
constexpr int KNN_WAVES = 4;          // waves (queries) per block
constexpr int KNN_MIN_STEPS = 1024;   // steps (64 rows looked up, or 64 candidates read) every ring search may take, whatever the cloud's size

struct KnnSorted { double* x; double* y; double* z; int* idx; };

// an index outside the cloud (a permutation that is none) is clamped: the result is then meaningless, but every access stays inside
__global__ __launch_bounds__(256) void knn_gather_kernel(const double* __restrict__ pts, const long long* __restrict__ perm, long long n, KnnSorted s) {
    const long long j = blockIdx.x * 256LL + threadIdx.x;
    if (j >= n) return;
    long long i = perm[j];
    i = i < 0 ? 0 : (i >= n ? n - 1 : i);
    s.x[j] = pts[3 * i]; s.y[j] = pts[3 * i + 1]; s.z[j] = pts[3 * i + 2];
    s.idx[j] = (int)i;
}

// the sorted positions [b, e) of the cells ix0..ix1 of row (iy, iz): one contiguous range of the sorted cloud
__device__ __forceinline__ void knn_row_range(const KnnGrid& g, const int* __restrict__ start, int n, int ix0, int ix1, int iy, int iz, int& b, int& e) {
    const long long k0 = knn_key(g, ix0, iy, iz), k1 = knn_key(g, ix1, iy, iz) + 1;
    b = start[k0];
    e = start[k1];
    b = b < 0 ? 0 : b;
    e = e > n ? n : e;          // offsets that are none read nothing outside the cloud
}

// The steps a ring search may take before it is given up for one scan of the whole cloud, which takes n / 64 of them: a query far from
// everything (the lone outlier of a cloud whose grid is long and thin, a line of 2^24 cells) would otherwise walk up to 2^24 empty rings.
__device__ __forceinline__ long long knn_step_budget(int n) { return KNN_MIN_STEPS + n / (IM_WAVE / 2); }

// what the three entry points refuse about the grid; nullptr when it is fine
inline const char* bad_grid(const double* h_grid, int nx, int ny, int nz, KnnGrid& g) {
    if (!h_grid) return "null grid";
    const double s = h_grid[3];
    if (!(s > 0.0) || std::isinf(s)) return "the cell size must be finite and positive";
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(h_grid[a])) return "the origin must be finite";
    if (nx < 1 || ny < 1 || nz < 1) return "a grid dimension is below 1";
    if ((long long)nx * ny > KNN_MAX_CELLS || (long long)nx * ny * nz > KNN_MAX_CELLS) return "more cells than im_knn_max_cells()";
    g.o[0] = h_grid[0]; g.o[1] = h_grid[1]; g.o[2] = h_grid[2];
    g.s = s;
    g.n[0] = nx; g.n[1] = ny; g.n[2] = nz;
    return nullptr;
}

}  // namespace
}  // namespace im
