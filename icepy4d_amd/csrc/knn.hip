// Point-cloud neighbourhoods on the device: the exact k nearest neighbours of every point of a cloud within the same cloud, and on top of
// them the statistic of statistical outlier removal and the normals (`core/point_cloud.py`: `PointCloud.sor_filter`;
// `post_processing/open3d_fun.py`: `MeshingPoisson.SOR`, `estimate_normals(KDTreeSearchParamHybrid)`). The reference goes through Open3D,
// an un-vendored dependency: the k nearest neighbours have a definition of their own (ascending d2, the lower index first among equal
// distances) and are pinned bit for bit against tests/knn_oracle.py; Open3D's published SOR and normal algorithms are restated on top.
//
//   knn_cells_kernel    one thread per point: the key (iz * ny + iy) * nx + ix of its cell in a uniform grid (knn_point.h)
//   knn_ranges_kernel   one thread per cell: the first position of the cell in the key-sorted order (binary search; the stable sort by
//                       key between the two is torch's, plumbing)
//   knn_gather_kernel   (knn_sorted.h, shared with ballfeat.hip) the cloud in cell order as three coordinate planes plus the original
//                       indices (scratch of the context)
//   knn_self_kernel     one wave per query, queries in cell order so that neighbouring waves read the same cells. The wave visits the
//                       query's cell, then the shells of cells at Chebyshev ring 1, 2, ... clipped to the grid; a shell is walked as its six
//                       faces (only those inside the grid), inside a face every run of cells along x is one contiguous range of the
//                       sorted cloud; the lanes look up the ranges of 64 rows at a time and the ranges that hold points are read 64
//                       candidates at a time as coalesced loads. A search whose rings have cost more steps than one pass over the whole
//                       cloud (n / 64) is given up for that pass: the work of a query is bounded whatever the grid.
//                       The list and the search are knn_list.h's, shared with cloud_distance.hip. The best-k list lives one slot per lane (k <= 64), ascending; a batch is filtered against the k-th entry with one
//                       ballot and the survivors are inserted one by one by rank counting (ballot + popcount, a shift by one lane): no
//                       per-thread array, no LDS, no barrier. The search ends by knn_done (knn_point.h): the k-th d2 strictly below the
//                       conservative bound of everything unvisited, the box covering the grid, or the bound beyond the radius.
// float64 throughout, contraction off in knn_point.h.
#include <cmath>

#include "common.h"
#include "ctx.h"
#include "stage_scratch.h"
#include "knn_sorted.h"
#include "knn_list.h"

namespace im {
namespace {

__global__ __launch_bounds__(256) void knn_cells_kernel(KnnGrid g, const double* __restrict__ pts, long long n, long long* __restrict__ key) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= n) return;
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = knn_cell_of(knn_cell_coord(pts[3 * i + a], g.o[a], g.s), g.n[a]);
    key[i] = knn_key(g, c[0], c[1], c[2]);
}

// start[c] = the number of sorted keys below c, c = 0..cells
__global__ __launch_bounds__(256) void knn_ranges_kernel(const long long* __restrict__ skey, long long n, long long cells, int* __restrict__ start) {
    const long long c = blockIdx.x * 256LL + threadIdx.x;
    if (c > cells) return;
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (skey[mid] < c) lo = mid + 1; else hi = mid;
    }
    start[c] = (int)lo;
}

struct KnnArgs : KnnSearch {
    const double* pts;      // [n][3], original order
    int* count; int* idx; double* d2; double* mean; double* normal; int* rings;
};

__global__ __launch_bounds__(IM_WAVE * KNN_WAVES) void knn_self_kernel(KnnArgs a) {
    const int lane = threadIdx.x & (IM_WAVE - 1);
    const long long q = (unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * KNN_WAVES + threadIdx.x / IM_WAVE));      // < 2^31 + 4
    if (q >= a.n) return;                                             // the whole wave
    const double qx = a.s.x[q], qy = a.s.y[q], qz = a.s.z[q];
    const int qi = a.s.idx[q];
    const double t[3] = {knn_cell_coord(qx, a.g.o[0], a.g.s), knn_cell_coord(qy, a.g.o[1], a.g.s), knn_cell_coord(qz, a.g.o[2], a.g.s)};
    const int c[3] = {knn_cell_of(t[0], a.g.n[0]), knn_cell_of(t[1], a.g.n[1]), knn_cell_of(t[2], a.g.n[2])};
    KnnList L{knn_inf(), KNN_NONE, knn_inf(), KNN_NONE};
    const int rings = knn_ring_search(a, L, lane, qx, qy, qz, t, c);
    const bool held = L.idx != KNN_NONE;
    const int count = __popcll(__ballot(held));
    if (lane < a.k) {
        if (a.idx) a.idx[(long long)qi * a.k + lane] = held ? L.idx : -1;
        if (a.d2) a.d2[(long long)qi * a.k + lane] = held ? L.d2 : knn_inf();
    }
    if (lane == 0) {
        if (a.count) a.count[qi] = count;
        if (a.rings) a.rings[qi] = rings;
    }
    if (a.mean) {
        const double m = knn_mean_distance([&](int j) { return __shfl(L.d2, j); }, count);
        if (lane == 0) a.mean[qi] = m;
    }
    if (a.normal) {
        double px = 0.0, py = 0.0, pz = 0.0;
        if (held) { px = a.pts[3LL * L.idx]; py = a.pts[3LL * L.idx + 1]; pz = a.pts[3LL * L.idx + 2]; }
        double nrm[3];
        knn_normal([&](int j, double& x, double& y, double& z) { x = __shfl(px, j); y = __shfl(py, j); z = __shfl(pz, j); }, count, nrm);
        if (lane == 0) { a.normal[3LL * qi] = nrm[0]; a.normal[3LL * qi + 1] = nrm[1]; a.normal[3LL * qi + 2] = nrm[2]; }
    }
}

static_assert(IM_WAVE * KNN_WAVES == 256, "knn_self_kernel takes the block of the file's other kernels: 256 threads");

}  // namespace
}  // namespace im

using namespace im;

extern "C" {

int im_knn_max_cells(void) { return (int)KNN_MAX_CELLS; }

int im_knn_cells(im_ctx* ctx, const double* d_pts, long long n, const double* h_grid, int nx, int ny, int nz, long long* d_key, void* stream) {
    IM_CHECK_CTX(ctx);
    KnnGrid g;
    if (!d_pts || !d_key) return ctx->fail(-75, "im_knn_cells: null pointer");
    if (n < 0 || n >= (1LL << 31)) return ctx->fail(-75, "im_knn_cells: n must be 0..2^31-1");
    if (const char* why = bad_grid(h_grid, nx, ny, nz, g)) return ctx->fail(-75, "im_knn_cells: %s", why);
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    IM_LAUNCH(ctx, "knn_cells", s, launch(knn_cells_kernel, blocks_of(n, 256), 256, 0, s, g, d_pts, n, d_key));
    IM_GUARD_CHECK(ctx, s, "im_knn_cells");
    return 0;
}

int im_knn_cell_ranges(im_ctx* ctx, const long long* d_sorted_keys, long long n, long long cells, int32_t* d_start, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_sorted_keys || !d_start) return ctx->fail(-75, "im_knn_cell_ranges: null pointer");
    if (n < 0 || n >= (1LL << 31)) return ctx->fail(-75, "im_knn_cell_ranges: n must be 0..2^31-1");
    if (cells < 1 || cells > KNN_MAX_CELLS) return ctx->fail(-75, "im_knn_cell_ranges: cells must be 1..im_knn_max_cells()");
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    IM_LAUNCH(ctx, "knn_ranges", s, launch(knn_ranges_kernel, blocks_of(cells + 1, 256), 256, 0, s, d_sorted_keys, n, cells, d_start));
    IM_GUARD_CHECK(ctx, s, "im_knn_cell_ranges");
    return 0;
}

int im_knn_self(im_ctx* ctx, const double* d_pts, const long long* d_perm, const int32_t* d_start, long long n, const double* h_grid, int nx,
                int ny, int nz, int k, double radius2, int32_t* d_count, int32_t* d_idx, double* d_d2, double* d_mean, double* d_normal,
                int32_t* d_rings, void* stream) {
    IM_CHECK_CTX(ctx);
    KnnArgs a;
    if (!d_pts || !d_perm || !d_start) return ctx->fail(-75, "im_knn_self: null pointer");
    if (n < 0 || n >= (1LL << 31)) return ctx->fail(-75, "im_knn_self: n must be 0..2^31-1");
    if (k < 1 || k > IM_WAVE) return ctx->fail(-75, "im_knn_self: k must be 1..64");
    if (const char* why = bad_grid(h_grid, nx, ny, nz, a.g)) return ctx->fail(-75, "im_knn_self: %s", why);
    if (!(radius2 >= 0.0)) return ctx->fail(-75, "im_knn_self: radius2 must be >= 0 (+inf: no radius)");
    if (n == 0) return 0;
    const KnnSortedScratch lay(n);
    IM_GROW(ctx, ctx->grow(ctx->scratch.knn, lay.bytes, "knn_sorted"), -22, "im_knn_self: allocation failed");
    void* const base = ctx->scratch.knn.p;
    a.s.x = lay.x.at(base); a.s.y = lay.y.at(base); a.s.z = lay.z.at(base); a.s.idx = lay.idx.at(base);
    a.pts = d_pts; a.start = d_start; a.n = (int)n; a.k = k; a.radius2 = radius2;
    a.count = d_count; a.idx = d_idx; a.d2 = d_d2; a.mean = d_mean; a.normal = d_normal; a.rings = d_rings;
    hipStream_t s = (hipStream_t)stream;
    IM_LAUNCH(ctx, "knn_gather", s, launch(knn_gather_kernel, blocks_of(n, 256), 256, 0, s, d_pts, d_perm, n, a.s));
    IM_LAUNCH(ctx, "knn_self", s, launch(knn_self_kernel, blocks_of(n, KNN_WAVES), IM_WAVE * KNN_WAVES, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_knn_self");
    return 0;
}

}  // extern "C"
