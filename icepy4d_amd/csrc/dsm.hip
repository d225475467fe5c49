// DSM and orthophoto rasters (`src/icepy4d/utils/dsm_orthophoto.py`: `build_dsm`, `generate_ortophoto`; `sfm/interpolate_colors.py`:
// `interpolate_point_colors`, `bilinear_interpolate`; `sfm/geometry.py`: `project_points`). The reference bins the cloud with pandas,
// triangulates with qhull and interpolates with scipy's `LinearNDInterpolator`, one grid cell at a time. Here the binning, the
// per-cell triangle search and interpolation, and the projection + colour sampling are device kernels; the sorts of the binning are
// torch's (plumbing) and the Delaunay triangulation stays qhull's on the host (only qhull on the same input reproduces
// the reference's triangle set on these highly cocircular grids).
//
//   dsm_round_kernel        one thread per point: float32 rounding of x, y to the step and the sort keys
//   dsm_zero_first_kernel   the first row (in the reference's sort order) whose x or y key is +-0: the sign the group keeps
//   scan_*_kernel (scan.h)  exclusive scans (block sums, one block over them, block-local scan + write) for the group starts
//                           and for the row spans of the triangles
//   dsm_group_mean_kernel   one thread per group: pandas' Kahan mean of the group's z in ascending-z order
//   dsm_raster_kernel       one thread per (triangle, grid row) span: the exact inside test on the span's cells, atomicMin of the
//                           triangle index per cell (the lowest index that contains the cell wins: deterministic)
//   dsm_eval_kernel         one thread per cell: barycentric interpolation in scipy's operation order, float64
//   proj_color_kernel       one thread per point / cell: cv2.projectPoints restated in float64, bilinear sampling of the image,
//                           float32 projections, float64 colours and uint8 orthophoto cells
// The arithmetic of every item is dsm_cell.h's, which a host program compiles too (tests/dsm_host_harness.cpp); the kernels here are the
// launch geometry, the scans, the search of a span's triangle and the atomicMin. Every function that must reproduce the reference's
// rounding keeps contraction off: whether a * b + c becomes one fused operation is otherwise the compiler's choice (`__fmul_rn` /
// `__fadd_rn` do not prevent it on this toolchain, lg_misc.hip).
// What is pinned: the lowest simplex index that contains a cell, on every cell, and every output bit for bit against the brute-force
// restatement (tests/dsm_oracle.py; tests/test_dsm_cpu.py on the host build, tests/test_gpu_dsm_edges.py on the device, on the cases
// of tests/dsm_cases.py). The comparison with scipy's `find_simplex` (tests/test_gpu_dsm.py) remains the statement about the
// reference: its walk may stop in a neighbour on a shared edge or vertex, so it is exact on cells with a unique triangle only.
#include <climits>
#include <cmath>

#include "common.h"
#include "ctx.h"
#include "dsm_cell.h"
#include "stage_scratch.h"

namespace im {
namespace {

__global__ __launch_bounds__(256) void dsm_round_kernel(const double* __restrict__ pts, long long n, float step, float* __restrict__ xr,
                                                        float* __restrict__ yr, long long* __restrict__ xykey, long long* __restrict__ ykey,
                                                        long long* __restrict__ zkey) {
#pragma clang fp contract(off)
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    dsm_round_point(pts, i, step, xr, yr, xykey, ykey, zkey);
}

__global__ __launch_bounds__(256) void dsm_zero_first_kernel(const float* __restrict__ xr, const float* __restrict__ yr,
                                                             const long long* __restrict__ perm_b, int n, int* __restrict__ first) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const long long i = perm_b[j];
    if (dsm_zero_key(xr[i])) atomicMin(&first[0], j);
    if (dsm_zero_key(yr[i])) atomicMin(&first[1], j);
}

// ---- exclusive scans over per-item counts (group starts: 0 / 1 per sorted row; triangles: grid rows per triangle): scan.h -----------
#include "scan.h"

struct GroupScan {            // 1 where a sorted row starts a new (x, y) group
    const long long* key;     // [n] (x, y) keys
    const long long* perm;    // [n] rows in group order
    long long n;
    long long* starts;        // [G] first sorted position of each group
    __device__ long long count(long long j) const { return dsm_group_count(key, perm, n, j); }
    __device__ void write(long long j, long long pos) const { if (j < n && count(j)) starts[pos] = j; }
};

struct RowScan {              // grid rows (spans) per triangle
    TriGrid g;
    long long* offs;          // [T] first span of each triangle
    __device__ long long count(long long t) const { return tri_span_count(g, t); }
    __device__ void write(long long t, long long pos) const { if (t < g.T) offs[t] = pos; }
};

__global__ __launch_bounds__(256) void dsm_group_mean_kernel(const double* __restrict__ pts, const float* __restrict__ xr,
                                                             const float* __restrict__ yr, const long long* __restrict__ perm_b,
                                                             const long long* __restrict__ perm_c, const int* __restrict__ zero_first,
                                                             const long long* __restrict__ starts, const long long* __restrict__ n_groups,
                                                             long long n, float* __restrict__ bx, float* __restrict__ by, float* __restrict__ bz) {
#pragma clang fp contract(off)
    const long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const long long G = *n_groups;
    if (g >= G) return;
    dsm_group_mean(pts, xr, yr, perm_b, perm_c, zero_first, starts, G, n, g, bx, by, bz);
}

__global__ __launch_bounds__(256) void dsm_raster_kernel(TriGrid g, const long long* __restrict__ offs, const long long* __restrict__ n_spans,
                                                         int* __restrict__ win) {
#pragma clang fp contract(off)
    const long long total = *n_spans;
    for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < total; q += (long long)gridDim.x * blockDim.x) {
        long long lo = 0, hi = g.T;          // the last triangle whose first span is <= q (empty triangles share its offset)
        while (hi - lo > 1) {
            const long long mid = (lo + hi) >> 1;
            if (offs[mid] <= q) lo = mid; else hi = mid;
        }
        const long long t = lo;
        int r0, r1;
        tri_rows(g, t, r0, r1);
        const int r = r0 + (int)(q - offs[t]);
        tri_span_cells(g, t, r, [&](long long cell) {
            if ((int)t < win[cell]) atomicMin(&win[cell], (int)t);
        });
    }
}

__global__ __launch_bounds__(256) void dsm_eval_kernel(TriGrid g, const float* __restrict__ bz, const int* __restrict__ win,
                                                       double4 bounds, double fill, double* __restrict__ z) {
#pragma clang fp contract(off)
    const long long cell = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (cell >= (long long)g.nx * g.ny) return;
    z[cell] = dsm_eval_cell(g, bz, win, bounds.x, bounds.y, bounds.z, bounds.w, fill, cell);
}

__global__ __launch_bounds__(256) void proj_color_kernel(ColorArgs a, CamParams p) {
#pragma clang fp contract(off)
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= (long long)a.rows * a.cols) return;
    proj_color_item(a, p, i);
}

}  // namespace
}  // namespace im

using namespace im;

extern "C" int im_dsm_round(im_ctx* ctx, const double* d_pts, long long n, float step, float* d_xr, float* d_yr, long long* d_xykey,
                            long long* d_ykey, long long* d_zkey, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_pts || !d_xr || !d_yr || !d_xykey || !d_ykey || !d_zkey || n < 0 || n >= INT_MAX) return ctx->fail(-72, "im_dsm_round: bad arguments");
    if (step == 0.f || !std::isfinite(step)) return ctx->fail(-72, "im_dsm_round: the step must be non-zero and finite");
    if (!n) return 0;
    hipStream_t s = (hipStream_t)stream;
    IM_LAUNCH(ctx, "dsm_round", s, launch(dsm_round_kernel, blocks_of(n, 256), 256, 0, s, d_pts, n, step, d_xr, d_yr, d_xykey, d_ykey, d_zkey));
    IM_GUARD_CHECK(ctx, s, "im_dsm_round");
    return 0;
}

extern "C" int im_dsm_group_mean(im_ctx* ctx, const double* d_pts, const float* d_xr, const float* d_yr, const long long* d_xykey,
                                 const long long* d_perm_b, const long long* d_perm_c, long long n, float* d_bx, float* d_by, float* d_bz,
                                 long long* d_n_groups, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_pts || !d_xr || !d_yr || !d_xykey || !d_perm_b || !d_perm_c || !d_bx || !d_by || !d_bz || !d_n_groups || n < 0 || n >= INT_MAX)
        return ctx->fail(-72, "im_dsm_group_mean: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (!n) {
        IM_HIP(ctx, hipMemsetAsync(d_n_groups, 0, sizeof(long long), s));
        return 0;
    }
    const DsmGroupScratch lay(n);
    IM_GROW(ctx, ctx->grow(ctx->scratch.dsm, lay.bytes, "dsm.scratch"), -71, "im_dsm_group_mean: out of device memory");
    void* const sc = ctx->scratch.dsm.p;
    long long* starts = lay.starts.at(sc);
    int* first = lay.first.at(sc);
    IM_HIP(ctx, hipMemsetAsync(first, 0x7f, 2 * sizeof(int), s));
    IM_LAUNCH(ctx, "dsm_zero_first", s, launch(dsm_zero_first_kernel, blocks_of(n, 256), 256, 0, s, d_xr, d_yr, d_perm_b, (int)n, first));
    const GroupScan gs{d_xykey, d_perm_c, n, starts};
    IM_LAUNCH(ctx, "dsm_group_scan", s, launch_scan(gs, n, lay.sums.at(sc), d_n_groups, s));
    IM_LAUNCH(ctx, "dsm_group_mean", s, launch(dsm_group_mean_kernel, blocks_of(n, 256), 256, 0, s, d_pts, d_xr,
                                                            d_yr, d_perm_b, d_perm_c, (const int*)first, (const long long*)starts,
                                                            (const long long*)d_n_groups, n, d_bx, d_by, d_bz));
    IM_GUARD_CHECK(ctx, s, "im_dsm_group_mean");
    return 0;
}

extern "C" int im_dsm_rasterize(im_ctx* ctx, const float* d_bx, const float* d_by, const float* d_bz, const int32_t* d_simplices,
                                const double* d_transform, long long n_simplices, const double* h_bounds, const double* d_xq, int nx,
                                const double* d_yq, int ny, double x0, double dx, double y0, double dy, double fill, double* d_z, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_bx || !d_by || !d_bz || !d_simplices || !d_transform || !h_bounds || !d_xq || !d_yq || !d_z || n_simplices < 0 ||
        n_simplices >= WIN_NONE || nx < 0 || ny < 0)
        return ctx->fail(-72, "im_dsm_rasterize: bad arguments");
    if (!(dx > 0.0) || !(dy > 0.0) || !std::isfinite(x0) || !std::isfinite(y0)) return ctx->fail(-72, "im_dsm_rasterize: the grid spacing must be positive");
    const long long cells = (long long)nx * ny;
    if (!cells) return 0;
    hipStream_t s = (hipStream_t)stream;
    const TriGrid g{d_bx, d_by, d_simplices, d_transform, n_simplices, d_xq, d_yq, nx, ny, x0, dx, y0, dy};
    const long long T = n_simplices;
    const DsmRasterScratch lay(cells, T);
    IM_GROW(ctx, ctx->grow(ctx->scratch.dsm, lay.bytes, "dsm.scratch"), -71, "im_dsm_rasterize: out of device memory (%lld cells)", cells);
    void* const sc = ctx->scratch.dsm.p;
    int* win = lay.win.at(sc);
    long long* offs = lay.offs.at(sc);
    long long* total = lay.total.at(sc);
    IM_HIP(ctx, hipMemsetAsync(win, 0x7f, cells * sizeof(int), s));
    if (T > 0) {
        const RowScan rs{g, offs};
        IM_LAUNCH(ctx, "dsm_span_scan", s, launch_scan(rs, T, lay.sums.at(sc), total, s));
        int dev_cus = 0;
        IM_HIP(ctx, device_cu_count(&dev_cus));
        IM_LAUNCH(ctx, "dsm_raster", s, launch(dsm_raster_kernel, (dev_cus * 16), 256, 0, s, g, (const long long*)offs, (const long long*)total, win));
    }
    const double4 bounds = make_double4(h_bounds[0], h_bounds[1], h_bounds[2], h_bounds[3]);
    IM_LAUNCH(ctx, "dsm_eval", s, launch(dsm_eval_kernel, blocks_of(cells, 256), 256, 0, s, g, d_bz, (const int*)win, bounds, fill, d_z));
    IM_GUARD_CHECK(ctx, s, "im_dsm_rasterize");
    return 0;
}

extern "C" int im_project_colors(im_ctx* ctx, const double* d_x, long long sxr, long long sxc, const double* d_y, long long syr, long long syc,
                                 const double* d_zc, long long szr, long long szc, int rows, int cols, int cells, const double* h_cam,
                                 const unsigned char* d_img, int h, int w, int cin, const int32_t* h_chmap, int cout, float* d_proj,
                                 double* d_col, unsigned char* d_ortho, void* stream) {
    IM_CHECK_CTX(ctx);
    // cout bounds the channel map below whether or not colours are asked for
    if (!d_x || !d_y || !d_zc || !h_cam || rows < 0 || cols < 0 || cout < 0 || cout > 4) return ctx->fail(-72, "im_project_colors: bad arguments");
    if ((d_col || d_ortho) && (!d_img || !h_chmap || h < 1 || w < 1 || cin < 1 || cout < 1 || cout > 4))
        return ctx->fail(-72, "im_project_colors: bad image arguments");
    if (d_ortho && cout != 3) return ctx->fail(-72, "im_project_colors: an orthophoto has 3 channels (got %d)", cout);
    ColorArgs a{d_x, sxr, sxc, d_y, syr, syc, d_zc, szr, szc, rows, cols, cells, d_img, h, w, cin, cout, {0, 0, 0, 0}, d_proj, d_col, d_ortho};
    for (int ch = 0; ch < cout && h_chmap; ++ch) {
        if (h_chmap[ch] < 0 || h_chmap[ch] >= cin) return ctx->fail(-72, "im_project_colors: bad channel map");
        a.chmap[ch] = h_chmap[ch];
    }
    CamParams p;
    p.fx = h_cam[0]; p.fy = h_cam[1]; p.cx = h_cam[2]; p.cy = h_cam[3];
    for (int k = 0; k < 9; ++k) p.R[k] = h_cam[4 + k];
    for (int k = 0; k < 3; ++k) p.t[k] = h_cam[13 + k];
    for (int k = 0; k < 12; ++k) p.k[k] = h_cam[16 + k];
    const long long n = (long long)rows * cols;
    if (!n) return 0;
    hipStream_t s = (hipStream_t)stream;
    IM_LAUNCH(ctx, "proj_color", s, launch(proj_color_kernel, blocks_of(n, 256), 256, 0, s, a, p));
    IM_GUARD_CHECK(ctx, s, "im_project_colors");
    return 0;
}
