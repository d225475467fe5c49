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
// Every function that must reproduce the reference's rounding keeps contraction off: whether a * b + c becomes one fused operation
// is otherwise the compiler's choice (`__fmul_rn` / `__fadd_rn` do not prevent it on this toolchain, lg_misc.hip).
#include <climits>
#include <cmath>

#include "common.h"
#include "ctx.h"
#include "stage_scratch.h"

namespace im {
namespace {

constexpr double DSM_EPS = 100.0 * 2.220446049250313e-16;   // scipy's inside tolerance, 100 * DBL_EPSILON
constexpr int WIN_NONE = 0x7f7f7f7f;                           // hipMemset byte 0x7f: no triangle contains the cell

// sortable keys: ascending unsigned order == ascending value; -0.0 folded into +0.0 (pandas groups by value)
__device__ __forceinline__ uint32_t f32_key(float f) {
    uint32_t u = __float_as_uint(f);
    if (u == 0x80000000u) u = 0;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ long long f64_key(double d) {   // NaN after everything, all NaN equal (numpy's sort order)
    if (d != d) return LLONG_MAX;
    unsigned long long u = (unsigned long long)__double_as_longlong(d);
    if (u == 0x8000000000000000ull) u = 0;
    u = (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
    return (long long)(u ^ 0x8000000000000000ull);
}

__global__ __launch_bounds__(256) void dsm_round_kernel(const double* __restrict__ pts, long long n, float step, float* __restrict__ xr,
                                                        float* __restrict__ yr, long long* __restrict__ xykey, long long* __restrict__ ykey,
                                                        long long* __restrict__ zkey) {
#pragma clang fp contract(off)
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = (float)pts[3 * i], y = (float)pts[3 * i + 1];
    const float qx = rintf(__fdiv_rn(x, step)) * step;   // np.round: half to even
    const float qy = rintf(__fdiv_rn(y, step)) * step;
    xr[i] = qx;
    yr[i] = qy;
    const uint32_t kx = f32_key(qx), ky = f32_key(qy);
    xykey[i] = (long long)((((unsigned long long)kx << 32) | ky) ^ 0x8000000000000000ull);
    ykey[i] = (long long)ky;
    zkey[i] = f64_key(pts[3 * i + 2]);
}

__global__ __launch_bounds__(256) void dsm_zero_first_kernel(const float* __restrict__ xr, const float* __restrict__ yr,
                                                             const long long* __restrict__ perm_b, int n, int* __restrict__ first) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const long long i = perm_b[j];
    if (xr[i] == 0.f) atomicMin(&first[0], j);
    if (yr[i] == 0.f) atomicMin(&first[1], j);
}

// ---- exclusive scans over per-item counts (group starts: 0 / 1 per sorted row; triangles: grid rows per triangle): scan.h -----------
#include "scan.h"

struct GroupScan {            // 1 where a sorted row starts a new (x, y) group
    const long long* key;     // [n] (x, y) keys
    const long long* perm;    // [n] rows in group order
    long long n;
    long long* starts;        // [G] first sorted position of each group
    __device__ long long count(long long j) const { return j < n && (j == 0 || key[perm[j]] != key[perm[j - 1]]) ? 1 : 0; }
    __device__ void write(long long j, long long pos) const { if (j < n && count(j)) starts[pos] = j; }
};

struct TriGrid {
    const float* bx; const float* by;   // binned points (float32; float64 of them is what qhull saw)
    const int* simp;                    // [T][3]
    const double* tr;                   // [T][3][2] scipy's barycentric transforms
    long long T;
    const double* xq; const double* yq; int nx, ny;
    double x0, dx, y0, dy;              // xq[c] == x0 + c * dx (np.arange's own delta), likewise yq
};

__device__ __forceinline__ void tri_rows(const TriGrid& g, long long t, int& r0, int& r1) {
    r0 = 0; r1 = -1;
    if (!(g.tr[6 * t] == g.tr[6 * t])) return;   // NaN transform: a degenerate simplex never contains a cell
    const double ya = g.by[g.simp[3 * t]], yb = g.by[g.simp[3 * t + 1]], yc = g.by[g.simp[3 * t + 2]];
    const double lo = fmin(ya, fmin(yb, yc)), hi = fmax(ya, fmax(yb, yc));
    const double a = fmax(floor((lo - g.y0) / g.dy) - 1.0, 0.0), b = fmin(ceil((hi - g.y0) / g.dy) + 1.0, (double)(g.ny - 1));
    if (!(a <= b)) return;
    r0 = (int)a; r1 = (int)b;
}

struct RowScan {              // grid rows (spans) per triangle
    TriGrid g;
    long long* offs;          // [T] first span of each triangle
    __device__ long long count(long long t) const {
        if (t >= g.T) return 0;
        int r0, r1;
        tri_rows(g, t, r0, r1);
        return r1 - r0 + 1;
    }
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
    const long long j0 = starts[g], j1 = g + 1 < G ? starts[g + 1] : n;
    const long long i0 = perm_c[j0];
    float x = xr[i0], y = yr[i0];
    // a zero key keeps the sign of its first occurrence in the reference's sorted table (pandas factorises each key column)
    if (x == 0.f) x = xr[perm_b[zero_first[0]]];
    if (y == 0.f) y = yr[perm_b[zero_first[1]]];
    double s = 0.0, c = 0.0;
    long long cnt = 0;
    for (long long j = j0; j < j1; ++j) {
        const double v = pts[3 * perm_c[j] + 2];
        if (v != v) continue;
        ++cnt;
        const double yv = v - c;
        const double t = s + yv;
        c = (t - s) - yv;
        if (c != c) c = 0.0;    // pandas: an infinite value makes the compensation NaN; it is reset
        s = t;
    }
    bx[g] = x;
    by[g] = y;
    bz[g] = cnt ? (float)(s / (double)cnt) : __int_as_float(0x7fc00000);
}

// scipy's `_barycentric_inside` (2-D): c_i = 0 + T[i][0] dx + T[i][1] dy, c_2 = (1 - c_0) - c_1, all within [-eps, 1 + eps]
__device__ __forceinline__ bool bary(const double* __restrict__ T, double qx, double qy, double& c0, double& c1, double& c2) {
#pragma clang fp contract(off)
    const double dx = qx - T[4], dy = qy - T[5];
    c0 = (0.0 + T[0] * dx) + T[1] * dy;
    c1 = (0.0 + T[2] * dx) + T[3] * dy;
    c2 = (1.0 - c0) - c1;
    return c0 >= -DSM_EPS && c0 <= 1.0 + DSM_EPS && c1 >= -DSM_EPS && c1 <= 1.0 + DSM_EPS && c2 >= -DSM_EPS && c2 <= 1.0 + DSM_EPS;
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
        const double y = g.yq[r];
        const double* T = g.tr + 6 * t;
        double vx[3], vy[3];
        for (int k = 0; k < 3; ++k) { vx[k] = g.bx[g.simp[3 * t + k]]; vy[k] = g.by[g.simp[3 * t + k]]; }
        const double ylo = fmin(vy[0], fmin(vy[1], vy[2])), yhi = fmax(vy[0], fmax(vy[1], vy[2]));
        const double yc = fmin(fmax(y, ylo), yhi);   // rows of the margin use the nearest row of the triangle
        double xlo = INFINITY, xhi = -INFINITY;
        for (int k = 0; k < 3; ++k) {
            const int m = k == 2 ? 0 : k + 1;
            const double ya = vy[k], yb = vy[m];
            if (yc < fmin(ya, yb) || yc > fmax(ya, yb)) continue;
            if (ya == yb) { xlo = fmin(xlo, fmin(vx[k], vx[m])); xhi = fmax(xhi, fmax(vx[k], vx[m])); continue; }
            const double x = vx[k] + (yc - ya) * ((vx[m] - vx[k]) / (yb - ya));
            xlo = fmin(xlo, x); xhi = fmax(xhi, x);
        }
        if (!(xlo <= xhi)) continue;
        // one column of margin on each side: the exact test below decides
        const double a = fmax(floor((xlo - g.x0) / g.dx) - 1.0, 0.0), b = fmin(ceil((xhi - g.x0) / g.dx) + 1.0, (double)(g.nx - 1));
        if (!(a <= b)) continue;
        int* row = win + (long long)r * g.nx;
        for (int c = (int)a; c <= (int)b; ++c) {
            double c0, c1, c2;
            if (bary(T, g.xq[c], y, c0, c1, c2) && (int)t < row[c]) atomicMin(&row[c], (int)t);
        }
    }
}

__global__ __launch_bounds__(256) void dsm_eval_kernel(TriGrid g, const float* __restrict__ bz, const int* __restrict__ win,
                                                       double4 bounds, double fill, double* __restrict__ z) {
#pragma clang fp contract(off)
    const long long cell = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (cell >= (long long)g.nx * g.ny) return;
    const int r = (int)(cell / g.nx), c = (int)(cell - (long long)r * g.nx);
    const double qx = g.xq[c], qy = g.yq[r];
    const int s = win[cell];
    // scipy's `_is_point_fully_outside`: outside the points' bounding box (+- eps) is outside
    if (s == WIN_NONE || qx < bounds.x - DSM_EPS || qx > bounds.z + DSM_EPS || qy < bounds.y - DSM_EPS || qy > bounds.w + DSM_EPS) {
        z[cell] = fill;
        return;
    }
    double c0, c1, c2;
    bary(g.tr + 6 * (long long)s, qx, qy, c0, c1, c2);
    const double v0 = bz[g.simp[3 * s]], v1 = bz[g.simp[3 * s + 1]], v2 = bz[g.simp[3 * s + 2]];
    z[cell] = ((0.0 + c0 * v0) + c1 * v1) + c2 * v2;
}

// ---- projection + bilinear colours -------------------------------------------------------------------------------------------
struct CamParams { double fx, fy, cx, cy, R[9], t[3], k[12]; };

struct ColorArgs {
    const double* x; long long xr, xc;     // element (r, c) of each coordinate plane at r * xr + c * xc
    const double* y; long long yr, yc;
    const double* z; long long zr, zc;
    int rows, cols, cells;                 // cells: a NaN z is an invalid cell (black, nothing sampled)
    const unsigned char* img; int h, w, cin, cout;
    int chmap[4];                          // output channel -> image channel (BGR -> RGB reverses)
    float* proj; double* col; unsigned char* ortho;   // [n][2], [n][cout], [n][3]; each may be null
};

__device__ __forceinline__ long long floor_index(float u) {   // np.floor(u).astype(int) on x86: out of range / NaN -> INT64_MIN
    const float f = floorf(u);
    return (f == f && fabsf(f) < 9.2e18f) ? (long long)f : LLONG_MIN;
}
__device__ __forceinline__ long long clip(long long v, long long hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ unsigned char to_u8(double v) {    // np.uint8(float64) on x86: truncation to int32, low byte
    return (v == v && v > -2147483649.0 && v < 2147483648.0) ? (unsigned char)((int)v & 0xff) : 0;
}

__global__ __launch_bounds__(256) void proj_color_kernel(ColorArgs a, CamParams p) {
#pragma clang fp contract(off)
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= (long long)a.rows * a.cols) return;
    const long long r = i / a.cols, c = i - r * a.cols;
    const double X = a.x[r * a.xr + c * a.xc], Y = a.y[r * a.yr + c * a.yc], Z = a.z[r * a.zr + c * a.zc];
    if (a.cells && Z != Z) {
        if (a.ortho) a.ortho[3 * i] = a.ortho[3 * i + 1] = a.ortho[3 * i + 2] = 0;
        return;
    }
    // cv2.projectPoints (cvProjectPoints2Internal), float64
    double x = ((p.R[0] * X + p.R[1] * Y) + p.R[2] * Z) + p.t[0];
    double y = ((p.R[3] * X + p.R[4] * Y) + p.R[5] * Z) + p.t[1];
    double zz = ((p.R[6] * X + p.R[7] * Y) + p.R[8] * Z) + p.t[2];
    zz = zz != 0.0 ? 1.0 / zz : 1.0;
    x *= zz;
    y *= zz;
    const double* k = p.k;
    const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
    const double a1 = 2 * x * y, a2 = r2 + 2 * x * x, a3 = r2 + 2 * y * y;
    const double cdist = ((1 + k[0] * r2) + k[1] * r4) + k[4] * r6;
    const double icdist2 = 1.0 / (((1 + k[5] * r2) + k[6] * r4) + k[7] * r6);
    const double xd = ((((x * cdist) * icdist2 + k[2] * a1) + k[3] * a2) + k[8] * r2) + k[9] * r4;
    const double yd = ((((y * cdist) * icdist2 + k[2] * a3) + k[3] * a1) + k[10] * r2) + k[11] * r4;
    const float u = (float)(xd * p.fx + p.cx), v = (float)(yd * p.fy + p.cy);
    if (a.proj) { a.proj[2 * i] = u; a.proj[2 * i + 1] = v; }
    if (!a.col && !a.ortho) return;
    // bilinear_interpolate: clipped corners, weights from the unclipped position, float64
    const long long fu = floor_index(u), fv = floor_index(v);
    const long long x0 = clip(fu, a.w - 1), x1 = clip(fu + 1, a.w - 1), y0 = clip(fv, a.h - 1), y1 = clip(fv + 1, a.h - 1);
    const double du = (double)u, dv = (double)v;
    const double wa = ((double)x1 - du) * ((double)y1 - dv);
    const double wb = ((double)x1 - du) * (dv - (double)y0);
    const double wc = (du - (double)x0) * ((double)y1 - dv);
    const double wd = (du - (double)x0) * (dv - (double)y0);
    const unsigned char* pa = a.img + (y0 * a.w + x0) * a.cin;
    const unsigned char* pb = a.img + (y1 * a.w + x0) * a.cin;
    const unsigned char* pc = a.img + (y0 * a.w + x1) * a.cin;
    const unsigned char* pd = a.img + (y1 * a.w + x1) * a.cin;
    for (int ch = 0; ch < a.cout; ++ch) {
        const int m = a.chmap[ch];
        const double Ia = __fdiv_rn((float)pa[m], 255.0f), Ib = __fdiv_rn((float)pb[m], 255.0f);
        const double Ic = __fdiv_rn((float)pc[m], 255.0f), Id = __fdiv_rn((float)pd[m], 255.0f);
        const double sum = ((wa * Ia + wb * Ib) + wc * Ic) + wd * Id;
        if (a.col) a.col[i * a.cout + ch] = sum;
        if (a.ortho) a.ortho[3 * i + ch] = to_u8((double)(float)sum * 255.0);
    }
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
        n_simplices >= INT_MAX || nx < 0 || ny < 0)
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
    if (!d_x || !d_y || !d_zc || !h_cam || rows < 0 || cols < 0) return ctx->fail(-72, "im_project_colors: bad arguments");
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
