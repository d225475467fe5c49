// The arithmetic of one point, one group, one (triangle, grid row) span, one cell and one coloured item of csrc/dsm.hip: the float32
// rounding of the binning and its sort keys, pandas' Kahan mean of a group, the grid rows and columns a triangle can reach, scipy's
// barycentric inside test and interpolation, and cv2.projectPoints with the bilinear sampling of the image. IEEE float32 / float64 with
// contraction off, a header of its own without the context or any launch code, like dod_cell.h, voxel_cell.h and warp_pixel.h: a host
// program compiles the very text the kernels compile (tests/dsm_host_harness.cpp, through a stub <hip/hip_runtime.h>) and is compared
// with the numpy restatement (tests/dsm_oracle.py) bit for bit on tests/dsm_cases.py.
// Divisions are plain `/`: float32 and float64 division are correctly rounded on the device and the library is built without a
// fast-math flag, so no rounding intrinsic is needed and the host compiles the same expression. Bit casts go through __builtin_memcpy.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

namespace im {
namespace {

constexpr double DSM_EPS = 100.0 * 2.220446049250313e-16;   // scipy's inside tolerance, 100 * DBL_EPSILON
constexpr int WIN_NONE = 0x7f7f7f7f;                           // hipMemset byte 0x7f: no triangle contains the cell

// sortable keys: ascending unsigned order == ascending value; -0.0 folded into +0.0 (pandas groups by value)
__device__ __forceinline__ uint32_t f32_key(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    if (u == 0x80000000u) u = 0;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ long long f64_key(double d) {   // NaN after everything, all NaN equal (numpy's sort order)
    if (d != d) return LLONG_MAX;
    unsigned long long u;
    __builtin_memcpy(&u, &d, 8);
    if (u == 0x8000000000000000ull) u = 0;
    u = (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
    return (long long)(u ^ 0x8000000000000000ull);
}

// point i: float32 rounding of x, y to the step and the three sort keys
__device__ __forceinline__ void dsm_round_point(const double* __restrict__ pts, long long i, float step, float* __restrict__ xr,
                                                float* __restrict__ yr, long long* __restrict__ xykey, long long* __restrict__ ykey,
                                                long long* __restrict__ zkey) {
#pragma clang fp contract(off)
    const float x = (float)pts[3 * i], y = (float)pts[3 * i + 1];
    const float qx = rintf(x / step) * step;   // np.round: half to even
    const float qy = rintf(y / step) * step;
    xr[i] = qx;
    yr[i] = qy;
    const uint32_t kx = f32_key(qx), ky = f32_key(qy);
    xykey[i] = (long long)((((unsigned long long)kx << 32) | ky) ^ 0x8000000000000000ull);
    ykey[i] = (long long)ky;
    zkey[i] = f64_key(pts[3 * i + 2]);
}

// a rounded coordinate whose key is +-0: the group keeps the sign of the first such row in the reference's sort order
__device__ __forceinline__ bool dsm_zero_key(float v) { return v == 0.f; }

// 1 where sorted row j starts a new (x, y) group
__device__ __forceinline__ long long dsm_group_count(const long long* key, const long long* perm, long long n, long long j) {
    return j < n && (j == 0 || key[perm[j]] != key[perm[j - 1]]) ? 1 : 0;
}

// group g of G: its x, y (a zero with the sign the reference keeps) and pandas' Kahan mean of its z in ascending-z order
__device__ __forceinline__ void dsm_group_mean(const double* __restrict__ pts, const float* __restrict__ xr, const float* __restrict__ yr,
                                               const long long* __restrict__ perm_b, const long long* __restrict__ perm_c,
                                               const int* __restrict__ zero_first, const long long* __restrict__ starts, long long G, long long n,
                                               long long g, float* __restrict__ bx, float* __restrict__ by, float* __restrict__ bz) {
#pragma clang fp contract(off)
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
    bz[g] = cnt ? (float)(s / (double)cnt) : __builtin_nanf("");
}

struct TriGrid {
    const float* bx; const float* by;   // binned points (float32; float64 of them is what qhull saw)
    const int* simp;                    // [T][3]
    const double* tr;                   // [T][3][2] scipy's barycentric transforms
    long long T;
    const double* xq; const double* yq; int nx, ny;
    double x0, dx, y0, dy;              // xq[c] == x0 + c * dx (np.arange's own delta), likewise yq
};

// the grid rows r0..r1 a triangle can reach, one row of margin on each side (r1 < r0: none)
__device__ __forceinline__ void tri_rows(const TriGrid& g, long long t, int& r0, int& r1) {
    r0 = 0; r1 = -1;
    if (!(g.tr[6 * t] == g.tr[6 * t])) return;   // NaN transform: a degenerate simplex never contains a cell
    const double ya = g.by[g.simp[3 * t]], yb = g.by[g.simp[3 * t + 1]], yc = g.by[g.simp[3 * t + 2]];
    const double lo = fmin(ya, fmin(yb, yc)), hi = fmax(ya, fmax(yb, yc));
    const double a = fmax(floor((lo - g.y0) / g.dy) - 1.0, 0.0), b = fmin(ceil((hi - g.y0) / g.dy) + 1.0, (double)(g.ny - 1));
    if (!(a <= b)) return;
    r0 = (int)a; r1 = (int)b;
}

// spans (grid rows) of triangle t, 0 beyond the last triangle
__device__ __forceinline__ long long tri_span_count(const TriGrid& g, long long t) {
    if (t >= g.T) return 0;
    int r0, r1;
    tri_rows(g, t, r0, r1);
    return r1 - r0 + 1;
}

// the columns c0..c1 of grid row r that triangle t can reach: the x-range of the triangle at the row (rows of the margin use the nearest
// row of the triangle) and one column of margin on each side; false: none
__device__ __forceinline__ bool tri_span_columns(const TriGrid& g, long long t, int r, int& c0, int& c1) {
#pragma clang fp contract(off)
    const double y = g.yq[r];
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
    if (!(xlo <= xhi)) return false;
    // one column of margin on each side: the exact test decides
    const double a = fmax(floor((xlo - g.x0) / g.dx) - 1.0, 0.0), b = fmin(ceil((xhi - g.x0) / g.dx) + 1.0, (double)(g.nx - 1));
    if (!(a <= b)) return false;
    c0 = (int)a; c1 = (int)b;
    return true;
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

// span (t, r): claim(cell) for every cell of the row that triangle t contains; the caller keeps the lowest t per cell
template <typename Claim>
__device__ __forceinline__ void tri_span_cells(const TriGrid& g, long long t, int r, Claim claim) {
#pragma clang fp contract(off)
    int ca, cb;
    if (!tri_span_columns(g, t, r, ca, cb)) return;
    const double y = g.yq[r];
    const double* T = g.tr + 6 * t;
    for (int c = ca; c <= cb; ++c) {
        double c0, c1, c2;
        if (bary(T, g.xq[c], y, c0, c1, c2)) claim((long long)r * g.nx + c);
    }
}

// z of one cell from its winning triangle: barycentric interpolation in scipy's operation order, float64. bounds: min x, min y, max x,
// max y of the triangulated points.
__device__ __forceinline__ double dsm_eval_cell(const TriGrid& g, const float* __restrict__ bz, const int* __restrict__ win, double bx0, double by0,
                                                double bx1, double by1, double fill, long long cell) {
#pragma clang fp contract(off)
    const int r = (int)(cell / g.nx), c = (int)(cell - (long long)r * g.nx);
    const double qx = g.xq[c], qy = g.yq[r];
    const int s = win[cell];
    // scipy's `_is_point_fully_outside`: outside the points' bounding box (+- eps) is outside
    if (s == WIN_NONE || qx < bx0 - DSM_EPS || qx > bx1 + DSM_EPS || qy < by0 - DSM_EPS || qy > by1 + DSM_EPS) return fill;
    double c0, c1, c2;
    bary(g.tr + 6 * (long long)s, qx, qy, c0, c1, c2);
    const double v0 = bz[g.simp[3 * s]], v1 = bz[g.simp[3 * s + 1]], v2 = bz[g.simp[3 * s + 2]];
    return ((0.0 + c0 * v0) + c1 * v1) + c2 * v2;
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

// np.floor(u).astype(int) on x86: out of range / NaN -> INT64_MIN. The cast is valid for every |f| < 2^63 (the largest such float32 is
// 2^63 - 2^39) and -2^63 itself casts to INT64_MIN: a tighter bound sends a corner to column 0 that numpy clips to the last column.
__device__ __forceinline__ long long floor_index(float u) {
    const float f = floorf(u);
    return (f == f && fabsf(f) < 9223372036854775808.0f) ? (long long)f : LLONG_MIN;
}
__device__ __forceinline__ long long clip(long long v, long long hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ unsigned char to_u8(double v) {    // np.uint8(float64) on x86: truncation to int32, low byte
    return (v == v && v > -2147483649.0 && v < 2147483648.0) ? (unsigned char)((int)v & 0xff) : 0;
}

// item i (a point, or cell i of a grid): its projection, colours and orthophoto bytes, each where asked for
__device__ __forceinline__ void proj_color_item(const ColorArgs& a, const CamParams& p, long long i) {
#pragma clang fp contract(off)
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
        const double Ia = (float)pa[m] / 255.0f, Ib = (float)pb[m] / 255.0f;
        const double Ic = (float)pc[m] / 255.0f, Id = (float)pd[m] / 255.0f;
        const double sum = ((wa * Ia + wb * Ib) + wc * Ic) + wd * Id;
        if (a.col) a.col[i * a.cout + ch] = sum;
        if (a.ortho) a.ortho[3 * i + ch] = to_u8((double)(float)sum * 255.0);
    }
}

}  // namespace
}  // namespace im
