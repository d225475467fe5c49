// The arithmetic of one point, one cell and one report of csrc/dod.hip: the DEM of difference between two clouds (CloudCompare's 2.5D
// volume, restated in DESIGN §4) and the even-odd polygon rule of the crop. IEEE float64 with contraction off, a header of its own without
// the context or any launch code, like knn_point.h and warp_pixel.h: a host program compiles the very text the kernels compile
// (tests/dod_host_harness.cpp, through a stub <hip/hip_runtime.h>) and is compared with the numpy restatement (tests/dod_oracle.py) bit
// for bit. The host half of dod.hip calls the same functions for the grid of a pair, so the cell cap is decided by this text too.
#pragma once
#include <hip/hip_runtime.h>

// the host half of dod.hip calls these too; a plain host compiler (the stub <hip/hip_runtime.h>) knows no __host__
#if defined(__HIP__) || defined(__HIPCC__)
#define DOD_FN __host__ __device__ __forceinline__
#else
#define DOD_FN inline
#endif

namespace im {
namespace {

constexpr int DOD_CHUNK = 1024;                // B: consecutive cells whose H are summed in ascending cell index, partials in chunk order
constexpr int DOD_REPORT = 16;                 // doubles per pair of the report, the DOD_* slots below
constexpr int DOD_MAX_VERTS = 1024;            // vertices of a crop polygon (16 KB of LDS)
enum { DOD_VOLUME, DOD_ADDED, DOD_REMOVED, DOD_SURFACE, DOD_MATCHING, DOD_GROUND_ONLY, DOD_CEIL_ONLY, DOD_NEIGHBOURS, DOD_VALID_CELLS,
       DOD_CELL_COUNT, DOD_WIDTH, DOD_HEIGHT, DOD_MIN_X, DOD_MIN_Y, DOD_STEP, DOD_AREA };
enum { DOD_N_VALID, DOD_N_FILLED, DOD_N_GROUND_ONLY, DOD_N_CEIL_ONLY, DOD_N_NEIGHBOURS, DOD_N_COUNTS };

DOD_FN double dod_nan() { return __builtin_nan(""); }
DOD_FN double dod_inf() { return __builtin_huge_val(); }
DOD_FN bool dod_finite(double v) { return __builtin_isfinite(v); }

// a point with any non-finite coordinate is ignored everywhere
DOD_FN bool dod_kept(double x, double y, double z) { return dod_finite(x) && dod_finite(y) && dod_finite(z); }

// vertDim d: the grid's axes are X = (d + 1) mod 3 and Y = (d + 2) mod 3
DOD_FN int dod_axis_x(int d) { return (d + 1) % 3; }
DOD_FN int dod_axis_y(int d) { return (d + 2) % 3; }

// Ascending unsigned order == ascending value (-0.0 below +0.0); a finite value never maps to 0 or to ~0, so that 0 can stand for "no
// point yet" under atomicMax of the key (a maximum) and of its complement (a minimum).
DOD_FN unsigned long long dod_order_key(double v) {
    unsigned long long u;
    __builtin_memcpy(&u, &v, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
DOD_FN double dod_order_value(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k ^ 0x8000000000000000ull) : ~k;
    double v;
    __builtin_memcpy(&v, &u, 8);
    return v;
}

// floor((v - min) / s + 0.5): the column or row of a coordinate, cells centred on min + k s
DOD_FN double dod_cell_coord(double v, double mn, double s) {
#pragma clang fp contract(off)
    return __builtin_floor((v - mn) / s + 0.5);
}
// cells along an axis: 1 + floor((max - min) / s + 0.5), as a double (it may exceed any integer); 0 when no point was kept (min > max)
DOD_FN double dod_grid_dim(double mn, double mx, double s) {
#pragma clang fp contract(off)
    if (!(mn <= mx)) return 0.0;
    return 1.0 + dod_cell_coord(mx, mn, s);
}
// The grid of a pair from the bounds (min_x, min_y, max_x, max_y) of its two clouds, +inf / -inf where a cloud kept no point: the union
// box, of zeros of either sign the minimum -0.0 and the maximum +0.0 as the keys order them. wd and hd are 0.0 when neither kept a point.
DOD_FN void dod_pair_grid(const double* bg, const double* bc, double s, double& min_x, double& min_y, double& wd, double& hd) {
    min_x = dod_order_key(bg[0]) <= dod_order_key(bc[0]) ? bg[0] : bc[0];
    min_y = dod_order_key(bg[1]) <= dod_order_key(bc[1]) ? bg[1] : bc[1];
    const double max_x = dod_order_key(bg[2]) >= dod_order_key(bc[2]) ? bg[2] : bc[2];
    const double max_y = dod_order_key(bg[3]) >= dod_order_key(bc[3]) ? bg[3] : bc[3];
    wd = dod_grid_dim(min_x, max_x, s);
    hd = dod_grid_dim(min_y, max_y, s);
    if (wd == 0.0 || hd == 0.0) { wd = hd = 0.0; min_x = min_y = 0.0; }
}
// j w + i, or -1 for a coordinate outside the grid (none is, for the grid of the pair's own bounds)
DOD_FN long long dod_cell_of(double x, double y, double min_x, double min_y, double s, long long w, long long h) {
    const double ti = dod_cell_coord(x, min_x, s), tj = dod_cell_coord(y, min_y, s);
    if (!(ti >= 0.0 && ti < (double)w && tj >= 0.0 && tj < (double)h)) return -1;
    return (long long)tj * w + (long long)ti;
}

// the mean of a cell: get(k) = the d-coordinate of its k-th point in ascending input index, summed from +0.0
template <typename Get>
DOD_FN double dod_mean(Get get, long long count) {
#pragma clang fp contract(off)
    double sum = 0.0;
    for (long long k = 0; k < count; ++k) sum += get(k);
    return sum / (double)count;
}

// H of a cell whose two counts are > 0
DOD_FN double dod_diff(double mean_ground, double mean_ceil) {
#pragma clang fp contract(off)
    return mean_ceil - mean_ground;
}
DOD_FN bool dod_valid(double H) { return dod_finite(H); }

// The three sums over the n <= DOD_CHUNK cells of one chunk (which = DOD_VOLUME: every valid H, DOD_ADDED: H > 0, DOD_REMOVED: H < 0), in
// ascending cell index from +0.0; and the sum of the n chunk partials in ascending chunk index, which is the same loop over them.
DOD_FN bool dod_counts_for(double H, int which) {
    return dod_valid(H) && (which == DOD_VOLUME || (which == DOD_ADDED ? H > 0.0 : H < 0.0));
}
template <typename Get>
DOD_FN double dod_chunk_sum(Get get, long long n, int which) {
#pragma clang fp contract(off)
    double sum = 0.0;
    for (long long k = 0; k < n; ++k) {
        const double H = get(k);
        if (dod_counts_for(H, which)) sum += H;
    }
    return sum;
}
template <typename Get>
DOD_FN double dod_partial_sum(Get get, long long n) {
#pragma clang fp contract(off)
    double sum = 0.0;
    for (long long k = 0; k < n; ++k) sum += get(k);
    return sum;
}

// how many of the 8 in-grid neighbours of cell (i, j) are valid; valid_at(i, j) is asked for cells inside the grid only
template <typename ValidAt>
DOD_FN int dod_neighbours(ValidAt valid_at, long long i, long long j, long long w, long long h) {
    int n = 0;
    for (int dj = -1; dj <= 1; ++dj)
        for (int di = -1; di <= 1; ++di) {
            const long long ii = i + di, jj = j + dj;
            if ((di || dj) && ii >= 0 && ii < w && jj >= 0 && jj < h && valid_at(ii, jj)) ++n;
        }
    return n;
}

// the report of one pair from its three sums and five integer counts
DOD_FN void dod_report(double* r, const double* sums, const unsigned long long* n, double s, long long w, long long h,
                                           double min_x, double min_y) {
#pragma clang fp contract(off)
    const double a = s * s, valid = (double)n[DOD_N_VALID], filled = (double)n[DOD_N_FILLED];
    for (int k = 0; k < DOD_REPORT; ++k) r[k] = 0.0;
    r[DOD_CELL_COUNT] = filled; r[DOD_WIDTH] = (double)w; r[DOD_HEIGHT] = (double)h;
    r[DOD_MIN_X] = w ? min_x : 0.0; r[DOD_MIN_Y] = h ? min_y : 0.0;
    r[DOD_STEP] = s; r[DOD_AREA] = a;
    if (!n[DOD_N_VALID]) return;                                       // no valid cell: every figure is +0.0
    r[DOD_VOLUME] = a * sums[DOD_VOLUME];
    r[DOD_ADDED] = a * sums[DOD_ADDED];
    r[DOD_REMOVED] = a * (0.0 - sums[DOD_REMOVED]);                    // 0 - sum: nothing removed reads +0.0, not -0.0
    r[DOD_SURFACE] = a * valid;
    r[DOD_MATCHING] = (100.0 * valid) / filled;
    r[DOD_GROUND_ONLY] = (100.0 * (double)n[DOD_N_GROUND_ONLY]) / filled;
    r[DOD_CEIL_ONLY] = (100.0 * (double)n[DOD_N_CEIL_ONLY]) / filled;
    r[DOD_NEIGHBOURS] = (double)n[DOD_N_NEIGHBOURS] / valid;
    r[DOD_VALID_CELLS] = valid;
}

// Even-odd crossing rule: (x, y) against the closed polygon of nv vertices, vert(k, vx, vy) its k-th. A point with a non-finite
// coordinate is outside.
template <typename Vert>
DOD_FN bool dod_in_polygon(Vert vert, int nv, double x, double y) {
#pragma clang fp contract(off)
    if (!dod_finite(x) || !dod_finite(y)) return false;
    bool in = false;
    double x0, y0;
    vert(nv - 1, x0, y0);
    for (int k = 0; k < nv; ++k) {
        double x1, y1;
        vert(k, x1, y1);
        if ((y0 > y) != (y1 > y) && x < (x1 - x0) * (y - y0) / (y1 - y0) + x0) in = !in;
        x0 = x1; y0 = y1;
    }
    return in;
}

}  // namespace
}  // namespace im
