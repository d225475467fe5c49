// The arithmetic of two-view dense stereo (csrc/dense.hip): one sample of a plane sweep over fronto-parallel planes of the reference view,
// the zero-mean normalised cross-correlation of a window out of exact integer sums, the choice of the best plane with its sub-plane
// offset, the consistency of a depth against the other view's map, and the world point and camera-oriented normal of a kept pixel.
// Metashape's matcher (`metashape.py:198-240`: buildDepthMaps, buildDenseCloud) is closed and is NOT reproduced: this is a definition of
// this project's own, restated in numpy by tests/dense_oracle.py. Every quantity behind the coordinate rounding of a sample is
// an integer, so the kernels may sum in any order; what is float64 uses only + - * / sqrt with contraction off, in the association
// written here. A header of its own without the context or any launch code, like warp_pixel.h (whose fix_coord rounds the coordinates):
// tests/dense_host_harness.cpp compiles this very text behind a stub <hip/hip_runtime.h>.
// The later dense stages take from here what they share with the sweep, defined once: the window test and the window sums, the score (with
// the scale of the second window's samples as a parameter), the parabola, the update of the running best and the back-projection
// (refine_pixel.h, flow_pixel.h, fuse_pixel.h). What the kernels share beyond arithmetic is dense_tile.h's, the host checks dense_host.h's.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "warp_pixel.h"

namespace im {
namespace {

constexpr int DENSE_MAX_SIDE = 16384, DENSE_MAX_PLANES = 4096, DENSE_MAX_RADIUS = 7;
constexpr int DENSE_TILE_W = 64, DENSE_TILE_H = 16;      // the ref pixels one block of the sweep owns (not part of the definition)

// H = A + w B entry by entry: the homography of the plane of inverse depth w from ref pixels to src pixels
__device__ __forceinline__ void dense_plane_at(const double* A, const double* B, double w, double* H) {
#pragma clang fp contract(off)
    for (int i = 0; i < 9; ++i) H[i] = A[i] + w * B[i];
}
// plane k of the schedule: w_k = w_first + k w_step
__device__ __forceinline__ void dense_plane(const double* A, const double* B, double w_first, double w_step, int k, double* H) {
#pragma clang fp contract(off)
    dense_plane_at(A, B, w_first + (double)k * w_step, H);
}

// The warped value of ref pixel (u, v): false if z <= 0 (or NaN), a coordinate is not finite or one of the four taps lies outside src
// [h1][w1] (a tap of weight zero included). b = sum of (5-bit weight products) * pixel, the four weights adding up to 1024: 0..261120.
__device__ __forceinline__ bool dense_sample(const uint8_t* src, int h1, int w1, const double* H, int u, int v, int& b) {
#pragma clang fp contract(off)
    const double du = (double)u, dv = (double)v;
    const double x = (H[0] * du + H[1] * dv) + H[2];
    const double y = (H[3] * du + H[4] * dv) + H[5];
    const double z = (H[6] * du + H[7] * dv) + H[8];
    b = 0;
    if (!(z > 0.0)) return false;
    int xi = 0, yi = 0, fx = 0, fy = 0;
    if (!fix_coord((x / z) * 32.0, xi, fx) || !fix_coord((y / z) * 32.0, yi, fy)) return false;
    if (xi < 0 || xi + 1 >= w1 || yi < 0 || yi + 1 >= h1) return false;
    const uint8_t* p = src + (long)yi * w1 + xi;
    const int p00 = p[0], p01 = p[1], p10 = p[w1], p11 = p[w1 + 1];
    b = ((32 - fx) * (32 - fy)) * p00 + (fx * (32 - fy)) * p01 + ((32 - fx) * fy) * p10 + (fx * fy) * p11;
    return true;
}

// does the window of radius r centred on (x, y) lie inside an image [h][w]?
__device__ __forceinline__ bool window_inside(int x, int y, int r, int h, int w) { return x >= r && x < w - r && y >= r && y < h - r; }

// Sum and sum of squares of the (2 r + 1)^2 byte window centred on *c (rows of `stride` bytes: an image itself, or a staged tile). Up to
// r = 15 (flow_pixel.h) 961 * 255^2 < 2^26, so 32 bits would hold either sum; the accumulators are int64 all the same, because with uint32
// the compiler gathers four bytes into a word for a dot product, and that form measured slower on the MI355X in the sweep and the costs
// (r = 3) and in the flow match (r = 7 and 15) alike.
__device__ __forceinline__ void dense_window_sums(const uint8_t* c, int stride, int r, long long& s1, long long& s2) {
    s1 = s2 = 0;
    for (int dy = -r; dy <= r; ++dy)
        for (int dx = -r; dx <= r; ++dx) {
            const long long p = c[dy * stride + dx];
            s1 += p; s2 += p * p;
        }
}

// The score of two windows of n = (2 r + 1)^2 samples each from their integer sums. false: too little texture in either window (or none: a
// zero variance would divide by zero, so it is invalid whatever min_var is). scale_b, the last argument, is the scale of the second window's
// samples against bytes, which its variance threshold carries: DENSE_WARPED for warped samples (sums of weights adding up to 1024, so 2^20
// in a variance), which is what the sweep's callers get by leaving it out, and 1 for bytes. n sbb <= 225^2 2^36 < 2^52 (warped, r <= 7) and
// 961^2 2^26 < 2^46 (bytes, r <= 15): every product fits an int64.
constexpr long long DENSE_WARPED = 1LL << 20;
__device__ __forceinline__ bool dense_score(long long n, long long sa, long long saa, long long sb, long long sbb, long long sab, long long min_var,
                                            double& s, long long scale_b = DENSE_WARPED) {
#pragma clang fp contract(off)
    const long long VA = n * saa - sa * sa, VB = n * sbb - sb * sb, C = n * sab - sa * sb;
    s = 0.0;
    if (VA < n * n * min_var || VB < n * n * min_var * scale_b || VA <= 0 || VB <= 0) return false;
    s = (double)C / sqrt((double)VA * (double)VB);
    return true;
}

// The sub-step offset of a best score s0 between its two neighbours sm and sp: the vertex of the parabola through the three where it is a
// maximum (a negative denominator), else 0.
__device__ __forceinline__ double parabola_offset(double sm, double s0, double sp) {
#pragma clang fp contract(off)
    const double den = (sm - 2.0 * s0) + sp;
    return den < 0.0 ? (0.5 * (sm - sp)) / den : 0.0;
}

// The running choice of one pixel over the planes in ascending order: the best valid score, its predecessor and its successor.
// flags: 1 = the predecessor of the best scored, 2 = its successor did, 4 = the plane before the next one did (one word and not three
// bools: on the device a bool per lane is a 64-bit mask in two scalar registers, and four pixels' worth of them spilled)
struct DenseBest {
    double s0, sm, sp, prev;
    int k, flags;
};
__device__ __forceinline__ void dense_best_init(DenseBest& b) {
    b.s0 = b.sm = b.sp = b.prev = 0.0;
    b.k = -1;
    b.flags = 0;
}
// Plane k scored s (valid) or did not (s is ignored then): it becomes the best (take), or it is the successor of the best, and either way
// it is remembered as the predecessor of the next. `take` is the caller's rule; it implies valid.
__device__ __forceinline__ void dense_best_update(DenseBest& b, int k, bool take, bool valid, double s) {
    if (take) {
        b.s0 = s; b.k = k;
        b.sm = b.prev; b.sp = 0.0;
        b.flags = (b.flags >> 2) & 1;
    } else if (b.k >= 0 && k == b.k + 1) {
        b.sp = s; b.flags |= valid ? 2 : 0;
    }
    b.prev = valid ? s : 0.0;
    b.flags = (b.flags & 3) | (valid ? 4 : 0);
}
// The sweep's rule: a later plane replaces the best only if strictly greater.
__device__ __forceinline__ void dense_best_step(DenseBest& b, int k, bool valid, double s) {
    dense_best_update(b, k, valid && (b.k < 0 || s > b.s0), valid, s);
}
// plane = -1, w = 0, score = 0 where no plane scored or the best is below min_score
__device__ __forceinline__ void dense_best_finish(const DenseBest& b, int D, double w_first, double w_step, double min_score, int16_t& plane,
                                                  double& w, float& score) {
#pragma clang fp contract(off)
    plane = -1; w = 0.0; score = 0.0f;
    if (b.k < 0 || b.s0 < min_score) return;
    const double off = b.k >= 1 && b.k <= D - 2 && (b.flags & 3) == 3 ? parabola_offset(b.sm, b.s0, b.sp) : 0.0;
    plane = (int16_t)b.k;
    w = w_first + ((double)b.k + off) * w_step;
    score = (float)b.s0;
}

// The pose behind the consistency check: Ki = inv(K0) [9], R [9] and t [3] of X1 = R X0 + t, K1 [9]; all row-major
struct DensePose { double Ki[9], R[9], t[3], K1[9]; };
static_assert(sizeof(DensePose) == 30 * sizeof(double), "h_pose of im_dense_consistency is 30 doubles");

// X0 = Ki (x, y, 1) / w, at a position that need not be a pixel centre (flow_pixel.h), and at pixel (u, v): an int converts exactly
__device__ __forceinline__ void dense_backproject_at(const double* Ki, double x, double y, double w, double* X) {
#pragma clang fp contract(off)
    X[0] = ((Ki[0] * x + Ki[1] * y) + Ki[2]) / w;
    X[1] = ((Ki[3] * x + Ki[4] * y) + Ki[5]) / w;
    X[2] = ((Ki[6] * x + Ki[7] * y) + Ki[8]) / w;
}
__device__ __forceinline__ void dense_backproject(const double* Ki, int u, int v, double w, double* X) {
    dense_backproject_at(Ki, (double)u, (double)v, w, X);
}

// Is the depth of kept pixel (u, v) of map 0 (inverse depth w) met by map 1 [h1][w1] (plane1 < 0: dropped)? The nearest pixel of view 1
// by rint; tol = tau |w_step1|.
__device__ __forceinline__ bool dense_consistent(const DensePose& P, int u, int v, double w, const int16_t* plane1, const double* wmap1, int h1, int w1,
                                                 double tol) {
#pragma clang fp contract(off)
    double X0[3], X1[3];
    dense_backproject(P.Ki, u, v, w, X0);
    for (int i = 0; i < 3; ++i) X1[i] = ((P.R[3 * i] * X0[0] + P.R[3 * i + 1] * X0[1]) + P.R[3 * i + 2] * X0[2]) + P.t[i];
    if (!(X1[2] > 0.0)) return false;
    const double px = (P.K1[0] * X1[0] + P.K1[1] * X1[1]) + P.K1[2] * X1[2];
    const double py = (P.K1[3] * X1[0] + P.K1[4] * X1[1]) + P.K1[5] * X1[2];
    const double pz = (P.K1[6] * X1[0] + P.K1[7] * X1[1]) + P.K1[8] * X1[2];
    const double ju = rint(px / pz), jv = rint(py / pz);
    if (!(ju >= 0.0 && ju <= (double)(w1 - 1) && jv >= 0.0 && jv <= (double)(h1 - 1))) return false;      // NaN fails
    const long j = (long)jv * w1 + (long)ju;
    if (plane1[j] < 0) return false;
    return fabs(wmap1[j] - 1.0 / X1[2]) <= tol;
}

// The camera of the cloud: Ki = inv(K0) [9], R0 [9], t0 [3] of X_cam = R0 X_world + t0
struct DenseCam { double Ki[9], R[9], t[3]; };
static_assert(sizeof(DenseCam) == 21 * sizeof(double), "h_cam of im_dense_cloud is 21 doubles");

// world = R0^T (X0 - t0)
__device__ __forceinline__ void dense_to_world(const DenseCam& c, const double* X0, double* W) {
#pragma clang fp contract(off)
    const double d0 = X0[0] - c.t[0], d1 = X0[1] - c.t[1], d2 = X0[2] - c.t[2];
    for (int i = 0; i < 3; ++i) W[i] = (c.R[i] * d0 + c.R[3 + i] * d1) + c.R[6 + i] * d2;
}
__device__ __forceinline__ void dense_world_point(const DenseCam& c, int u, int v, double w, double* W) {
    double X0[3];
    dense_backproject(c.Ki, u, v, w, X0);
    dense_to_world(c, X0, W);
}

// The difference of the world points along one image direction at kept pixel i (stride `step` pixels; lo / hi: the neighbour exists):
// central where both neighbours are kept, one-sided where one is, false where neither is.
__device__ __forceinline__ bool dense_tangent(const DenseCam& c, const uint8_t* keep, const double* wmap, long i, long step, bool lo, bool hi, int u, int v,
                                              int du, int dv, const double* W, double* T) {
#pragma clang fp contract(off)
    const bool kl = lo && keep[i - step] != 0, kh = hi && keep[i + step] != 0;
    if (!kl && !kh) return false;
    double L[3] = {W[0], W[1], W[2]}, Hh[3] = {W[0], W[1], W[2]};
    if (kl) dense_world_point(c, u - du, v - dv, wmap[i - step], L);
    if (kh) dense_world_point(c, u + du, v + dv, wmap[i + step], Hh);
    for (int a = 0; a < 3; ++a) T[a] = Hh[a] - L[a];
    return true;
}

// The world point W and the unit normal N of kept pixel (u, v): the cross product of the two tangents, turned towards the camera centre
// (N . (C0 - W) >= 0); zero where a direction has no kept neighbour or the product has no finite positive length.
__device__ __forceinline__ void dense_point(const DenseCam& c, const uint8_t* keep, const double* wmap, int h, int w, int u, int v, double* W, double* N) {
#pragma clang fp contract(off)
    const long i = (long)v * w + u;
    dense_world_point(c, u, v, wmap[i], W);
    N[0] = N[1] = N[2] = 0.0;
    double Tu[3], Tv[3];
    if (!dense_tangent(c, keep, wmap, i, 1, u > 0, u + 1 < w, u, v, 1, 0, W, Tu)) return;
    if (!dense_tangent(c, keep, wmap, i, w, v > 0, v + 1 < h, u, v, 0, 1, W, Tv)) return;
    const double nx = Tu[1] * Tv[2] - Tu[2] * Tv[1], ny = Tu[2] * Tv[0] - Tu[0] * Tv[2], nz = Tu[0] * Tv[1] - Tu[1] * Tv[0];
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    if (!(len > 0.0) || !(len <= 1.7976931348623157e308)) return;
    const double zero[3] = {0.0, 0.0, 0.0};
    double C0[3];
    dense_to_world(c, zero, C0);
    double n[3] = {nx / len, ny / len, nz / len};
    const double dot = (n[0] * (C0[0] - W[0]) + n[1] * (C0[1] - W[1])) + n[2] * (C0[2] - W[2]);
    const bool flip = dot < 0.0;
    for (int a = 0; a < 3; ++a) N[a] = flip ? -n[a] : n[a];
}

}  // namespace
}  // namespace im
