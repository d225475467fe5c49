// The arithmetic of the slanted-window refinement of a dense-stereo depth map (csrc/dense_refine.hip): the slant of a pixel, a least-squares
// plane through the inverse depths of its neighbourhood out of exact integer sums, and the refined inverse depth of a pixel, the best of a
// few candidates around the current one, each scored over a window whose samples follow the slant instead of sharing the centre's depth.
// Metashape's matcher is closed and is NOT reproduced: this is a definition of this project's own, restated in numpy by
// tests/refine_oracle.py. Slants are in plane steps per pixel. Every sum is an integer, so the kernels may sum in any order; what is float64
// uses only + - * / with contraction off, in the association written here. The sample, the window sums, the score, the update of the running
// best and the parabola are dense_pixel.h's, defined once.
// A header of its own without the context or any launch code: tests/refine_host_harness.cpp compiles this very text behind a stub
// <hip/hip_runtime.h>.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>

#include "dense_pixel.h"

namespace im {
namespace {

constexpr int REFINE_MAX_FIT_RADIUS = 7, REFINE_MIN_COUNT = 3, REFINE_MAX_COUNT = 225, REFINE_MAX_SPAN = 4, REFINE_MAX_SUB = 8;
constexpr double REFINE_MAX_DIFF = 64.0;                  // plane steps: the largest gate, so that a height fits 17 bits and a sign
constexpr long long REFINE_Q = 1024;                      // heights are counted in 1024ths of a plane step

// The headroom of the fit in int64: n <= 225, |dx|, |dy| <= 7, |q| <= 64 * 1024. a11, a22 and a12 are differences of two terms of at most
// 225^2 * 49 each, b1 and b2 of two terms of at most 225^2 * 7 * 2^16; the numerators of gu and gv are differences of two products a * b,
// det of two products a * a.
constexpr long long REFINE_A_MAX = 2LL * 225 * 225 * 49, REFINE_B_MAX = 2LL * 225 * 225 * 7 * 64 * REFINE_Q;
static_assert(REFINE_MAX_COUNT == (2 * REFINE_MAX_FIT_RADIUS + 1) * (2 * REFINE_MAX_FIT_RADIUS + 1), "n is at most one neighbourhood");
static_assert(REFINE_A_MAX < (1LL << 23) && REFINE_B_MAX < (1LL << 36) && 2 * REFINE_A_MAX * REFINE_B_MAX < (1LL << 60) &&
                  2 * REFINE_A_MAX * REFINE_A_MAX < (1LL << 47),
              "the normal equations of the slant fit stay inside an int64");

// ---- (1) the slant ------------------------------------------------------------------------------------------------------------------------
struct SlantSums { long long n, sx, sy, sxx, syy, sxy, sq, sqx, sqy; };

// Does neighbour j (inverse depth w_j) count for pixel i, and at which height q = llrint(1024 d), d = (w_j - w_i) / w_step? A NaN fails.
__device__ __forceinline__ bool slant_height(double w_i, double w_j, double w_step, double max_diff, long long& q) {
#pragma clang fp contract(off)
    const double d = (w_j - w_i) / w_step;
    q = 0;
    if (!(fabs(d) <= max_diff)) return false;
    q = llrint(d * 1024.0);                                // ties to even; |d| <= 64: no overflow
    return true;
}

__device__ __forceinline__ void slant_add(SlantSums& s, long long dx, long long dy, long long q) {
    s.n += 1; s.sx += dx; s.sy += dy; s.sxx += dx * dx; s.syy += dy * dy; s.sxy += dx * dy;
    s.sq += q; s.sqx += q * dx; s.sqy += q * dy;
}

// The least-squares plane q = q0 + 1024 (gu dx + gv dy) through the counted neighbours: fitted if there are at least min_count of them and they
// do not lie on one line (det > 0; det >= 0 always). gu = gv = 0 otherwise.
__device__ __forceinline__ bool slant_fit(const SlantSums& s, int min_count, double& gu, double& gv) {
#pragma clang fp contract(off)
    const long long a11 = s.n * s.sxx - s.sx * s.sx, a22 = s.n * s.syy - s.sy * s.sy, a12 = s.n * s.sxy - s.sx * s.sy;
    const long long b1 = s.n * s.sqx - s.sx * s.sq, b2 = s.n * s.sqy - s.sy * s.sq;
    const long long det = a11 * a22 - a12 * a12;
    gu = gv = 0.0;
    if (s.n < min_count || det <= 0) return false;
    gu = ((double)(a22 * b1 - a12 * b2) / (double)det) / 1024.0;
    gv = ((double)(a11 * b2 - a12 * b1) / (double)det) / 1024.0;
    return true;
}

// The slant of a KEPT pixel. wc and kc point at the pixel in arrays of `stride` entries per row (the maps themselves, or a staged tile);
// kc != 0: kept. dx runs over dx_lo..dx_hi and dy over dy_lo..dy_hi: the part of the (2 R + 1)^2 neighbourhood inside the map.
__device__ __forceinline__ bool slant_pixel(const double* wc, const uint8_t* kc, int stride, int dx_lo, int dx_hi, int dy_lo, int dy_hi, double w_step,
                                            double max_diff, int min_count, double& gu, double& gv) {
    SlantSums s = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const double w_i = wc[0];
    for (int dy = dy_lo; dy <= dy_hi; ++dy)
        for (int dx = dx_lo; dx <= dx_hi; ++dx) {
            long long q;
            if (kc[dy * stride + dx] != 0 && slant_height(w_i, wc[dy * stride + dx], w_step, max_diff, q)) slant_add(s, dx, dy, q);
        }
    return slant_fit(s, min_count, gu, gv);
}

// ---- (2) the refined depth ----------------------------------------------------------------------------------------------------------------
// Candidate c of -span sub .. span sub is index k = c + span sub of the running choice. The definition visits the candidates in the order
// 0, -1, +1, -2, +2, ... and lets a later one replace the best only if it scores strictly more: the winner is the greatest score and, among
// equal scores, the candidate visited first, i.e. the least |c|, and -c before +c. In ASCENDING order that is: replace on a greater score, or
// on an equal one when |c| < |c_best| (the best so far lies below c, so an equal |c| means c = -c_best > 0, which was visited later and
// loses). The rest is dense_best_update: the best, its predecessor and its successor.
__device__ __forceinline__ void refine_best_step(DenseBest& b, int k, int c, bool valid, double s) {
    const int c_best = c - (k - b.k);                      // meaningful when b.k >= 0
    dense_best_update(b, k, valid && (b.k < 0 || s > b.s0 || (s == b.s0 && abs(c) < abs(c_best))), valid, s);
}

// The refined (w, score) of a kept pixel (u, v) whose window of radius r lies inside ref. ref_c points at the pixel's ref byte in an array of
// ref_stride bytes per row (ref itself, or a staged tile). Sample (dx, dy) of candidate c lies on the plane of inverse depth
// w_i + t w_step, t = double(c) / double(sub) + (gu dx + gv dy). true: taken (the best candidate scores strictly more than score_i); false:
// w_out = w_i, score_out = score_i.
__device__ __forceinline__ bool refine_pixel(const uint8_t* ref_c, int ref_stride, const uint8_t* src, int h1, int w1, const double* A, const double* B, int u,
                                             int v, int r, double w_i, float score_i, double gu, double gv, double w_step, int span, int sub,
                                             long long min_var, double& w_out, float& score_out) {
#pragma clang fp contract(off)
    const int side = 2 * r + 1, half = span * sub;
    const long long n = (long long)side * side;
    long long sa, saa;
    dense_window_sums(ref_c, ref_stride, r, sa, saa);
    DenseBest best;
    dense_best_init(best);
    for (int c = -half; c <= half; ++c) {
        const double tc = (double)c / (double)sub;
        long long sb = 0, sbb = 0, sab = 0;
        int inv = 0;
        for (int dy = -r; dy <= r; ++dy)
            for (int dx = -r; dx <= r; ++dx) {
                const double t = tc + (gu * (double)dx + gv * (double)dy);
                double H[9];
                dense_plane_at(A, B, w_i + t * w_step, H);
                int b = 0;
                if (!dense_sample(src, h1, w1, H, u + dx, v + dy, b)) ++inv;      // b = 0 then
                const long long av = ref_c[dy * ref_stride + dx], bv = b;
                sb += bv; sbb += bv * bv; sab += av * bv;
            }
        double s = 0.0;
        const bool valid = inv == 0 && dense_score(n, sa, saa, sb, sbb, sab, min_var, s);
        refine_best_step(best, c + half, c, valid, s);
    }
    w_out = w_i; score_out = score_i;
    if (best.k < 0 || !(best.s0 > (double)score_i)) return false;      // a NaN score takes nothing
    const double off = best.k >= 1 && best.k <= 2 * half - 1 && (best.flags & 3) == 3 ? parabola_offset(best.sm, best.s0, best.sp) : 0.0;
    w_out = w_i + (((double)(best.k - half) + off) / (double)sub) * w_step;
    score_out = (float)best.s0;
    return true;
}

}  // namespace
}  // namespace im
