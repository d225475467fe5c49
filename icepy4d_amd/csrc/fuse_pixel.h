// The per-pixel rules of the fusion of the two depth maps (csrc/dense_fuse.hip): the link of a kept pixel of one view to a kept pixel of the
// other, the other view's measurement carried onto the pixel's own ray, the fused inverse depth and score, and which pixels of the other
// view the cloud still lacks. Metashape's buildDenseCloud (`metashape.py:198-240`) merges its depth maps by a closed rule that is NOT
// reproduced: this is a definition of this project's own, restated in numpy by tests/fuse_oracle.py. Parity with Metashape
// is unpinned by construction. Everything is float64 with contraction off, uses only + - * /, rint, fabs and comparisons, in the
// association written here; every pixel is decided from the inputs alone, so the order of execution does not matter. A header of its own
// without the context or any launch code, like depth_pixel.h: tests/fuse_host_harness.cpp compiles this very text behind a stub
// <hip/hip_runtime.h>.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "dense_pixel.h"

namespace im {
namespace {

constexpr int FUSE_MAX_SIDE = DENSE_MAX_SIDE;            // h w <= 2^28: a linear index is an int
constexpr double FUSE_DBL_MAX = 1.7976931348623157e308;

// The link of kept pixel (u, v) of view a (inverse depth w) into view b [hb][wb]: the test of dense_consistent with one change, the target
// must be KEPT (keep_b != 0), not merely hold a plane. The linear index of the target, -1 where there is none. P = inv(Ka), R, t, Kb with
// Xb = R Xa + t; tol is an inverse depth of view b.
__device__ __forceinline__ int fuse_link(const DensePose& P, int u, int v, double w, const uint8_t* keep_b, const double* w_b, int hb, int wb, double tol) {
#pragma clang fp contract(off)
    double Xa[3], Xb[3];
    dense_backproject(P.Ki, u, v, w, Xa);
    for (int i = 0; i < 3; ++i) Xb[i] = ((P.R[3 * i] * Xa[0] + P.R[3 * i + 1] * Xa[1]) + P.R[3 * i + 2] * Xa[2]) + P.t[i];
    if (!(Xb[2] > 0.0)) return -1;
    const double px = (P.K1[0] * Xb[0] + P.K1[1] * Xb[1]) + P.K1[2] * Xb[2];
    const double py = (P.K1[3] * Xb[0] + P.K1[4] * Xb[1]) + P.K1[5] * Xb[2];
    const double pz = (P.K1[6] * Xb[0] + P.K1[7] * Xb[1]) + P.K1[8] * Xb[2];
    const double ju = rint(px / pz), jv = rint(py / pz);
    if (!(ju >= 0.0 && ju <= (double)(wb - 1) && jv >= 0.0 && jv <= (double)(hb - 1))) return -1;      // NaN fails
    const int j = (int)jv * wb + (int)ju;
    if (keep_b[j] == 0) return -1;
    if (!(fabs(w_b[j] - 1.0 / Xb[2]) <= tol)) return -1;
    return j;
}

// The inverse depth along the ray of pixel (u, v) of view a at which view b's measurement wb_j (an inverse depth of view b) lies:
// Xb.z = g / w + t_z with g = (R Ki (u, v, 1)).z, so w' = g / (1 / wb_j - t_z). false unless w' is finite and positive.
__device__ __forceinline__ bool fuse_second(const DensePose& P, int u, int v, double wb_j, double& w2) {
#pragma clang fp contract(off)
    const double du = (double)u, dv = (double)v;
    const double d0 = (P.Ki[0] * du + P.Ki[1] * dv) + P.Ki[2];
    const double d1 = (P.Ki[3] * du + P.Ki[4] * dv) + P.Ki[5];
    const double d2 = (P.Ki[6] * du + P.Ki[7] * dv) + P.Ki[8];
    const double g = (P.R[6] * d0 + P.R[7] * d1) + P.R[8] * d2;
    w2 = g / (1.0 / wb_j - P.t[2]);
    return w2 > 0.0 && w2 <= FUSE_DBL_MAX;
}

// What one pixel of view a becomes. link >= 0: views = 2 and the caller sets claimed[link]; kept and unlinked: copied through, views = 1;
// not kept: all zero.
struct FusedPixel {
    int link;
    double w;
    float score;
    uint8_t views;
};

__device__ __forceinline__ FusedPixel fuse_pixel(const DensePose& P, int u, int v, uint8_t keep, double w, float score, const uint8_t* keep_b,
                                                 const double* w_b, const float* score_b, int hb, int wb, double tol) {
#pragma clang fp contract(off)
    FusedPixel o{-1, 0.0, 0.0f, 0};
    if (keep == 0) return o;
    o.w = w; o.score = score; o.views = 1;
    o.link = fuse_link(P, u, v, w, keep_b, w_b, hb, wb, tol);
    if (o.link < 0) return o;
    o.views = 2;
    double w2 = 0.0;
    if (!fuse_second(P, u, v, w_b[o.link], w2)) return o;
    const float sb = score_b[o.link];
    const double a = (double)score > 0.0 ? (double)score : 0.0, b = (double)sb > 0.0 ? (double)sb : 0.0;      // max(score, 0); NaN counts as 0
    o.w = a + b > 0.0 ? (a * w + b * w2) / (a + b) : 0.5 * (w + w2);
    o.score = sb > score ? sb : score;
    return o;
}

// Does the cloud still lack pixel (u, v) of view b? It is kept, no pixel of view a claimed it, and its own link into view a fails
// (P = inv(Kb), R^T, -R^T t, Ka; tol an inverse depth of view a): it sees a surface that view a does not represent.
__device__ __forceinline__ bool fuse_rest(const DensePose& P, int u, int v, uint8_t keep, uint8_t claimed, double w, const uint8_t* keep_a,
                                          const double* w_a, int ha, int wa, double tol) {
    if (keep == 0 || claimed != 0) return false;
    return fuse_link(P, u, v, w, keep_a, w_a, ha, wa, tol) < 0;
}

}  // namespace
}  // namespace im
