// The arithmetic of the dense surface displacement between two epochs (csrc/dense_flow.hip): the match of a pixel of one camera's image at
// epoch A in the same camera's image at epoch B by the zero-mean normalised cross-correlation of exact integer window sums over an integer
// search range with a parabola between the best candidate's neighbours, the forward-backward check of two such fields, and the lift of both
// ends of a match to world points through each epoch's own depth map and pose. The reference has no such step (its velocities come from
// tracked keypoints): this is a definition of this project's own, restated in numpy by tests/flow_oracle.py. Everything up to a
// score is an integer, so the kernels may sum in any order; what is float64 uses only + - * / sqrt rint floor with contraction off, in the
// association written here. A header of its own without the context or any launch code, like dense_pixel.h:
// tests/flow_host_harness.cpp compiles this very text behind a stub <hip/hip_runtime.h>.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "dense_pixel.h"

namespace im {
namespace {

constexpr int FLOW_MAX_RADIUS = 15, FLOW_MAX_SEARCH = 16, FLOW_MAX_PRIOR = 4096;
constexpr long long FLOW_MAX_MIN_VAR = 1LL << 26;
// n = 31^2 = 961 bytes: sb <= 961 * 255 < 2^18, sbb and sab <= 961 * 255^2 < 2^26, so n sbb < 2^36, sb^2 < 2^36 and
// n^2 min_var <= 961^2 2^26 < 2^46: every product and every difference below fits an int64 by a wide margin (and sb, sbb a uint32 each).
static_assert(961LL * 255 < (1LL << 18) && 961LL * 255 * 255 < (1LL << 26) && 961LL * 961 * FLOW_MAX_MIN_VAR < (1LL << 46), "the window sums");

// ---- match ----------------------------------------------------------------------------------------------------------------------------------
// The window test, the window sums and the score are dense_pixel.h's: window_inside, dense_window_sums, and dense_score with the scale 1 of
// bytes in either window.

// sum of products of the two windows centred on *ca and *cb
__device__ __forceinline__ long long flow_window_ab(const uint8_t* ca, int stride_a, const uint8_t* cb, int stride_b, int r) {
    unsigned ab = 0;
    for (int dy = -r; dy <= r; ++dy)
        for (int dx = -r; dx <= r; ++dx) ab += (unsigned)ca[dy * stride_a + dx] * cb[dy * stride_b + dx];
    return ab;
}

// Candidates are visited in ascending (dx^2 + dy^2, dy, dx) and a later one replaces the best only on a strictly greater score: the best is
// the greatest score, and among equal scores the candidate that comes first in that order. A valid score is finite (VA, VB > 0), so the
// comparison below gives that very candidate in whatever order the candidates arrive. have = a best exists.
__device__ __forceinline__ bool flow_before(int dx, int dy, int dx0, int dy0) {
    const int q = dx * dx + dy * dy, q0 = dx0 * dx0 + dy0 * dy0;
    return (q < q0) | ((q == q0) & ((dy < dy0) | ((dy == dy0) & (dx < dx0))));
}
// without short-circuits: three comparisons and a few bit operations, no branch for a compiler to lay out
__device__ __forceinline__ bool flow_better(bool have, double s, int dx, int dy, double s0, int dx0, int dy0) {
    return !have | (s > s0) | ((s == s0) & flow_before(dx, dy, dx0, dy0));
}

// The sub-pixel offset along one axis: the sweep's parabola (dense_pixel.h) over the best's two neighbours where both lie inside the
// search range and scored (both: 1); else 0.
__device__ __forceinline__ double flow_offset(bool both, double sm, double s0, double sp) { return both ? parabola_offset(sm, s0, sp) : 0.0; }

// The whole match of pixel (u, v) on the images themselves, candidate after candidate: what the kernel computes tile-wise from LDS.
// a and b are [h][w]. false (and zeros) where no candidate scored or the best is below min_score.
__device__ __forceinline__ bool flow_candidate(const uint8_t* a, const uint8_t* b, int h, int w, int u, int v, int r, int bx, int by, long long sa,
                                               long long saa, long long min_var, double& s) {
    s = 0.0;
    if (!window_inside(bx, by, r, h, w)) return false;
    const uint8_t* cb = b + (long)by * w + bx;
    long long sb, sbb;
    dense_window_sums(cb, w, r, sb, sbb);
    const long long n = (long long)(2 * r + 1) * (2 * r + 1);
    return dense_score(n, sa, saa, sb, sbb, flow_window_ab(a + (long)v * w + u, w, cb, w, r), min_var, s, 1);
}
__device__ __forceinline__ bool flow_match_pixel(const uint8_t* a, const uint8_t* b, int h, int w, int u, int v, int r, int S, int pu, int pv,
                                                 long long min_var, double min_score, double& du, double& dv, float& score) {
#pragma clang fp contract(off)
    du = dv = 0.0; score = 0.0f;
    if (!window_inside(u, v, r, h, w)) return false;
    long long sa, saa;
    dense_window_sums(a + (long)v * w + u, w, r, sa, saa);
    bool have = false;
    double s0 = 0.0;
    int bx = 0, by = 0;
    for (int dy = -S; dy <= S; ++dy)
        for (int dx = -S; dx <= S; ++dx) {
            double s;
            if (flow_candidate(a, b, h, w, u, v, r, u + pu + dx, v + pv + dy, sa, saa, min_var, s) && flow_better(have, s, dx, dy, s0, bx, by)) {
                have = true; s0 = s; bx = dx; by = dy;
            }
        }
    if (!have || s0 < min_score) return false;
    double sm = 0.0, sp = 0.0;
    bool both = bx - 1 >= -S && bx + 1 <= S;
    both = both && flow_candidate(a, b, h, w, u, v, r, u + pu + bx - 1, v + pv + by, sa, saa, min_var, sm);
    both = both && flow_candidate(a, b, h, w, u, v, r, u + pu + bx + 1, v + pv + by, sa, saa, min_var, sp);
    du = (double)(pu + bx) + flow_offset(both, sm, s0, sp);
    both = by - 1 >= -S && by + 1 <= S;
    both = both && flow_candidate(a, b, h, w, u, v, r, u + pu + bx, v + pv + by - 1, sa, saa, min_var, sm);
    both = both && flow_candidate(a, b, h, w, u, v, r, u + pu + bx, v + pv + by + 1, sa, saa, min_var, sp);
    dv = (double)(pv + by) + flow_offset(both, sm, s0, sp);
    score = (float)s0;
    return true;
}

// ---- check ----------------------------------------------------------------------------------------------------------------------------------
// Is the valid forward match (du, dv) of pixel (u, v) met by the backward field [h][w]? The backward pixel by rint; a NaN fails.
__device__ __forceinline__ bool flow_consistent(int u, int v, double du, double dv, const double* du_b, const double* dv_b, const uint8_t* valid_b,
                                                int h, int w, double tol) {
#pragma clang fp contract(off)
    const double ju = rint((double)u + du), jv = rint((double)v + dv);
    if (!(ju >= 0.0 && ju <= (double)(w - 1) && jv >= 0.0 && jv <= (double)(h - 1))) return false;
    const long j = (long)jv * w + (long)ju;
    if (valid_b[j] == 0) return false;
    const double ex = du + du_b[j], ey = dv + dv_b[j];
    return ex * ex + ey * ey <= tol * tol;
}

// ---- lift -----------------------------------------------------------------------------------------------------------------------------------
// The inverse depth of map B [hb][wb] at (x, y): all four taps floor(x) .. floor(x) + 1, floor(y) .. floor(y) + 1 inside the map (a tap of
// weight zero included), with a plane and kept, and spanning at most `span` = max_diff |w_step_b|; then their bilinear mean, along x first.
__device__ __forceinline__ bool flow_depth_at(const int16_t* plane_b, const double* w_b, const uint8_t* keep_b, int hb, int wb, double x, double y,
                                              double span, double& w) {
#pragma clang fp contract(off)
    w = 0.0;
    const double fx = floor(x), fy = floor(y);
    if (!(fx >= 0.0 && fx + 1.0 <= (double)(wb - 1) && fy >= 0.0 && fy + 1.0 <= (double)(hb - 1))) return false;      // a NaN fails
    const long i = (long)fy * wb + (long)fx;
    const long tap[4] = {i, i + 1, i + wb, i + wb + 1};
    for (int k = 0; k < 4; ++k)
        if (plane_b[tap[k]] < 0 || keep_b[tap[k]] == 0) return false;
    const double w00 = w_b[tap[0]], w01 = w_b[tap[1]], w10 = w_b[tap[2]], w11 = w_b[tap[3]];
    double lo = w00, hi = w00;
    const double rest[3] = {w01, w10, w11};
    for (int k = 0; k < 3; ++k) {
        if (rest[k] < lo) lo = rest[k];
        if (rest[k] > hi) hi = rest[k];
    }
    if (!(hi - lo <= span)) return false;
    const double tx = x - fx, ty = y - fy;
    const double top = w00 + tx * (w01 - w00), bot = w10 + tx * (w11 - w10);
    w = top + ty * (bot - top);
    return true;
}

// P = the world point of pixel (u, v) of map A (inverse depth w_a), Q = that of (u + du, v + dv) through map B, D = Q - P
__device__ __forceinline__ bool flow_lift_pixel(const DenseCam& ca, const DenseCam& cb, int u, int v, double w_a, double du, double dv,
                                                const int16_t* plane_b, const double* w_b, const uint8_t* keep_b, int hb, int wb, double span, double* P,
                                                double* D) {
#pragma clang fp contract(off)
    P[0] = P[1] = P[2] = D[0] = D[1] = D[2] = 0.0;
    const double x = (double)u + du, y = (double)v + dv;
    double wq;
    if (!flow_depth_at(plane_b, w_b, keep_b, hb, wb, x, y, span, wq)) return false;
    double X[3], Q[3];
    dense_world_point(ca, u, v, w_a, P);
    dense_backproject_at(cb.Ki, x, y, wq, X);
    dense_to_world(cb, X, Q);
    for (int i = 0; i < 3; ++i) D[i] = Q[i] - P[i];
    return true;
}

}  // namespace
}  // namespace im
