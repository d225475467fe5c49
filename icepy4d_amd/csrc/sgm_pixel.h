// The arithmetic of the semi-global regularisation of a dense-stereo depth map (csrc/dense_sgm.hip): the 8-bit cost of one (pixel, plane)
// out of the sweep's score, one step of the min-plus recurrence along a path, and the choice of the plane of least summed cost with its
// sub-plane offset. A definition of this project's own, restated in numpy by tests/sgm_oracle.py; it is not Metashape's depth
// filter. Costs, path costs and their sums are integers, so the kernels may walk the paths in any order; what is float64 uses only
// + - * / and floor with contraction off, in the association written here. A header of its own without the context or any launch code,
// like dense_pixel.h: tests/sgm_host_harness.cpp compiles this very text behind a stub <hip/hip_runtime.h>.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace im {
namespace {

constexpr int SGM_MAX_PLANES = 256;       // a wave holds a line's path costs in registers, four planes per lane
constexpr int SGM_MAX_PENALTY = 4095;     // L <= 255 + P2 <= 4350, and the sum over eight paths <= 34800 fits 16 bits
constexpr int SGM_INVALID = 255;          // the cost of a plane the sweep did not score at a pixel
constexpr int SGM_FAR = 1 << 20;          // stands for an absent term (d - 1 < 0, d + 1 >= D): above every L + P2, far below INT_MAX
constexpr unsigned SGM_NO_KEY = 0xFFFFFFFFu;

// The directions (dy, dx) of the paths in the order of the definition: `paths` = 4 takes the first four
constexpr int SGM_DY[8] = {0, 0, 1, -1, 1, -1, 1, -1};
constexpr int SGM_DX[8] = {1, -1, 0, 0, 1, -1, -1, 1};

// c = 255 where the sweep scored nothing, else min(254, max(0, floor((1 - s) 127)))
__device__ __forceinline__ int sgm_cost(bool valid, double s) {
#pragma clang fp contract(off)
    if (!valid) return SGM_INVALID;
    double q = floor((1.0 - s) * 127.0);
    q = q < 0.0 ? 0.0 : q;
    q = q > 254.0 ? 254.0 : q;
    return (int)q;
}

// L(p, d) = c + min(L(q, d), L(q, d - 1) + P1, L(q, d + 1) + P1, m + P2) - m with m = min_k L(q, k); lm / lp = SGM_FAR where absent
__device__ __forceinline__ int sgm_step(int c, int l0, int lm, int lp, int m, int P1, int P2) {
    int best = l0;
    best = lm + P1 < best ? lm + P1 : best;
    best = lp + P1 < best ? lp + P1 : best;
    best = m + P2 < best ? m + P2 : best;
    return c + best - m;
}

// The order of the choice in one word: the least S wins, ties go to the lower plane, a plane invalid at the pixel never wins.
// S <= 34800 and k <= 255: S 2^16 + k < 2^32
__device__ __forceinline__ unsigned sgm_key(int c, unsigned S, int k) { return c == SGM_INVALID ? SGM_NO_KEY : (S << 16) | (unsigned)k; }

// The map entries of a pixel whose least key is `key`; cm, Sm / cp, Sp are the cost and the sum of the planes below and above the chosen
// one (read only where 1 <= k <= D - 2). plane = -1, w = 0, score = 0 where no plane is valid or the dequantised score is below min_score.
__device__ __forceinline__ void sgm_finish(unsigned key, int D, int c0, int cm, int cp, int Sm, int Sp, double w_first, double w_step, double min_score,
                                           int16_t& plane, double& w, float& score) {
#pragma clang fp contract(off)
    plane = -1; w = 0.0; score = 0.0f;
    if (key == SGM_NO_KEY) return;
    const int k = (int)(key & 0xFFFFu), S0 = (int)(key >> 16);
    const double sc = 1.0 - (double)c0 / 127.0;
    if (sc < min_score) return;
    double off = 0.0;
    if (k >= 1 && k <= D - 2 && cm != SGM_INVALID && cp != SGM_INVALID) {
        const int den = (Sm - 2 * S0) + Sp;
        if (den > 0) off = (0.5 * (double)(Sm - Sp)) / (double)den;
    }
    plane = (int16_t)k;
    w = w_first + ((double)k + off) * w_step;
    score = (float)sc;
}

}  // namespace
}  // namespace im
