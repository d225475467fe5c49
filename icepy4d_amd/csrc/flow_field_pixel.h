// The arithmetic of the coarse-to-fine dense displacement (csrc/dense_flow_field.hip) beyond flow_pixel.h's: the prior of a fine pixel from
// the displacement field of the level above (the lower median of the valid, finite displacements around the pixel's parent, doubled and
// rounded), the test of a pixel of a prior field that is to be matched, and the size of the box of priors that one tile of the match may
// span and still stage its region of b in LDS. A definition of this project's own, restated in numpy by tests/pyrflow_oracle.py.
// The median picks one of its inputs and never adds two, so the only float64 operations are 2.0 * x and rint. A header of its own without
// the context or any launch code, like flow_pixel.h: tests/flow_field_host_harness.cpp compiles this very text behind a stub
// <hip/hip_runtime.h>.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "flow_pixel.h"

namespace im {
namespace {

constexpr int FLOW_MAX_MEDIAN_RADIUS = 2;
// The widest box of priors, per axis, that a tile may span on the tiled path: max - min of the priors of its pixels that are to be matched.
// Above it, or above what the LDS of the launch holds at this r and S (flow_field_spread), the tile takes the direct path.
constexpr int FLOW_FIELD_MAX_SPREAD = 8;
constexpr long long FLOW_FIELD_LDS_BUDGET = 64 * 1024 - 1024;      // what a launch asks for; the rest is the block's static share

// The bytes of LDS of the tiled path for a tile of tw x th pixels whose priors span ex, ey: the bytes of a with a halo of r, the bytes of b
// that the box's candidates read (halo r + S around the tile moved over the box), a sum and a sum of squares of b (4 bytes each) per
// position that a candidate can be centred on, and a 4-byte row partial per row of a and column of the tile; the byte arrays end on
// multiples of 8. constexpr: host and device alike.
constexpr long long flow_field_up8(long long v) { return (v + 7) & ~7LL; }
constexpr long long flow_field_lds_bytes(int tw, int th, int r, int S, int ex, int ey) {
    return flow_field_up8((long long)(tw + 2 * r) * (th + 2 * r)) + flow_field_up8((long long)(tw + ex + 2 * (r + S)) * (th + ey + 2 * (r + S))) +
           (long long)(tw + ex + 2 * S) * (th + ey + 2 * S) * 8 + (long long)(th + 2 * r) * tw * 4;
}
// The spread a launch at (r, S) allows on either axis: the greatest E <= FLOW_FIELD_MAX_SPREAD whose square box fits the budget. E = 0
// always fits: that is flow_match_kernel's own 62800 bytes at r = 15, S = 16.
constexpr int flow_field_spread(int tw, int th, int r, int S) {
    int E = FLOW_FIELD_MAX_SPREAD;
    while (E > 0 && flow_field_lds_bytes(tw, th, r, S, E, E) > FLOW_FIELD_LDS_BUDGET) --E;
    return E;
}
static_assert(flow_field_lds_bytes(64, 16, FLOW_MAX_RADIUS, FLOW_MAX_SEARCH, 0, 0) == 62800 && 62800 <= FLOW_FIELD_LDS_BUDGET, "the largest launch");

// Is a pixel of a prior field to be matched? have set, asked for (ask: 1 where there is no mask), both components of the prior in range.
__device__ __forceinline__ bool flow_field_wanted(int have, int ask, int pu, int pv) {
    return have != 0 && ask != 0 && pu >= -FLOW_MAX_PRIOR && pu <= FLOW_MAX_PRIOR && pv >= -FLOW_MAX_PRIOR && pv <= FLOW_MAX_PRIOR;
}

// Element k (from 0) of the ascending order of the values v[i] whose bit i of `use` is set; k < their number. By ranks and not by a sort:
// the rank of a value is the number of used values before it (smaller, or equal with a smaller index), every index is a constant after
// unrolling, and the values stay in registers. Used values are finite, so every comparison is decided.
template <int N>
__device__ __forceinline__ double flow_kth(const double (&v)[N], unsigned use, int k) {
    double out = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        int rank = 0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const bool before = (v[j] < v[i]) | ((v[j] == v[i]) & (j < i));
            rank += ((use >> j) & 1u) & (unsigned)before;
        }
        out = (((use >> i) & 1u) != 0 && rank == k) ? v[i] : out;
    }
    return out;
}

// One component of the prior from its lower median: false where 2 med rounds beyond the range of a prior.
__device__ __forceinline__ bool flow_prior_of(double med, int& p) {
#pragma clang fp contract(off)
    const double d = rint(2.0 * med);
    p = 0;
    if (!(d >= -(double)FLOW_MAX_PRIOR && d <= (double)FLOW_MAX_PRIOR)) return false;
    p = (int)d;
    return true;
}

// The prior of fine pixel (u, v) from the field of the level above, [hc][wc]: the coarse pixels of the (2 M + 1)^2 neighbourhood of
// (u >> 1, v >> 1) inside the coarse image that are valid with a finite du and a finite dv; fewer than min_count of them: no prior. Else
// each component is rint(2 x the lower median of its values), the two medians taken independently. false (and zeros) where there is none.
template <int M>
__device__ __forceinline__ bool flow_prior_up_pixel(const double* du_c, const double* dv_c, const uint8_t* valid_c, int hc, int wc, int u, int v,
                                                    int min_count, int& pu, int& pv) {
    constexpr int SIDE = 2 * M + 1, N = SIDE * SIDE;
    const int cx = u >> 1, cy = v >> 1;
    double xs[N], ys[N];
    unsigned use = 0;
    int n = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int x = cx + i % SIDE - M, y = cy + i / SIDE - M;
        xs[i] = ys[i] = 0.0;
        if (x < 0 || x >= wc || y < 0 || y >= hc) continue;
        const long g = (long)y * wc + x;
        if (valid_c[g] == 0) continue;
        const double a = du_c[g], b = dv_c[g];
        if (!(__builtin_isfinite(a) && __builtin_isfinite(b))) continue;
        xs[i] = a; ys[i] = b;
        use |= 1u << i;
        ++n;
    }
    pu = pv = 0;
    if (n < min_count) return false;      // min_count >= 1: an empty neighbourhood ends here
    int qu, qv;
    const bool ok_u = flow_prior_of(flow_kth<N>(xs, use, (n - 1) / 2), qu);
    const bool ok_v = flow_prior_of(flow_kth<N>(ys, use, (n - 1) / 2), qv);
    if (!(ok_u && ok_v)) return false;
    pu = qu; pv = qv;
    return true;
}

}  // namespace
}  // namespace im
