// The per-pixel rules of the depth-map clean-up (csrc/depth_clean.hip): who is a member of the join graph, which neighbours are joined,
// `find` and `link` of the union-find that labels the connected components, the interpolation of a filled pixel and the rounding of its
// plane. A definition of this project's own, restated by tests/depth_oracle.py; it is not OpenCV's filterSpeckles and not
// Metashape's depth filter. Labels, sizes and rims are integers, so the kernels may visit pixels and joins in any order; what is float64
// uses only + - * / and rint with contraction off, in the association written here. A header of its own without the context or any launch
// code, like sgm_pixel.h: tests/depth_host_harness.cpp compiles this very text behind a stub <hip/hip_runtime.h> and defines
// IM_DEPTH_HOST_ATOMICS with its own depth_load, depth_store and atomicMin.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace im {
namespace {

constexpr int DEPTH_TILE_W = 64, DEPTH_TILE_H = 16;      // the pixels one block labels in LDS; no part of the definition
constexpr int DEPTH_MAX_SIDE = 16384;                    // h w <= 2^28: a linear index is an int
constexpr int DEPTH_MAX_DIFF = 4095, DEPTH_MAX_HOLE = 4096, DEPTH_MAX_PLANES = 4096;
constexpr int DEPTH_SURFACES = 0, DEPTH_HOLES = 1;
constexpr int DEPTH_NO_RIM = 0x7FFFFFFF;                 // `lo` of a hole none of whose neighbours holds a plane yet
constexpr int DEPTH_BORDER = 1 << 30;                    // set in `hi` of a hole with a pixel in the first or last row or column

#ifndef IM_DEPTH_HOST_ATOMICS
// A parent is read and written while other blocks link: relaxed, device scope. A stale parent is still an ancestor.
__device__ __forceinline__ int depth_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void depth_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#endif

// mode 0: the pixels that hold a plane; mode 1: those that hold none
__device__ __forceinline__ bool depth_member(int plane, int mode) { return mode == DEPTH_SURFACES ? plane >= 0 : plane < 0; }

// two neighbouring pixels: both members, and in mode 0 |p - q| <= max_diff as integers (planes are int16: no overflow)
__device__ __forceinline__ bool depth_joined(int p, int q, int mode, int max_diff) {
    if (!depth_member(p, mode) || !depth_member(q, mode)) return false;
    if (mode != DEPTH_SURFACES) return true;
    const int d = p - q;
    return (d < 0 ? -d : d) <= max_diff;
}

// The root of i: parent[j] <= j everywhere, so the walk descends and ends at parent[r] == r
__device__ __forceinline__ int depth_find(const int* parent, int i) {
    for (int p = depth_load(parent + i); p != i; p = depth_load(parent + i)) i = p;
    return i;
}

// Unites the components of a and b without a lock: the larger root goes under the smaller by atomicMin on its slot. What the atomic
// returns tells whether the slot was still a root; if not, its former parent `old` must end up with b as well (the minimum may have cut
// that edge), so the pair (old, b) goes round again. Indices only fall: the loop ends. The root of a finished component is its least index.
__device__ __forceinline__ void depth_link(int* parent, int a, int b) {
    for (;;) {
        a = depth_find(parent, a);
        b = depth_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + a, b);
        if (old == a) return;
        a = old;
    }
}

// wl + (wr - wl) (x - xl) / (xr - xl) between the anchors xl < x < xr of a row (or a column)
__device__ __forceinline__ double depth_between(double wl, double wr, int x, int xl, int xr) {
#pragma clang fp contract(off)
    return wl + (wr - wl) * ((double)(x - xl) / (double)(xr - xl));
}

// the value of a filled pixel out of its row value a and its column value b
__device__ __forceinline__ double depth_fill(double a, double b) {
#pragma clang fp contract(off)
    return 0.5 * (a + b);
}

// min(D - 1, max(0, rint((w - w_first) / w_step))), ties to even; what is no number counts as below 0
__device__ __forceinline__ int depth_plane_of(double w, double w_first, double w_step, int D) {
#pragma clang fp contract(off)
    double q = rint((w - w_first) / w_step);
    if (!(q >= 0.0)) q = 0.0;
    if (q > (double)(D - 1)) q = (double)(D - 1);
    return (int)q;
}

// a hole qualifies: no pixel on the border, at most max_hole pixels, and its rim spreads over at most max_diff planes
__device__ __forceinline__ bool depth_hole_qualifies(int size, int lo, int hi, int max_hole, int max_diff) {
    return size >= 1 && size <= max_hole && (hi & DEPTH_BORDER) == 0 && lo != DEPTH_NO_RIM && hi - lo <= max_diff;
}

}  // namespace
}  // namespace im
