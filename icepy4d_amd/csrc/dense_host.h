// The host-side checks that the entry points of the dense stages share (dense.hip, dense_sgm.hip, depth_clean.hip, dense_fuse.hip,
// dense_refine.hip, dense_flow.hip): the refusal code, the limits on an image side and on a number, and the copy of the sweep's two matrices
// into a kernel's arguments. Each entry point keeps its own messages.
#pragma once
#include <cmath>

#include "dense_pixel.h"

namespace im {
namespace {

constexpr int DENSE_REFUSED = -83;                       // what every refusal of a dense stage returns

inline bool bad_side(int v) { return v < 1 || v > DENSE_MAX_SIDE; }
inline bool bad_step(double w_step) { return !std::isfinite(w_step) || w_step == 0.0; }
inline bool positive(double v) { return std::isfinite(v) && v > 0.0; }
inline bool finite_all(const double* p, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}

// h_A and h_B of a sweep, nine doubles each, into the arguments that travel to the kernel by value
inline void copy_matrices(const double* h_A, const double* h_B, double* A, double* B) {
    for (int i = 0; i < 9; ++i) { A[i] = h_A[i]; B[i] = h_B[i]; }
}

}  // namespace
}  // namespace im
