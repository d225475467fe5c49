// The arithmetic of one point of csrc/sfm.hip: the undistortion of one image point and the (iterative) least-squares triangulation of one
// matched pair, float64, contraction off. A header of its own, without the context or any launch code, so that a host program can compile the
// very text the kernels compile (tests/sfm_host_harness.cpp, through a stub <hip/hip_runtime.h> that defines __device__ and
// __forceinline__ away) and be compared with the numpy restatement (tests/sfm_oracle.py) bit for bit where no device is at hand.
// The unnamed namespace is the one of sfm.hip's kernels: the kernels take CamParam / CamPair by value, so the structs stay where they were
// and every kernel keeps its symbol. An unnamed namespace gives each including translation unit types of its own: of the library's
// sources only sfm.hip includes this header.
#pragma once
#include <cmath>

#include "lstsq_jacobi.h"

namespace im {
namespace {

// one camera: P (3 x 4, row-major), fx fy cx cy, k1 k2 p1 p2 k3 k4 k5 k6
struct CamParam { double P[12]; double in[4]; double k[8]; };
struct CamPair { CamParam c[2]; };
static_assert(sizeof(CamPair) == 48 * sizeof(double), "camera table rows are 48 doubles");

__device__ __forceinline__ void undistort_one(double u, double v, const CamParam& c, float& ou, float& ov) {
#pragma clang fp contract(off)
    const double fx = c.in[0], fy = c.in[1], cx = c.in[2], cy = c.in[3];
    const double k1 = c.k[0], k2 = c.k[1], p1 = c.k[2], p2 = c.k[3], k3 = c.k[4], k4 = c.k[5], k5 = c.k[6], k6 = c.k[7];
    const double x0 = (u - cx) / fx, y0 = (v - cy) / fy;
    double x = x0, y = y0;
    for (int it = 0; it < 5; ++it) {
        const double r2 = x * x + y * y;
        const double icdist = (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2);
        if (icdist < 0.0) { x = x0; y = y0; break; }
        const double dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
        const double dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
        x = (x0 - dx) * icdist;
        y = (y0 - dy) * icdist;
    }
    ou = (float)(fx * x + cx);
    ov = (float)(fy * y + cy);
}

// one point from its two (undistorted) image points; returns the status
__device__ __forceinline__ int triangulate_one(double u1x, double u1y, double u2x, double u2y, const double (&P1)[12], const double (&P2)[12],
                                               double tol, int max_solves, double (&X)[3]) {
#pragma clang fp contract(off)
    double A[4][3], b[4];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        A[0][j] = u1x * P1[8 + j] - P1[j];
        A[1][j] = u1y * P1[8 + j] - P1[4 + j];
        A[2][j] = u2x * P2[8 + j] - P2[j];
        A[3][j] = u2y * P2[8 + j] - P2[4 + j];
    }
    b[0] = -(u1x * P1[11] - P1[3]);
    b[1] = -(u1y * P1[11] - P1[7]);
    b[2] = -(u2x * P2[11] - P2[3]);
    b[3] = -(u2y * P2[11] - P2[7]);
    double d1 = 1.0, d2 = 1.0, d1n = 1.0, d2n = 1.0;
    for (int i = 0; i < max_solves; ++i) {
        lstsq43_svd(A, b, X);
        d1n = ((P1[8] * X[0] + P1[9] * X[1]) + P1[10] * X[2]) + P1[11];
        d2n = ((P2[8] * X[0] + P2[9] * X[1]) + P2[10] * X[2]) + P2[11];
        if (fabs(d1n - d1) <= tol && fabs(d2n - d2) <= tol) break;
        const double i1 = 1.0 / d1n, i2 = 1.0 / d2n;     // cumulative: the rows keep the weights of the earlier solves
#pragma unroll
        for (int j = 0; j < 3; ++j) { A[0][j] *= i1; A[1][j] *= i1; A[2][j] *= i2; A[3][j] *= i2; }
        b[0] *= i1; b[1] *= i1; b[2] *= i2; b[3] *= i2;
        d1 = d1n;
        d2 = d2n;
    }
    if (max_solves == 1) return 1;
    int st = (d1n > 0.0 && d2n > 0.0) ? 1 : 0;
    if (d1n <= 0.0) st -= 1;
    if (d2n <= 0.0) st -= 2;
    return st;
}

}  // namespace
}  // namespace im
