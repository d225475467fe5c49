// Host build of the per-point arithmetic of csrc/sfm.hip (csrc/sfm_point.h, csrc/lstsq_jacobi.h) for tests/test_sfm_cpu.py: the very
// text the kernels compile, as flat loops over arrays. Compiled with a stub <hip/hip_runtime.h> that defines __device__ and
// __forceinline__ away; no arithmetic is written here.
#include "sfm_point.h"

// cam: fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6, as `im_undistort_points` takes it
extern "C" void sfm_host_undistort(const float* pts, long long n, const double* cam, float* out) {
    im::CamParam c;
    for (int j = 0; j < 12; ++j) c.P[j] = 0.0;
    for (int j = 0; j < 4; ++j) c.in[j] = cam[j];
    for (int j = 0; j < 8; ++j) c.k[j] = cam[4 + j];
    for (long long i = 0; i < n; ++i) im::undistort_one((double)pts[2 * i], (double)pts[2 * i + 1], c, out[2 * i], out[2 * i + 1]);
}

// u1, u2 [n, 2] float64 (float32 points widen exactly, as in the float32 kernel); P1, P2 row-major 3 x 4
extern "C" void sfm_host_triangulate(const double* u1, const double* u2, long long n, const double* P1, const double* P2, double tolerance,
                                     int max_solves, double* X, int* status) {
    double p1[12], p2[12];
    for (int j = 0; j < 12; ++j) { p1[j] = P1[j]; p2[j] = P2[j]; }
    for (long long i = 0; i < n; ++i) {
        double x[3];
        status[i] = im::triangulate_one(u1[2 * i], u1[2 * i + 1], u2[2 * i], u2[2 * i + 1], p1, p2, tolerance, max_solves, x);
        X[3 * i] = x[0]; X[3 * i + 1] = x[1]; X[3 * i + 2] = x[2];
    }
}
