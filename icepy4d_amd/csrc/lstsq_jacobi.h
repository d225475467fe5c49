// Least-squares solution of a 4 x 3 system as `cv2.solve(A, b, x, DECOMP_SVD)` defines it: x = V S^+ U^T b from the singular value
// decomposition of A, singular values <= 2 DBL_EPSILON (s0 + s1 + s2) treated as zero (the minimum-norm solution of a rank-deficient
// system). One-sided Jacobi (Hestenes) on the three columns of A: the column pairs (0,1), (0,2), (1,2) are rotated until they are
// orthogonal, V collects the rotations, the singular values are the column norms and U S the rotated columns, so that
//   x = sum_j [s_j > threshold]  v_j (a_j . b) / (a_j . a_j)
// with the sum taken in column order (the singular values are not sorted: the sum has three terms whatever their order).
// Every index is a compile-time constant (the pair is a template argument, the loops over rows are unrolled): A, V and the sums live in
// registers, nothing in scratch. Contraction is off: tests/sfm_oracle.py restates these operations one by one in numpy.
// (csrc/geometry.hip has a square one-sided Jacobi that returns one singular vector; its operation order is pinned by fp64 oracles, so this
// rectangular solver is a routine of its own.)
#pragma once
#include <hip/hip_runtime.h>

namespace im {

constexpr double LSQ_EPS = 2.220446049250313e-16;   // DBL_EPSILON
constexpr int LSQ_MAX_SWEEPS = 30;

__device__ __forceinline__ double dot4(double a0, double a1, double a2, double a3, double b0, double b1, double b2, double b3) {
#pragma clang fp contract(off)
    return ((a0 * b0 + a1 * b1) + a2 * b2) + a3 * b3;
}

// one rotation of columns P < Q; false when they are orthogonal to rounding (or a sum is not a number: nothing to rotate)
template <int P, int Q>
__device__ __forceinline__ bool lsq_rotate(double (&a)[4][3], double (&v)[3][3]) {
#pragma clang fp contract(off)
    const double al = dot4(a[0][P], a[1][P], a[2][P], a[3][P], a[0][P], a[1][P], a[2][P], a[3][P]);
    const double be = dot4(a[0][Q], a[1][Q], a[2][Q], a[3][Q], a[0][Q], a[1][Q], a[2][Q], a[3][Q]);
    const double ga = dot4(a[0][P], a[1][P], a[2][P], a[3][P], a[0][Q], a[1][Q], a[2][Q], a[3][Q]);
    if (!(fabs(ga) > LSQ_EPS * sqrt(al * be))) return false;
    const double zeta = (be - al) / (2.0 * ga);
    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double x = a[k][P], y = a[k][Q];
        a[k][P] = c * x - s * y;
        a[k][Q] = s * x + c * y;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double x = v[k][P], y = v[k][Q];
        v[k][P] = c * x - s * y;
        v[k][Q] = s * x + c * y;
    }
    return true;
}

__device__ __forceinline__ void lstsq43_svd(const double (&A)[4][3], const double (&b)[4], double (&x)[3]) {
#pragma clang fp contract(off)
    double a[4][3], v[3][3];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) a[k][j] = A[k][j];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) v[k][j] = k == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < LSQ_MAX_SWEEPS; ++sweep) {
        const bool r01 = lsq_rotate<0, 1>(a, v);
        const bool r02 = lsq_rotate<0, 2>(a, v);
        const bool r12 = lsq_rotate<1, 2>(a, v);
        if (!(r01 || r02 || r12)) break;
    }
    double w2[3], w[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        w2[j] = dot4(a[0][j], a[1][j], a[2][j], a[3][j], a[0][j], a[1][j], a[2][j], a[3][j]);
        w[j] = sqrt(w2[j]);
    }
    const double thr = (2.0 * LSQ_EPS) * ((w[0] + w[1]) + w[2]);
    x[0] = x[1] = x[2] = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (w[j] > thr) {
            const double coef = dot4(a[0][j], a[1][j], a[2][j], a[3][j], b[0], b[1], b[2], b[3]) / w2[j];
            x[0] = x[0] + v[0][j] * coef;
            x[1] = x[1] + v[1][j] * coef;
            x[2] = x[2] + v[2][j] * coef;
        }
    }
}

}  // namespace im
