// The arithmetic of one candidate and one query of csrc/ballfeat.hip: the geometric features of the ball of radius r around a point
// (CloudCompare's computeFeature, restated with a definition of its own). Launch-free like knn_point.h, which it builds on:
// tests/ball_host_harness.cpp compiles this very text for the host and tests/ball_oracle.py restates it in numpy with Python integers,
// bit for bit.
// The neighbours of q are the points p with knn_d2(q, p) <= r2 = fl(r * r), q among them. Each component of the offset fl(p - q) becomes
// the integer rint(u / h), h = r * 2^-18 (|i| <= 2^18 since d2 <= r2, clamped to 2^18 + 1 all the same), and the ball is summed in int64:
// a product is at most (2^18 + 1)^2, a cloud at most 2^26 points, so no sum reaches 2^63 and every sum is exact: the result is a function
// of the input alone, whatever the grid, the lanes and the order of accumulation. Everything after the sums is float64 with contraction off.
#pragma once
#include "knn_point.h"
#include "../../include/icematch.h"

namespace im {
namespace {

constexpr int BALL_QBITS = 18;
constexpr int BALL_QMAX = (1 << BALL_QBITS) + 1;
constexpr long long BALL_MAX_POINTS = 1LL << 26;
constexpr int BALL_MAX_KINDS = 16;
constexpr int BALL_SUMS = 10;          // count, Sx Sy Sz, Sxx Sxy Sxz Syy Syz Szz

struct BallSums { long long s[BALL_SUMS]; };

__device__ __forceinline__ double ball_nan() { return __builtin_nan(""); }

// the quantisation step h = r * BALL_STEP: a power-of-two scaling, exact while the result is a normal number (the entry point refuses the others)
constexpr double BALL_STEP = 0x1p-18;

// rint(u / h): an IEEE division, rounded to the nearest integer, ties to even
__device__ __forceinline__ int ball_quantise(double u, double h) {
#pragma clang fp contract(off)
    const double m = (double)BALL_QMAX;
    double i = rint(u / h);
    i = i < -m ? -m : (i > m ? m : i);
    return (int)i;
}

__device__ __forceinline__ void ball_zero(BallSums& S) {
#pragma unroll
    for (int k = 0; k < BALL_SUMS; ++k) S.s[k] = 0;
}

// offsets fit int32, so each product-and-add is one 32 x 32 -> 64 bit multiply-add
__device__ __forceinline__ void ball_add(BallSums& S, int ix, int iy, int iz) {
    S.s[0] += 1;
    S.s[1] += ix; S.s[2] += iy; S.s[3] += iz;
    S.s[4] += (long long)ix * ix; S.s[5] += (long long)ix * iy; S.s[6] += (long long)ix * iz;
    S.s[7] += (long long)iy * iy; S.s[8] += (long long)iy * iz; S.s[9] += (long long)iz * iz;
}

__device__ __forceinline__ void ball_merge(BallSums& a, const BallSums& b) {
#pragma unroll
    for (int k = 0; k < BALL_SUMS; ++k) a.s[k] += b.s[k];
}

// the candidate p against the query q: added to the sums iff it lies in the ball (d2 == r2 is inside)
__device__ __forceinline__ bool ball_candidate(BallSums& S, double px, double py, double pz, double qx, double qy, double qz, double r2, double h) {
    if (knn_outside(knn_d2(qx, qy, qz, px, py, pz), r2)) return false;
    ball_add(S, ball_quantise(px - qx, h), ball_quantise(py - qy, h), ball_quantise(pz - qz, h));
    return true;
}

// covariance (xx xy xz yy yz zz) in quantised units; int64 -> float64 is the correctly rounded conversion
__device__ __forceinline__ void ball_covariance(const BallSums& S, double (&cov)[6]) {
#pragma clang fp contract(off)
    const double cnt = (double)S.s[0];
    const double mx = (double)S.s[1] / cnt, my = (double)S.s[2] / cnt, mz = (double)S.s[3] / cnt;
    cov[0] = (double)S.s[4] / cnt - mx * mx; cov[1] = (double)S.s[5] / cnt - mx * my; cov[2] = (double)S.s[6] / cnt - mx * mz;
    cov[3] = (double)S.s[7] / cnt - my * my; cov[4] = (double)S.s[8] / cnt - my * mz; cov[5] = (double)S.s[9] / cnt - mz * mz;
}

// cyclic Jacobi as knn_smallest_eigenvector runs it (knn_rotate, KNN_MAX_SWEEPS): a ends (nearly) diagonal, the columns of v are the eigenvectors
__device__ __forceinline__ void ball_jacobi(const double (&cov)[6], double (&a)[3][3], double (&v)[3][3]) {
#pragma clang fp contract(off)
    a[0][0] = cov[0]; a[0][1] = cov[1]; a[0][2] = cov[2];
    a[1][0] = cov[1]; a[1][1] = cov[3]; a[1][2] = cov[4];
    a[2][0] = cov[2]; a[2][1] = cov[4]; a[2][2] = cov[5];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < KNN_MAX_SWEEPS; ++sweep) {
        const bool r01 = knn_rotate<0, 1, 2>(a, v);
        const bool r02 = knn_rotate<0, 2, 1>(a, v);
        const bool r12 = knn_rotate<1, 2, 0>(a, v);
        if (!(r01 || r02 || r12)) break;
    }
}

// (x, y, z) scaled to unit length with the sign rule of the k-NN's normals: the first non-zero of (n_z, n_y, n_x) is positive
__device__ __forceinline__ void ball_unit_signed(double x, double y, double z, double (&nrm)[3]) {
#pragma clang fp contract(off)
    const double len = sqrt(((x * x) + (y * y)) + (z * z));
    if (!(len > 0.0)) { nrm[0] = 0.0; nrm[1] = 0.0; nrm[2] = 1.0; return; }
    x = x / len; y = y / len; z = z / len;
    const bool flip = z != 0.0 ? z < 0.0 : (y != 0.0 ? y < 0.0 : x < 0.0);
    nrm[0] = flip ? -x : x; nrm[1] = flip ? -y : y; nrm[2] = flip ? -z : z;
}

// Eigenvalues descending in squared metres (hh = h * h) and the unit eigenvector of the smallest. The smallest diagonal entry after Jacobi
// is picked by the `<=` chain of knn_smallest_eigenvector; of the other two the larger is the first, the lower index on a tie; what is not above 0 becomes 0.0.
__device__ __forceinline__ void ball_eigen(const double (&cov)[6], double hh, double (&eig)[3], double (&e3)[3]) {
#pragma clang fp contract(off)
    double a[3][3], v[3][3];
    ball_jacobi(cov, a, v);
    const double d0 = a[0][0], d1 = a[1][1], d2 = a[2][2];
    const int k = (d0 <= d1 && d0 <= d2) ? 0 : (d1 <= d2 ? 1 : 2);
    double la, lb, l3;
    if (k == 0) { l3 = a[0][0]; la = a[1][1]; lb = a[2][2]; ball_unit_signed(v[0][0], v[1][0], v[2][0], e3); }
    else if (k == 1) { l3 = a[1][1]; la = a[0][0]; lb = a[2][2]; ball_unit_signed(v[0][1], v[1][1], v[2][1], e3); }
    else { l3 = a[2][2]; la = a[0][0]; lb = a[1][1]; ball_unit_signed(v[0][2], v[1][2], v[2][2], e3); }
    const double l1 = la >= lb ? la : lb, l2 = la >= lb ? lb : la;
    eig[0] = (l1 > 0.0 ? l1 : 0.0) * hh;
    eig[1] = (l2 > 0.0 ? l2 : 0.0) * hh;
    eig[2] = (l3 > 0.0 ? l3 : 0.0) * hh;
}

// a ball that defines no feature: fewer than three points, or no extent at all
__device__ __forceinline__ bool ball_degenerate(const double (&eig)[3], long long count) { return count < 3 || !(eig[0] > 0.0); }

// from the sums of a ball to its eigenvalues and normal; NaN throughout for a degenerate ball
__device__ __forceinline__ void ball_finish(const BallSums& S, double hh, double (&eig)[3], double (&e3)[3]) {
    double cov[6];
    ball_covariance(S, cov);
    ball_eigen(cov, hh, eig, e3);
    if (ball_degenerate(eig, S.s[0])) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { eig[a] = ball_nan(); e3[a] = ball_nan(); }
    }
}

// one feature (im_ball_kind of icematch.h) of a finished ball
__device__ __forceinline__ double ball_feature(int kind, const double (&eig)[3], const double (&e3)[3], long long count) {
#pragma clang fp contract(off)
    if (ball_degenerate(eig, count)) return ball_nan();
    const double l1 = eig[0], l2 = eig[1], l3 = eig[2];
    const double sum = (l1 + l2) + l3;
    switch (kind) {
        case IM_BALL_EIGENVALUES_SUM: return sum;
        case IM_BALL_PCA1: return l1 / sum;
        case IM_BALL_PCA2: return l2 / sum;
        case IM_BALL_SURFACE_VARIATION: return l3 / sum;
        case IM_BALL_LINEARITY: return (l1 - l2) / l1;
        case IM_BALL_PLANARITY: return (l2 - l3) / l1;
        case IM_BALL_ANISOTROPY: return (l1 - l3) / l1;
        case IM_BALL_SPHERICITY: return l3 / l1;
        case IM_BALL_VERTICALITY: return 1.0 - fabs(e3[2]);
        case IM_BALL_EIGENVALUE1: return l1;
        case IM_BALL_EIGENVALUE2: return l2;
        case IM_BALL_EIGENVALUE3: return l3;
        case IM_BALL_NUMBER_OF_NEIGHBORS: return (double)count;
        default: return ball_nan();
    }
}

// The half-width R of the box of cells [c - R, c + R] that holds the whole ball: the smallest r at which the k-NN's stop rule holds with no
// k-th distance (the box covers the grid, or the conservative bound of everything outside it exceeds r2), so the rounding margin of
// knn_face_bound2 carries over unchanged. The rule is monotone in r (every face bound grows with r under monotone rounding, and faces only
// leave the minimum as they reach the grid's edge), hence a binary search over 0 .. max(n) - 1, where the box covers the grid.
__device__ __forceinline__ int ball_rings(const KnnGrid& g, const double (&t)[3], const int (&c)[3], double r2) {
    int lo = 0, hi = g.n[0] > g.n[1] ? g.n[0] : g.n[1];
    hi = (hi > g.n[2] ? hi : g.n[2]) - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (knn_done(g, t, c, mid, knn_inf(), r2)) hi = mid; else lo = mid + 1;
    }
    return lo;
}

}  // namespace
}  // namespace im
