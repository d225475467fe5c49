// The arithmetic of csrc/icp.hip: a rigid transform applied to a point, the rows one correspondence adds to the normal equations of an ICP
// iteration, the tree that sums them, the 6x6 solve, the update of the transform and the measures. Launch-free like
// cyl_point.h: tests/icp_host_harness.cpp compiles this very text for the host and tests/icp_oracle.py restates it in elementwise numpy,
// bit for bit. float64, contraction off, only + - * / and sqrt.
//  apply      p_a = ((M_a0*x + M_a1*y) + M_a2*z) + M_a3, M row-major 4x4 with last row (0, 0, 0, 1); as a vector the + M_a3 is left out.
//  usable     source point i with 0 <= idx[i] < n_target, a finite transformed point and, point-to-plane, a finite target normal. An
//             unusable point adds a row of +0.0 to every sum: no branch changes the order of summation.
//  rows       about the centre c: p' = fl(p - c), e = fl(p - q). Point-to-plane: r = ((ex*nx) + (ey*ny)) + (ez*nz), J = (p' x n, n), each
//             cross component fl(fl(a*b) - fl(c*d)); the normal as given; J and r change sign together under n -> -n, so every product
//             keeps its bits. Point-to-point: the three rows of the unit vectors u_k with r = e_k, added one after the other.
//  sums       ICP_SUMS = 30 terms per point: the 21 upper entries J_a*J_b (a <= b, row-major), the 6 J_a*r, r*r, d2 as the search
//             returned it, 1.0. Held as ICP_TERMS = 32 doubles, the last two +0.0.
//  order      chunks of ICP_CHUNK consecutive source points; inside a chunk thread t of 256 adds points t, t + 256, ... ascending to
//             sums that start at +0.0; the 64 lanes of a wave meet in the butterfly v += v[lane ^ o], o = 1, 2, 4, 8, 16, 32; the four
//             waves as (w0 + w1) + (w2 + w3). Across chunks the same: thread t adds the partials of chunks t, t + 256, ... ascending,
//             then the same tree. A sum is never -0.0 (x + y is -0.0 only for two -0.0, and the sums start at +0.0), so adding a row of
//             +0.0 and adding nothing give the same bits.
//  solve      A x = -b by LDL^T without pivoting (icp_solve); update by the Cayley map (icp_update); measures (icp_finish).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#pragma clang fp contract(off)

namespace im {
namespace {

constexpr int ICP_CHUNK = 1024;        // source points per partial: part of the definition of every sum
constexpr int ICP_BLOCK = 256;         // threads of a chunk; ICP_BLOCK / 64 = 4 waves
constexpr int ICP_SUMS = 30;
constexpr int ICP_TERMS = 32;
constexpr int ICP_N_UPPER = 21, ICP_B = 21, ICP_RR = 27, ICP_D2 = 28, ICP_COUNT = 29;
constexpr int ICP_POINT_TO_POINT = 0, ICP_POINT_TO_PLANE = 1;
constexpr int ICP_OK = 0, ICP_EMPTY = 1, ICP_DEGENERATE = 2;
constexpr double ICP_PIVOT = 0x1p-40;  // a pivot must exceed this fraction of its diagonal entry
// the record im_icp_finish writes, in doubles: M_next [16], fitness, rmse, count, status, x [6], pivots [6], sums [30]
constexpr int ICP_REC_M = 0, ICP_REC_FITNESS = 16, ICP_REC_RMSE = 17, ICP_REC_COUNT = 18, ICP_REC_STATUS = 19, ICP_REC_X = 20,
              ICP_REC_PIVOT = 26, ICP_REC_SUMS = 32, ICP_RECORD = 64;

__device__ __forceinline__ bool icp_finite(double v) { return v - v == 0.0; }      // false for an infinity and for a NaN

__device__ __forceinline__ void icp_apply(const double* M, double x, double y, double z, bool as_vector, double (&out)[3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double v = ((M[4 * a] * x) + (M[4 * a + 1] * y)) + (M[4 * a + 2] * z);
        out[a] = as_vector ? v : v + M[4 * a + 3];
    }
}

// one row: its 28 products added to the sums
__device__ __forceinline__ void icp_add_row(double (&S)[ICP_TERMS], const double (&J)[6], double r) {
#pragma clang fp contract(off)
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) { S[k] = S[k] + J[a] * J[b]; ++k; }
#pragma unroll
    for (int a = 0; a < 6; ++a) S[ICP_B + a] = S[ICP_B + a] + J[a] * r;
    S[ICP_RR] = S[ICP_RR] + r * r;
}

// J = (p' x n, n), each cross component fl(fl(a*b) - fl(c*d))
__device__ __forceinline__ void icp_jacobian(const double (&pc)[3], double nx, double ny, double nz, double (&J)[6]) {
#pragma clang fp contract(off)
    J[0] = (pc[1] * nz) - (pc[2] * ny);
    J[1] = (pc[2] * nx) - (pc[0] * nz);
    J[2] = (pc[0] * ny) - (pc[1] * nx);
    J[3] = nx; J[4] = ny; J[5] = nz;
}

// Source point p (already transformed) against its correspondence: q = tgt[idx], n = nrm[idx] gathered here. idx outside 0..n_tgt-1 reads
// nothing. nrm may be null for point-to-point.
__device__ __forceinline__ void icp_point(double (&S)[ICP_TERMS], double px, double py, double pz, const double* tgt, const double* nrm,
                                          long long n_tgt, int idx, double d2, const double (&c)[3], int method) {
#pragma clang fp contract(off)
    const bool plane = method == ICP_POINT_TO_PLANE;
    bool ok = idx >= 0 && idx < n_tgt && icp_finite(px) && icp_finite(py) && icp_finite(pz);
    double q[3] = {0.0, 0.0, 0.0}, n[3] = {0.0, 0.0, 0.0};
    if (idx >= 0 && idx < n_tgt) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            q[a] = tgt[3 * (long long)idx + a];
            if (plane) n[a] = nrm[3 * (long long)idx + a];
        }
    }
    if (plane) ok = ok && icp_finite(n[0]) && icp_finite(n[1]) && icp_finite(n[2]);
    const double pc[3] = {px - c[0], py - c[1], pz - c[2]};
    const double e[3] = {px - q[0], py - q[1], pz - q[2]};
    double J[6];
    if (plane) {
        const double r = ((e[0] * n[0]) + (e[1] * n[1])) + (e[2] * n[2]);
        icp_jacobian(pc, n[0], n[1], n[2], J);
#pragma unroll
        for (int a = 0; a < 6; ++a) J[a] = ok ? J[a] : 0.0;
        icp_add_row(S, J, ok ? r : 0.0);
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            icp_jacobian(pc, k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0, J);
#pragma unroll
            for (int a = 0; a < 6; ++a) J[a] = ok ? J[a] : 0.0;
            icp_add_row(S, J, ok ? e[k] : 0.0);
        }
    }
    S[ICP_D2] = S[ICP_D2] + (ok ? d2 : 0.0);
    S[ICP_COUNT] = S[ICP_COUNT] + (ok ? 1.0 : 0.0);
}

__device__ __forceinline__ void icp_zero(double (&S)[ICP_TERMS]) {
#pragma unroll
    for (int k = 0; k < ICP_TERMS; ++k) S[k] = 0.0;
}

// the four waves' sums of one term
__device__ __forceinline__ double icp_join_waves(double w0, double w1, double w2, double w3) {
#pragma clang fp contract(off)
    return (w0 + w1) + (w2 + w3);
}

// A x = -b for the symmetric 6x6 A held by its upper entries S[0..20] and b = S[21..26]: A = L D L^T, L unit lower, no pivoting.
//   column j = 0..5: w_k = L_jk * d_k (k < j); d_j = A_jj - L_j0*w_0 - ... - L_j,j-1*w_j-1, subtracted in ascending k;
//                    L_ij = (A_ij - L_i0*w_0 - ... - L_i,j-1*w_j-1) / d_j for i > j, likewise;
//   forward  y_i = (-b_i) - L_i0*y_0 - ... ascending; scaled z_i = y_i / d_i; backward x_i = z_i - L_i+1,i*x_i+1 - ... - L_5i*x_5, ascending k.
// True iff every pivot passes d_j > ICP_PIVOT * A_jj, written so that a NaN fails. x and d are computed whatever the pivots are.
__device__ __forceinline__ bool icp_solve(const double* S, double (&x)[6], double (&d)[6]) {
#pragma clang fp contract(off)
    double A[6][6], L[6][6], w[6], y[6];
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) { A[a][b] = S[k]; A[b][a] = S[k]; ++k; }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
#pragma unroll
        for (int m = 0; m < j; ++m) w[m] = L[j][m] * d[m];
        double v = A[j][j];
#pragma unroll
        for (int m = 0; m < j; ++m) v = v - L[j][m] * w[m];
        d[j] = v;
        ok = ok && (v > ICP_PIVOT * A[j][j]);
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double u = A[i][j];
#pragma unroll
            for (int m = 0; m < j; ++m) u = u - L[i][m] * w[m];
            L[i][j] = u / v;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = -S[ICP_B + i];
#pragma unroll
        for (int m = 0; m < i; ++m) v = v - L[i][m] * y[m];
        y[i] = v;
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double v = y[i] / d[i];
#pragma unroll
        for (int m = i + 1; m < 6; ++m) v = v - L[m][i] * x[m];
        x[i] = v;
    }
    return ok;
}

// The rotation of w = (x0, x1, x2) by the Cayley map: a = w / 2, aa = ((ax*ax) + (ay*ay)) + (az*az), s = 1 + aa,
// R_ii = ((1 - aa) + 2*(a_i*a_i)) / s, R_ij = (2*(a_i*a_j) -+ 2*a_k) / s with the signs of [a]x. Not re-orthonormalised.
__device__ __forceinline__ void icp_cayley(double wx, double wy, double wz, double (&R)[9]) {
#pragma clang fp contract(off)
    const double ax = wx / 2.0, ay = wy / 2.0, az = wz / 2.0;
    const double aa = ((ax * ax) + (ay * ay)) + (az * az);
    const double s = 1.0 + aa, u = 1.0 - aa;
    R[0] = (u + 2.0 * (ax * ax)) / s;
    R[1] = (2.0 * (ax * ay) - 2.0 * az) / s;
    R[2] = (2.0 * (ax * az) + 2.0 * ay) / s;
    R[3] = (2.0 * (ax * ay) + 2.0 * az) / s;
    R[4] = (u + 2.0 * (ay * ay)) / s;
    R[5] = (2.0 * (ay * az) - 2.0 * ax) / s;
    R[6] = (2.0 * (ax * az) - 2.0 * ay) / s;
    R[7] = (2.0 * (ay * az) + 2.0 * ax) / s;
    R[8] = (u + 2.0 * (az * az)) / s;
}

// M_new = [R | T] o M with T_a = fl(fl(t_a + c_a) - ((R_a0*cx + R_a1*cy) + R_a2*cz)): the step x = (w, t) was taken about c.
// M_new_aj = ((R_a0*M_0j + R_a1*M_1j) + R_a2*M_2j) [+ T_a for j = 3]; the last row is (0, 0, 0, 1). M and out may not overlap.
__device__ __forceinline__ void icp_update(const double (&x)[6], const double (&c)[3], const double* M, double* out) {
#pragma clang fp contract(off)
    double R[9];
    icp_cayley(x[0], x[1], x[2], R);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double Rc = ((R[3 * a] * c[0]) + (R[3 * a + 1] * c[1])) + (R[3 * a + 2] * c[2]);
        const double T = (x[3 + a] + c[a]) - Rc;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double v = ((R[3 * a] * M[j]) + (R[3 * a + 1] * M[4 + j])) + (R[3 * a + 2] * M[8 + j]);
            out[4 * a + j] = j == 3 ? v + T : v;
        }
    }
    out[12] = 0.0; out[13] = 0.0; out[14] = 0.0; out[15] = 1.0;
}

// The record of one iteration from the 32 sums S, the transform M the sums were taken at, the centre and the number of source points.
// count == 0: EMPTY; else count < 6 or a failed pivot: DEGENERATE; M_next = M with either, and with solve == 0 (where x and the pivots are 0
// and the status is EMPTY or OK). fitness = count / n (0 for n == 0), rmse = sqrt(sum d2 / count) (0 for count 0).
__device__ __forceinline__ void icp_finish(const double* S, const double* M, const double (&c)[3], long long n, bool solve, double* rec) {
#pragma clang fp contract(off)
    const double count = S[ICP_COUNT];
    double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, d[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int status = ICP_OK;
    if (solve) status = icp_solve(S, x, d) && count >= 6.0 ? ICP_OK : ICP_DEGENERATE;
    if (!(count > 0.0)) status = ICP_EMPTY;
    double Mi[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) Mi[k] = M[k];
    if (solve && status == ICP_OK) {
        icp_update(x, c, Mi, rec + ICP_REC_M);
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) rec[ICP_REC_M + k] = Mi[k];
    }
    rec[ICP_REC_FITNESS] = n > 0 ? count / (double)n : 0.0;
    rec[ICP_REC_RMSE] = count > 0.0 ? sqrt(S[ICP_D2] / count) : 0.0;
    rec[ICP_REC_COUNT] = count;
    rec[ICP_REC_STATUS] = (double)status;
#pragma unroll
    for (int k = 0; k < 6; ++k) { rec[ICP_REC_X + k] = x[k]; rec[ICP_REC_PIVOT + k] = d[k]; }
#pragma unroll
    for (int k = 0; k < ICP_SUMS; ++k) rec[ICP_REC_SUMS + k] = S[k];
    rec[ICP_REC_SUMS + 30] = 0.0; rec[ICP_REC_SUMS + 31] = 0.0;
}

}  // namespace
}  // namespace im
