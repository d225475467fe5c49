// The arithmetic of csrc/ba.hip: two-view bundle adjustment with control points. One problem is one epoch: two cameras, tie
// points and control points. Launch-free like icp_point.h: tests/ba_host_harness.cpp compiles this very text for the host and
// tests/ba_oracle.py restates it in elementwise numpy, bit for bit. float64, contraction off, only + - * / and sqrt. A definition of its
// own: parity with Metashape's optimizeCameras is unpinned.
//  camera     BA_CAMSTATE = 24 doubles: R [9] row-major, C [3], fx fy cx cy, k1 k2 p1 p2 k3 k4 k5 k6; Xc = R (X - C). An epoch holds two.
//  project    d = X - C, Xc_a = ((R_a0*d0) + (R_a1*d1)) + (R_a2*d2), x = Xc0 / Xc2, y = Xc1 / Xc2, r2 = (x*x) + (y*y),
//             num = 1 + ((k3 r2 + k2) r2 + k1) r2, den = 1 + ((k6 r2 + k5) r2 + k4) r2, radial = num / den,
//             dx = ((2 p1) x) y + p2 (r2 + (2 x) x), dy = p1 (r2 + (2 y) y) + ((2 p2) x) y, xd = x radial + dx, yd = y radial + dy,
//             u = fx xd + cx, v = fy yd + cy: the forward model that undistort_one (sfm_point.h) inverts, with its groupings.
//  parameters BA_CAM = 14 per camera: w [3] (R <- Cayley(w) R, the map of icp_cayley), dC [3], df (added to fx and fy), dcx, dcy, dk1, dk2,
//             dp1, dp2, dk3; k4..k6 stay. BA_DIM = 28. Bit p of the mask frees parameter p; a fixed one has row and column p replaced by
//             the identity and its right-hand side by 0.
//  point      X [3], obs (u0, v0, u1, v1) in pixels (a NaN u or v: that camera does not see it), sigma in pixels, prior (X0 [3], sX [3]),
//             sX_k > 0 puts (X_k - X0_k) / sX_k into the cost. Usable iff X is finite, sigma > 0 and finite, every present observation is
//             finite with Xc2 > 0 and a finite projection, every prior residual is finite, and there are two observations or one and a
//             full prior. An unusable point adds +0.0 to every sum and does not move. Rows: per observing camera c the two residuals
//             r = ((u - u_obs) / sigma, (v - v_obs) / sigma) as products with is = 1 / sigma, Jc (2 x 14) and Jp (2 x 3), analytic.
//  factors    V = Jp^T Jp + diag(1 / sX^2), g = Jp^T r + prior, V' = V + lambda diag(V), V' = L D L^T (3 x 3, explicit, ba_ldl3);
//             per parameter a: W_a = Jc_a^T Jp (3), t = L^-1 W_a, Y_ak = t_k / sqrt(d_k); z = D^-1/2 L^-1 g. Then W V'^-1 W^T = Y Y^T and
//             W V'^-1 g = Y z. BA_FAC = 155 doubles per point: Jc [4][14], r [4], Y [28][3], z [3], L (l10 l20 l21), D [3], cost, usable.
//  sums       BA_SUMS = 436: the 406 upper entries (a <= b, row-major) JJ_ab - YY_ab, the 28 right-hand sides Jr_a - Yz_a, the cost
//             0.5 * ((((r0 r0 + r1 r1) + r2 r2) + r3 r3) + ((q0 q0 + q1 q1) + q2 q2)), the usable count. JJ_ab = (J_2c,a J_2c,b) + (J_2c+1,a
//             J_2c+1,b) when a and b belong to one camera c, +0.0 otherwise; YY_ab = ((Y_a0 Y_b0) + (Y_a1 Y_b1)) + (Y_a2 Y_b2);
//             Jr_a = (J_2c,a r_2c) + (J_2c+1,a r_2c+1); Yz_a = ((Y_a0 z0) + (Y_a1 z1)) + (Y_a2 z2). Held as BA_TERMS = 448 doubles.
//  order      chunks of BA_CHUNK consecutive points of one epoch; every sum starts at +0.0 and takes the chunk's points in ascending
//             index; the chunk partials of an epoch are then added in ascending chunk order to +0.0. A sum is never -0.0, so a term of
//             either zero leaves it as it is. Nothing depends on the launch shape, the number of epochs or the place of an epoch.
//  solve      ba_reduced: centre priors (linear in dC), damping A_pp += lambda A_pp, mask, A x = -b by LDL^T without pivoting with the
//             pivot rule of icp_solve (ba_solve, n = 28), candidate cameras (ba_step_camera).
//  points     dX = -L^-T D^-1/2 (z + Y^T x), the 28 products added in ascending parameter (ba_point_step).
//  schedule   ba_decide: accept iff the candidate's cost is strictly lower; lambda / 10 (floored) or lambda * 10; OK on a relative decrease
//             <= ftol or a cost <= ctol at an accepted step, STALLED when lambda passes its ceiling, MAX_ITER, EMPTY, DEGENERATE (the state stays).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "icp_point.h"

#pragma clang fp contract(off)

namespace im {
namespace {

constexpr int BA_CHUNK = 256;          // points per partial: part of the definition of every sum
constexpr int BA_TILE = 32;            // points whose factors sit in LDS at a time: BA_TILE * BA_FAC * 8 = 39680 bytes
constexpr int BA_BLOCK = 256;          // threads of a chunk
constexpr int BA_CAM = 14, BA_DIM = 28, BA_CAMSTATE = 24, BA_EPOCH = 48;
constexpr int BA_N_UPPER = 406, BA_B = 406, BA_COST = 434, BA_COUNT = 435, BA_SUMS = 436, BA_TERMS = 448;
constexpr int BA_F_J = 0, BA_F_R = 56, BA_F_Y = 60, BA_F_Z = 144, BA_F_L = 147, BA_F_D = 150, BA_F_COST = 153, BA_F_OK = 154, BA_FAC = 155;
constexpr int BA_KEEP = BA_FAC - BA_F_Y;   // what the back-substitution reads per point: Y, z, L, D, cost, usable = 95 doubles
constexpr int BA_RUNNING = -1, BA_OK = 0, BA_MAX_ITER = 1, BA_STALLED = 2, BA_EMPTY = 3, BA_DEGENERATE = 4;
constexpr unsigned BA_MASK_DEFAULT = 0x7Fu | (0x7Fu << 14);   // both poses and f of both cameras
constexpr double BA_PIVOT = ICP_PIVOT;
// the state of an epoch, in doubles: lambda, parity of the current buffers, done, status, iterations recorded
constexpr int BA_ST_LAMBDA = 0, BA_ST_PARITY = 1, BA_ST_DONE = 2, BA_ST_STATUS = 3, BA_ST_ITER = 4, BA_STATE = 8;
// the record of an iteration, in doubles: cost before, cost after, lambda, accepted, usable count, status after, x [28], pivots [28], iteration
constexpr int BA_REC_COST0 = 0, BA_REC_COST1 = 1, BA_REC_LAMBDA = 2, BA_REC_ACCEPTED = 3, BA_REC_COUNT = 4, BA_REC_STATUS = 5, BA_REC_X = 6,
              BA_REC_PIVOT = 34, BA_REC_ITER = 62, BA_RECORD = 64;
// what im_ba_solve leaves per epoch: the 448 sums, then the draft of the record (cost before with the centre priors, lambda, count, x, pivots;
// BA_REC_ACCEPTED holds 1.0 where the solve passed the pivot rule)
constexpr int BA_SOL_REC = 448, BA_SOL = 512;
// the options, in doubles: lambda floor, lambda ceiling, ftol, max_iter, ctol (a cost at or below it is converged: 0 leaves it to ftol)
constexpr int BA_OPT_LMIN = 0, BA_OPT_LMAX = 1, BA_OPT_FTOL = 2, BA_OPT_MAX_ITER = 3, BA_OPT_CTOL = 4, BA_OPTS = 5;

struct BaProj { double Xc[3], x, y, r2, num, den, radial, xd, yd, u, v; };

__device__ __forceinline__ void ba_project(const double* cam, const double (&X)[3], BaProj& p) {
#pragma clang fp contract(off)
    const double d0 = X[0] - cam[9], d1 = X[1] - cam[10], d2 = X[2] - cam[11];
#pragma unroll
    for (int a = 0; a < 3; ++a) p.Xc[a] = ((cam[3 * a] * d0) + (cam[3 * a + 1] * d1)) + (cam[3 * a + 2] * d2);
    const double fx = cam[12], fy = cam[13], cx = cam[14], cy = cam[15];
    const double k1 = cam[16], k2 = cam[17], p1 = cam[18], p2 = cam[19], k3 = cam[20], k4 = cam[21], k5 = cam[22], k6 = cam[23];
    const double x = p.Xc[0] / p.Xc[2], y = p.Xc[1] / p.Xc[2];
    const double r2 = (x * x) + (y * y);
    p.num = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
    p.den = 1.0 + ((k6 * r2 + k5) * r2 + k4) * r2;
    p.radial = p.num / p.den;
    const double dx = ((2.0 * p1) * x) * y + p2 * (r2 + (2.0 * x) * x);
    const double dy = p1 * (r2 + (2.0 * y) * y) + ((2.0 * p2) * x) * y;
    p.x = x; p.y = y; p.r2 = r2;
    p.xd = x * p.radial + dx;
    p.yd = y * p.radial + dy;
    p.u = fx * p.xd + cx;
    p.v = fy * p.yd + cy;
}

// The two rows of camera `cam` seeing X at (uo, vo): r [2], Jp [2][3], Jc [2][14] written to J[0..13] and J[14..27]. is = 1 / sigma.
__device__ __forceinline__ void ba_rows(const double* cam, const BaProj& p, double uo, double vo, double is, double* J, double (&Jp)[2][3],
                                        double (&r)[2]) {
#pragma clang fp contract(off)
    const double fx = cam[12], fy = cam[13];
    const double k1 = cam[16], k2 = cam[17], p1 = cam[18], p2 = cam[19], k3 = cam[20], k4 = cam[21], k5 = cam[22], k6 = cam[23];
    const double x = p.x, y = p.y, r2 = p.r2;
    const double dnum = ((3.0 * k3) * r2 + 2.0 * k2) * r2 + k1;
    const double dden = ((3.0 * k6) * r2 + 2.0 * k5) * r2 + k4;
    const double drad = ((dnum * p.den) - (p.num * dden)) / (p.den * p.den);
    const double tx = (2.0 * x) * drad, ty = (2.0 * y) * drad;                  // d radial / dx, d radial / dy
    const double xx = ((p.radial + x * tx) + (2.0 * p1) * y) + (6.0 * p2) * x;  // d xd / dx
    const double xy = (x * ty + (2.0 * p1) * x) + (2.0 * p2) * y;               // d xd / dy
    const double yx = (y * tx + (2.0 * p1) * x) + (2.0 * p2) * y;               // d yd / dx
    const double yy = ((p.radial + y * ty) + (6.0 * p1) * y) + (2.0 * p2) * x;  // d yd / dy
    const double G[2][2] = {{fx * xx, fx * xy}, {fy * yx, fy * yy}};
    const double iz = 1.0 / p.Xc[2];
    double B[2][3];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        B[i][0] = (G[i][0] * iz) * is;
        B[i][1] = (G[i][1] * iz) * is;
        B[i][2] = (-(((G[i][0] * x) + (G[i][1] * y)) * iz)) * is;
    }
    const double e1 = r2 / p.den, e2 = (r2 * r2) / p.den, e3 = ((r2 * r2) * r2) / p.den;
    const double xyp = (2.0 * x) * y;
    const double s[2] = {fx, fy}, c[2] = {x, y}, dd[2] = {p.xd, p.yd};
    const double t1[2] = {xyp, r2 + (2.0 * y) * y}, t2[2] = {r2 + (2.0 * x) * x, xyp};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        double* Ji = J + BA_CAM * i;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            Jp[i][k] = ((B[i][0] * cam[k]) + (B[i][1] * cam[3 + k])) + (B[i][2] * cam[6 + k]);
            Ji[3 + k] = -Jp[i][k];
        }
        Ji[0] = (B[i][2] * p.Xc[1]) - (B[i][1] * p.Xc[2]);
        Ji[1] = (B[i][0] * p.Xc[2]) - (B[i][2] * p.Xc[0]);
        Ji[2] = (B[i][1] * p.Xc[0]) - (B[i][0] * p.Xc[1]);
        Ji[6] = dd[i] * is;
        Ji[7] = i == 0 ? is : 0.0;
        Ji[8] = i == 1 ? is : 0.0;
        Ji[9] = ((s[i] * c[i]) * e1) * is;
        Ji[10] = ((s[i] * c[i]) * e2) * is;
        Ji[11] = (s[i] * t1[i]) * is;
        Ji[12] = (s[i] * t2[i]) * is;
        Ji[13] = ((s[i] * c[i]) * e3) * is;
    }
    r[0] = (p.u - uo) * is;
    r[1] = (p.v - vo) * is;
}

// Whether the point is usable in this state, the residuals of its present observations in pixels (res [2][2], 0.0 where absent), its prior
// residuals q [3] and its projections. seen [c]: camera c has an observation (neither u nor v is a NaN).
__device__ __forceinline__ bool ba_usable(const double* cams, const double (&X)[3], const double* obs, double sigma, const double* prior,
                                          BaProj (&pr)[2], bool (&seen)[2], double (&q)[3]) {
#pragma clang fp contract(off)
    bool ok = icp_finite(X[0]) && icp_finite(X[1]) && icp_finite(X[2]) && sigma > 0.0 && icp_finite(sigma);
    int n_obs = 0;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const double uo = obs[2 * c], vo = obs[2 * c + 1];
        seen[c] = uo == uo && vo == vo;
        ba_project(cams + BA_CAMSTATE * c, X, pr[c]);
        if (seen[c]) {
            ++n_obs;
            ok = ok && icp_finite(uo) && icp_finite(vo) && pr[c].Xc[2] > 0.0 && icp_finite(pr[c].u) && icp_finite(pr[c].v);
        }
    }
    bool full = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const bool has = prior[3 + k] > 0.0;
        q[k] = has ? (X[k] - prior[k]) / prior[3 + k] : 0.0;
        ok = ok && icp_finite(q[k]);
        full = full && has;
    }
    return ok && (n_obs == 2 || (n_obs == 1 && full));
}

__device__ __forceinline__ double ba_half_squares(const double (&r)[4], const double (&q)[3]) {
#pragma clang fp contract(off)
    return 0.5 * (((((r[0] * r[0]) + (r[1] * r[1])) + (r[2] * r[2])) + (r[3] * r[3])) + (((q[0] * q[0]) + (q[1] * q[1])) + (q[2] * q[2])));
}

// V = L D L^T, V symmetric 3 x 3 by its upper entries (v00 v01 v02 v11 v12 v22): d0 = v00, l10 = v01 / d0, l20 = v02 / d0,
// d1 = v11 - l10 * (l10 * d0), l21 = (v12 - l20 * (l10 * d0)) / d1, d2 = (v22 - l20 * (l20 * d0)) - l21 * (l21 * d1).
__device__ __forceinline__ void ba_ldl3(const double (&V)[6], double (&L)[3], double (&D)[3]) {
#pragma clang fp contract(off)
    D[0] = V[0];
    L[0] = V[1] / D[0];
    L[1] = V[2] / D[0];
    const double w10 = L[0] * D[0];
    D[1] = V[3] - L[0] * w10;
    L[2] = (V[4] - L[1] * w10) / D[1];
    D[2] = (V[5] - L[1] * (L[1] * D[0])) - L[2] * (L[2] * D[1]);
}

// t = L^-1 w, out_k = t_k / sqrt(d_k)
__device__ __forceinline__ void ba_forward3(const double (&L)[3], const double (&sd)[3], double w0, double w1, double w2, double* out) {
#pragma clang fp contract(off)
    const double t0 = w0;
    const double t1 = w1 - L[0] * t0;
    const double t2 = (w2 - L[1] * t0) - L[2] * t1;
    out[0] = t0 / sd[0]; out[1] = t1 / sd[1]; out[2] = t2 / sd[2];
}

// The factors of one point: f [BA_FAC]. cams: the epoch's two cameras [48]; obs [4]; prior [6]. An unusable point: every entry +0.0.
__device__ __forceinline__ void ba_point_factors(const double* cams, const double (&X)[3], const double* obs, double sigma, const double* prior,
                                                 double lambda, double* f) {
#pragma clang fp contract(off)
    BaProj pr[2];
    bool seen[2];
    double q[3];
    const bool ok = ba_usable(cams, X, obs, sigma, prior, pr, seen, q);
    const double is = 1.0 / sigma;
    double Jp[4][3], r[4];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        double jp[2][3], rr[2];
        ba_rows(cams + BA_CAMSTATE * c, pr[c], obs[2 * c], obs[2 * c + 1], is, f + BA_F_J + 2 * BA_CAM * c, jp, rr);
        const bool use = ok && seen[c];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            r[2 * c + i] = use ? rr[i] : 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) Jp[2 * c + i][k] = use ? jp[i][k] : 0.0;
        }
        for (int j = 0; j < 2 * BA_CAM; ++j) f[BA_F_J + 2 * BA_CAM * c + j] = use ? f[BA_F_J + 2 * BA_CAM * c + j] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) f[BA_F_R + i] = r[i];
    double V[6], g[3];
    int m = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double ip = ok && prior[3 + a] > 0.0 ? 1.0 / prior[3 + a] : 0.0;
        const double qa = ok ? q[a] : 0.0;
        q[a] = qa;
        g[a] = ((((Jp[0][a] * r[0]) + (Jp[1][a] * r[1])) + (Jp[2][a] * r[2])) + (Jp[3][a] * r[3])) + qa * ip;
#pragma unroll
        for (int b = a; b < 3; ++b) {
            double v = (((Jp[0][a] * Jp[0][b]) + (Jp[1][a] * Jp[1][b])) + (Jp[2][a] * Jp[2][b])) + (Jp[3][a] * Jp[3][b]);
            if (b == a) { v = v + ip * ip; v = v + lambda * v; }
            V[m++] = v;
        }
    }
    double L[3], D[3], sd[3];
    ba_ldl3(V, L, D);
#pragma unroll
    for (int k = 0; k < 3; ++k) sd[k] = sqrt(D[k]);
    for (int a = 0; a < BA_DIM; ++a) {
        const double* j0 = f + BA_F_J + 2 * BA_CAM * (a / BA_CAM) + a % BA_CAM;
        const int i0 = 2 * (a / BA_CAM);
        const double ja = j0[0], jb = j0[BA_CAM];
        double y[3];
        ba_forward3(L, sd, (ja * Jp[i0][0]) + (jb * Jp[i0 + 1][0]), (ja * Jp[i0][1]) + (jb * Jp[i0 + 1][1]),
                    (ja * Jp[i0][2]) + (jb * Jp[i0 + 1][2]), y);
#pragma unroll
        for (int k = 0; k < 3; ++k) f[BA_F_Y + 3 * a + k] = ok ? y[k] : 0.0;
    }
    double z[3];
    ba_forward3(L, sd, g[0], g[1], g[2], z);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        f[BA_F_Z + k] = ok ? z[k] : 0.0;
        f[BA_F_L + k] = ok ? L[k] : 0.0;
        f[BA_F_D + k] = ok ? D[k] : 0.0;
    }
    f[BA_F_COST] = ok ? ba_half_squares(r, q) : 0.0;
    f[BA_F_OK] = ok ? 1.0 : 0.0;
}

// What one point adds to sum e (0 .. BA_TERMS - 1) from its factors.
__device__ __forceinline__ double ba_term(const double* f, int e_kind, int a, int b) {
#pragma clang fp contract(off)
    // e_kind 0: upper entry (a, b); 1: right-hand side a; 2: cost; 3: count; 4: padding
    if (e_kind == 0) {
        const double* ya = f + BA_F_Y + 3 * a;
        const double* yb = f + BA_F_Y + 3 * b;
        const double yy = ((ya[0] * yb[0]) + (ya[1] * yb[1])) + (ya[2] * yb[2]);
        double jj = 0.0;
        if (a / BA_CAM == b / BA_CAM) {
            const double* j = f + BA_F_J + 2 * BA_CAM * (a / BA_CAM);
            jj = (j[a % BA_CAM] * j[b % BA_CAM]) + (j[BA_CAM + a % BA_CAM] * j[BA_CAM + b % BA_CAM]);
        }
        return jj - yy;
    }
    if (e_kind == 1) {
        const double* ya = f + BA_F_Y + 3 * a;
        const double yz = ((ya[0] * f[BA_F_Z]) + (ya[1] * f[BA_F_Z + 1])) + (ya[2] * f[BA_F_Z + 2]);
        const double* j = f + BA_F_J + 2 * BA_CAM * (a / BA_CAM);
        const double* r = f + BA_F_R + 2 * (a / BA_CAM);
        const double jr = (j[a % BA_CAM] * r[0]) + (j[BA_CAM + a % BA_CAM] * r[1]);
        return jr - yz;
    }
    if (e_kind == 2) return f[BA_F_COST];
    if (e_kind == 3) return f[BA_F_OK];
    return 0.0;
}

// sum e -> what it is: upper entries row-major (a <= b), then the right-hand sides, the cost, the count, padding
__device__ __forceinline__ void ba_entry(int e, int& kind, int& a, int& b) {
    a = 0; b = 0;
    if (e < BA_N_UPPER) {
        kind = 0;
        int row = 0, left = e;
        while (left >= BA_DIM - row) { left -= BA_DIM - row; ++row; }
        a = row; b = row + left;
    } else if (e < BA_COST) { kind = 1; a = e - BA_B; }
    else if (e == BA_COST) kind = 2;
    else if (e == BA_COUNT) kind = 3;
    else kind = 4;
}

// 0.5 * sum of the squared centre-prior residuals of the epoch's cameras, camera 0 then 1, x y z: cprior [2][6] = (C0 [3], sC [3]), sC_k > 0
__device__ __forceinline__ double ba_centre_cost(const double* cams, const double* cprior) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int c = 0; c < 2; ++c)
        for (int k = 0; k < 3; ++k) {
            const double sc = cprior[6 * c + 3 + k];
            const double rp = sc > 0.0 ? (cams[BA_CAMSTATE * c + 9 + k] - cprior[6 * c + k]) / sc : 0.0;
            s = s + 0.5 * (rp * rp);
        }
    return s;
}

// The reduced system of an epoch from its 448 sums: A [28][28] (full, symmetric) and b [28] with the centre priors added
// (A_pp += (1 / sC) * (1 / sC), b_p += rp * (1 / sC), p = 14 c + 3 + k), the diagonal damped (A_pp += lambda * A_pp) and the mask applied.
__device__ __forceinline__ void ba_reduced(const double* S, const double* cams, const double* cprior, double lambda, unsigned mask, double* A,
                                           double* b) {
#pragma clang fp contract(off)
    int m = 0;
    for (int a = 0; a < BA_DIM; ++a)
        for (int c = a; c < BA_DIM; ++c) { A[BA_DIM * a + c] = S[m]; A[BA_DIM * c + a] = S[m]; ++m; }
    for (int a = 0; a < BA_DIM; ++a) b[a] = S[BA_B + a];
    for (int c = 0; c < 2; ++c)
        for (int k = 0; k < 3; ++k) {
            const double sc = cprior[6 * c + 3 + k];
            if (sc > 0.0) {
                const int p = BA_CAM * c + 3 + k;
                const double ip = 1.0 / sc;
                const double rp = (cams[BA_CAMSTATE * c + 9 + k] - cprior[6 * c + k]) / sc;
                A[BA_DIM * p + p] = A[BA_DIM * p + p] + ip * ip;
                b[p] = b[p] + rp * ip;
            }
        }
    for (int p = 0; p < BA_DIM; ++p) A[BA_DIM * p + p] = A[BA_DIM * p + p] + lambda * A[BA_DIM * p + p];
    for (int p = 0; p < BA_DIM; ++p)
        if (!((mask >> p) & 1u)) {
            for (int a = 0; a < BA_DIM; ++a) { A[BA_DIM * p + a] = 0.0; A[BA_DIM * a + p] = 0.0; }
            A[BA_DIM * p + p] = 1.0;
            b[p] = 0.0;
        }
}

// A x = -b, A symmetric 28 x 28: icp_solve's LDL^T without pivoting and its pivot rule, n = 28. L overwrites the strict lower triangle of A
// (the upper one keeps A). w: 2 * 28 doubles of work space. True iff every pivot passes d_j > BA_PIVOT * A_jj.
__device__ __forceinline__ bool ba_solve(double* A, const double* b, double* x, double* d, double* w) {
#pragma clang fp contract(off)
    constexpr int n = BA_DIM;
    double* y = w + n;
    bool ok = true;
    for (int j = 0; j < n; ++j) {
        for (int m = 0; m < j; ++m) w[m] = A[n * j + m] * d[m];
        double v = A[n * j + j];
        for (int m = 0; m < j; ++m) v = v - A[n * j + m] * w[m];
        d[j] = v;
        ok = ok && (v > BA_PIVOT * A[n * j + j]);
        for (int i = j + 1; i < n; ++i) {
            double u = A[n * j + i];                    // the upper triangle still holds A_ij
            for (int m = 0; m < j; ++m) u = u - A[n * i + m] * w[m];
            A[n * i + j] = u / v;
        }
    }
    for (int i = 0; i < n; ++i) {
        double v = -b[i];
        for (int m = 0; m < i; ++m) v = v - A[n * i + m] * y[m];
        y[i] = v;
    }
    for (int i = n - 1; i >= 0; --i) {
        double v = y[i] / d[i];
        for (int m = i + 1; m < n; ++m) v = v - A[n * m + i] * x[m];
        x[i] = v;
    }
    return ok;
}

// One camera stepped by its 14 parameters: R' = Cayley(w) R, R'_aj = ((Q_a0*R_0j) + (Q_a1*R_1j)) + (Q_a2*R_2j); the rest added.
__device__ __forceinline__ void ba_step_camera(const double* cam, const double* x, double* out) {
#pragma clang fp contract(off)
    double Q[9];
    icp_cayley(x[0], x[1], x[2], Q);
    for (int a = 0; a < 3; ++a)
        for (int j = 0; j < 3; ++j) out[3 * a + j] = ((Q[3 * a] * cam[j]) + (Q[3 * a + 1] * cam[3 + j])) + (Q[3 * a + 2] * cam[6 + j]);
    for (int k = 0; k < 3; ++k) out[9 + k] = cam[9 + k] + x[3 + k];
    out[12] = cam[12] + x[6];
    out[13] = cam[13] + x[6];
    out[14] = cam[14] + x[7];
    out[15] = cam[15] + x[8];
    out[16] = cam[16] + x[9];
    out[17] = cam[17] + x[10];
    out[18] = cam[18] + x[11];
    out[19] = cam[19] + x[12];
    out[20] = cam[20] + x[13];
    out[21] = cam[21]; out[22] = cam[22]; out[23] = cam[23];
}

// The step of one point from what the accumulation kept (keep [BA_KEEP]: Y, z, L, D, cost, usable) and the cameras' step x [28]:
// q_k = z_k + Y_0k x_0 + ... + Y_27k x_27 (ascending), s_k = q_k / sqrt(d_k), e2 = s2, e1 = s1 - l21 e2, e0 = (s0 - l10 e1) - l20 e2,
// X' = X + (-e). An unusable point stays.
__device__ __forceinline__ void ba_point_step(const double* keep, const double* x, const double (&X)[3], double (&out)[3]) {
#pragma clang fp contract(off)
    const double* Y = keep;
    const double* z = keep + (BA_F_Z - BA_F_Y);
    const double* L = keep + (BA_F_L - BA_F_Y);
    const double* D = keep + (BA_F_D - BA_F_Y);
    const bool ok = keep[BA_F_OK - BA_F_Y] != 0.0;
    double q[3] = {z[0], z[1], z[2]};
    for (int a = 0; a < BA_DIM; ++a) {
        const double xa = x[a];
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = q[k] + Y[3 * a + k] * xa;
    }
    const double s0 = q[0] / sqrt(D[0]), s1 = q[1] / sqrt(D[1]), s2 = q[2] / sqrt(D[2]);
    const double e2 = s2;
    const double e1 = s1 - L[2] * e2;
    const double e0 = (s0 - L[0] * e1) - L[1] * e2;
    out[0] = ok ? X[0] + (-e0) : X[0];
    out[1] = ok ? X[1] + (-e1) : X[1];
    out[2] = ok ? X[2] + (-e2) : X[2];
}

// The cost term of a point at a candidate state: its half squares where it is usable there, +inf where a point that was usable is not
// (the step is then rejected), +0.0 for a point that was not.
__device__ __forceinline__ double ba_point_cost(const double* cams, const double (&X)[3], const double* obs, double sigma, const double* prior,
                                                bool was_usable) {
#pragma clang fp contract(off)
    BaProj pr[2];
    bool seen[2];
    double q[3], r[4];
    const bool ok = ba_usable(cams, X, obs, sigma, prior, pr, seen, q);
    const double is = 1.0 / sigma;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        r[2 * c] = seen[c] ? (pr[c].u - obs[2 * c]) * is : 0.0;
        r[2 * c + 1] = seen[c] ? (pr[c].v - obs[2 * c + 1]) * is : 0.0;
    }
    if (!was_usable) return 0.0;
    return ok ? ba_half_squares(r, q) : HUGE_VAL;
}

// The reprojection residuals of one point in pixels: res [2][3] = (u - u_obs, v - v_obs, sqrt((x*x) + (y*y))) per camera, NaN where the
// camera does not see the point or the point is unusable.
__device__ __forceinline__ void ba_point_residuals(const double* cams, const double (&X)[3], const double* obs, double* res) {
#pragma clang fp contract(off)
    const double no_prior[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    BaProj pr[2];
    bool seen[2];
    double q[3];
    ba_usable(cams, X, obs, 1.0, no_prior, pr, seen, q);
    const double nan = __builtin_nan("");
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const double ex = pr[c].u - obs[2 * c], ey = pr[c].v - obs[2 * c + 1];
        const bool fine = seen[c] && icp_finite(ex) && icp_finite(ey) && pr[c].Xc[2] > 0.0;
        res[3 * c] = fine ? ex : nan;
        res[3 * c + 1] = fine ? ey : nan;
        res[3 * c + 2] = fine ? sqrt((ex * ex) + (ey * ey)) : nan;
    }
}

// The draft of an epoch's record from its sums: rec [BA_RECORD], and the candidate cameras cand [48]. A, b, x-work: caller's memory
// (A [784], wk [28 + 28 + 56]). An epoch without a usable point, or with a failed pivot, keeps its cameras.
__device__ __forceinline__ void ba_solve_epoch(const double* S, const double* cams, const double* cprior, double lambda, unsigned mask,
                                               double* A, double* wk, double* rec, double* cand) {
#pragma clang fp contract(off)
    double* b = wk;
    double* x = wk + BA_DIM;
    double* d = wk + 2 * BA_DIM;
    double* w = wk + 3 * BA_DIM;
    ba_reduced(S, cams, cprior, lambda, mask, A, b);
    const bool ok = ba_solve(A, b, x, d, w);
    const double count = S[BA_COUNT];
    const bool step = ok && count > 0.0;
    for (int k = 0; k < BA_RECORD; ++k) rec[k] = 0.0;
    rec[BA_REC_COST0] = S[BA_COST] + ba_centre_cost(cams, cprior);
    rec[BA_REC_LAMBDA] = lambda;
    rec[BA_REC_ACCEPTED] = ok ? 1.0 : 0.0;
    rec[BA_REC_COUNT] = count;
    for (int k = 0; k < BA_DIM; ++k) { rec[BA_REC_X + k] = step ? x[k] : 0.0; rec[BA_REC_PIVOT + k] = d[k]; }
    for (int c = 0; c < 2; ++c) {
        if (step) ba_step_camera(cams + BA_CAMSTATE * c, rec + BA_REC_X + BA_CAM * c, cand + BA_CAMSTATE * c);
        else
            for (int k = 0; k < BA_CAMSTATE; ++k) cand[BA_CAMSTATE * c + k] = cams[BA_CAMSTATE * c + k];
    }
}

// The decision of an iteration: draft (im_ba_solve's), the candidate's cost cost1 (points and centre priors), the options. Completes the record
// rec [BA_RECORD] and updates the state st [BA_STATE].
__device__ __forceinline__ void ba_decide(const double* draft, double cost1, const double* opts, double* st, double* rec) {
#pragma clang fp contract(off)
    for (int k = 0; k < BA_RECORD; ++k) rec[k] = draft[k];
    const double cost0 = draft[BA_REC_COST0], lambda = draft[BA_REC_LAMBDA], iter = st[BA_ST_ITER];
    int status = BA_RUNNING;
    bool accepted = false;
    double next = lambda;
    if (!(draft[BA_REC_COUNT] > 0.0)) status = BA_EMPTY;
    else if (draft[BA_REC_ACCEPTED] == 0.0) status = BA_DEGENERATE;
    else {
        accepted = cost1 < cost0;
        if (accepted) {
            next = lambda / 10.0;
            next = next < opts[BA_OPT_LMIN] ? opts[BA_OPT_LMIN] : next;
            if ((cost0 - cost1) <= opts[BA_OPT_FTOL] * cost0 || cost1 <= opts[BA_OPT_CTOL]) status = BA_OK;
        } else {
            next = lambda * 10.0;
            if (next > opts[BA_OPT_LMAX]) status = BA_STALLED;
        }
        if (status == BA_RUNNING && iter + 1.0 >= opts[BA_OPT_MAX_ITER]) status = BA_MAX_ITER;
    }
    rec[BA_REC_COST1] = status == BA_EMPTY || status == BA_DEGENERATE ? cost0 : cost1;
    rec[BA_REC_ACCEPTED] = accepted ? 1.0 : 0.0;
    rec[BA_REC_STATUS] = (double)status;
    rec[BA_REC_ITER] = iter;
    st[BA_ST_LAMBDA] = next;
    if (accepted) st[BA_ST_PARITY] = 1.0 - st[BA_ST_PARITY];
    if (status != BA_RUNNING) { st[BA_ST_DONE] = 1.0; st[BA_ST_STATUS] = (double)status; }
    st[BA_ST_ITER] = iter + 1.0;
}

}  // namespace
}  // namespace im
