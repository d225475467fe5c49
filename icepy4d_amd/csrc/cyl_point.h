// The arithmetic of one candidate, one query and one core point of csrc/cloud_distance.hip: the statistics of a cloud inside a cylinder
// along a normal, and M3C2's distance with its level of detection (Lague et al. 2013, restated with a definition of its own).
// Launch-free like ball_point.h, which it builds on: tests/cyl_host_harness.cpp compiles this very text for the host and
// tests/cloud_distance_oracle.py restates it in numpy with Python integers, bit for bit.
// A candidate p against the centre c, the normal nrm (used as given, never renormalised), the radius rho and the half-length L:
// u = fl(p - c) per axis, t = ((ux*nx) + (uy*ny)) + (uz*nz), d2 = ((ux*ux) + (uy*uy)) + (uz*uz), rad2 = d2 - t*t; inside iff
// |t| <= L and rad2 <= fl(rho * rho): cap and wall belong to the cylinder, and a NaN anywhere makes a comparison false. An inside candidate
// adds the integer it = rint(t / h), h = L * 2^-18 (|it| <= 2^18, clamped to 2^18 + 1 all the same), to three int64 sums: count, St, Stt.
// Stt stays below 2^36 * 2^26 = 2^62 for a cloud of at most 2^26 points: every sum is exact, a function of the input alone.
#pragma once
#include "ball_point.h"

namespace im {
namespace {

constexpr int CYL_SUMS = 3;            // count, St, Stt
constexpr double CYL_PAD = 1.0 + 0x1p-18;       // the box of a cylinder: relative margin of every half-extent
constexpr double CYL_SLACK = 0x1p-18;           // ... what a normal of squared length within CYL_UNIT of 1 may add to the wall, in L^2 and in n_a^2
constexpr double CYL_UNIT = 0x1p-21;
constexpr double CYL_Z = 1.96;                  // the 95 % quantile M3C2's level of detection uses

struct CylSums { long long s[CYL_SUMS]; };

__device__ __forceinline__ void cyl_zero(CylSums& S) { S.s[0] = 0; S.s[1] = 0; S.s[2] = 0; }

__device__ __forceinline__ void cyl_merge(CylSums& a, const CylSums& b) { a.s[0] += b.s[0]; a.s[1] += b.s[1]; a.s[2] += b.s[2]; }

// the projection t of the candidate on the normal and whether it lies in the cylinder
__device__ __forceinline__ bool cyl_inside(double px, double py, double pz, double cx, double cy, double cz, double nx, double ny, double nz,
                                           double rho2, double L, double& t) {
#pragma clang fp contract(off)
    const double ux = px - cx, uy = py - cy, uz = pz - cz;
    t = ((ux * nx) + (uy * ny)) + (uz * nz);
    const double d2 = ((ux * ux) + (uy * uy)) + (uz * uz);
    const double rad2 = d2 - t * t;
    return fabs(t) <= L && rad2 <= rho2;
}

// the candidate p against the query: added to the sums iff it lies in the cylinder
__device__ __forceinline__ bool cyl_candidate(CylSums& S, double px, double py, double pz, double cx, double cy, double cz, double nx, double ny,
                                              double nz, double rho2, double L, double h) {
    double t;
    if (!cyl_inside(px, py, pz, cx, cy, cz, nx, ny, nz, rho2, L, t)) return false;
    const int it = ball_quantise(t, h);
    S.s[0] += 1;
    S.s[1] += it;
    S.s[2] += (long long)it * it;
    return true;
}

// mean and sample standard deviation of the projections, in metres; int64 -> float64 is the correctly rounded conversion
__device__ __forceinline__ void cyl_finish(long long count, long long St, long long Stt, double h, double& mean, double& std) {
#pragma clang fp contract(off)
    const double cnt = (double)count;
    const double m = (double)St / cnt;
    mean = count < 1 ? ball_nan() : m * h;
    double v = (double)Stt / cnt - m * m;
    v = v < 0.0 ? 0.0 : v;
    std = count < 2 ? ball_nan() : sqrt(v * (cnt / (cnt - 1.0))) * h;
}

// M3C2 of one core point from the sums of its two cylinders: the distance, the level of detection and whether the change is significant
__device__ __forceinline__ void cyl_m3c2(long long cnt1, long long St1, long long Stt1, long long cnt2, long long St2, long long Stt2, double h,
                                         double reg_error, int min_points, double& dist, double& lod, bool& sig) {
#pragma clang fp contract(off)
    double mean1, std1, mean2, std2;
    cyl_finish(cnt1, St1, Stt1, h, mean1, std1);
    cyl_finish(cnt2, St2, Stt2, h, mean2, std2);
    dist = mean2 - mean1;
    const double var = (std1 * std1) / (double)cnt1 + (std2 * std2) / (double)cnt2;
    lod = (cnt1 < min_points || cnt2 < min_points) ? ball_nan() : CYL_Z * (sqrt(var) + reg_error);
    sig = fabs(dist) > lod;
}

// Half-extents e[a] of an axis-aligned box around the centre that holds every inside candidate. For a unit normal the cylinder's own box
// is L |n_a| + rho sqrt(1 - n_a^2). The normal is used as given, so the bound has to hold for whatever comes in:
//  - any normal: d2 = rad2 + t*t <= rho^2 + L^2, so the ball of radius sqrt(L^2 + rho^2) always holds the region (a zero normal makes
//    t = 0 and rad2 = d2: the ball of radius rho);
//  - |n|^2 = 1 + d with |d| <= CYL_UNIT: along the unit direction the region reaches L / |n| <= L (1 + 2^-21), across it
//    sqrt(rho^2 + |d| L^2), and the unit direction's n_a^2 differs from the given one by at most 2^-20: the wall becomes
//    sqrt(rho^2 + 2^-18 L^2) and the sine sqrt(max(0, 1 - n_a^2) + 2^-18), which also covers the cancellation in rad2 (2^-52 L^2).
// CYL_PAD covers the rounding of these few operations, of u = fl(p - c) and of the test itself (2^-50 relative). A non-finite value gives
// +inf or NaN, which knn_cell_of turns into the grid's edge: the box then covers the grid along that axis.
__device__ __forceinline__ void cyl_extent(double nx, double ny, double nz, double rho, double L, double (&e)[3]) {
#pragma clang fp contract(off)
    const double n[3] = {nx, ny, nz};
    const double s = ((nx * nx) + (ny * ny)) + (nz * nz);
    const double ball = (s == 0.0 ? rho : sqrt(L * L + rho * rho)) * CYL_PAD;
    const bool unit = fabs(s - 1.0) <= CYL_UNIT;
    const double wall = sqrt(rho * rho + CYL_SLACK * (L * L));
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double c2 = 1.0 - n[a] * n[a];
        const double f = (L * fabs(n[a]) + wall * sqrt((c2 > 0.0 ? c2 : 0.0) + CYL_SLACK)) * CYL_PAD;
        e[a] = unit && f < ball ? f : ball;
    }
}

}  // namespace
}  // namespace im
