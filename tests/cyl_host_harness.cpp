// Host build of the per-candidate, per-query and per-core-point arithmetic of csrc/cloud_distance.hip (csrc/cyl_point.h) for
// tests/test_cloud_distance_cpu.py: the very text the kernels compile, behind a stub <hip/hip_runtime.h>. No arithmetic is written here:
// every cylinder is found by brute force over the whole cloud with cyl_candidate, accumulated in two halves that cyl_merge joins (the
// kernel's lanes and its reduction in small), and finished by the header's functions.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "cyl_point.h"

// the candidates of one cylinder: inside [n] (0 / 1), the projection t [n] and its quantised value it [n] (0 for the points outside)
extern "C" void cyl_host_inside(const double* pts, long long n, const double* c, const double* nrm, double rho, double L, int* inside, double* t,
                                int* it) {
    const double h = L * im::BALL_STEP, rho2 = rho * rho;
    for (long long p = 0; p < n; ++p) {
        im::CylSums one;
        im::cyl_zero(one);
        inside[p] = im::cyl_inside(pts[3 * p], pts[3 * p + 1], pts[3 * p + 2], c[0], c[1], c[2], nrm[0], nrm[1], nrm[2], rho2, L, t[p]) ? 1 : 0;
        im::cyl_candidate(one, pts[3 * p], pts[3 * p + 1], pts[3 * p + 2], c[0], c[1], c[2], nrm[0], nrm[1], nrm[2], rho2, L, h);
        it[p] = (int)one.s[1];
    }
}

// every query: count [m], sums [m][2], mean [m], std [m]; a query or normal with a non-finite component skips the cloud, as the kernel does
extern "C" void cyl_host_stats(const double* pts, long long n, const double* q, const double* nrm, long long m, double rho, double L, int* count,
                               long long* sums, double* mean, double* sd) {
    const double h = L * im::BALL_STEP, rho2 = rho * rho;
    for (long long i = 0; i < m; ++i) {
        im::CylSums even, odd;
        im::cyl_zero(even);
        im::cyl_zero(odd);
        bool finite = true;
        for (int a = 0; a < 3; ++a) finite = finite && std::isfinite(q[3 * i + a]) && std::isfinite(nrm[3 * i + a]);
        for (long long p = 0; finite && p < n; ++p)
            im::cyl_candidate(p % 2 ? odd : even, pts[3 * p], pts[3 * p + 1], pts[3 * p + 2], q[3 * i], q[3 * i + 1], q[3 * i + 2], nrm[3 * i],
                              nrm[3 * i + 1], nrm[3 * i + 2], rho2, L, h);
        im::cyl_merge(even, odd);
        count[i] = (int)even.s[0];
        sums[2 * i] = even.s[1];
        sums[2 * i + 1] = even.s[2];
        im::cyl_finish(even.s[0], even.s[1], even.s[2], h, mean[i], sd[i]);
    }
}

extern "C" void cyl_host_finish(const int* count1, const long long* sums1, const int* count2, const long long* sums2, long long m, double L,
                                double reg_error, int min_points, double* dist, double* lod, unsigned char* sig) {
    for (long long i = 0; i < m; ++i) {
        bool s;
        im::cyl_m3c2(count1[i], sums1[2 * i], sums1[2 * i + 1], count2[i], sums2[2 * i], sums2[2 * i + 1], L * im::BALL_STEP, reg_error, min_points,
                     dist[i], lod[i], s);
        sig[i] = s ? 1 : 0;
    }
}

extern "C" void cyl_host_extent(const double* nrm, double rho, double L, double* e) {
    double out[3];
    im::cyl_extent(nrm[0], nrm[1], nrm[2], rho, L, out);
    for (int a = 0; a < 3; ++a) e[a] = out[a];
}
