// Host build of the per-candidate and per-query arithmetic of csrc/ballfeat.hip (csrc/ball_point.h) for tests/test_ballfeat_cpu.py: the
// very text the kernel compiles, behind a stub <hip/hip_runtime.h>. No arithmetic is written here: every ball is found by brute force
// over the whole cloud with ball_candidate, accumulated in two halves that ball_merge joins (the kernel's lanes and its reduction in small),
// and finished by the header's functions.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ball_point.h"

extern "C" int ball_host_qmax(void) { return im::BALL_QMAX; }
extern "C" int ball_host_kinds(void) { return IM_BALL_KINDS; }
extern "C" int ball_host_quantise(double u, double radius) { return im::ball_quantise(u, radius * im::BALL_STEP); }

// the candidates of query q: inside [n] (0 / 1) and the quantised offsets [n][3] of those inside (0 for the others)
extern "C" void ball_host_offsets(const double* pts, long long n, long long q, double radius, int* inside, int* off) {
    const double h = radius * im::BALL_STEP, r2 = radius * radius;
    for (long long p = 0; p < n; ++p) {
        im::BallSums one;
        im::ball_zero(one);
        inside[p] = im::ball_candidate(one, pts[3 * p], pts[3 * p + 1], pts[3 * p + 2], pts[3 * q], pts[3 * q + 1], pts[3 * q + 2], r2, h) ? 1 : 0;
        for (int a = 0; a < 3; ++a) off[3 * p + a] = (int)one.s[1 + a];
    }
}

// every query of the cloud: sums [n][10], covariance [n][6], eig [n][3], e3 [n][3], feat [n][IM_BALL_KINDS]
extern "C" void ball_host_all(const double* pts, long long n, double radius, long long* sums, double* cov, double* eig, double* e3, double* feat) {
    const double h = radius * im::BALL_STEP, hh = h * h, r2 = radius * radius;
    for (long long q = 0; q < n; ++q) {
        im::BallSums even, odd;
        im::ball_zero(even);
        im::ball_zero(odd);
        for (long long p = 0; p < n; ++p)
            im::ball_candidate(p % 2 ? odd : even, pts[3 * p], pts[3 * p + 1], pts[3 * p + 2], pts[3 * q], pts[3 * q + 1], pts[3 * q + 2], r2, h);
        im::ball_merge(even, odd);
        for (int k = 0; k < im::BALL_SUMS; ++k) sums[q * im::BALL_SUMS + k] = even.s[k];
        double cv[6], ev[3], nv[3];
        im::ball_covariance(even, cv);
        im::ball_finish(even, hh, ev, nv);
        for (int k = 0; k < 6; ++k) cov[6 * q + k] = cv[k];
        for (int a = 0; a < 3; ++a) { eig[3 * q + a] = ev[a]; e3[3 * q + a] = nv[a]; }
        for (int k = 0; k < IM_BALL_KINDS; ++k) feat[q * IM_BALL_KINDS + k] = im::ball_feature(k, ev, nv, even.s[0]);
    }
}

// the half-width of every query's box of cells on the grid (origin x y z, cell size; dims)
extern "C" void ball_host_rings(const double* pts, long long n, const double* grid, const int* dims, double radius, int* rings) {
    im::KnnGrid g;
    for (int a = 0; a < 3; ++a) { g.o[a] = grid[a]; g.n[a] = dims[a]; }
    g.s = grid[3];
    for (long long q = 0; q < n; ++q) {
        double t[3];
        int c[3];
        for (int a = 0; a < 3; ++a) {
            t[a] = im::knn_cell_coord(pts[3 * q + a], g.o[a], g.s);
            c[a] = im::knn_cell_of(t[a], g.n[a]);
        }
        rings[q] = im::ball_rings(g, t, c, radius * radius);
    }
}
