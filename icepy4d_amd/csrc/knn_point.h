// The arithmetic of one candidate and one query of csrc/knn.hip: the grid cell of a point, the squared distance, the order among
// candidates, the bound that ends the ring search, and the covariance of a neighbourhood with the eigenvector of its smallest eigenvalue.
// IEEE float64 with contraction off, a header of its own without the context or any launch code, like sfm_point.h and warp_pixel.h: a
// host program compiles the very text the kernels compile (tests/knn_host_harness.cpp, through a stub <hip/hip_runtime.h>) and is
// compared with the numpy restatement (tests/knn_oracle.py) bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

namespace im {
namespace {

// the uniform grid: origin = the cloud's minimum corner, cubic cells of side s, n[a] >= 1 cells per axis
struct KnnGrid { double o[3]; double s; int n[3]; };

constexpr double KNN_MARGIN = 9.094947017729282e-13;     // 2^-40
constexpr double KNN_EPS = 2.220446049250313e-16;        // DBL_EPSILON
constexpr int KNN_MAX_SWEEPS = 30;
constexpr int KNN_NONE = INT_MAX;                         // index of an empty slot of the best-k list (its d2 is +inf)

__device__ __forceinline__ double knn_inf() { return __builtin_huge_val(); }

// the coordinate of p in cells: a monotone function of p (a rounded subtraction and a rounded division by s > 0), and so is the cell
__device__ __forceinline__ double knn_cell_coord(double p, double o, double s) {
#pragma clang fp contract(off)
    return (p - o) / s;
}

// min(n - 1, floor(t)); a point below the origin or a NaN (neither occurs for a grid made from the cloud) lands in cell 0, so that a key
// always addresses the grid
__device__ __forceinline__ int knn_cell_of(double t, int n) {
    const double f = floor(t);
    if (!(f > 0.0)) return 0;
    if (f >= (double)(n - 1)) return n - 1;
    return (int)f;
}

__device__ __forceinline__ long long knn_key(const KnnGrid& g, int ix, int iy, int iz) {
    return ((long long)iz * g.n[1] + iy) * g.n[0] + ix;
}

__device__ __forceinline__ double knn_d2(double px, double py, double pz, double qx, double qy, double qz) {
#pragma clang fp contract(off)
    const double dx = px - qx, dy = py - qy, dz = pz - qz;
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

// the order of the best-k list: ascending d2, the lower original index first among equal distances
__device__ __forceinline__ bool knn_less(double d2a, int ia, double d2b, int ib) { return d2a < d2b || (d2a == d2b && ia < ib); }

// Hybrid search: a neighbour is dropped iff d2 > radius2 (radius2 = +inf: never)
__device__ __forceinline__ bool knn_outside(double d2, double radius2) { return d2 > radius2; }

// the box of cells [c - r, c + r] holds every cell of the grid
__device__ __forceinline__ bool knn_covers(const KnnGrid& g, const int (&c)[3], int r) {
    bool all = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) all = all && c[a] - r <= 0 && c[a] + r >= g.n[a] - 1;
    return all;
}

// One face of the box: `gap` = distance of the query to the face in cells. Returns a lower bound, squared, of the computed d2 of every
// point in a cell beyond that face.
// The choice made here: the gap is shrunk by 2^-40 n[a] cells AND by a relative 2^-40, and a gap that is then not positive gives the
// bound 0, which never ends a search ("continue"). Why a relative margin alone would not do: a point is assigned by its rounded cell
// coordinate t = fl(fl(p - o) / s), whose error is up to 2^-52 t <= 2^-52 n[a] cells, however close to the face the query sits. Why this
// suffices: the cell is monotone in p, so a point in a cell below L = c - r has t_p < L <= t_q, and the true distance along the axis is
// at least s ((t_q - t_p) - 2^-51 n[a]) > s ((t_q - L) - 2^-40 n[a]); the relative 2^-40 covers the rounding of the gap, of the product
// with s, of its square and the 2^-51 relative error of a computed d2 with room to spare. Cost: a query within 2^-40 n[a] cells of a face
// (at most 2^-16 of a cell at the cap of 2^24 cells) visits one more ring than it had to.
__device__ __forceinline__ double knn_face_bound2(double gap, double n_axis, double s) {
#pragma clang fp contract(off)
    const double g = (gap - KNN_MARGIN * n_axis) * (1.0 - KNN_MARGIN);
    if (!(g > 0.0)) return 0.0;
    const double d = g * s;
    return d * d;
}

// After ring r every unvisited point lies outside the box [c - r, c + r]: the smallest face bound over the faces that still have cells
// beyond them (faces at the grid's edge do not count); +inf when there is none. t = the query's cell coordinates.
__device__ __forceinline__ double knn_ring_bound2(const KnnGrid& g, const double (&t)[3], const int (&c)[3], int r) {
#pragma clang fp contract(off)
    double best = knn_inf();
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double na = (double)g.n[a];
        if (c[a] - r > 0) {
            const double b = knn_face_bound2(t[a] - (double)(c[a] - r), na, g.s);
            best = b < best ? b : best;
        }
        if (c[a] + r < g.n[a] - 1) {
            const double b = knn_face_bound2((double)(c[a] + r + 1) - t[a], na, g.s);
            best = b < best ? b : best;
        }
    }
    return best;
}

// whether the search may end after ring r; kth_d2 = +inf while fewer than k neighbours are held. Strict: an unvisited point at exactly
// the k-th distance may carry a lower index.
__device__ __forceinline__ bool knn_done(const KnnGrid& g, const double (&t)[3], const int (&c)[3], int r, double kth_d2, double radius2) {
    if (knn_covers(g, c, r)) return true;
    const double b2 = knn_ring_bound2(g, t, c, r);
    return kth_d2 < b2 || b2 > radius2;
}

// one Jacobi rotation of the symmetric 3 x 3 matrix a that zeroes a[P][Q] (P < Q, R the third index); v collects the rotations
template <int P, int Q, int R>
__device__ __forceinline__ bool knn_rotate(double (&a)[3][3], double (&v)[3][3]) {
#pragma clang fp contract(off)
    const double apq = a[P][Q], app = a[P][P], aqq = a[Q][Q];
    const double small = fabs(app) < fabs(aqq) ? fabs(app) : fabs(aqq);
    if (!(fabs(apq) > (0.125 * KNN_EPS) * small)) return false;       // also a NaN: nothing to rotate
    const double theta = (aqq - app) / (2.0 * apq);
    const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(1.0 + theta * theta));
    const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = cs * tt;
    a[P][P] = app - tt * apq;
    a[Q][Q] = aqq + tt * apq;
    a[P][Q] = a[Q][P] = 0.0;
    const double arp = a[R][P], arq = a[R][Q];
    a[R][P] = a[P][R] = cs * arp - sn * arq;
    a[R][Q] = a[Q][R] = sn * arp + cs * arq;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double x = v[k][P], y = v[k][Q];
        v[k][P] = cs * x - sn * y;
        v[k][Q] = sn * x + cs * y;
    }
    return true;
}

// unit eigenvector of the smallest eigenvalue of the symmetric matrix (xx xy xz; xy yy yz; xz yz zz) by cyclic Jacobi, with the sign that
// makes the first non-zero component of (n_z, n_y, n_x) positive
__device__ __forceinline__ void knn_smallest_eigenvector(const double (&cov)[6], double (&nrm)[3]) {
#pragma clang fp contract(off)
    double a[3][3] = {{cov[0], cov[1], cov[2]}, {cov[1], cov[3], cov[4]}, {cov[2], cov[4], cov[5]}};
    double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < KNN_MAX_SWEEPS; ++sweep) {
        const bool r01 = knn_rotate<0, 1, 2>(a, v);
        const bool r02 = knn_rotate<0, 2, 1>(a, v);
        const bool r12 = knn_rotate<1, 2, 0>(a, v);
        if (!(r01 || r02 || r12)) break;
    }
    const double l0 = a[0][0], l1 = a[1][1], l2 = a[2][2];
    double x, y, z;
    if (l0 <= l1 && l0 <= l2) { x = v[0][0]; y = v[1][0]; z = v[2][0]; }
    else if (l1 <= l2) { x = v[0][1]; y = v[1][1]; z = v[2][1]; }
    else { x = v[0][2]; y = v[1][2]; z = v[2][2]; }
    const double len = sqrt(((x * x) + (y * y)) + (z * z));
    if (!(len > 0.0)) { nrm[0] = 0.0; nrm[1] = 0.0; nrm[2] = 1.0; return; }
    x = x / len; y = y / len; z = z / len;
    const bool flip = z != 0.0 ? z < 0.0 : (y != 0.0 ? y < 0.0 : x < 0.0);
    nrm[0] = flip ? -x : x; nrm[1] = flip ? -y : y; nrm[2] = flip ? -z : z;
}

// Mean (3) and covariance (xx xy xz yy yz zz) of `count` neighbours in the order get(j, x, y, z) hands them out (ascending distance), by
// the plain two-pass formula: the sums start from 0.0, run left to right and are divided by (double)count.
template <typename Get>
__device__ __forceinline__ void knn_covariance(Get get, int count, double (&mean)[3], double (&cov)[6]) {
#pragma clang fp contract(off)
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int j = 0; j < count; ++j) {
        double x, y, z;
        get(j, x, y, z);
        sx = sx + x; sy = sy + y; sz = sz + z;
    }
    const double cnt = (double)count;
    mean[0] = sx / cnt; mean[1] = sy / cnt; mean[2] = sz / cnt;
    double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
    for (int j = 0; j < count; ++j) {
        double x, y, z;
        get(j, x, y, z);
        const double dx = x - mean[0], dy = y - mean[1], dz = z - mean[2];
        xx = xx + dx * dx; xy = xy + dx * dy; xz = xz + dx * dz;
        yy = yy + dy * dy; yz = yz + dy * dz; zz = zz + dz * dz;
    }
    cov[0] = xx / cnt; cov[1] = xy / cnt; cov[2] = xz / cnt; cov[3] = yy / cnt; cov[4] = yz / cnt; cov[5] = zz / cnt;
}

// the normal of a neighbourhood: fewer than three neighbours give (0, 0, 1)
template <typename Get>
__device__ __forceinline__ void knn_normal(Get get, int count, double (&nrm)[3]) {
    if (count < 3) { nrm[0] = 0.0; nrm[1] = 0.0; nrm[2] = 1.0; return; }
    double mean[3], cov[6];
    knn_covariance(get, count, mean, cov);
    knn_smallest_eigenvector(cov, nrm);
}

// SOR's statistic: the sum of sqrt(d2_j) in ascending order from 0.0, divided by (double)count; -1.0 for an empty neighbourhood
template <typename GetD2>
__device__ __forceinline__ double knn_mean_distance(GetD2 get, int count) {
#pragma clang fp contract(off)
    if (count == 0) return -1.0;
    double sum = 0.0;
    for (int j = 0; j < count; ++j) sum = sum + sqrt(get(j));
    return sum / (double)count;
}

}  // namespace
}  // namespace im
