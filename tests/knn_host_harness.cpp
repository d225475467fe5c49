// Host build of the per-candidate arithmetic of csrc/knn.hip (csrc/knn_point.h) for tests/test_pointcloud_cpu.py: the very text the
// kernels compile, behind a stub <hip/hip_runtime.h> that defines __device__ and __forceinline__ away. No arithmetic is written here:
// the search below only walks the rings of cells in the kernel's order (by comparing cells, without a sorted copy) and keeps the best-k
// list with knn_less; distances, cells, the bound and the stop rule are the header's.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <vector>

#include "knn_point.h"

namespace {

im::KnnGrid grid_of(const double* grid, const int* dims) {
    im::KnnGrid g;
    for (int a = 0; a < 3; ++a) { g.o[a] = grid[a]; g.n[a] = dims[a]; }
    g.s = grid[3];
    return g;
}

}  // namespace

// cell coordinates t [n][3], cells c [n][3] and keys [n] of every point
extern "C" void knn_host_cells(const double* pts, long long n, const double* grid, const int* dims, double* t, int* c, long long* key) {
    const im::KnnGrid g = grid_of(grid, dims);
    for (long long i = 0; i < n; ++i) {
        for (int a = 0; a < 3; ++a) {
            t[3 * i + a] = im::knn_cell_coord(pts[3 * i + a], g.o[a], g.s);
            c[3 * i + a] = im::knn_cell_of(t[3 * i + a], g.n[a]);
        }
        key[i] = im::knn_key(g, c[3 * i], c[3 * i + 1], c[3 * i + 2]);
    }
}

extern "C" double knn_host_d2(const double* p, const double* q) { return im::knn_d2(p[0], p[1], p[2], q[0], q[1], q[2]); }

// the bound after ring r and the three decisions that hang on it
extern "C" double knn_host_ring_bound2(const double* t, const int* c, int r, const double* grid, const int* dims) {
    const double tt[3] = {t[0], t[1], t[2]};
    const int cc[3] = {c[0], c[1], c[2]};
    return im::knn_ring_bound2(grid_of(grid, dims), tt, cc, r);
}
extern "C" int knn_host_done(const double* t, const int* c, int r, const double* grid, const int* dims, double kth_d2, double radius2) {
    const double tt[3] = {t[0], t[1], t[2]};
    const int cc[3] = {c[0], c[1], c[2]};
    return im::knn_done(grid_of(grid, dims), tt, cc, r, kth_d2, radius2) ? 1 : 0;
}

// mean [3], covariance sums [6] and the normal [3] of `count` neighbours nb [count][3] in the order given
extern "C" void knn_host_covariance(const double* nb, int count, double* mean, double* cov, double* normal) {
    auto get = [&](int j, double& x, double& y, double& z) { x = nb[3 * j]; y = nb[3 * j + 1]; z = nb[3 * j + 2]; };
    double m[3], cv[6], nr[3];
    im::knn_covariance(get, count, m, cv);
    im::knn_normal(get, count, nr);
    for (int a = 0; a < 3; ++a) { mean[a] = m[a]; normal[a] = nr[a]; }
    for (int a = 0; a < 6; ++a) cov[a] = cv[a];
}

// the arguments of im_knn_self in host memory, without the sorted copy: every ring is found by comparing cells
extern "C" void knn_host_self(const double* pts, long long n, const double* grid, const int* dims, int k, double radius2, int* count, int* idx,
                              double* d2, double* mean, int* rings) {
    const im::KnnGrid g = grid_of(grid, dims);
    std::vector<double> t(3 * n);
    std::vector<int> c(3 * n);
    std::vector<long long> key(n);
    knn_host_cells(pts, n, grid, dims, t.data(), c.data(), key.data());
    std::vector<double> bd(k);
    std::vector<int> bi(k);
    for (long long q = 0; q < n; ++q) {
        for (int j = 0; j < k; ++j) { bd[j] = im::knn_inf(); bi[j] = im::KNN_NONE; }
        const double tq[3] = {t[3 * q], t[3 * q + 1], t[3 * q + 2]};
        const int cq[3] = {c[3 * q], c[3 * q + 1], c[3 * q + 2]};
        int r = 0;
        for (;; ++r) {
            for (long long p = 0; p < n; ++p) {
                int ring = 0;
                for (int a = 0; a < 3; ++a) ring = std::max(ring, std::abs(c[3 * p + a] - cq[a]));
                if (ring != r) continue;
                const double d = im::knn_d2(pts[3 * q], pts[3 * q + 1], pts[3 * q + 2], pts[3 * p], pts[3 * p + 1], pts[3 * p + 2]);
                if (im::knn_outside(d, radius2) || !im::knn_less(d, (int)p, bd[k - 1], bi[k - 1])) continue;
                int pos = 0;
                while (im::knn_less(bd[pos], bi[pos], d, (int)p)) ++pos;
                for (int j = k - 1; j > pos; --j) { bd[j] = bd[j - 1]; bi[j] = bi[j - 1]; }
                bd[pos] = d; bi[pos] = (int)p;
            }
            if (im::knn_done(g, tq, cq, r, bd[k - 1], radius2)) break;
        }
        int cnt = 0;
        while (cnt < k && bi[cnt] != im::KNN_NONE) ++cnt;
        for (int j = 0; j < k; ++j) { idx[q * k + j] = j < cnt ? bi[j] : -1; d2[q * k + j] = j < cnt ? bd[j] : im::knn_inf(); }
        count[q] = cnt;
        mean[q] = im::knn_mean_distance([&](int j) { return bd[j]; }, cnt);
        rings[q] = r + 1;
    }
}
