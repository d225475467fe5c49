// The best-k list of one wave and the ring search that fills it, shared by knn.hip (every point of a cloud about its own cloud) and
// cloud_distance.hip (external queries about a cloud): one text, so both searches select, order and stop alike.
// The list lives one slot per lane (k <= 64), ascending; a batch of 64 candidates is filtered against the k-th entry with one ballot and
// the survivors are inserted one by one by rank counting (ballot + popcount, a shift by one lane): no per-thread array, no LDS, no barrier.
#pragma once
#include "knn_sorted.h"

namespace im {
namespace {

// what a search reads: the grid, the cloud in cell order, the cell ranges, and what it selects
struct KnnSearch {
    KnnGrid g;
    KnnSorted s;
    const int* start;       // [cells + 1]
    int n, k;
    double radius2;
};

// The best-k list of one wave: slot `lane` holds (d2, idx), ascending by knn_less; empty slots and the slots from k on hold (+inf,
// KNN_NONE). (thr_d2, thr_idx) is slot k - 1, the same in every lane.
struct KnnList {
    double d2; int idx;
    double thr_d2; int thr_idx;
};

// the candidates at sorted positions [b, e) against the list
__device__ __forceinline__ void knn_scan(const KnnSearch& a, KnnList& L, int lane, double qx, double qy, double qz, int b, int e) {
    for (long long base = b; base < e; base += IM_WAVE) {
        const long long j = base + lane;
        double cd2 = knn_inf();
        int ci = KNN_NONE;
        if (j < e) {
            cd2 = knn_d2(qx, qy, qz, a.s.x[j], a.s.y[j], a.s.z[j]);
            ci = a.s.idx[j];
        }
        const bool ok = j < e && !knn_outside(cd2, a.radius2) && knn_less(cd2, ci, L.thr_d2, L.thr_idx);
        unsigned long long m = __ballot(ok);
        while (m) {
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            const double d = __shfl(cd2, src);
            const int i = __shfl(ci, src);
            if (!knn_less(d, i, L.thr_d2, L.thr_idx)) continue;      // the list has moved on since the ballot
            const int pos = __popcll(__ballot(knn_less(L.d2, L.idx, d, i)));      // the entries before the candidate are a prefix
            const double ud2 = __shfl_up(L.d2, 1);
            const int uidx = __shfl_up(L.idx, 1);
            if (lane == pos) { L.d2 = d; L.idx = i; }
            else if (lane > pos && lane < a.k) { L.d2 = ud2; L.idx = uidx; }
            L.thr_d2 = __shfl(L.d2, a.k - 1);
            L.thr_idx = __shfl(L.idx, a.k - 1);
        }
    }
}

// One strip of a shell: the rows (iy, iz) with iy in ya..yb and iz in za..zb, of each the cells xa..xb (one contiguous range of the
// sorted cloud). 64 rows per step, one per lane: every lane looks its range up, a ballot keeps the ranges that hold points, and those are
// scanned one after the other. An empty strip (ya > yb or za > zb) costs nothing. Returns the steps taken, the measure of the search's work.
__device__ __forceinline__ int knn_strip(const KnnSearch& a, KnnList& L, int lane, double qx, double qy, double qz, int xa, int xb, int ya, int yb,
                                         int za, int zb) {
    if (ya > yb || za > zb) return 0;
    const int wy = yb - ya + 1, rows = wy * (zb - za + 1);              // <= 2^24
    int steps = 0;
    for (int base = 0; base < rows; base += IM_WAVE) {
        const int row = base + lane;
        int b = 0, e = 0;
        if (row < rows) knn_row_range(a.g, a.start, a.n, xa, xb, ya + row % wy, za + row / wy, b, e);
        unsigned long long m = __ballot(e > b);
        ++steps;
        while (m) {
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int sb = __shfl(b, src), se = __shfl(e, src);
            knn_scan(a, L, lane, qx, qy, qz, sb, se);
            steps += (se - sb + IM_WAVE - 1) / IM_WAVE;
        }
    }
    return steps;
}

// The whole search of one query (qx, qy, qz) with cell coordinates t and cell c: the cell, then the shells of cells at Chebyshev ring 1,
// 2, ... until knn_done. Returns the rings visited, the query's cell counted; negated where the rings had cost more than knn_step_budget
// and the search ended by one scan of the whole cloud. L must come in empty.
// A query outside the grid (cloud_distance.hip) has its cell clamped while t keeps the real coordinate; knn_face_bound2's margin covers
// it: only the faces on the grid's side of the query count, their gap is at least |t| - n[a] on that axis, the rounding of t is
// at most 2^-51 |t| <= 2^-51 (gap + n[a]), and the relative 2^-40 and the absolute 2^-40 n[a] of the margin take one part each.
__device__ __forceinline__ int knn_ring_search(const KnnSearch& a, KnnList& L, int lane, double qx, double qy, double qz, const double (&t)[3],
                                               const int (&c)[3]) {
    const int nx = a.g.n[0], ny = a.g.n[1], nz = a.g.n[2];
    const long long budget = knn_step_budget(a.n);
    long long steps = knn_strip(a, L, lane, qx, qy, qz, c[0], c[0], c[1], c[1], c[2], c[2]);      // ring 0: the query's cell
    int rings = 1;
    for (int r = 1; !knn_done(a.g, t, c, r - 1, L.thr_d2, a.radius2); ++r) {
        if (steps > budget) {
            // the rings have cost more than the whole cloud would: start again and scan it all, which needs no stop rule
            L = KnnList{knn_inf(), KNN_NONE, knn_inf(), KNN_NONE};
            knn_scan(a, L, lane, qx, qy, qz, 0, a.n);
            rings = -rings;
            break;
        }
        // The shell of ring r, clipped to the grid, as six strips that share no cell: the two z faces over the whole box in x and y,
        // the two y faces between them, the two x faces between those. Only faces inside the grid are walked, so a grid that is
        // thin along an axis pays nothing for the faces it does not have.
        const int x0 = max(0, c[0] - r), x1 = min(nx - 1, c[0] + r);
        const int y0 = max(0, c[1] - r), y1 = min(ny - 1, c[1] + r);
        const int yi0 = max(0, c[1] - r + 1), yi1 = min(ny - 1, c[1] + r - 1);
        const int zi0 = max(0, c[2] - r + 1), zi1 = min(nz - 1, c[2] + r - 1);
        if (c[2] - r >= 0) steps += knn_strip(a, L, lane, qx, qy, qz, x0, x1, y0, y1, c[2] - r, c[2] - r);
        if (c[2] + r <= nz - 1) steps += knn_strip(a, L, lane, qx, qy, qz, x0, x1, y0, y1, c[2] + r, c[2] + r);
        if (c[1] - r >= 0) steps += knn_strip(a, L, lane, qx, qy, qz, x0, x1, c[1] - r, c[1] - r, zi0, zi1);
        if (c[1] + r <= ny - 1) steps += knn_strip(a, L, lane, qx, qy, qz, x0, x1, c[1] + r, c[1] + r, zi0, zi1);
        if (c[0] - r >= 0) steps += knn_strip(a, L, lane, qx, qy, qz, c[0] - r, c[0] - r, yi0, yi1, zi0, zi1);
        if (c[0] + r <= nx - 1) steps += knn_strip(a, L, lane, qx, qy, qz, c[0] + r, c[0] + r, yi0, yi1, zi0, zi1);
        rings = r + 1;
    }
    return rings;
}

// The rows of the box of cells x0..x1, y0..y1, z0..z1 (inside the grid), each one contiguous range of the sorted cloud, for the kernels
// that accumulate over a region instead of selecting: 64 rows looked up per step, the ranges that hold points handed to scan(b, e) one
// after the other. A box whose lookups alone exceed knn_step_budget is given up for scan(0, n) before it starts. Returns the steps taken,
// negated (-ceil(n / 64)) after the whole-cloud scan.
template <typename Scan>
__device__ __forceinline__ int knn_box_walk(const KnnGrid& g, const int* __restrict__ start, int n, int lane, int x0, int x1, int y0, int y1, int z0,
                                            int z1, Scan scan) {
    const int wy = y1 - y0 + 1, rows = wy * (z1 - z0 + 1);            // <= ny * nz <= 2^24
    if ((rows + IM_WAVE - 1) / IM_WAVE > knn_step_budget(n)) {
        // looking the rows up would cost more than reading the whole cloud: a tiny cell size, or a grid stretched by a far outlier
        scan(0, n);
        return -((n + IM_WAVE - 1) / IM_WAVE);
    }
    int steps = 0;
    for (int base = 0; base < rows; base += IM_WAVE) {
        const int row = base + lane;
        int b = 0, e = 0;
        if (row < rows) knn_row_range(g, start, n, x0, x1, y0 + row % wy, z0 + row / wy, b, e);
        unsigned long long m = __ballot(e > b);
        ++steps;
        while (m) {
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int sb = __shfl(b, src), se = __shfl(e, src);
            scan(sb, se);
            steps += (se - sb + IM_WAVE - 1) / IM_WAVE;
        }
    }
    return steps;
}

}  // namespace
}  // namespace im
