// Host build of the per-point, per-cell and per-report arithmetic of csrc/dod.hip (csrc/dod_cell.h) for tests/test_dod_cpu.py: the very
// text the kernels compile, behind a stub <hip/hip_runtime.h>. No arithmetic is written here: the loops below only visit the points, cells
// and chunks in the kernels' order (a cell's points in ascending input index, a chunk's cells in ascending index, the chunks in ascending
// index); bounds, cells, means, H, the sums and the report are the header's. Also the bytes the entry points ask their context for
// (csrc/stage_scratch.h).
#include <hip/hip_runtime.h>

#include <vector>

#include "dod_cell.h"
#include "stage_scratch.h"

extern "C" int dod_host_chunk() { return im::DOD_CHUNK; }
extern "C" int dod_host_report_size() { return im::DOD_REPORT; }

// min_x, min_y, max_x, max_y of the kept points through the kernels' keys, and the dropped points
extern "C" long long dod_host_bounds(const double* pts, long long n, int d, double* out) {
    unsigned long long k[4] = {0, 0, 0, 0};
    long long dropped = 0;
    const int ax = im::dod_axis_x(d), ay = im::dod_axis_y(d);
    for (long long i = 0; i < n; ++i) {
        const double* c = pts + 3 * i;
        if (!im::dod_kept(c[0], c[1], c[2])) { ++dropped; continue; }
        const unsigned long long kx = im::dod_order_key(c[ax]), ky = im::dod_order_key(c[ay]);
        if (~kx > k[0]) k[0] = ~kx;
        if (~ky > k[1]) k[1] = ~ky;
        if (kx > k[2]) k[2] = kx;
        if (ky > k[3]) k[3] = ky;
    }
    for (int a = 0; a < 4; ++a) out[a] = k[a] ? im::dod_order_value(a < 2 ? ~k[a] : k[a]) : (a < 2 ? im::dod_inf() : -im::dod_inf());
    return dropped;
}

// grid [4] = min_x, min_y, w, h (as doubles) of the pair whose clouds have the bounds bg and bc
extern "C" void dod_host_grid(const double* bg, const double* bc, double s, double* grid) {
    im::dod_pair_grid(bg, bc, s, grid[0], grid[1], grid[2], grid[3]);
}

extern "C" void dod_host_cells(const double* pts, long long n, int d, const double* grid, double s, long long* cell) {
    const int ax = im::dod_axis_x(d), ay = im::dod_axis_y(d);
    for (long long i = 0; i < n; ++i) {
        const double* c = pts + 3 * i;
        cell[i] = im::dod_kept(c[0], c[1], c[2]) ? im::dod_cell_of(c[ax], c[ay], grid[0], grid[1], s, (long long)grid[2], (long long)grid[3]) : -1;
    }
}

namespace {

// count and mean (NaN where empty) per cell: the points of a cell in ascending input index
void means_of(const double* pts, long long n, int d, const long long* cell, long long cells, long long* count, double* mean) {
    std::vector<long long> start(cells + 1, 0), fill(cells, 0), order(n);
    for (long long i = 0; i < n; ++i)
        if (cell[i] >= 0) ++start[cell[i] + 1];
    for (long long c = 0; c < cells; ++c) start[c + 1] += start[c];
    for (long long i = 0; i < n; ++i)
        if (cell[i] >= 0) order[start[cell[i]] + fill[cell[i]]++] = i;
    for (long long c = 0; c < cells; ++c) {
        count[c] = start[c + 1] - start[c];
        const long long* seg = order.data() + start[c];
        mean[c] = count[c] ? im::dod_mean([&](long long k) { return pts[3 * seg[k] + d]; }, count[c]) : im::dod_nan();
    }
}

}  // namespace

// one pair: cells of every point, counts and means per cloud and cell, H [h][w], the report [16]
extern "C" void dod_host_pair(const double* ground, long long n0, const double* ceil, long long n1, int d, double s, const double* grid,
                              long long* cell_g, long long* cell_c, long long* count_g, long long* count_c, double* mean_g, double* mean_c, double* H,
                              double* report) {
    const long long w = (long long)grid[2], h = (long long)grid[3], cells = w * h;
    dod_host_cells(ground, n0, d, grid, s, cell_g);
    dod_host_cells(ceil, n1, d, grid, s, cell_c);
    means_of(ground, n0, d, cell_g, cells, count_g, mean_g);
    means_of(ceil, n1, d, cell_c, cells, count_c, mean_c);
    unsigned long long n[im::DOD_N_COUNTS] = {0, 0, 0, 0, 0};
    for (long long c = 0; c < cells; ++c) {
        H[c] = count_g[c] > 0 && count_c[c] > 0 ? im::dod_diff(mean_g[c], mean_c[c]) : im::dod_nan();
        n[im::DOD_N_FILLED] += count_g[c] > 0 || count_c[c] > 0;
        n[im::DOD_N_GROUND_ONLY] += count_g[c] > 0 && count_c[c] == 0;
        n[im::DOD_N_CEIL_ONLY] += count_c[c] > 0 && count_g[c] == 0;
    }
    for (long long c = 0; c < cells; ++c)
        if (im::dod_valid(H[c])) {
            ++n[im::DOD_N_VALID];
            n[im::DOD_N_NEIGHBOURS] += im::dod_neighbours([&](long long i, long long j) { return im::dod_valid(H[j * w + i]); }, c % w, c / w, w, h);
        }
    const long long chunks = im::blocks_of(cells, im::DOD_CHUNK);
    std::vector<double> parts(3 * chunks + 1);
    double sums[3];
    for (int which = 0; which < 3; ++which) {
        for (long long ch = 0; ch < chunks; ++ch) {
            const long long c0 = ch * im::DOD_CHUNK, m = cells - c0 < im::DOD_CHUNK ? cells - c0 : im::DOD_CHUNK;
            parts[3 * ch + which] = im::dod_chunk_sum([&](long long k) { return H[c0 + k]; }, m, which);
        }
        sums[which] = im::dod_partial_sum([&](long long k) { return parts[3 * k + which]; }, chunks);
    }
    im::dod_report(report, sums, n, s, w, h, grid[0], grid[1]);
}

extern "C" void dod_host_in_polygon(const double* poly, int nv, const double* x, const double* y, long long n, unsigned char* mask) {
    for (long long i = 0; i < n; ++i)
        mask[i] = im::dod_in_polygon([&](int k, double& vx, double& vy) { vx = poly[2 * k]; vy = poly[2 * k + 1]; }, nv, x[i], y[i]) ? 1 : 0;
}

extern "C" unsigned long long carve_dod(long long E, long long P, long long cells, long long chunks, int own_h) {
    return im::DodScratch(E, P, cells, chunks, own_h != 0).bytes;
}
extern "C" unsigned long long carve_crop_polygon(long long n) { return im::CropScratch(n).bytes; }
