// Host build of the per-point, per-group, per-span, per-cell and per-item arithmetic of csrc/dsm.hip (csrc/dsm_cell.h) for
// tests/test_dsm_cpu.py: the very text the kernels compile, behind a stub <hip/hip_runtime.h>. No arithmetic is written here: the loops
// below are flat loops over the arguments of the four entry points in host memory, in any order the kernels may take (every item is
// independent; a cell keeps the lowest triangle that claims it, as atomicMin does). The only bookkeeping is the prefix sum of a scan: a
// running sum of count().
#include <hip/hip_runtime.h>

#include <vector>

#include "dsm_cell.h"

extern "C" int dsm_host_win_none() { return im::WIN_NONE; }
extern "C" long long dsm_host_floor_index(float u) { return im::floor_index(u); }
extern "C" unsigned char dsm_host_to_u8(double v) { return im::to_u8(v); }

// im_dsm_round
extern "C" void dsm_host_round(const double* pts, long long n, float step, float* xr, float* yr, long long* xykey, long long* ykey,
                               long long* zkey) {
    for (long long i = 0; i < n; ++i) im::dsm_round_point(pts, i, step, xr, yr, xykey, ykey, zkey);
}

// im_dsm_group_mean: the number of groups; bx, by, bz [G] written
extern "C" long long dsm_host_group_mean(const double* pts, const float* xr, const float* yr, const long long* xykey, const long long* perm_b,
                                         const long long* perm_c, long long n, float* bx, float* by, float* bz) {
    int first[2] = {im::WIN_NONE, im::WIN_NONE};                 // the byte 0x7f of the entry point's memset
    for (long long j = n - 1; j >= 0; --j) {                     // descending: the lowest j is written last, as atomicMin leaves it
        if (im::dsm_zero_key(xr[perm_b[j]])) first[0] = (int)j;
        if (im::dsm_zero_key(yr[perm_b[j]])) first[1] = (int)j;
    }
    std::vector<long long> starts(n > 0 ? n : 1);
    long long G = 0;
    for (long long j = 0; j < n; ++j) {
        if (im::dsm_group_count(xykey, perm_c, n, j)) starts[G] = j;
        G += im::dsm_group_count(xykey, perm_c, n, j);
    }
    for (long long g = 0; g < G; ++g) im::dsm_group_mean(pts, xr, yr, perm_b, perm_c, first, starts.data(), G, n, g, bx, by, bz);
    return G;
}

// im_dsm_rasterize: z [ny][nx] written, win [ny][nx] the winning triangle of every cell (WIN_NONE: none); the number of spans
extern "C" long long dsm_host_rasterize(const float* bx, const float* by, const float* bz, const int* simplices, const double* transform,
                                        long long n_simplices, const double* bounds, const double* xq, int nx, const double* yq, int ny, double x0,
                                        double dx, double y0, double dy, double fill, double* z, int* win) {
    const im::TriGrid g{bx, by, simplices, transform, n_simplices, xq, yq, nx, ny, x0, dx, y0, dy};
    const long long cells = (long long)nx * ny;
    for (long long c = 0; c < cells; ++c) win[c] = im::WIN_NONE;
    long long spans = 0;
    for (long long t = 0; t < n_simplices; ++t) {
        int r0, r1;
        im::tri_rows(g, t, r0, r1);
        for (int r = r0; r <= r1; ++r)
            im::tri_span_cells(g, t, r, [&](long long cell) {
                if ((int)t < win[cell]) win[cell] = (int)t;
            });
        spans += im::tri_span_count(g, t);
    }
    for (long long c = 0; c < cells; ++c) z[c] = im::dsm_eval_cell(g, bz, win, bounds[0], bounds[1], bounds[2], bounds[3], fill, c);
    return spans;
}

// im_project_colors
extern "C" void dsm_host_project_colors(const double* x, long long sxr, long long sxc, const double* y, long long syr, long long syc, const double* z,
                                        long long szr, long long szc, int rows, int cols, int cells, const double* cam, const unsigned char* img,
                                        int h, int w, int cin, const int* chmap, int cout, float* proj, double* col, unsigned char* ortho) {
    im::ColorArgs a{x, sxr, sxc, y, syr, syc, z, szr, szc, rows, cols, cells, img, h, w, cin, cout, {0, 0, 0, 0}, proj, col, ortho};
    for (int ch = 0; ch < cout && chmap; ++ch) a.chmap[ch] = chmap[ch];
    im::CamParams p;
    p.fx = cam[0]; p.fy = cam[1]; p.cx = cam[2]; p.cy = cam[3];
    for (int k = 0; k < 9; ++k) p.R[k] = cam[4 + k];
    for (int k = 0; k < 3; ++k) p.t[k] = cam[13 + k];
    for (int k = 0; k < 12; ++k) p.k[k] = cam[16 + k];
    for (long long i = 0; i < (long long)rows * cols; ++i) im::proj_color_item(a, p, i);
}
