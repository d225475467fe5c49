// Host build of the per-point, per-voxel and per-corner arithmetic of csrc/voxel.hip (csrc/voxel_cell.h) for tests/test_voxel_cpu.py: the
// very text the kernels compile, behind a stub <hip/hip_runtime.h>. No arithmetic is written here: the loops below only visit the points,
// voxels and corners in the kernels' order (a stable sort by key, so a voxel's points come in ascending input index and a vertex's voxels
// in ascending voxel); sizes, kept flags, keys, indices, means, centres, corner keys and positions are the header's. Also the bytes the
// entry points ask their context for (csrc/stage_scratch.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "voxel_cell.h"
#include "stage_scratch.h"

extern "C" long long vox_host_max_cells() { return im::VOX_MAX_CELLS; }
extern "C" long long vox_host_max_points() { return im::VOX_MAX_POINTS; }
extern "C" long long vox_host_max_mesh_items() { return im::VOX_MAX_MESH_ITEMS; }
extern "C" long long vox_host_dropped_key() { return im::VOX_DROPPED; }

// n [3] and the number of voxels (corner keys when `corners`), or -1 for a grid that is refused
extern "C" long long vox_host_dims(const double* grid, long long* n, int corners) { return im::vox_grid_cells(grid, n, corners != 0); }

// key [n] and kept [n] of every point; returns the dropped points
extern "C" long long vox_host_keys(const double* pts, long long n, const double* grid, long long* key, unsigned char* kept) {
    long long dims[3], dropped = 0;
    if (im::vox_grid_cells(grid, dims) < 0) return -1;
    for (long long i = 0; i < n; ++i) {
        kept[i] = im::vox_kept(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], grid) ? 1 : 0;
        key[i] = im::vox_point_key(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], grid, dims);
        dropped += key[i] == im::VOX_DROPPED;
    }
    return dropped;
}

namespace {

std::vector<long long> stable_order(const long long* key, long long n) {
    std::vector<long long> perm(n);
    std::iota(perm.begin(), perm.end(), 0LL);
    std::stable_sort(perm.begin(), perm.end(), [&](long long a, long long b) { return key[a] < key[b]; });
    return perm;
}

}  // namespace

// the voxels of one cloud in ascending key; outputs sized for n rows, NULL attributes are skipped; returns V
extern "C" long long vox_host_voxels(const double* pts, const double* col, const double* nrm, long long n, const double* grid, const long long* key,
                                     int* grid_index, int* count, int* first, double* mean_pts, double* mean_col, double* mean_nrm, double* centre) {
    long long dims[3];
    if (im::vox_grid_cells(grid, dims) < 0) return -1;
    const std::vector<long long> perm = stable_order(key, n);
    long long V = 0;
    for (long long j0 = 0; j0 < n && key[perm[j0]] != im::VOX_DROPPED;) {
        long long j1 = j0;
        while (j1 < n && key[perm[j1]] == key[perm[j0]]) ++j1;
        im::vox_unkey(key[perm[j0]], dims[1], dims[2], grid_index + 3 * V);
        count[V] = (int)(j1 - j0);
        first[V] = (int)perm[j0];
        const auto rows = [&](const double* a) { return [&, a](long long k) { return a + 3 * perm[j0 + k]; }; };
        im::vox_mean3(rows(pts), j1 - j0, mean_pts + 3 * V);
        if (col) im::vox_mean3(rows(col), j1 - j0, mean_col + 3 * V);
        if (nrm) im::vox_mean3(rows(nrm), j1 - j0, mean_nrm + 3 * V);
        for (int a = 0; a < 3; ++a) centre[3 * V + a] = im::vox_centre(grid[a], grid_index[3 * V + a], grid[6]);
        ++V;
        j0 = j1;
    }
    return V;
}

// the box mesh of V voxels in ascending key: corner keys [8 V], vertices and colours (sized 8 V rows), triangles [12 V][3]; returns the vertices
extern "C" long long vox_host_mesh(const double* grid, const int* grid_index, long long V, const double* col, long long* corner_key, double* vertices,
                                   double* vcol, int* tri) {
    long long dims[3];
    if (im::vox_grid_cells(grid, dims, true) < 0) return -1;
    const long long items = 8 * V;
    for (long long t = 0; t < items; ++t) {
        const long long v = t >> 3;
        const int l = (int)(t & 7);
        corner_key[t] = im::vox_corner_key(grid_index[3 * v] + im::vox_corner_dx(l), grid_index[3 * v + 1] + im::vox_corner_dy(l),
                                           grid_index[3 * v + 2] + im::vox_corner_dz(l), dims[1], dims[2]);
    }
    const std::vector<long long> perm = stable_order(corner_key, items);
    std::vector<int> vertex(items);
    long long U = 0;
    for (long long j0 = 0; j0 < items;) {
        long long j1 = j0;
        while (j1 < items && corner_key[perm[j1]] == corner_key[perm[j0]]) ++j1;
        long long c[3];
        im::vox_corner_unkey(corner_key[perm[j0]], dims[1], dims[2], c);
        for (int a = 0; a < 3; ++a) vertices[3 * U + a] = im::vox_corner_pos(grid[a], c[a], grid[6]);
        if (col) im::vox_mean3([&](long long k) { return col + 3 * (perm[j0 + k] >> 3); }, j1 - j0, vcol + 3 * U);
        for (long long j = j0; j < j1; ++j) vertex[perm[j]] = (int)U;
        ++U;
        j0 = j1;
    }
    for (long long v = 0; v < V; ++v)
        for (int t = 0; t < 12; ++t)
            for (int k = 0; k < 3; ++k) tri[36 * v + 3 * t + k] = vertex[8 * v + im::vox_triangle(t, k)];
    return U;
}

extern "C" unsigned long long carve_voxel(long long E, long long G, long long n) { return im::VoxelScratch(E, G, n).bytes; }
extern "C" unsigned long long carve_voxel_mesh(long long items) { return im::VoxelMeshScratch(items).bytes; }
