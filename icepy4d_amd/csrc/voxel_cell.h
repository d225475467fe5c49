// The arithmetic of one point, one voxel and one mesh corner of csrc/voxel.hip: voxel grids, voxel down-sampling and voxel box meshes
// (Open3D's VoxelGrid.create_from_point_cloud_within_bounds / voxel_down_sample and the cube mesh of the reference's
// `scripts/pcd_postprocessing/voxelization.py`, restated in DESIGN §4). IEEE float64 with contraction off, a header of its own without
// the context or any launch code, like dod_cell.h: a host program compiles the very text the kernels compile
// (tests/voxel_host_harness.cpp, through a stub <hip/hip_runtime.h>) and is compared with the numpy restatement (tests/voxel_oracle.py)
// bit for bit. The host half of voxel.hip calls the same functions for the sizes of a grid, so the caps are decided by this text too.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// the host half of voxel.hip calls these too; a plain host compiler (the stub <hip/hip_runtime.h>) knows no __host__
#if defined(__HIP__) || defined(__HIPCC__)
#define VOX_FN __host__ __device__ __forceinline__
#else
#define VOX_FN inline
#endif

namespace im {
namespace {

constexpr int VOX_GRID = 7;                              // doubles of one grid: origin = min_bound [3], max_bound [3], voxel_size
constexpr long long VOX_MAX_CELLS = 1LL << 62;           // voxels of the grids of one call together; corner keys of one mesh
constexpr long long VOX_MAX_POINTS = 1LL << 26;          // points of one call
constexpr long long VOX_MAX_MESH_ITEMS = 1LL << 27;      // 8 V of one mesh
constexpr long long VOX_DROPPED = 0x7fffffffffffffffLL;  // the key of a point that is not kept: behind every voxel key in a signed sort

VOX_FN bool vox_finite(double v) { return __builtin_isfinite(v); }

// kept: every coordinate finite and min_a <= p_a <= max_a on every axis; g = one grid (VOX_GRID doubles)
VOX_FN bool vox_kept(double x, double y, double z, const double* g) {
    return vox_finite(x) && vox_finite(y) && vox_finite(z) && g[0] <= x && x <= g[3] && g[1] <= y && y <= g[4] && g[2] <= z && z <= g[5];
}
// floor((v - min) / s): a true division, not a multiplication by 1 / s
VOX_FN double vox_index(double v, double mn, double s) {
#pragma clang fp contract(off)
    return __builtin_floor((v - mn) / s);
}
// voxels along an axis, floor((max - min) / s) + 1, as a double: it may exceed any integer
VOX_FN double vox_dim(double mn, double mx, double s) {
#pragma clang fp contract(off)
    return vox_index(mx, mn, s) + 1.0;
}
// n = (n_x, n_y, n_z) of grid g and their product; -1 for a grid that is refused: a bound or s not finite, s <= 0, max < min, or more
// than VOX_MAX_CELLS voxels or (n_x + 1)(n_y + 1)(n_z + 1) > VOX_MAX_CELLS corner keys when `corners`
VOX_FN long long vox_grid_cells(const double* g, long long* n, bool corners = false) {
    for (int k = 0; k < VOX_GRID; ++k)
        if (!vox_finite(g[k])) return -1;
    if (!(g[6] > 0.0)) return -1;
    long long cells = 1;
    for (int a = 0; a < 3; ++a) {
        if (!(g[3 + a] >= g[a])) return -1;
        const double nd = vox_dim(g[a], g[3 + a], g[6]);
        if (!(nd >= 1.0 && nd <= (double)VOX_MAX_CELLS)) return -1;
        n[a] = (long long)nd;
        const long long m = n[a] + (corners ? 1 : 0);
        if (m > VOX_MAX_CELLS / cells) return -1;          // cells * m > 2^62
        cells *= m;
    }
    return cells;
}
VOX_FN long long vox_key(long long ix, long long iy, long long iz, long long ny, long long nz) { return (ix * ny + iy) * nz + iz; }
VOX_FN void vox_unkey(long long key, long long ny, long long nz, int32_t* idx) {
    idx[2] = (int32_t)(key % nz);
    const long long q = key / nz;
    idx[1] = (int32_t)(q % ny);
    idx[0] = (int32_t)(q / ny);
}
// the key of a point inside grid g of n = (n_x, n_y, n_z) voxels, or VOX_DROPPED
VOX_FN long long vox_point_key(double x, double y, double z, const double* g, const long long* n) {
    if (!vox_kept(x, y, z, g)) return VOX_DROPPED;
    return vox_key((long long)vox_index(x, g[0], g[6]), (long long)vox_index(y, g[1], g[6]), (long long)vox_index(z, g[2], g[6]), n[1], n[2]);
}

// the mean of a voxel: get(k) = the attribute of its k-th point in ascending input index, summed from +0.0
template <typename Get>
VOX_FN double vox_mean(Get get, long long count) {
#pragma clang fp contract(off)
    double sum = 0.0;
    for (long long k = 0; k < count; ++k) sum += get(k);
    return sum / (double)count;
}

// the same for the three columns of a row: row(k) = the k-th point's three values; every column is summed on its own, in the same order
template <typename Row>
VOX_FN void vox_mean3(Row row, long long count, double* mean) {
#pragma clang fp contract(off)
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (long long k = 0; k < count; ++k) {
        const double* r = row(k);
        s0 += r[0]; s1 += r[1]; s2 += r[2];
    }
    mean[0] = s0 / (double)count; mean[1] = s1 / (double)count; mean[2] = s2 / (double)count;
}

// origin + (i + 0.5) * s, evaluated as written
VOX_FN double vox_centre(double origin, long long i, double s) {
#pragma clang fp contract(off)
    return origin + ((double)i + 0.5) * s;
}

// ---- the box mesh: local corner l = 0..7 of a voxel sits at grid_index + d(l), Open3D's create_box order -----------------------------------
VOX_FN int vox_corner_dx(int l) { return l & 1; }
VOX_FN int vox_corner_dy(int l) { return (l >> 2) & 1; }
VOX_FN int vox_corner_dz(int l) { return (l >> 1) & 1; }
VOX_FN long long vox_corner_key(long long cx, long long cy, long long cz, long long ny, long long nz) { return (cx * (ny + 1) + cy) * (nz + 1) + cz; }
VOX_FN void vox_corner_unkey(long long key, long long ny, long long nz, long long* c) {
    c[2] = key % (nz + 1);
    const long long q = key / (nz + 1);
    c[1] = q % (ny + 1);
    c[0] = q / (ny + 1);
}
// origin + c * s
VOX_FN double vox_corner_pos(double origin, long long c, double s) {
#pragma clang fp contract(off)
    return origin + (double)c * s;
}
// the 12 outward-facing triangles of a cube in local corner numbers
VOX_FN int vox_triangle(int t, int k) {
    constexpr int T[12][3] = {{4, 7, 5}, {4, 6, 7}, {0, 2, 4}, {2, 6, 4}, {0, 1, 2}, {1, 3, 2}, {1, 5, 7}, {1, 7, 3}, {2, 3, 7}, {2, 7, 6}, {0, 4, 1}, {1, 4, 5}};
    return T[t][k];
}

}  // namespace
}  // namespace im
