// Voxel grids, voxel down-sampling and voxel box meshes on the device: Open3D's `VoxelGrid.create_from_point_cloud_within_bounds`,
// `create_from_point_cloud` and `voxel_down_sample`, and the cube mesh the reference's `scripts/pcd_postprocessing/voxelization.py` builds
// one voxel at a time. Open3D is an un-vendored dependency: the algorithm has a definition of its own and is pinned bit for bit
// against tests/voxel_oracle.py. The key space is sparse (the script's box holds 195 M voxels, a surface cloud fills well under 1 % of
// them), so nothing here is sized by the grid: a voxel is a run of equal keys in the sorted key list. One call serves E clouds that sit
// in one buffer, all under one grid or each under its own.
//
//   vox_bounds_kernel     per cloud the minimum and maximum of the finite points along the three axes: wave reductions, then atomicMax on
//                         order-preserving integer keys (dod_cell.h; exact, order-free)
//   vox_keys_kernel       one thread per point: first key of its cloud + (i_x n_y + i_y) n_z + i_z (voxel_cell.h), or VOX_DROPPED; the
//                         dropped points per cloud by one ballot and one atomic per wave. The stable sort by key between this and the rest is
//                         torch's, plumbing: every voxel becomes a contiguous segment in input order
//   scan_*_kernel         (scan.h) over the head flags: the voxel numbers, the first sorted position of every voxel, the number of voxels
//   vox_voxels_kernel     one thread per voxel: grid index, count, first input index, and the means of the point, colour and normal columns
//                         summed in segment order = ascending input index
//   vox_nvox_kernel       one thread per cloud: its first voxel, by bisection over the voxels' keys
//   vox_corners_kernel    one thread per (voxel, local corner): the corner key; sorted by torch (stable) like the voxel keys
//   scan_*_kernel         over the corner heads: vertex numbers, scattered back to (voxel, local corner) through the permutation
//   vox_vertices_kernel   one thread per vertex: position, and the colour mean over its at most 8 voxels in ascending voxel order
//   vox_triangles_kernel  one thread per voxel: its 12 triangles
// float64 throughout, contraction off in voxel_cell.h. No launch geometry and no property of the device enters a result.
#include <cmath>
#include <vector>

#include "common.h"
#include "ctx.h"
#include "stage_scratch.h"
#include "dod_cell.h"
#include "voxel_cell.h"

namespace im {
namespace {

#include "scan.h"

constexpr int VOX_MAX_CLOUDS = 65535;         // clouds of one call
constexpr int VOX_BOUNDS_BLOCKS = 256;        // blocks per cloud of vox_bounds_kernel at the most, of 1024 points or more each

// the tables of a call in device memory (VoxelScratch::table, ::grids)
struct VoxTab {
    const long long* offsets;     // [E + 1] first point of every cloud
    const long long* kbase;       // [E + 1] first key of every cloud; [E] = the number of keys
    const long long* dims;        // [G][3] n_x, n_y, n_z
    const double* grids;          // [G][7]
    int E, per_cloud;
};

// the last k in 0..n-1 with base[k] <= v (base ascending); 0 when there is none
__device__ __forceinline__ int vox_last_at_or_below(const long long* __restrict__ base, int n, long long v) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (base[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ long long vox_clamp(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// bkeys [E][6]: the complements of the least keys along x, y, z, then the greatest keys; 0 = no finite point
__global__ __launch_bounds__(256) void vox_bounds_kernel(const double* __restrict__ pts, const long long* __restrict__ offsets,
                                                         unsigned long long* __restrict__ bkeys) {
    const int e = blockIdx.y;
    const long long p0 = offsets[e], p1 = offsets[e + 1];
    unsigned long long k[6] = {0, 0, 0, 0, 0, 0};
    for (long long i = p0 + blockIdx.x * 256LL + threadIdx.x; i < p1; i += gridDim.x * 256LL) {
        const double c[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
        if (!dod_kept(c[0], c[1], c[2])) continue;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const unsigned long long ka = dod_order_key(c[a]);
            k[a] = max(k[a], ~ka); k[3 + a] = max(k[3 + a], ka);
        }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int o = IM_WAVE / 2; o > 0; o >>= 1) k[a] = max(k[a], (unsigned long long)__shfl_xor(k[a], o));
        if ((threadIdx.x & (IM_WAVE - 1)) == 0 && k[a]) atomicMax(&bkeys[6 * e + a], k[a]);
    }
}

// min x y z, max x y z per cloud; +inf / -inf for a cloud without a finite point
__global__ __launch_bounds__(256) void vox_bounds_decode_kernel(const unsigned long long* __restrict__ bkeys, int n, double* __restrict__ bounds) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const unsigned long long k = bkeys[t];
    const bool is_min = (t % 6) < 3;
    bounds[t] = k ? dod_order_value(is_min ? ~k : k) : (is_min ? dod_inf() : -dod_inf());
}

__global__ __launch_bounds__(256) void vox_keys_kernel(VoxTab T, const double* __restrict__ pts, long long n, long long* __restrict__ key,
                                                       unsigned long long* __restrict__ dropped) {
    const long long t = blockIdx.x * 256LL + threadIdx.x;
    const long long i = t < n ? t : n - 1;                   // the lanes behind the end stay for the ballot
    const int e = vox_last_at_or_below(T.offsets, T.E, i), g = T.per_cloud ? e : 0;
    const long long k = vox_point_key(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], T.grids + VOX_GRID * g, T.dims + 3 * g);
    const bool drop = t < n && k == VOX_DROPPED;
    if (t < n) key[t] = drop ? VOX_DROPPED : T.kbase[e] + k;
    const unsigned long long b = __ballot(drop);
    if (b) {
        if (__shfl(e, 0) == __shfl(e, IM_WAVE - 1)) {        // one cloud in the wave (the clouds ascend with the points): one atomic
            if ((threadIdx.x & (IM_WAVE - 1)) == 0) atomicAdd(&dropped[e], (unsigned long long)__popcll(b));
        } else if (drop) {
            atomicAdd(&dropped[e], 1ull);
        }
    }
}

// Item j = sorted position 0..n; n is the end. A key outside 0..cells-1 (VOX_DROPPED, or a wrong one) belongs to no voxel.
struct VoxHeadScan {
    const long long* skey; long long n, cells; int* seg;
    __device__ bool valid(long long j) const { return j < n && skey[j] >= 0 && skey[j] < cells; }
    __device__ bool head(long long j) const { return valid(j) && (j == 0 || skey[j - 1] != skey[j]); }
    __device__ long long count(long long j) const { return head(j) ? 1 : 0; }
    __device__ void write(long long j, long long pos) const {
        if (j > n) return;
        if (head(j) || (!valid(j) && (j == 0 || valid(j - 1)))) seg[pos] = (int)j;       // the start of voxel `pos`, or the end of voxel pos - 1
    }
};

// Positions, keys and permutation entries that are none are clamped: the result is then meaningless, but every access stays inside.
__global__ __launch_bounds__(256) void vox_voxels_kernel(VoxTab T, const long long* __restrict__ skey, const long long* __restrict__ perm, long long n,
                                                         const int* __restrict__ seg, const long long* __restrict__ n_vox,
                                                         const double* __restrict__ pts, const double* __restrict__ col, const double* __restrict__ nrm,
                                                         int32_t* __restrict__ grid_index, int32_t* __restrict__ count, int32_t* __restrict__ first,
                                                         double* __restrict__ mean_pts, double* __restrict__ mean_col, double* __restrict__ mean_nrm) {
    const long long v = blockIdx.x * 256LL + threadIdx.x;
    if (v >= vox_clamp(*n_vox, 0, n)) return;
    const long long j0 = vox_clamp(seg[v], 0, n - 1), j1 = vox_clamp(seg[v + 1], j0, n), cnt = j1 - j0;
    const long long key = skey[j0];
    const int e = vox_last_at_or_below(T.kbase, T.E, key), g = T.per_cloud ? e : 0;
    if (grid_index) vox_unkey(key - T.kbase[e], T.dims[3 * g + 1], T.dims[3 * g + 2], grid_index + 3 * v);
    if (count) count[v] = (int32_t)cnt;
    if (first) first[v] = (int32_t)(vox_clamp(perm[j0], 0, n - 1) - T.offsets[e]);
    const auto row_of = [&](const double* a) { return [=](long long k) { return a + 3 * vox_clamp(perm[j0 + k], 0, n - 1); }; };
    if (pts && mean_pts) vox_mean3(row_of(pts), cnt, mean_pts + 3 * v);
    if (col && mean_col) vox_mean3(row_of(col), cnt, mean_col + 3 * v);
    if (nrm && mean_nrm) vox_mean3(row_of(nrm), cnt, mean_nrm + 3 * v);
}

// nvox [E + 1]: the first voxel of every cloud, [E] = the number of voxels
__global__ __launch_bounds__(256) void vox_nvox_kernel(VoxTab T, const long long* __restrict__ skey, long long n, const int* __restrict__ seg,
                                                       const long long* __restrict__ n_vox, long long* __restrict__ nvox) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e > T.E) return;
    const long long V = vox_clamp(*n_vox, 0, n), want = T.kbase[e];
    long long lo = 0, hi = V;                                 // the first voxel whose key is >= want
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (skey[vox_clamp(seg[mid], 0, n - 1)] < want) lo = mid + 1; else hi = mid;
    }
    nvox[e] = lo;
}

// ---- the box mesh of one grid -------------------------------------------------------------------------------------------------------------
struct VoxGrid { double origin[3], s; long long ny, nz; };

__global__ __launch_bounds__(256) void vox_corners_kernel(const int32_t* __restrict__ grid_index, long long items, long long ny, long long nz,
                                                          long long* __restrict__ ckey) {
    const long long t = blockIdx.x * 256LL + threadIdx.x;
    if (t >= items) return;
    const long long v = t >> 3;
    const int l = (int)(t & 7);
    ckey[t] = vox_corner_key(grid_index[3 * v] + vox_corner_dx(l), grid_index[3 * v + 1] + vox_corner_dy(l), grid_index[3 * v + 2] + vox_corner_dz(l), ny, nz);
}

// Item j = sorted position 0..items; `items` is the end. vertex [8 v + l] receives the vertex of every item.
struct VoxVertexScan {
    const long long* skey; const long long* perm; long long items; int* vstart; int* vertex;
    __device__ bool head(long long j) const { return j < items && (j == 0 || skey[j - 1] != skey[j]); }
    __device__ long long count(long long j) const { return head(j) ? 1 : 0; }
    __device__ void write(long long j, long long pos) const {
        if (j > items) return;
        const bool h = head(j);
        if (h || j == items) vstart[pos] = (int)j;
        if (j < items) vertex[vox_clamp(perm[j], 0, items - 1)] = (int)(pos + (h ? 1 : 0) - 1);
    }
};

__global__ __launch_bounds__(256) void vox_vertices_kernel(VoxGrid G, const long long* __restrict__ skey, const long long* __restrict__ perm, long long items,
                                                           const int* __restrict__ vstart, const long long* __restrict__ n_vert,
                                                           const double* __restrict__ col, double* __restrict__ vertices, double* __restrict__ vcol) {
    const long long u = blockIdx.x * 256LL + threadIdx.x;
    if (u >= vox_clamp(*n_vert, 0, items)) return;
    const long long j0 = vox_clamp(vstart[u], 0, items - 1), j1 = vox_clamp(vstart[u + 1], j0, items), cnt = j1 - j0 < 8 ? j1 - j0 : 8;
    long long c[3];
    vox_corner_unkey(skey[j0], G.ny, G.nz, c);
#pragma unroll
    for (int a = 0; a < 3; ++a) vertices[3 * u + a] = vox_corner_pos(G.origin[a], c[a], G.s);
    if (col && vcol) vox_mean3([&](long long k) { return col + 3 * (vox_clamp(perm[j0 + k], 0, items - 1) >> 3); }, cnt, vcol + 3 * u);
}

__global__ __launch_bounds__(256) void vox_triangles_kernel(const int* __restrict__ vertex, long long V, int32_t* __restrict__ tri) {
    const long long v = blockIdx.x * 256LL + threadIdx.x;
    if (v >= V) return;
    int at[8];
#pragma unroll
    for (int l = 0; l < 8; ++l) at[l] = vertex[8 * v + l];
#pragma unroll
    for (int t = 0; t < 12; ++t)
#pragma unroll
        for (int k = 0; k < 3; ++k) tri[36 * v + 3 * t + k] = at[vox_triangle(t, k)];
}

// ---- the host half: what a call refuses, the sizes of its grids, its tables -----------------------------------------------------------------
struct VoxPlan {
    std::vector<long long> table;          // offsets [E + 1], kbase [E + 1], dims [G][3]
    std::vector<double> grids;             // [G][7]
    long long n = 0, cells = 0;
    int G = 0;
    VoxTab tab(const long long* d, const double* d_grids, int E, int per_cloud) const {
        return VoxTab{d, d + E + 1, d + 2 * (E + 1), d_grids, E, per_cloud};
    }
};

const char* vox_clouds(const long long* h_offsets, int E, long long& n) {
    if (E < 0 || E > VOX_MAX_CLOUDS) return "the number of clouds must be 0..65535";
    if (!h_offsets) return "null offsets";
    if (h_offsets[0] != 0) return "the first cloud must start at point 0";
    for (int e = 0; e < E; ++e)
        if (h_offsets[e + 1] < h_offsets[e]) return "a cloud with a negative number of points";
    n = h_offsets[E];
    if (n > VOX_MAX_POINTS) return "more than 2^26 points: split the call";
    return nullptr;
}

const char* vox_plan(const long long* h_offsets, int E, const double* h_grids, int per_cloud, VoxPlan& pl) {
    if (const char* why = vox_clouds(h_offsets, E, pl.n)) return why;
    if (E == 0) return nullptr;
    if (!h_grids) return "null grids";
    pl.G = per_cloud ? E : 1;
    pl.table.assign(2 * (E + 1) + 3 * (size_t)pl.G, 0);
    pl.grids.assign(h_grids, h_grids + (size_t)VOX_GRID * pl.G);
    long long* t = pl.table.data();
    for (int e = 0; e <= E; ++e) t[e] = h_offsets[e];
    long long* kbase = t + E + 1;
    long long* dims = t + 2 * (E + 1);
    for (int g = 0; g < pl.G; ++g) {
        const long long cells = vox_grid_cells(h_grids + VOX_GRID * g, dims + 3 * g);
        if (cells < 0) return "a grid needs finite bounds with max >= min, a finite voxel size > 0 and at most 2^62 voxels";
        if (per_cloud) {
            if (cells > VOX_MAX_CELLS - pl.cells) return "the grids of the call hold more than 2^62 voxels";
            kbase[g] = pl.cells;
            pl.cells += cells;
        } else {
            if (cells > VOX_MAX_CELLS / E) return "the grid times the number of clouds exceeds 2^62 voxels";
            for (int e = 0; e <= E; ++e) kbase[e] = e * cells;
            pl.cells = E * cells;
        }
    }
    kbase[E] = pl.cells;
    return nullptr;
}

int vox_upload(im_ctx* ctx, const VoxPlan& pl, const VoxelScratch& lay, hipStream_t s) {
    void* const base = ctx->scratch.voxel.p;
    IM_HIP(ctx, hipMemcpyAsync(lay.table.at(base), pl.table.data(), pl.table.size() * sizeof(long long), hipMemcpyHostToDevice, s));
    IM_HIP(ctx, hipMemcpyAsync(lay.grids.at(base), pl.grids.data(), pl.grids.size() * sizeof(double), hipMemcpyHostToDevice, s));
    IM_HIP(ctx, hipStreamSynchronize(s));          // the source is host memory of this call
    return 0;
}

}  // namespace
}  // namespace im

using namespace im;

extern "C" {

int im_voxel_max_points(void) { return (int)VOX_MAX_POINTS; }

int im_voxel_bounds(im_ctx* ctx, const double* d_pts, const long long* h_offsets, int n_clouds, double* d_bounds, void* stream) {
    IM_CHECK_CTX(ctx);
    long long n = 0;
    if (const char* why = vox_clouds(h_offsets, n_clouds, n)) return ctx->fail(-77, "im_voxel_bounds: %s", why);
    const int E = n_clouds;
    if (E == 0) return 0;
    if (!d_bounds || (n && !d_pts)) return ctx->fail(-77, "im_voxel_bounds: null pointer");
    const VoxelScratch lay(E, 0, 0);
    IM_GROW(ctx, ctx->grow(ctx->scratch.voxel, lay.bytes, "voxel.scratch"), -22, "im_voxel_bounds: allocation failed");
    void* const base = ctx->scratch.voxel.p;
    long long* d_offsets = lay.table.at(base);
    unsigned long long* bkeys = lay.bkeys.at(base);
    hipStream_t s = (hipStream_t)stream;
    IM_HIP(ctx, hipMemcpyAsync(d_offsets, h_offsets, (E + 1) * sizeof(long long), hipMemcpyHostToDevice, s));
    IM_HIP(ctx, hipStreamSynchronize(s));          // the source is host memory of this call
    IM_HIP(ctx, hipMemsetAsync(bkeys, 0, 6 * E * sizeof(unsigned long long), s));
    long long largest = 0;
    for (int e = 0; e < E; ++e) largest = std::max(largest, h_offsets[e + 1] - h_offsets[e]);
    if (largest) {
        const dim3 grid((unsigned)std::min<long long>(blocks_of(largest, 1024), VOX_BOUNDS_BLOCKS), (unsigned)E);
        IM_LAUNCH(ctx, "vox_bounds", s, launch(vox_bounds_kernel, grid, 256, 0, s, d_pts, (const long long*)d_offsets, bkeys));
    }
    IM_LAUNCH(ctx, "vox_bounds_decode", s, launch(vox_bounds_decode_kernel, blocks_of(6 * E, 256), 256, 0, s, (const unsigned long long*)bkeys, 6 * E, d_bounds));
    IM_GUARD_CHECK(ctx, s, "im_voxel_bounds");
    return 0;
}

int im_voxel_keys(im_ctx* ctx, const double* d_pts, const long long* h_offsets, int n_clouds, const double* h_grids, int per_cloud, long long* d_key,
                  long long* d_dropped, void* stream) {
    IM_CHECK_CTX(ctx);
    VoxPlan pl;
    if (const char* why = vox_plan(h_offsets, n_clouds, h_grids, per_cloud, pl)) return ctx->fail(-77, "im_voxel_keys: %s", why);
    const int E = n_clouds;
    if (E == 0) return 0;
    if (!d_dropped || (pl.n && (!d_pts || !d_key))) return ctx->fail(-77, "im_voxel_keys: null pointer");
    hipStream_t s = (hipStream_t)stream;
    IM_HIP(ctx, hipMemsetAsync(d_dropped, 0, E * sizeof(long long), s));
    if (pl.n == 0) return 0;
    const VoxelScratch lay(E, pl.G, 0);
    IM_GROW(ctx, ctx->grow(ctx->scratch.voxel, lay.bytes, "voxel.scratch"), -22, "im_voxel_keys: allocation failed");
    if (const int rc = vox_upload(ctx, pl, lay, s)) return rc;
    const VoxTab T = pl.tab(lay.table.at(ctx->scratch.voxel.p), lay.grids.at(ctx->scratch.voxel.p), E, per_cloud != 0);
    IM_LAUNCH(ctx, "vox_keys", s, launch(vox_keys_kernel, blocks_of(pl.n, 256), 256, 0, s, T, d_pts, pl.n, d_key, reinterpret_cast<unsigned long long*>(d_dropped)));
    IM_GUARD_CHECK(ctx, s, "im_voxel_keys");
    return 0;
}

int im_voxel_reduce(im_ctx* ctx, const long long* h_offsets, int n_clouds, const double* h_grids, int per_cloud, const long long* d_sorted_keys,
                    const long long* d_perm, const double* d_pts, const double* d_colors, const double* d_normals, long long* d_nvox,
                    int32_t* d_grid_index, int32_t* d_count, int32_t* d_first, double* d_mean_pts, double* d_mean_colors, double* d_mean_normals,
                    void* stream) {
    IM_CHECK_CTX(ctx);
    VoxPlan pl;
    if (const char* why = vox_plan(h_offsets, n_clouds, h_grids, per_cloud, pl)) return ctx->fail(-77, "im_voxel_reduce: %s", why);
    const int E = n_clouds;
    if (E == 0) return 0;
    if (!d_nvox || (pl.n && (!d_sorted_keys || !d_perm))) return ctx->fail(-77, "im_voxel_reduce: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (pl.n == 0) {
        IM_HIP(ctx, hipMemsetAsync(d_nvox, 0, (E + 1) * sizeof(long long), s));
        return 0;
    }
    const long long n = pl.n;
    const VoxelScratch lay(E, pl.G, n);
    IM_GROW(ctx, ctx->grow(ctx->scratch.voxel, lay.bytes, "voxel.scratch"), -22, "im_voxel_reduce: allocation failed (%lld points)", n);
    if (const int rc = vox_upload(ctx, pl, lay, s)) return rc;
    void* const base = ctx->scratch.voxel.p;
    const VoxTab T = pl.tab(lay.table.at(base), lay.grids.at(base), E, per_cloud != 0);
    int* seg = lay.seg.at(base);
    long long* total = lay.total.at(base);
    const VoxHeadScan hs{d_sorted_keys, n, pl.cells, seg};
    IM_LAUNCH(ctx, "vox_heads_scan", s, launch_scan(hs, n + 1, lay.sums.at(base), total, s));
    IM_LAUNCH(ctx, "vox_voxels", s, launch(vox_voxels_kernel, blocks_of(n, 256), 256, 0, s, T, d_sorted_keys, d_perm, n, (const int*)seg, (const long long*)total,
                                           d_pts, d_colors, d_normals, d_grid_index, d_count, d_first, d_mean_pts, d_mean_colors, d_mean_normals));
    IM_LAUNCH(ctx, "vox_nvox", s, launch(vox_nvox_kernel, blocks_of(E + 1, 256), 256, 0, s, T, d_sorted_keys, n, (const int*)seg, (const long long*)total, d_nvox));
    IM_GUARD_CHECK(ctx, s, "im_voxel_reduce");
    return 0;
}

int im_voxel_mesh_corners(im_ctx* ctx, const double* h_grid, const int32_t* d_grid_index, long long n_voxels, long long* d_corner_keys, void* stream) {
    IM_CHECK_CTX(ctx);
    long long dims[3];
    if (!h_grid) return ctx->fail(-77, "im_voxel_mesh_corners: null grid");
    if (vox_grid_cells(h_grid, dims, true) < 0)
        return ctx->fail(-77, "im_voxel_mesh_corners: a grid needs finite bounds with max >= min, a finite voxel size > 0 and at most 2^62 corner keys");
    if (n_voxels < 0 || 8 * n_voxels > VOX_MAX_MESH_ITEMS) return ctx->fail(-77, "im_voxel_mesh_corners: 8 V must be 0..2^27");
    if (n_voxels == 0) return 0;
    if (!d_grid_index || !d_corner_keys) return ctx->fail(-77, "im_voxel_mesh_corners: null pointer");
    hipStream_t s = (hipStream_t)stream;
    IM_LAUNCH(ctx, "vox_corners", s, launch(vox_corners_kernel, blocks_of(8 * n_voxels, 256), 256, 0, s, d_grid_index, 8 * n_voxels, dims[1], dims[2], d_corner_keys));
    IM_GUARD_CHECK(ctx, s, "im_voxel_mesh_corners");
    return 0;
}

int im_voxel_mesh(im_ctx* ctx, const double* h_grid, long long n_voxels, const double* d_colors, const long long* d_sorted_keys, const long long* d_perm,
                  long long* d_n_vertices, double* d_vertices, double* d_vertex_colors, int32_t* d_triangles, void* stream) {
    IM_CHECK_CTX(ctx);
    long long dims[3];
    if (!h_grid) return ctx->fail(-77, "im_voxel_mesh: null grid");
    if (vox_grid_cells(h_grid, dims, true) < 0)
        return ctx->fail(-77, "im_voxel_mesh: a grid needs finite bounds with max >= min, a finite voxel size > 0 and at most 2^62 corner keys");
    if (n_voxels < 0 || 8 * n_voxels > VOX_MAX_MESH_ITEMS) return ctx->fail(-77, "im_voxel_mesh: 8 V must be 0..2^27");
    if (!d_n_vertices) return ctx->fail(-77, "im_voxel_mesh: null pointer");
    if (n_voxels && (!d_sorted_keys || !d_perm || !d_vertices || !d_triangles)) return ctx->fail(-77, "im_voxel_mesh: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (n_voxels == 0) {
        IM_HIP(ctx, hipMemsetAsync(d_n_vertices, 0, sizeof(long long), s));
        return 0;
    }
    const long long items = 8 * n_voxels;
    const VoxelMeshScratch lay(items);
    IM_GROW(ctx, ctx->grow(ctx->scratch.voxel, lay.bytes, "voxel.scratch"), -22, "im_voxel_mesh: allocation failed (%lld voxels)", n_voxels);
    void* const base = ctx->scratch.voxel.p;
    int* vstart = lay.vstart.at(base);
    int* vertex = lay.vertex.at(base);
    const VoxGrid G{{h_grid[0], h_grid[1], h_grid[2]}, h_grid[6], dims[1], dims[2]};
    const VoxVertexScan vs{d_sorted_keys, d_perm, items, vstart, vertex};
    IM_LAUNCH(ctx, "vox_vertex_scan", s, launch_scan(vs, items + 1, lay.sums.at(base), d_n_vertices, s));
    IM_LAUNCH(ctx, "vox_vertices", s, launch(vox_vertices_kernel, blocks_of(items, 256), 256, 0, s, G, d_sorted_keys, d_perm, items, (const int*)vstart,
                                             (const long long*)d_n_vertices, d_colors, d_vertices, d_vertex_colors));
    IM_LAUNCH(ctx, "vox_triangles", s, launch(vox_triangles_kernel, blocks_of(n_voxels, 256), 256, 0, s, (const int*)vertex, n_voxels, d_triangles));
    IM_GUARD_CHECK(ctx, s, "im_voxel_mesh");
    return 0;
}

}  // extern "C"
