// Triangle-mesh filters, the convex-hull crop and uniform mesh sampling on the device: what `MeshingPoisson.run()` of the reference's
// `post_processing/open3d_fun.py` does to a reconstructed surface behind the Poisson solve (Open3D's `remove_vertices_by_mask`,
// `remove_degenerate_triangles`, `remove_duplicated_triangles`, `remove_duplicated_vertices`, `remove_unreferenced_vertices`,
// `remove_non_manifold_edges` (its census), `select_by_index`, `sample_points_uniformly`, and `utils/geospatial.py: point_in_hull`).
// Open3D is an un-vendored dependency: every operation has a definition of its own and is pinned bit for bit against
// tests/mesh_oracle.py. The per-item arithmetic is mesh_tri.h. Sorting between the entry points is torch's stable sort, plumbing.
//
//   mesh_tri_flag_kernel      one thread per triangle: kept iff its mask allows it, its three indices (through the merge map, when given)
//                             lie in [0, V) and are kept, and - on request - are distinct; marks the vertices it references
//   mesh_vertex_flag_kernel   one thread per vertex: kept iff its mask allows it and - on request - a kept triangle references it
//   scan_*_kernel             (scan.h) over the vertex flags: the vertex map (-1 = dropped) and the kept list; over the triangle flags:
//                             the renumbered triangles and their old positions
//   mesh_*_keys_kernel        triangle keys (rotation to smallest-index-first), vertex keys (bits, -0.0 = 0.0, a NaN vertex unique), edge keys
//   scan_*_kernel             over the heads of the sorted keys: the first item of every segment; mesh_first_kernel spreads it to the items
//   mesh_census_kernel        one thread per sorted edge item: heads of segments of more than two items, counted by integer atomics
//   mesh_in_hull_kernel       one thread per point, the facets staged through LDS 512 at a time, a running maximum in facet order
//   mesh_area_kernel          one thread per triangle: the area, and the largest by atomicMax on its bits (areas are >= 0: bits order them)
//   scan_*_kernel             over the quantised areas: exact integer cumulative counts; mesh_allocation_kernel: samples per triangle
//   mesh_sample_kernel        one thread per sample: bisection in the allocation table, a counter-based generator, the barycentric point
// An index outside [0, V) is skipped where a triangle is judged (the triangle is dropped; its area is 0) and clamped where a table the
// caller supplies is followed (the permutation, the allocation table): the figures are then meaningless, every access stays inside.
// float64 throughout, contraction off in mesh_tri.h. No launch geometry and no property of the device enters a result.
#include <cmath>
#include <initializer_list>

#include "common.h"
#include "ctx.h"
#include "stage_scratch.h"
#include "mesh_tri.h"

namespace im {
namespace {

#include "scan.h"

__device__ __forceinline__ long long mesh_clamp(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the index a triangle corner stands for: through the merge map when there is one; -1 for an index outside [0, V) on either side of it
__device__ __forceinline__ int mesh_corner(const int* __restrict__ tri, long long t, int k, const int* __restrict__ merge, long long V) {
    int i = tri[3 * t + k];
    if (!mesh_index_ok(i, V)) return -1;
    if (merge) {
        i = merge[i];
        if (!mesh_index_ok(i, V)) return -1;
    }
    return i;
}

__global__ __launch_bounds__(256) void mesh_tri_flag_kernel(const int* __restrict__ tri, long long T, long long V, const unsigned char* __restrict__ vkeep,
                                                            const int* __restrict__ merge, const unsigned char* __restrict__ tkeep, int drop_degenerate,
                                                            unsigned char* __restrict__ tflag, unsigned char* __restrict__ ref) {
    const long long t = blockIdx.x * 256LL + threadIdx.x;
    if (t >= T) return;
    const int a = mesh_corner(tri, t, 0, merge, V), b = mesh_corner(tri, t, 1, merge, V), c = mesh_corner(tri, t, 2, merge, V);
    bool keep = (!tkeep || tkeep[t]) && a >= 0 && b >= 0 && c >= 0;
    if (keep && vkeep) keep = vkeep[a] && vkeep[b] && vkeep[c];
    if (keep && drop_degenerate) keep = a != b && b != c && a != c;
    tflag[t] = keep ? 1 : 0;
    if (keep) { ref[a] = 1; ref[b] = 1; ref[c] = 1; }         // the same value from every writer
}

__global__ __launch_bounds__(256) void mesh_vertex_flag_kernel(long long V, const unsigned char* __restrict__ vkeep, const unsigned char* __restrict__ ref,
                                                               int drop_unreferenced, unsigned char* __restrict__ vflag) {
    const long long v = blockIdx.x * 256LL + threadIdx.x;
    if (v >= V) return;
    vflag[v] = ((!vkeep || vkeep[v]) && (!drop_unreferenced || ref[v])) ? 1 : 0;
}

struct MeshVertexScan {       // the vertex map and the kept vertices in ascending old index
    const unsigned char* vflag; long long V; int* vmap; int* vlist;
    __device__ long long count(long long j) const { return j < V && vflag[j] ? 1 : 0; }
    __device__ void write(long long j, long long pos) const {
        if (j >= V) return;
        const bool k = vflag[j] != 0;
        vmap[j] = k ? (int)pos : -1;
        if (k) vlist[pos] = (int)j;
    }
};

struct MeshTriScan {          // the kept triangles in their old order, renumbered
    const unsigned char* tflag; const int* tri; const int* merge; const int* vmap; long long T, V; int* tri_out; int* tri_pos;
    __device__ long long count(long long j) const { return j < T && tflag[j] ? 1 : 0; }
    __device__ void write(long long j, long long pos) const {
        if (!count(j)) return;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int i = mesh_corner(tri, j, k, merge, V);     // >= 0: the triangle is kept
            tri_out[3 * pos + k] = vmap[mesh_clamp(i, 0, V - 1)];
        }
        tri_pos[pos] = (int)j;
    }
};

__global__ __launch_bounds__(256) void mesh_triangle_keys_kernel(const int* __restrict__ tri, long long T, long long* __restrict__ k0, long long* __restrict__ k1) {
    const long long t = blockIdx.x * 256LL + threadIdx.x;
    if (t >= T) return;
    mesh_tri_keys(tri[3 * t], tri[3 * t + 1], tri[3 * t + 2], k0 + t, k1 + t);
}

__global__ __launch_bounds__(256) void mesh_vertex_keys_kernel(const double* __restrict__ vert, long long V, long long* __restrict__ k0, long long* __restrict__ k1,
                                                               long long* __restrict__ k2) {
    const long long v = blockIdx.x * 256LL + threadIdx.x;
    if (v >= V) return;
    long long k[3];
    mesh_vertex_keys(vert[3 * v], vert[3 * v + 1], vert[3 * v + 2], v, k);
    k0[v] = k[0]; k1[v] = k[1]; k2[v] = k[2];
}

__global__ __launch_bounds__(256) void mesh_edge_keys_kernel(const int* __restrict__ tri, long long items, long long* __restrict__ key) {
    const long long j = blockIdx.x * 256LL + threadIdx.x;
    if (j >= items) return;
    const long long t = j / 3;
    const int e = (int)(j - 3 * t);
    key[j] = mesh_edge_key(tri[3 * t + e], tri[3 * t + (e + 1) % 3]);
}

// Item j = sorted position. The keys are in item order; perm [n] = sorted position -> item, clamped where it is none.
struct MeshSegmentScan {
    const long long* k0; const long long* k1; const long long* k2; const long long* perm; long long n; int* head; int* segment;
    __device__ long long item(long long j) const { return mesh_clamp(perm[j], 0, n - 1); }
    __device__ bool is_head(long long j) const {
        if (j >= n) return false;
        if (j == 0) return true;
        const long long a = item(j - 1), b = item(j);
        return k0[a] != k0[b] || (k1 && k1[a] != k1[b]) || (k2 && k2[a] != k2[b]);
    }
    __device__ long long count(long long j) const { return is_head(j) ? 1 : 0; }
    __device__ void write(long long j, long long pos) const {
        if (j >= n) return;
        const bool h = is_head(j);
        segment[j] = (int)(pos + (h ? 1 : 0) - 1);
        if (h) head[pos] = (int)item(j);
    }
};

__global__ __launch_bounds__(256) void mesh_first_kernel(const long long* __restrict__ perm, long long n, const int* __restrict__ head, const int* __restrict__ segment,
                                                         int* __restrict__ first, unsigned char* __restrict__ keep) {
    const long long j = blockIdx.x * 256LL + threadIdx.x;
    if (j >= n) return;
    const long long i = mesh_clamp(perm[j], 0, n - 1);
    const int f = head[mesh_clamp(segment[j], 0, n - 1)];
    if (first) first[i] = f;
    if (keep) keep[i] = f == i ? 1 : 0;
}

__global__ __launch_bounds__(256) void mesh_census_kernel(const long long* __restrict__ skey, long long n, unsigned long long* __restrict__ count) {
    const long long j = blockIdx.x * 256LL + threadIdx.x;
    const bool crowded = j + 2 < n && (j == 0 || skey[j - 1] != skey[j]) && skey[j + 2] == skey[j];
    const unsigned long long b = __ballot(crowded);
    if (b && (threadIdx.x & (IM_WAVE - 1)) == 0) atomicAdd(count, (unsigned long long)__popcll(b));
}

__global__ __launch_bounds__(256) void mesh_in_hull_kernel(const double* __restrict__ pts, long long n, const double* __restrict__ facets, int F,
                                                           unsigned char* __restrict__ inside) {
    __shared__ double sf[4 * MESH_HULL_CHUNK];
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    const long long at = i < n ? i : n - 1;                  // the lanes behind the end stay for the barriers
    const double x = pts[3 * at], y = pts[3 * at + 1], z = pts[3 * at + 2];
    double m = mesh_minus_inf();
    for (int c0 = 0; c0 < F; c0 += MESH_HULL_CHUNK) {
        const int nf = F - c0 < MESH_HULL_CHUNK ? F - c0 : MESH_HULL_CHUNK;
        __syncthreads();
        for (int k = threadIdx.x; k < 4 * nf; k += 256) sf[k] = facets[4LL * c0 + k];
        __syncthreads();
        for (int f = 0; f < nf; ++f) m = mesh_running_max(m, mesh_facet_value(sf + 4 * f, x, y, z));
    }
    if (i < n) inside[i] = mesh_inside(m) ? 1 : 0;
}

__device__ __forceinline__ double mesh_triangle_area(const double* __restrict__ vert, long long V, const int* __restrict__ tri, long long t) {
    const int a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    if (!mesh_index_ok(a, V) || !mesh_index_ok(b, V) || !mesh_index_ok(c, V)) return 0.0;
    return mesh_area(vert + 3LL * a, vert + 3LL * b, vert + 3LL * c);
}

__global__ __launch_bounds__(256) void mesh_area_kernel(const double* __restrict__ vert, long long V, const int* __restrict__ tri, long long T,
                                                        double* __restrict__ area, unsigned long long* __restrict__ amax) {
    const long long t = blockIdx.x * 256LL + threadIdx.x;
    const double a = t < T ? mesh_triangle_area(vert, V, tri, t) : 0.0;
    if (t < T) area[t] = a;
    unsigned long long k = (unsigned long long)mesh_double_bits(a);      // a >= 0 and finite: its bits order it
#pragma unroll
    for (int o = IM_WAVE / 2; o > 0; o >>= 1) k = max(k, (unsigned long long)__shfl_xor(k, o));
    if ((threadIdx.x & (IM_WAVE - 1)) == 0 && k) atomicMax(amax, k);
}

struct MeshCumScan {          // cum [t] = the quantised areas of triangles 0..t
    const double* area; const unsigned long long* amax; long long T; long long* cum;
    __device__ long long count(long long j) const {
        if (j >= T) return 0;
        double mx;
        const unsigned long long b = *amax;
        __builtin_memcpy(&mx, &b, sizeof(mx));
        return mesh_quantised_area(area[j], mx);
    }
    __device__ void write(long long j, long long pos) const { if (j < T) cum[j] = pos + count(j); }
};

__global__ __launch_bounds__(256) void mesh_allocation_kernel(const long long* __restrict__ cum, long long T, long long C, long long N, const double* __restrict__ area,
                                                              long long* __restrict__ count_end, double* __restrict__ area_out) {
    const long long t = blockIdx.x * 256LL + threadIdx.x;
    if (t >= T) return;
    count_end[t] = C > 0 ? mesh_allocation(cum[t], C, N) : 0;
    if (area_out) area_out[t] = area[t];
}

__global__ __launch_bounds__(256) void mesh_sample_kernel(const double* __restrict__ vert, long long V, const int* __restrict__ tri, long long T,
                                                          const long long* __restrict__ count_end, long long N, unsigned long long seed,
                                                          const double* __restrict__ vcol, const double* __restrict__ vnrm, double* __restrict__ points,
                                                          double* __restrict__ colors, double* __restrict__ normals, int* __restrict__ tri_index) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= N) return;
    long long lo = 0, hi = T - 1;                             // the first triangle with count_end > i; the last one when the table has none
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (count_end[mid] > i) hi = mid; else lo = mid + 1;
    }
    const long long a = mesh_clamp(tri[3 * lo], 0, V - 1), b = mesh_clamp(tri[3 * lo + 1], 0, V - 1), c = mesh_clamp(tri[3 * lo + 2], 0, V - 1);
    double w[3];
    mesh_weights(seed, (unsigned long long)i, w);
    mesh_blend(w, vert + 3 * a, vert + 3 * b, vert + 3 * c, points + 3 * i);
    if (vcol && colors) mesh_blend(w, vcol + 3 * a, vcol + 3 * b, vcol + 3 * c, colors + 3 * i);
    if (normals) {
        if (vnrm) mesh_blend(w, vnrm + 3 * a, vnrm + 3 * b, vnrm + 3 * c, normals + 3 * i);
        else mesh_unit_normal(vert + 3 * a, vert + 3 * b, vert + 3 * c, normals + 3 * i);
    }
    if (tri_index) tri_index[i] = (int)lo;
}

const char* mesh_bad_count(long long n, long long cap = MESH_MAX_ITEMS) { return n < 0 ? "a negative count" : (n > cap ? "more than 2^26 vertices, triangles or samples: split the call" : nullptr); }

}  // namespace
}  // namespace im

using namespace im;

extern "C" {

int im_mesh_max_items(void) { return (int)MESH_MAX_ITEMS; }
int im_mesh_hull_chunk(void) { return MESH_HULL_CHUNK; }

int im_mesh_select(im_ctx* ctx, const unsigned char* d_vertex_keep, long long n_vertices, const int32_t* d_triangles, long long n_triangles,
                   const int32_t* d_vertex_merge, const unsigned char* d_triangle_keep, int drop_degenerate, int drop_unreferenced, int32_t* d_vertex_map,
                   int32_t* d_vertex_list, int32_t* d_triangles_out, int32_t* d_triangle_pos, long long* d_counts, void* stream) {
    IM_CHECK_CTX(ctx);
    const long long V = n_vertices, T = n_triangles;
    if (const char* why = mesh_bad_count(V)) return ctx->fail(-78, "im_mesh_select: %s", why);
    if (const char* why = mesh_bad_count(T)) return ctx->fail(-78, "im_mesh_select: %s", why);
    if (!d_counts || (V && (!d_vertex_map || !d_vertex_list)) || (T && (!d_triangles || !d_triangles_out || !d_triangle_pos)))
        return ctx->fail(-78, "im_mesh_select: null pointer");
    hipStream_t s = (hipStream_t)stream;
    IM_HIP(ctx, hipMemsetAsync(d_counts, 0, 2 * sizeof(long long), s));
    if (V == 0 && T == 0) return 0;
    const MeshSelectScratch lay(V, T);
    IM_GROW(ctx, ctx->grow(ctx->scratch.mesh, lay.bytes, "mesh.scratch"), -22, "im_mesh_select: allocation failed");
    void* const base = ctx->scratch.mesh.p;
    unsigned char* tflag = lay.tflag.at(base);
    unsigned char* vflag = lay.vflag.at(base);
    unsigned char* ref = lay.ref.at(base);
    if (V) IM_HIP(ctx, hipMemsetAsync(ref, 0, V, s));
    if (T)
        IM_LAUNCH(ctx, "mesh_tri_flag", s, launch(mesh_tri_flag_kernel, blocks_of(T, 256), 256, 0, s, d_triangles, T, V, d_vertex_keep, d_vertex_merge, d_triangle_keep,
                                                  drop_degenerate, tflag, ref));
    if (V) {
        IM_LAUNCH(ctx, "mesh_vertex_flag", s, launch(mesh_vertex_flag_kernel, blocks_of(V, 256), 256, 0, s, V, d_vertex_keep, (const unsigned char*)ref, drop_unreferenced, vflag));
        const MeshVertexScan vs{vflag, V, d_vertex_map, d_vertex_list};
        IM_LAUNCH(ctx, "mesh_vertex_scan", s, launch_scan(vs, V, lay.sums.at(base), d_counts, s));
    }
    if (T) {
        const MeshTriScan ts{tflag, d_triangles, d_vertex_merge, d_vertex_map, T, V, d_triangles_out, d_triangle_pos};
        IM_LAUNCH(ctx, "mesh_triangle_scan", s, launch_scan(ts, T, lay.sums.at(base), d_counts + 1, s));
    }
    IM_GUARD_CHECK(ctx, s, "im_mesh_select");
    return 0;
}

int im_mesh_triangle_keys(im_ctx* ctx, const int32_t* d_triangles, long long n_triangles, long long* d_key0, long long* d_key1, void* stream) {
    IM_CHECK_CTX(ctx);
    if (const char* why = mesh_bad_count(n_triangles)) return ctx->fail(-78, "im_mesh_triangle_keys: %s", why);
    if (n_triangles == 0) return 0;
    if (!d_triangles || !d_key0 || !d_key1) return ctx->fail(-78, "im_mesh_triangle_keys: null pointer");
    hipStream_t s = (hipStream_t)stream;
    IM_LAUNCH(ctx, "mesh_triangle_keys", s, launch(mesh_triangle_keys_kernel, blocks_of(n_triangles, 256), 256, 0, s, d_triangles, n_triangles, d_key0, d_key1));
    IM_GUARD_CHECK(ctx, s, "im_mesh_triangle_keys");
    return 0;
}

int im_mesh_vertex_keys(im_ctx* ctx, const double* d_vertices, long long n_vertices, long long* d_key0, long long* d_key1, long long* d_key2, void* stream) {
    IM_CHECK_CTX(ctx);
    if (const char* why = mesh_bad_count(n_vertices)) return ctx->fail(-78, "im_mesh_vertex_keys: %s", why);
    if (n_vertices == 0) return 0;
    if (!d_vertices || !d_key0 || !d_key1 || !d_key2) return ctx->fail(-78, "im_mesh_vertex_keys: null pointer");
    hipStream_t s = (hipStream_t)stream;
    IM_LAUNCH(ctx, "mesh_vertex_keys", s, launch(mesh_vertex_keys_kernel, blocks_of(n_vertices, 256), 256, 0, s, d_vertices, n_vertices, d_key0, d_key1, d_key2));
    IM_GUARD_CHECK(ctx, s, "im_mesh_vertex_keys");
    return 0;
}

int im_mesh_edge_keys(im_ctx* ctx, const int32_t* d_triangles, long long n_triangles, long long* d_keys, void* stream) {
    IM_CHECK_CTX(ctx);
    if (const char* why = mesh_bad_count(n_triangles)) return ctx->fail(-78, "im_mesh_edge_keys: %s", why);
    if (n_triangles == 0) return 0;
    if (!d_triangles || !d_keys) return ctx->fail(-78, "im_mesh_edge_keys: null pointer");
    hipStream_t s = (hipStream_t)stream;
    IM_LAUNCH(ctx, "mesh_edge_keys", s, launch(mesh_edge_keys_kernel, blocks_of(3 * n_triangles, 256), 256, 0, s, d_triangles, 3 * n_triangles, d_keys));
    IM_GUARD_CHECK(ctx, s, "im_mesh_edge_keys");
    return 0;
}

int im_mesh_first_of_segment(im_ctx* ctx, long long n, const long long* d_key0, const long long* d_key1, const long long* d_key2, const long long* d_perm,
                             int32_t* d_first, unsigned char* d_keep, void* stream) {
    IM_CHECK_CTX(ctx);
    if (const char* why = mesh_bad_count(n)) return ctx->fail(-78, "im_mesh_first_of_segment: %s", why);
    if (n == 0) return 0;
    if (!d_key0 || !d_perm || (!d_key1 && d_key2)) return ctx->fail(-78, "im_mesh_first_of_segment: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const MeshSegmentScratch lay(n);
    IM_GROW(ctx, ctx->grow(ctx->scratch.mesh, lay.bytes, "mesh.scratch"), -22, "im_mesh_first_of_segment: allocation failed");
    void* const base = ctx->scratch.mesh.p;
    int* head = lay.head.at(base);
    int* segment = lay.segment.at(base);
    const MeshSegmentScan ss{d_key0, d_key1, d_key2, d_perm, n, head, segment};
    IM_LAUNCH(ctx, "mesh_segment_scan", s, launch_scan(ss, n, lay.sums.at(base), lay.total.at(base), s));
    IM_LAUNCH(ctx, "mesh_first", s, launch(mesh_first_kernel, blocks_of(n, 256), 256, 0, s, d_perm, n, (const int*)head, (const int*)segment, d_first, d_keep));
    IM_GUARD_CHECK(ctx, s, "im_mesh_first_of_segment");
    return 0;
}

int im_mesh_edge_census(im_ctx* ctx, const long long* d_sorted_keys, long long n_items, long long* d_count, void* stream) {
    IM_CHECK_CTX(ctx);
    if (const char* why = mesh_bad_count(n_items, 3 * MESH_MAX_ITEMS)) return ctx->fail(-78, "im_mesh_edge_census: %s", why);
    if (!d_count || (n_items && !d_sorted_keys)) return ctx->fail(-78, "im_mesh_edge_census: null pointer");
    hipStream_t s = (hipStream_t)stream;
    IM_HIP(ctx, hipMemsetAsync(d_count, 0, sizeof(long long), s));
    if (n_items == 0) return 0;
    IM_LAUNCH(ctx, "mesh_census", s, launch(mesh_census_kernel, blocks_of(n_items, 256), 256, 0, s, d_sorted_keys, n_items, reinterpret_cast<unsigned long long*>(d_count)));
    IM_GUARD_CHECK(ctx, s, "im_mesh_edge_census");
    return 0;
}

int im_mesh_in_hull(im_ctx* ctx, const double* d_points, long long n_points, const double* h_facets, int n_facets, unsigned char* d_inside, void* stream) {
    IM_CHECK_CTX(ctx);
    if (const char* why = mesh_bad_count(n_points)) return ctx->fail(-78, "im_mesh_in_hull: %s", why);
    if (n_facets <= 0 || n_facets > MESH_MAX_FACETS) return ctx->fail(-78, "im_mesh_in_hull: a hull has 1..2^22 facets");
    if (!h_facets) return ctx->fail(-78, "im_mesh_in_hull: null facets");
    for (long long k = 0; k < 4LL * n_facets; ++k)
        if (!std::isfinite(h_facets[k])) return ctx->fail(-78, "im_mesh_in_hull: a facet is not finite");
    if (n_points == 0) return 0;
    if (!d_points || !d_inside) return ctx->fail(-78, "im_mesh_in_hull: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const MeshHullScratch lay(n_facets);
    IM_GROW(ctx, ctx->grow(ctx->scratch.mesh, lay.bytes, "mesh.scratch"), -22, "im_mesh_in_hull: allocation failed");
    double* d_facets = lay.facets.at(ctx->scratch.mesh.p);
    IM_HIP(ctx, hipMemcpyAsync(d_facets, h_facets, 4 * sizeof(double) * n_facets, hipMemcpyHostToDevice, s));
    IM_HIP(ctx, hipStreamSynchronize(s));          // the source is host memory of this call
    IM_LAUNCH(ctx, "mesh_in_hull", s, launch(mesh_in_hull_kernel, blocks_of(n_points, 256), 256, 0, s, d_points, n_points, (const double*)d_facets, n_facets, d_inside));
    IM_GUARD_CHECK(ctx, s, "im_mesh_in_hull");
    return 0;
}

int im_mesh_sample_table(im_ctx* ctx, const double* d_vertices, long long n_vertices, const int32_t* d_triangles, long long n_triangles, long long n_samples,
                         double* d_area, long long* d_count_end, long long* h_total, void* stream) {
    IM_CHECK_CTX(ctx);
    const long long V = n_vertices, T = n_triangles, N = n_samples;
    for (long long c : {V, T, N})
        if (const char* why = mesh_bad_count(c)) return ctx->fail(-78, "im_mesh_sample_table: %s", why);
    if (T && (!d_triangles || !d_count_end || (V && !d_vertices))) return ctx->fail(-78, "im_mesh_sample_table: null pointer");
    if (T == 0) {
        if (N > 0) return ctx->fail(-78, "im_mesh_sample_table: no triangle has an area, nothing can be sampled");
        if (h_total) *h_total = 0;
        return 0;
    }
    hipStream_t s = (hipStream_t)stream;
    const MeshSampleScratch lay(T);
    IM_GROW(ctx, ctx->grow(ctx->scratch.mesh, lay.bytes, "mesh.scratch"), -22, "im_mesh_sample_table: allocation failed");
    void* const base = ctx->scratch.mesh.p;
    double* area = lay.area.at(base);
    long long* cum = lay.cum.at(base);
    unsigned long long* amax = lay.amax.at(base);
    long long* total = lay.total.at(base);
    IM_HIP(ctx, hipMemsetAsync(amax, 0, sizeof(unsigned long long), s));
    IM_LAUNCH(ctx, "mesh_area", s, launch(mesh_area_kernel, blocks_of(T, 256), 256, 0, s, d_vertices, V, d_triangles, T, area, amax));
    const MeshCumScan cs{area, amax, T, cum};
    IM_LAUNCH(ctx, "mesh_area_scan", s, launch_scan(cs, T, lay.sums.at(base), total, s));
    long long C = 0;
    IM_HIP(ctx, hipMemcpyAsync(&C, total, sizeof(long long), hipMemcpyDeviceToHost, s));
    IM_HIP(ctx, hipStreamSynchronize(s));          // the refusal below, before an output is written
    if (C <= 0 && N > 0) return ctx->fail(-78, "im_mesh_sample_table: no triangle has an area, nothing can be sampled");
    IM_LAUNCH(ctx, "mesh_allocation", s, launch(mesh_allocation_kernel, blocks_of(T, 256), 256, 0, s, (const long long*)cum, T, C, N, (const double*)area, d_count_end, d_area));
    if (h_total) *h_total = C;
    IM_GUARD_CHECK(ctx, s, "im_mesh_sample_table");
    return 0;
}

int im_mesh_sample(im_ctx* ctx, const double* d_vertices, long long n_vertices, const int32_t* d_triangles, long long n_triangles, const long long* d_count_end,
                   long long n_samples, long long seed, const double* d_vertex_colors, const double* d_vertex_normals, double* d_points, double* d_colors,
                   double* d_normals, int32_t* d_triangle_index, void* stream) {
    IM_CHECK_CTX(ctx);
    const long long V = n_vertices, T = n_triangles, N = n_samples;
    for (long long c : {V, T, N})
        if (const char* why = mesh_bad_count(c)) return ctx->fail(-78, "im_mesh_sample: %s", why);
    if (N == 0) return 0;
    if (V == 0 || T == 0) return ctx->fail(-78, "im_mesh_sample: samples of a mesh without vertices or triangles");
    if (!d_vertices || !d_triangles || !d_count_end || !d_points) return ctx->fail(-78, "im_mesh_sample: null pointer");
    hipStream_t s = (hipStream_t)stream;
    IM_LAUNCH(ctx, "mesh_sample", s, launch(mesh_sample_kernel, blocks_of(N, 256), 256, 0, s, d_vertices, V, d_triangles, T, d_count_end, N, (unsigned long long)seed,
                                            d_vertex_colors, d_vertex_normals, d_points, d_colors, d_normals, d_triangle_index));
    IM_GUARD_CHECK(ctx, s, "im_mesh_sample");
    return 0;
}

}  // extern "C"
