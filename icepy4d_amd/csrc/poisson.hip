// Poisson surface reconstruction of an oriented cloud on the dense grid of the finest octree level: what stands in for Open3D's
// `create_from_point_cloud_poisson` in the reference's `post_processing/open3d_fun.py: MeshingPoisson.poisson_meshing` (lines 191-203).
// Open3D's adaptive-octree solver is an un-vendored dependency and is not reproduced: the definition is DESIGN §4, restated in
// tests/poisson_oracle.py and pinned bit for bit. The per-item arithmetic is poisson_node.h. Fields live on the M^3 nodes of a cube of
// R = 2^depth cells per axis, M = R + 1, x fastest; they are the caller's memory.
//
//   poisson_splat_kernel      one thread per sample: its trilinear weights and weight x unit normal at the 8 nodes of its cell, quantised to
//                             2^-32 and added as int64 by integer atomics: the sums depend on no order
//   poisson_fields_kernel     the int64 sums become float64 fields in place
//   poisson_divergence_kernel central differences of V over 2 h on the interior nodes, 0 on the boundary
//   poisson_jacobi_kernel     one damped Jacobi sweep (weight 6/7) of the 7-point Laplacian from one buffer into another
//   poisson_residual_kernel   f - A u on the interior nodes, 0 on the boundary
//   poisson_restrict_kernel   one thread per coarse node: separable full weighting (1/4, 1/2, 1/4) along x, then y, then z
//   poisson_prolong_kernel    one thread per fine node: trilinear interpolation along x, then y, then z, added to u
//   poisson_coarse_kernel     the 3^3 level: its one interior node directly
//   poisson_reduce_kernel     one block per chunk of 1024 items: lane t adds items t, t + 256, t + 512, t + 768, then the lanes halve
//   poisson_mask_kernel       one thread per node: the 7-bit mask of its crossing edges (a node is inside iff chi < iso)
//   scan_*_kernel             (scan.h) over the masks' bit counts: the first vertex of every node; over the triangles of every cell: their
//                             count, and in the extraction their places, in (cell, tetrahedron, triangle) order
//   poisson_vertex_kernel     one thread per node: the vertices of its crossing edges, interpolated from the lower node, in ascending edge key
// The vertex of an edge is found through a dense table: the first vertex of its lower node plus the set bits of the node's mask below the
// edge's direction. Boundary nodes are never written by a sweep and stay 0, so every boundary node carries the same value and the surface
// is closed. float64 throughout, contraction off in poisson_node.h. No launch geometry and no property of the device enters a result.
#include <cmath>

#include "common.h"
#include "ctx.h"
#include "poisson_scratch.h"
#include "poisson_node.h"

namespace im {
namespace {

#include "scan.h"

constexpr int PSN_BX = 64, PSN_BY = 4;       // a block of 256 threads covers 64 x 4 nodes of one z plane

__device__ __forceinline__ bool psn_node(long long M, long long& i, long long& j, long long& k) {
    i = blockIdx.x * (long long)PSN_BX + (threadIdx.x & (PSN_BX - 1));
    j = blockIdx.y * (long long)PSN_BY + threadIdx.x / PSN_BX;
    k = blockIdx.z;
    return i < M && j < M && k < M;
}
__device__ __forceinline__ bool psn_interior(long long M, long long i, long long j, long long k) {
    return i > 0 && j > 0 && k > 0 && i < M - 1 && j < M - 1 && k < M - 1;
}
dim3 psn_grid(long long M) { return dim3((unsigned)blocks_of(M, PSN_BX), (unsigned)blocks_of(M, PSN_BY), (unsigned)M); }

__global__ __launch_bounds__(256) void poisson_splat_kernel(const double* __restrict__ pts, const double* __restrict__ nrm, long long n, double ox, double oy, double oz,
                                                            double h, long long R, unsigned long long* __restrict__ acc) {
    const long long p = blockIdx.x * 256LL + threadIdx.x;
    if (p >= n) return;
    const long long M = R + 1, N = M * M * M;
    long long c[3];
    double t[3], u[3];
    poisson_axis(pts[3 * p], ox, h, R, c, t);
    poisson_axis(pts[3 * p + 1], oy, h, R, c + 1, t + 1);
    poisson_axis(pts[3 * p + 2], oz, h, R, c + 2, t + 2);
    poisson_unit(nrm + 3 * p, u);
    const long long base = poisson_node_index(c[0], c[1], c[2], M);       // c in [0, R - 1]: base + every corner offset < N
#pragma unroll
    for (int corner = 0; corner < 8; ++corner) {
        const long long node = base + poisson_corner_offset(corner, M);
        const double w = poisson_corner_weight(t, corner);
        atomicAdd(acc + node, (unsigned long long)poisson_quantise(w));
#pragma unroll
        for (int a = 0; a < 3; ++a) atomicAdd(acc + (1 + a) * N + node, (unsigned long long)poisson_quantise(w * u[a]));
    }
}

__global__ __launch_bounds__(256) void poisson_fields_kernel(void* __restrict__ fields, long long count) {
    const long long j = blockIdx.x * 256LL + threadIdx.x;
    if (j >= count) return;
    const long long q = static_cast<const long long*>(fields)[j];
    static_cast<double*>(fields)[j] = poisson_unquantise(q);
}

__global__ __launch_bounds__(256) void poisson_divergence_kernel(const double* __restrict__ V, long long M, double two_h, double* __restrict__ rhs) {
    long long i, j, k;
    if (!psn_node(M, i, j, k)) return;
    const long long N = M * M * M, at = poisson_node_index(i, j, k, M);
    double v = 0.0;
    if (psn_interior(M, i, j, k))
        v = poisson_divergence(V[at - 1], V[at + 1], V[N + at - M], V[N + at + M], V[2 * N + at - M * M], V[2 * N + at + M * M], two_h);
    rhs[at] = v;
}

__device__ __forceinline__ double psn_sum6(const double* __restrict__ u, long long at, long long M) {
    return poisson_sum6(u[at - 1], u[at + 1], u[at - M], u[at + M], u[at - M * M], u[at + M * M]);
}

__global__ __launch_bounds__(256) void poisson_jacobi_kernel(const double* __restrict__ u, const double* __restrict__ f, long long M, double h2, double* __restrict__ out) {
    long long i, j, k;
    if (!psn_node(M, i, j, k)) return;
    const long long at = poisson_node_index(i, j, k, M);
    out[at] = psn_interior(M, i, j, k) ? poisson_jacobi(u[at], psn_sum6(u, at, M), f[at], h2) : u[at];
}

__global__ __launch_bounds__(256) void poisson_residual_kernel(const double* __restrict__ u, const double* __restrict__ f, long long M, double h2, double* __restrict__ r) {
    long long i, j, k;
    if (!psn_node(M, i, j, k)) return;
    const long long at = poisson_node_index(i, j, k, M);
    r[at] = psn_interior(M, i, j, k) ? poisson_residual(u[at], psn_sum6(u, at, M), f[at], h2) : 0.0;
}

// coarse node (I, J, K) of Mc = (M - 1) / 2 + 1 per axis sits on fine node (2 I, 2 J, 2 K); an interior one reads fine nodes 2 I - 1 .. 2 I + 1 <= M - 2
__global__ __launch_bounds__(256) void poisson_restrict_kernel(const double* __restrict__ r, long long M, long long Mc, double* __restrict__ fc) {
    long long I, J, K;
    if (!psn_node(Mc, I, J, K)) return;
    double v = 0.0;
    if (psn_interior(Mc, I, J, K)) {
        double z[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double y[3];
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const long long at = poisson_node_index(2 * I, 2 * J + b - 1, 2 * K + c - 1, M);
                y[b] = poisson_full_weight(r[at - 1], r[at], r[at + 1]);
            }
            z[c] = poisson_full_weight(y[0], y[1], y[2]);
        }
        v = poisson_full_weight(z[0], z[1], z[2]);
    }
    fc[poisson_node_index(I, J, K, Mc)] = v;
}

// fine node i lies on coarse node i / 2 (even) or between coarse nodes (i - 1) / 2 and (i + 1) / 2 <= Mc - 1 (odd)
__global__ __launch_bounds__(256) void poisson_prolong_kernel(const double* __restrict__ e, long long Mc, long long M, double* __restrict__ u) {
#pragma clang fp contract(off)
    long long i, j, k;
    if (!psn_node(M, i, j, k) || !psn_interior(M, i, j, k)) return;
    const int nx = (int)(i & 1), ny = (int)(j & 1), nz = (int)(k & 1);
    const long long i0 = i >> 1, j0 = j >> 1, k0 = k >> 1;
    double z[2];
    for (int c = 0; c <= nz; ++c) {
        double y[2];
        for (int b = 0; b <= ny; ++b) {
            const long long at = poisson_node_index(i0, j0 + b, k0 + c, Mc);
            y[b] = nx ? poisson_midpoint(e[at], e[at + 1]) : e[at];
        }
        z[c] = ny ? poisson_midpoint(y[0], y[1]) : y[0];
    }
    const double v = nz ? poisson_midpoint(z[0], z[1]) : z[0];
    const long long at = poisson_node_index(i, j, k, M);
    u[at] = u[at] + v;
}

__global__ __launch_bounds__(64) void poisson_coarse_kernel(const double* __restrict__ f, double h2, double* __restrict__ u) {
    if (threadIdx.x < 27) u[threadIdx.x] = threadIdx.x == 13 ? poisson_coarse(f[13], h2) : 0.0;
}

__global__ __launch_bounds__(256) void poisson_reduce_kernel(const double* __restrict__ a, const double* __restrict__ b, long long n, double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double s[256];
    const long long base = blockIdx.x * (long long)POISSON_CHUNK;
    double v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long long at = base + q * 256 + threadIdx.x;
        v[q] = at < n ? (b ? a[at] * b[at] : a[at]) : 0.0;
    }
    s[threadIdx.x] = ((v[0] + v[1]) + v[2]) + v[3];
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if ((int)threadIdx.x < st) s[threadIdx.x] = s[threadIdx.x] + s[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = s[0];
}

__global__ __launch_bounds__(256) void poisson_mask_kernel(const double* __restrict__ chi, double iso, long long M, unsigned char* __restrict__ mask) {
    long long i, j, k;
    if (!psn_node(M, i, j, k)) return;
    const long long at = poisson_node_index(i, j, k, M);
    const bool in = poisson_inside(chi[at], iso);
    unsigned m = 0;
#pragma unroll
    for (int d = 1; d < 8; ++d) {
        if (i + (d & 1) < M && j + ((d >> 1) & 1) < M && k + ((d >> 2) & 1) < M)
            m |= (poisson_inside(chi[at + poisson_corner_offset(d, M)], iso) != in ? 1u : 0u) << (d - 1);
    }
    mask[at] = (unsigned char)m;
}

struct PoissonNodeScan {      // base [node] = the vertices on the edges of all nodes before it
    const unsigned char* mask; long long N; int* base;
    __device__ long long count(long long j) const { return j < N ? poisson_popcount7(mask[j]) : 0; }
    __device__ void write(long long j, long long pos) const { if (j < N) base[j] = (int)pos; }
};

// the inside bits of the 8 corners of cell j (i + R (j + R k))
__device__ __forceinline__ unsigned psn_cell_bits(const double* __restrict__ chi, double iso, long long cell, long long R, long long& node) {
    const long long M = R + 1, i = cell % R, j = (cell / R) % R, k = cell / (R * R);
    node = poisson_node_index(i, j, k, M);
    unsigned bits = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) bits |= (poisson_inside(chi[node + poisson_corner_offset(c, M)], iso) ? 1u : 0u) << c;
    return bits;
}
__device__ __forceinline__ unsigned psn_tet_bits(unsigned cell_bits, const int* c) {
    return ((cell_bits >> c[0]) & 1u) | (((cell_bits >> c[1]) & 1u) << 1) | (((cell_bits >> c[2]) & 1u) << 2) | (((cell_bits >> c[3]) & 1u) << 3);
}

struct PoissonCellScan {      // the triangles of the cells; with `tri`, written at their places (those below n_tri)
    const double* chi; double iso; long long R; const unsigned char* mask; const int* base; long long n_tri; int* tri;
    __device__ long long count(long long cell) const {
        if (cell >= R * R * R) return 0;
        long long node;
        const unsigned bits = psn_cell_bits(chi, iso, cell, R, node);
        if (bits == 0 || bits == 255) return 0;
        int n = 0;
        for (int t = 0; t < 6; ++t) {
            int c[4];
            poisson_tet_corners(t, c);
            n += poisson_tet_triangle_count(psn_tet_bits(bits, c));
        }
        return n;
    }
    __device__ void write(long long cell, long long pos) const {
        if (!tri || cell >= R * R * R) return;
        long long node;
        const unsigned bits = psn_cell_bits(chi, iso, cell, R, node);
        if (bits == 0 || bits == 255) return;
        const long long M = R + 1;
        for (int t = 0; t < 6; ++t) {
            int c[4];
            poisson_tet_corners(t, c);
            PoissonTri tr[2];
            const int nt = poisson_tet_triangles(c, psn_tet_bits(bits, c), tr);
            for (int q = 0; q < nt; ++q, ++pos) {
                if (pos >= n_tri) return;
                for (int e = 0; e < 3; ++e) {
                    const int lo = c[tr[q].lo[e]], d = c[tr[q].hi[e]] ^ lo;
                    const long long at = node + poisson_corner_offset(lo, M);
                    tri[3 * pos + e] = base[at] + poisson_popcount7((unsigned)mask[at] & ((1u << (d - 1)) - 1u));
                }
            }
        }
    }
};

__global__ __launch_bounds__(256) void poisson_vertex_kernel(const double* __restrict__ chi, const double* __restrict__ W, double iso, long long M, double ox, double oy,
                                                             double oz, double h, const unsigned char* __restrict__ mask, const int* __restrict__ base,
                                                             long long n_vert, double* __restrict__ vert, double* __restrict__ weight) {
    long long i, j, k;
    if (!psn_node(M, i, j, k)) return;
    const long long at = poisson_node_index(i, j, k, M);
    const unsigned m = mask[at];
    if (!m) return;
    long long pos = base[at];
    const double fa = chi[at], wa = W[at];
    for (int d = 1; d < 8; ++d) {
        if (!((m >> (d - 1)) & 1u)) continue;
        if (pos < 0 || pos >= n_vert) return;
        // a set bit of a mask that the census wrote has its upper node inside the grid; one that it did not write is not followed outside it
        if (i + (d & 1) >= M || j + ((d >> 1) & 1) >= M || k + ((d >> 2) & 1) >= M) return;
        const long long up = at + poisson_corner_offset(d, M);
        const double t = poisson_edge_t(fa, chi[up], iso);
        vert[3 * pos] = poisson_edge_position(ox, i, d & 1, h, t);
        vert[3 * pos + 1] = poisson_edge_position(oy, j, (d >> 1) & 1, h, t);
        vert[3 * pos + 2] = poisson_edge_position(oz, k, (d >> 2) & 1, h, t);
        weight[pos] = poisson_edge_blend(wa, W[up], t);
        ++pos;
    }
}

bool psn_bad_depth(int depth) { return depth < POISSON_MIN_DEPTH || depth > POISSON_MAX_DEPTH; }

}  // namespace
}  // namespace im

using namespace im;

extern "C" {

int im_poisson_max_depth(void) { return POISSON_MAX_DEPTH; }
int im_poisson_max_points(void) { return (int)POISSON_MAX_POINTS; }

int im_poisson_splat(im_ctx* ctx, const double* d_points, const double* d_normals, long long n_points, const double* h_grid, int depth, double* d_fields, void* stream) {
    IM_CHECK_CTX(ctx);
    if (psn_bad_depth(depth)) return ctx->fail(-80, "im_poisson_splat: depth outside [2, 9]");
    if (n_points < 0 || n_points > POISSON_MAX_POINTS) return ctx->fail(-80, "im_poisson_splat: a negative count or more than 2^26 points: split the call");
    if (!h_grid || !d_fields || (n_points && (!d_points || !d_normals))) return ctx->fail(-80, "im_poisson_splat: null pointer");
    if (!(h_grid[3] > 0.0) || !std::isfinite(h_grid[0]) || !std::isfinite(h_grid[1]) || !std::isfinite(h_grid[2]) || !std::isfinite(h_grid[3]))
        return ctx->fail(-80, "im_poisson_splat: the grid is not finite or its cell size is not positive");
    if (n_points == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const long long R = 1LL << depth, N = poisson_node_count(depth);
    IM_HIP(ctx, hipMemsetAsync(d_fields, 0, (size_t)poisson_byte_offset(4 * N, sizeof(double)), s));
    IM_LAUNCH(ctx, "poisson_splat", s, launch(poisson_splat_kernel, blocks_of(n_points, 256), 256, 0, s, d_points, d_normals, n_points, h_grid[0], h_grid[1], h_grid[2],
                                              h_grid[3], R, reinterpret_cast<unsigned long long*>(d_fields)));
    IM_LAUNCH(ctx, "poisson_fields", s, launch(poisson_fields_kernel, blocks_of(4 * N, 256), 256, 0, s, (void*)d_fields, 4 * N));
    IM_GUARD_CHECK(ctx, s, "im_poisson_splat");
    return 0;
}

int im_poisson_divergence(im_ctx* ctx, const double* d_vectors, int depth, double h, double* d_rhs, void* stream) {
    IM_CHECK_CTX(ctx);
    if (psn_bad_depth(depth)) return ctx->fail(-80, "im_poisson_divergence: depth outside [2, 9]");
    if (!d_vectors || !d_rhs) return ctx->fail(-80, "im_poisson_divergence: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const long long M = poisson_axis_nodes(depth);
    IM_LAUNCH(ctx, "poisson_divergence", s, launch(poisson_divergence_kernel, psn_grid(M), 256, 0, s, d_vectors, M, 2.0 * h, d_rhs));
    IM_GUARD_CHECK(ctx, s, "im_poisson_divergence");
    return 0;
}

int im_poisson_jacobi(im_ctx* ctx, const double* d_u, const double* d_f, int depth, double h2, double* d_out, void* stream) {
    IM_CHECK_CTX(ctx);
    if (psn_bad_depth(depth)) return ctx->fail(-80, "im_poisson_jacobi: depth outside [2, 9]");
    if (!d_u || !d_f || !d_out || d_u == d_out) return ctx->fail(-80, "im_poisson_jacobi: null pointer, or a sweep in place");
    hipStream_t s = (hipStream_t)stream;
    const long long M = poisson_axis_nodes(depth);
    IM_LAUNCH(ctx, "poisson_jacobi", s, launch(poisson_jacobi_kernel, psn_grid(M), 256, 0, s, d_u, d_f, M, h2, d_out));
    IM_GUARD_CHECK(ctx, s, "im_poisson_jacobi");
    return 0;
}

int im_poisson_restrict(im_ctx* ctx, const double* d_u, const double* d_f, int depth, double h2, double* d_residual, double* d_coarse_f, void* stream) {
    IM_CHECK_CTX(ctx);
    if (psn_bad_depth(depth)) return ctx->fail(-80, "im_poisson_restrict: depth outside [2, 9]");
    if (!d_u || !d_f || !d_residual || !d_coarse_f || d_residual == d_u || d_residual == d_f) return ctx->fail(-80, "im_poisson_restrict: null pointer, or the residual over u or f");
    hipStream_t s = (hipStream_t)stream;
    const long long M = poisson_axis_nodes(depth), Mc = poisson_axis_nodes(depth - 1);
    IM_LAUNCH(ctx, "poisson_residual", s, launch(poisson_residual_kernel, psn_grid(M), 256, 0, s, d_u, d_f, M, h2, d_residual));
    IM_LAUNCH(ctx, "poisson_restrict", s, launch(poisson_restrict_kernel, psn_grid(Mc), 256, 0, s, (const double*)d_residual, M, Mc, d_coarse_f));
    IM_GUARD_CHECK(ctx, s, "im_poisson_restrict");
    return 0;
}

int im_poisson_prolong(im_ctx* ctx, const double* d_coarse_e, int depth, double* d_u, void* stream) {
    IM_CHECK_CTX(ctx);
    if (psn_bad_depth(depth)) return ctx->fail(-80, "im_poisson_prolong: depth outside [2, 9]");
    if (!d_coarse_e || !d_u) return ctx->fail(-80, "im_poisson_prolong: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const long long M = poisson_axis_nodes(depth), Mc = poisson_axis_nodes(depth - 1);
    IM_LAUNCH(ctx, "poisson_prolong", s, launch(poisson_prolong_kernel, psn_grid(M), 256, 0, s, d_coarse_e, Mc, M, d_u));
    IM_GUARD_CHECK(ctx, s, "im_poisson_prolong");
    return 0;
}

int im_poisson_coarse(im_ctx* ctx, const double* d_f, double h2, double* d_u, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_f || !d_u) return ctx->fail(-80, "im_poisson_coarse: null pointer");
    hipStream_t s = (hipStream_t)stream;
    IM_LAUNCH(ctx, "poisson_coarse", s, launch(poisson_coarse_kernel, 1, 64, 0, s, d_f, h2, d_u));
    IM_GUARD_CHECK(ctx, s, "im_poisson_coarse");
    return 0;
}

int im_poisson_reduce(im_ctx* ctx, const double* d_a, const double* d_b, long long n, double* d_out, void* stream) {
    IM_CHECK_CTX(ctx);
    if (n < 0 || n > 4 * poisson_node_count(POISSON_MAX_DEPTH)) return ctx->fail(-80, "im_poisson_reduce: a negative count or more items than four fields of depth 9");
    if (n == 0) return 0;
    if (!d_a || !d_out) return ctx->fail(-80, "im_poisson_reduce: null pointer");
    hipStream_t s = (hipStream_t)stream;
    IM_LAUNCH(ctx, "poisson_reduce", s, launch(poisson_reduce_kernel, blocks_of(n, POISSON_CHUNK), 256, 0, s, d_a, d_b, n, d_out));
    IM_GUARD_CHECK(ctx, s, "im_poisson_reduce");
    return 0;
}

int im_poisson_census(im_ctx* ctx, const double* d_chi, double iso, int depth, unsigned char* d_mask, int32_t* d_base, long long* d_counts, void* stream) {
    IM_CHECK_CTX(ctx);
    if (psn_bad_depth(depth)) return ctx->fail(-80, "im_poisson_census: depth outside [2, 9]");
    if (!d_chi || !d_mask || !d_base || !d_counts) return ctx->fail(-80, "im_poisson_census: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const long long R = 1LL << depth, M = R + 1, N = M * M * M;
    const PoissonScanScratch lay(N);
    IM_GROW(ctx, ctx->grow(ctx->scratch.poisson, lay.bytes, "poisson.scratch"), -22, "im_poisson_census: allocation failed");
    void* const sb = ctx->scratch.poisson.p;
    IM_LAUNCH(ctx, "poisson_mask", s, launch(poisson_mask_kernel, psn_grid(M), 256, 0, s, d_chi, iso, M, d_mask));
    const PoissonNodeScan ns{d_mask, N, d_base};
    IM_LAUNCH(ctx, "poisson_node_scan", s, launch_scan(ns, N, lay.sums.at(sb), d_counts, s));
    const PoissonCellScan cs{d_chi, iso, R, d_mask, d_base, 0, nullptr};
    IM_LAUNCH(ctx, "poisson_cell_count", s, launch_scan(cs, R * R * R, lay.sums.at(sb), d_counts + 1, s));
    IM_GUARD_CHECK(ctx, s, "im_poisson_census");
    return 0;
}

int im_poisson_extract(im_ctx* ctx, const double* d_chi, const double* d_weight_field, double iso, int depth, const double* h_grid, const unsigned char* d_mask,
                       const int32_t* d_base, long long n_vertices, long long n_triangles, double* d_vertices, double* d_weights, int32_t* d_triangles, void* stream) {
    IM_CHECK_CTX(ctx);
    if (psn_bad_depth(depth)) return ctx->fail(-80, "im_poisson_extract: depth outside [2, 9]");
    if (n_vertices < 0 || n_triangles < 0 || n_vertices > POISSON_MAX_POINTS || n_triangles > POISSON_MAX_POINTS)
        return ctx->fail(-80, "im_poisson_extract: a negative count or more than 2^26 vertices or triangles: reconstruct at a lower depth");
    if (!h_grid || !d_chi || !d_weight_field || !d_mask || !d_base || (n_vertices && (!d_vertices || !d_weights)) || (n_triangles && !d_triangles))
        return ctx->fail(-80, "im_poisson_extract: null pointer");
    if (n_vertices == 0 && n_triangles == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const long long R = 1LL << depth, M = R + 1, N = M * M * M;
    const PoissonScanScratch lay(N);
    IM_GROW(ctx, ctx->grow(ctx->scratch.poisson, lay.bytes, "poisson.scratch"), -22, "im_poisson_extract: allocation failed");
    void* const sb = ctx->scratch.poisson.p;
    if (n_vertices)
        IM_LAUNCH(ctx, "poisson_vertex", s, launch(poisson_vertex_kernel, psn_grid(M), 256, 0, s, d_chi, d_weight_field, iso, M, h_grid[0], h_grid[1], h_grid[2], h_grid[3],
                                                   d_mask, d_base, n_vertices, d_vertices, d_weights));
    if (n_triangles) {
        const PoissonCellScan cs{d_chi, iso, R, d_mask, d_base, n_triangles, d_triangles};
        IM_LAUNCH(ctx, "poisson_triangles", s, launch_scan(cs, R * R * R, lay.sums.at(sb), lay.total.at(sb), s));
    }
    IM_GUARD_CHECK(ctx, s, "im_poisson_extract");
    return 0;
}

}  // extern "C"
