// The arithmetic of one sample, one node, one edge and one tetrahedron of csrc/poisson.hip: a Poisson surface reconstruction on the dense
// grid of the finest octree level, which stands in for the solve of the reference's `post_processing/open3d_fun.py: MeshingPoisson`
// (definition in DESIGN §4). IEEE float64 with contraction off, a header of its own without the context or any launch code, like
// mesh_tri.h: a host program compiles the very text the kernels compile (tests/poisson_host_harness.cpp, through a stub
// <hip/hip_runtime.h>) and is compared with the numpy restatement (tests/poisson_oracle.py) bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#define PSN_FN __host__ __device__ __forceinline__
#else
#define PSN_FN inline
#endif

namespace im {
namespace {

constexpr int POISSON_MIN_DEPTH = 2;                 // 5 nodes per axis: one smoothed level above the direct solve
constexpr int POISSON_MAX_DEPTH = 9;                 // 513 nodes per axis: edge keys reach 2^30 and byte offsets of the fields 2^32, every key and offset is 64-bit
constexpr long long POISSON_MAX_POINTS = 1LL << 26;  // samples of one splat; vertices or triangles of one extraction
constexpr double POISSON_QUANTUM = 4294967296.0;     // addends are quantised to 2^-32: a weight is <= 1, so 2^26 of them stay below 2^58
constexpr double POISSON_UNQUANTUM = 0x1.0p-32;
constexpr int POISSON_CHUNK = 1024;                  // nodes of one partial sum of the iso reduction
constexpr double POISSON_OMEGA = 6.0 / 7.0;          // the weight of the damped Jacobi sweep

PSN_FN long long poisson_axis_nodes(int depth) { return (1LL << depth) + 1; }
PSN_FN long long poisson_node_count(int depth) { const long long M = poisson_axis_nodes(depth); return M * M * M; }
PSN_FN long long poisson_node_index(long long i, long long j, long long k, long long M) { return (k * M + j) * M + i; }
// the edge from `node` towards direction d = 1..7 (bit 0 = +x, bit 1 = +y, bit 2 = +z)
PSN_FN long long poisson_edge_key(long long node, int d) { return node * 8 + d; }
PSN_FN long long poisson_byte_offset(long long item, long long bytes_per_item) { return item * bytes_per_item; }
PSN_FN long long poisson_corner_offset(int corner, long long M) { return (long long)(corner & 1) + ((corner >> 1) & 1) * M + ((corner >> 2) & 1) * M * M; }

// ---- the splat: the cell of a sample along one axis, clamped to [0, R - 1], and its fraction in it, clamped to [0, 1] -----------------------
PSN_FN void poisson_axis(double p, double o, double h, long long R, long long* c, double* t) {
#pragma clang fp contract(off)
    const double u = (p - o) / h;
    double f = __builtin_floor(u);
    f = !(f >= 0.0) ? 0.0 : (f > (double)(R - 1) ? (double)(R - 1) : f);
    double r = u - f;
    r = !(r >= 0.0) ? 0.0 : (r > 1.0 ? 1.0 : r);
    *c = (long long)f;
    *t = r;
}
PSN_FN void poisson_unit(const double* n, double* u) {
#pragma clang fp contract(off)
    const double len = __builtin_sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    for (int a = 0; a < 3; ++a) u[a] = n[a] / len;
}
// the trilinear weight of cube corner `corner` (bit 0 = x, bit 1 = y, bit 2 = z)
PSN_FN double poisson_corner_weight(const double* t, int corner) {
#pragma clang fp contract(off)
    const double wx = (corner & 1) ? t[0] : 1.0 - t[0];
    const double wy = (corner & 2) ? t[1] : 1.0 - t[1];
    const double wz = (corner & 4) ? t[2] : 1.0 - t[2];
    return (wx * wy) * wz;
}
// rint(v * 2^32) as int64; a NaN adds nothing
PSN_FN long long poisson_quantise(double v) {
#pragma clang fp contract(off)
    const double r = __builtin_rint(v * POISSON_QUANTUM);
    return r == r ? (long long)r : 0;
}
PSN_FN double poisson_unquantise(long long q) {
#pragma clang fp contract(off)
    return (double)q * POISSON_UNQUANTUM;
}

// ---- the right-hand side and the multigrid stencils ----------------------------------------------------------------------------------------
PSN_FN double poisson_divergence(double xm, double xp, double ym, double yp, double zm, double zp, double two_h) {
#pragma clang fp contract(off)
    return (((xp - xm) + (yp - ym)) + (zp - zm)) / two_h;
}
PSN_FN double poisson_sum6(double xm, double xp, double ym, double yp, double zm, double zp) {
#pragma clang fp contract(off)
    return ((((xm + xp) + ym) + yp) + zm) + zp;
}
PSN_FN double poisson_jacobi(double u, double s6, double f, double h2) {
#pragma clang fp contract(off)
    const double j = (s6 - h2 * f) / 6.0;
    return u + POISSON_OMEGA * (j - u);
}
PSN_FN double poisson_residual(double u, double s6, double f, double h2) {
#pragma clang fp contract(off)
    return f - (s6 - 6.0 * u) / h2;
}
PSN_FN double poisson_full_weight(double a, double b, double c) {
#pragma clang fp contract(off)
    return (0.25 * a + 0.5 * b) + 0.25 * c;
}
PSN_FN double poisson_midpoint(double a, double b) {
#pragma clang fp contract(off)
    return 0.5 * (a + b);
}
// the one interior node of the 3^3 level: -6 u / h^2 = f
PSN_FN double poisson_coarse(double f, double h2) {
#pragma clang fp contract(off)
    return (h2 * f) / -6.0;
}

// ---- an edge crossing: the parameter from the lower node, the position along one axis and the interpolated weight --------------------------
PSN_FN bool poisson_inside(double chi, double iso) { return chi < iso; }
PSN_FN double poisson_edge_t(double fa, double fb, double iso) {
#pragma clang fp contract(off)
    return (iso - fa) / (fb - fa);
}
PSN_FN double poisson_edge_position(double o, long long ia, int step, double h, double t) {
#pragma clang fp contract(off)
    const double pa = o + (double)ia * h;
    return pa + t * ((double)step * h);
}
PSN_FN double poisson_edge_blend(double wa, double wb, double t) {
#pragma clang fp contract(off)
    return wa + t * (wb - wa);
}

// ---- the six Kuhn tetrahedra of a cell and their triangles, by rule ------------------------------------------------------------------------
// Tetrahedron t = 0..5 stands for the order (a0, a1, a2) of the axes, lexicographic in t: its corners are 0, e_a0, e_a0 + e_a1, 7 as
// cube-corner bit masks. Every edge runs from a corner to one that contains it, so its direction is the difference of the two masks.
PSN_FN void poisson_tet_corners(int t, int* c) {
    const int a0 = t >> 1, r0 = a0 == 0 ? 1 : 0, r1 = a0 == 2 ? 1 : 2;
    const int a1 = (t & 1) ? r1 : r0;
    c[0] = 0; c[1] = 1 << a0; c[2] = c[1] | (1 << a1); c[3] = 7;
}
// det (a - o, b - o, c - o) of four cube corners, in integers
PSN_FN int poisson_det(int a, int b, int c, int o) {
    int m[3][3];
    const int v[3] = {a, b, c};
    for (int r = 0; r < 3; ++r)
        for (int x = 0; x < 3; ++x) m[r][x] = ((v[r] >> x) & 1) - ((o >> x) & 1);
    return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
           m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}
struct PoissonTri { int lo[3], hi[3]; };     // the three edges of a triangle as (lower, upper) corners of the tetrahedron, positions 0..3
PSN_FN void poisson_tri_edge(PoissonTri* tr, int e, int p, int q) { tr->lo[e] = p < q ? p : q; tr->hi[e] = p < q ? q : p; }
PSN_FN int poisson_tet_triangle_count(unsigned inside) {
    const int n = (int)((inside & 1) + ((inside >> 1) & 1) + ((inside >> 2) & 1) + ((inside >> 3) & 1));
    return n == 0 || n == 4 ? 0 : (n == 2 ? 2 : 1);
}
// The triangles of a tetrahedron with corners c [4] whose corner p is inside iff bit p of `inside`. One corner against three: the
// triangle on the edges to the three, in their order. Two against two (a1 < a2 inside, b1 < b2 outside): the quad on the edges (a1, b1),
// (a1, b2), (a2, b2), (a2, b1), split along its first diagonal. The last two corners of a triangle are swapped where the sign of the
// integer determinant says that its normal would point to the inside.
PSN_FN int poisson_tet_triangles(const int* c, unsigned inside, PoissonTri* out) {
    int in[4], ou[4], nin = 0, nou = 0;
    for (int p = 0; p < 4; ++p) {
        if ((inside >> p) & 1) in[nin++] = p; else ou[nou++] = p;
    }
    if (nin == 0 || nin == 4) return 0;
    if (nin == 2) {
        const bool flip = poisson_det(c[in[1]], c[ou[0]], c[ou[1]], c[in[0]]) < 0;
        const int q[4][2] = {{in[0], ou[0]}, {in[0], ou[1]}, {in[1], ou[1]}, {in[1], ou[0]}};
        for (int k = 0; k < 2; ++k) {
            const int m = flip ? 2 + k : 1 + k, l = flip ? 1 + k : 2 + k;
            poisson_tri_edge(out + k, 0, q[0][0], q[0][1]);
            poisson_tri_edge(out + k, 1, q[m][0], q[m][1]);
            poisson_tri_edge(out + k, 2, q[l][0], q[l][1]);
        }
        return 2;
    }
    const bool lone_inside = nin == 1;
    const int a = lone_inside ? in[0] : ou[0];
    const int* b = lone_inside ? ou : in;
    const bool flip = (poisson_det(c[b[0]], c[b[1]], c[b[2]], c[a]) > 0) != lone_inside;
    poisson_tri_edge(out, 0, a, b[0]);
    poisson_tri_edge(out, 1, a, b[flip ? 2 : 1]);
    poisson_tri_edge(out, 2, a, b[flip ? 1 : 2]);
    return 1;
}

// ---- the crossing edges of a node are a 7-bit mask (bit d - 1 = direction d); the rank of an edge is the set bits below it ---------------
PSN_FN int poisson_popcount7(unsigned m) {
    m &= 127u;
    m = (m & 0x55u) + ((m >> 1) & 0x55u);
    m = (m & 0x33u) + ((m >> 2) & 0x33u);
    return (int)((m + (m >> 4)) & 0x0fu);
}

}  // namespace
}  // namespace im
