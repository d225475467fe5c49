// The arithmetic of one triangle, one vertex, one facet test and one sample of csrc/mesh.hip: the mesh filters, the convex-hull crop and
// the uniform sampling of the reference's `post_processing/open3d_fun.py: MeshingPoisson` (definition in DESIGN §4). IEEE float64 with
// contraction off, a header of its own without the context or any launch code, like voxel_cell.h: a host program compiles the very text
// the kernels compile (tests/mesh_host_harness.cpp, through a stub <hip/hip_runtime.h>) and is compared with the numpy restatement
// (tests/mesh_oracle.py) bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#define MESH_FN __host__ __device__ __forceinline__
#else
#define MESH_FN inline
#endif

namespace im {
namespace {

constexpr long long MESH_MAX_ITEMS = 1LL << 26;      // vertices, triangles or samples of one call (3 T edge items: 3 * 2^26)
constexpr int MESH_HULL_CHUNK = 512;                 // facets staged in LDS at a time: 512 x 4 doubles = 16 KiB
constexpr int MESH_MAX_FACETS = 1 << 22;             // facets of one hull
constexpr long long MESH_NAN_KEY = 0x7ff8000000000000LL;   // first key of a vertex with a NaN coordinate; its second key is its index

MESH_FN bool mesh_index_ok(int i, long long V) { return i >= 0 && i < V; }

// ---- duplicate triangles: the index triple rotated to smallest-index-first (orientation kept), as two keys a and b << 32 | c ---------------
MESH_FN void mesh_tri_canonical(int i0, int i1, int i2, int* c) {
    if (i0 <= i1 && i0 <= i2) { c[0] = i0; c[1] = i1; c[2] = i2; }
    else if (i1 <= i0 && i1 <= i2) { c[0] = i1; c[1] = i2; c[2] = i0; }
    else { c[0] = i2; c[1] = i0; c[2] = i1; }
}
MESH_FN long long mesh_pair_key(int hi, int lo) { return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo); }
MESH_FN void mesh_tri_keys(int i0, int i1, int i2, long long* k0, long long* k1) {
    int c[3];
    mesh_tri_canonical(i0, i1, i2, c);
    *k0 = c[0];
    *k1 = mesh_pair_key(c[1], c[2]);
}
// the undirected edge (u, v): min << 32 | max
MESH_FN long long mesh_edge_key(int u, int v) { return u <= v ? mesh_pair_key(u, v) : mesh_pair_key(v, u); }

// ---- duplicate vertices: the bits of x, y, z with -0.0 as +0.0; a vertex with a NaN coordinate gets (MESH_NAN_KEY, its index, 0) and so
// equals nothing (no vertex without a NaN has a NaN's bits as its first key)
MESH_FN long long mesh_double_bits(double v) {
    if (v == 0.0) v = 0.0;                                   // -0.0 == 0.0: both become +0.0
    long long b;
    __builtin_memcpy(&b, &v, sizeof(b));
    return b;
}
MESH_FN void mesh_vertex_keys(double x, double y, double z, long long index, long long* k) {
    if (x != x || y != y || z != z) { k[0] = MESH_NAN_KEY; k[1] = index; k[2] = 0; return; }
    k[0] = mesh_double_bits(x); k[1] = mesh_double_bits(y); k[2] = mesh_double_bits(z);
}

// ---- the area and the unit normal of a triangle -------------------------------------------------------------------------------------------
MESH_FN void mesh_cross(const double* v0, const double* v1, const double* v2, double* n) {
#pragma clang fp contract(off)
    const double ax = v1[0] - v0[0], ay = v1[1] - v0[1], az = v1[2] - v0[2];
    const double bx = v2[0] - v0[0], by = v2[1] - v0[1], bz = v2[2] - v0[2];
    n[0] = ay * bz - az * by;
    n[1] = az * bx - ax * bz;
    n[2] = ax * by - ay * bx;
}
MESH_FN double mesh_norm(const double* n) {
#pragma clang fp contract(off)
    return __builtin_sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
}
// 0.5 |(v1 - v0) x (v2 - v0)|; a non-finite area counts as 0
MESH_FN double mesh_area(const double* v0, const double* v1, const double* v2) {
#pragma clang fp contract(off)
    double n[3];
    mesh_cross(v0, v1, v2, n);
    const double a = 0.5 * mesh_norm(n);
    return __builtin_isfinite(a) ? a : 0.0;
}
// floor(area / max_area * 2^32), 0 when no triangle has an area
MESH_FN long long mesh_quantised_area(double area, double max_area) {
#pragma clang fp contract(off)
    if (!(max_area > 0.0)) return 0;
    return (long long)__builtin_floor(area / max_area * 4294967296.0);
}
// samples in front of the end of a triangle whose inclusive cumulative quantised area is c, of C in all: rint(c / C * N)
MESH_FN long long mesh_allocation(long long c, long long C, long long N) {
#pragma clang fp contract(off)
    return (long long)__builtin_rint((double)c / (double)C * (double)N);
}

// ---- point in hull: the running maximum of n . p + d over the facets; a NaN sticks, so the point is then outside ---------------------------
MESH_FN double mesh_facet_value(const double* f, double x, double y, double z) {
#pragma clang fp contract(off)
    return ((f[0] * x + f[1] * y) + f[2] * z) + f[3];
}
MESH_FN double mesh_running_max(double m, double v) { return (v > m || v != v) ? v : m; }
MESH_FN double mesh_minus_inf() { return -__builtin_inf(); }
MESH_FN bool mesh_inside(double m) { return m <= 0.0; }

// ---- the generator: splitmix64's finaliser over seed + counter * golden ratio; draw k of sample i has counter 2 i + 1 + k ---------------
MESH_FN unsigned long long mesh_mix64(unsigned long long z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ULL;
    z ^= z >> 27; z *= 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return z;
}
MESH_FN double mesh_uniform(unsigned long long seed, unsigned long long i, int k) {
    const unsigned long long z = mesh_mix64(seed + (2ULL * i + 1ULL + (unsigned long long)k) * 0x9E3779B97F4A7C15ULL);
    return (double)(z >> 11) * 0x1.0p-53;
}
// the barycentric weights of sample i: s = sqrt(r1), (1 - s, s (1 - r2), s r2)
MESH_FN void mesh_weights(unsigned long long seed, unsigned long long i, double* w) {
#pragma clang fp contract(off)
    const double r1 = mesh_uniform(seed, i, 0), r2 = mesh_uniform(seed, i, 1);
    const double s = __builtin_sqrt(r1);
    w[0] = 1.0 - s; w[1] = s * (1.0 - r2); w[2] = s * r2;
}
// a v0 + b v1 + c v2 per column, summed left to right
MESH_FN void mesh_blend(const double* w, const double* v0, const double* v1, const double* v2, double* out) {
#pragma clang fp contract(off)
    for (int a = 0; a < 3; ++a) out[a] = (w[0] * v0[a] + w[1] * v1[a]) + w[2] * v2[a];
}
// the unit normal of a triangle: cross / |cross|
MESH_FN void mesh_unit_normal(const double* v0, const double* v1, const double* v2, double* out) {
#pragma clang fp contract(off)
    double n[3];
    mesh_cross(v0, v1, v2, n);
    const double len = mesh_norm(n);
    for (int a = 0; a < 3; ++a) out[a] = n[a] / len;
}

}  // namespace
}  // namespace im
