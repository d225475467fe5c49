// Host build of the per-triangle, per-vertex, per-facet and per-sample arithmetic of csrc/mesh.hip (csrc/mesh_tri.h) for
// tests/test_mesh_cpu.py: the very text the kernels compile, behind a stub <hip/hip_runtime.h>. No arithmetic is written here: the loops
// below only visit the items in the kernels' order (a running maximum in facet order, an integer prefix sum, a bisection in the
// allocation table). Also the bytes the entry points ask their context for (csrc/stage_scratch.h).
#include <hip/hip_runtime.h>

#include "mesh_tri.h"
#include "stage_scratch.h"

extern "C" long long mesh_host_max_items() { return im::MESH_MAX_ITEMS; }
extern "C" long long mesh_host_hull_chunk() { return im::MESH_HULL_CHUNK; }
extern "C" long long mesh_host_max_facets() { return im::MESH_MAX_FACETS; }
extern "C" long long mesh_host_nan_key() { return im::MESH_NAN_KEY; }

extern "C" void mesh_host_triangle_keys(const int* tri, long long T, long long* k0, long long* k1) {
    for (long long t = 0; t < T; ++t) im::mesh_tri_keys(tri[3 * t], tri[3 * t + 1], tri[3 * t + 2], k0 + t, k1 + t);
}
extern "C" void mesh_host_vertex_keys(const double* v, long long V, long long* k0, long long* k1, long long* k2) {
    for (long long i = 0; i < V; ++i) {
        long long k[3];
        im::mesh_vertex_keys(v[3 * i], v[3 * i + 1], v[3 * i + 2], i, k);
        k0[i] = k[0]; k1[i] = k[1]; k2[i] = k[2];
    }
}
extern "C" void mesh_host_edge_keys(const int* tri, long long T, long long* key) {
    for (long long j = 0; j < 3 * T; ++j) key[j] = im::mesh_edge_key(tri[3 * (j / 3) + j % 3], tri[3 * (j / 3) + (j % 3 + 1) % 3]);
}
extern "C" void mesh_host_areas(const double* v, long long V, const int* tri, long long T, double* area) {
    for (long long t = 0; t < T; ++t) {
        const int a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
        area[t] = im::mesh_index_ok(a, V) && im::mesh_index_ok(b, V) && im::mesh_index_ok(c, V) ? im::mesh_area(v + 3LL * a, v + 3LL * b, v + 3LL * c) : 0.0;
    }
}
// q, c (inclusive) and count_end [T]; returns C. count_end is 0 when C == 0.
extern "C" long long mesh_host_table(const double* area, long long T, long long N, long long* q, long long* c, long long* count_end) {
    double mx = 0.0;
    for (long long t = 0; t < T; ++t) mx = area[t] > mx ? area[t] : mx;
    long long C = 0;
    for (long long t = 0; t < T; ++t) { q[t] = im::mesh_quantised_area(area[t], mx); C += q[t]; c[t] = C; }
    for (long long t = 0; t < T; ++t) count_end[t] = C > 0 ? im::mesh_allocation(c[t], C, N) : 0;
    return C;
}
extern "C" void mesh_host_hull(const double* p, long long n, const double* facets, long long F, double* value, unsigned char* inside) {
    for (long long i = 0; i < n; ++i) {
        double m = im::mesh_minus_inf();
        for (long long f = 0; f < F; ++f) m = im::mesh_running_max(m, im::mesh_facet_value(facets + 4 * f, p[3 * i], p[3 * i + 1], p[3 * i + 2]));
        value[i] = m;
        inside[i] = im::mesh_inside(m) ? 1 : 0;
    }
}
extern "C" double mesh_host_uniform(unsigned long long seed, unsigned long long i, int k) { return im::mesh_uniform(seed, i, k); }

// the samples 0..N-1 of a mesh with T > 0 triangles and V > 0 vertices; col, nrm, colors, normals may be NULL as in im_mesh_sample
extern "C" void mesh_host_sample(const double* v, long long V, const int* tri, long long T, const long long* count_end, long long N, unsigned long long seed,
                                 const double* col, const double* nrm, double* points, double* colors, double* normals, int* which, double* weights) {
    for (long long i = 0; i < N; ++i) {
        long long lo = 0, hi = T - 1;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (count_end[mid] > i) hi = mid; else lo = mid + 1;
        }
        long long c[3];
        for (int k = 0; k < 3; ++k) { c[k] = tri[3 * lo + k]; c[k] = c[k] < 0 ? 0 : (c[k] > V - 1 ? V - 1 : c[k]); }
        double* w = weights + 3 * i;
        im::mesh_weights(seed, (unsigned long long)i, w);
        im::mesh_blend(w, v + 3 * c[0], v + 3 * c[1], v + 3 * c[2], points + 3 * i);
        if (col && colors) im::mesh_blend(w, col + 3 * c[0], col + 3 * c[1], col + 3 * c[2], colors + 3 * i);
        if (normals) {
            if (nrm) im::mesh_blend(w, nrm + 3 * c[0], nrm + 3 * c[1], nrm + 3 * c[2], normals + 3 * i);
            else im::mesh_unit_normal(v + 3 * c[0], v + 3 * c[1], v + 3 * c[2], normals + 3 * i);
        }
        which[i] = (int)lo;
    }
}

extern "C" unsigned long long carve_mesh_select(long long V, long long T) { return im::MeshSelectScratch(V, T).bytes; }
extern "C" unsigned long long carve_mesh_segment(long long n) { return im::MeshSegmentScratch(n).bytes; }
extern "C" unsigned long long carve_mesh_hull(long long F) { return im::MeshHullScratch(F).bytes; }
extern "C" unsigned long long carve_mesh_sample(long long T) { return im::MeshSampleScratch(T).bytes; }
