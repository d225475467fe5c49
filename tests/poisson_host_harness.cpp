// Host build of the per-sample, per-node, per-edge and per-tetrahedron arithmetic of csrc/poisson.hip (csrc/poisson_node.h) for
// tests/test_poisson_cpu.py: the very text the kernels compile, behind a stub <hip/hip_runtime.h>. A stand-alone program, so that it also
// runs under the address and undefined-behaviour sanitizers: `poisson_host_harness DIR` reads the arrays the numpy restatement
// (tests/poisson_oracle.py) dumped into DIR as raw little-endian files, recomputes them and compares bit for bit. No arithmetic is
// written here: the loops below only visit the items in the kernels' order. It also checks the key and offset arithmetic at the corner
// of a depth-9 grid, which no small device case reaches, and the bytes the entry points ask their context for (csrc/poisson_scratch.h).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "poisson_node.h"
#include "poisson_scratch.h"

using namespace im;

static std::string g_dir;
static int g_bad = 0;

template <typename T>
static std::vector<T> load(const char* name) {
    const std::string path = g_dir + "/" + name + ".bin";
    std::vector<T> v;
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) { std::printf("MISSING %s\n", path.c_str()); ++g_bad; return v; }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)bytes / sizeof(T));
    if (!v.empty() && std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) { std::printf("SHORT %s\n", path.c_str()); ++g_bad; }
    std::fclose(f);
    return v;
}

template <typename T>
static void same(const char* what, const std::vector<T>& got, const std::vector<T>& want) {
    size_t first = 0;
    bool ok = got.size() == want.size();
    for (; ok && first < got.size(); ++first)
        if (std::memcmp(&got[first], &want[first], sizeof(T)) != 0) { ok = false; break; }
    std::printf("%s %s (%zu items)\n", ok ? "ok" : "DIFFERENT", what, want.size());
    if (!ok) { std::printf("  sizes %zu %zu, first difference at %zu\n", got.size(), want.size(), first); ++g_bad; }
}

static bool interior(long long M, long long i, long long j, long long k) { return i > 0 && j > 0 && k > 0 && i < M - 1 && j < M - 1 && k < M - 1; }
static double sum6(const std::vector<double>& u, long long at, long long M) {
    return poisson_sum6(u[at - 1], u[at + 1], u[at - M], u[at + M], u[at - M * M], u[at + M * M]);
}

static void check_splat() {
    const auto meta = load<double>("splat_meta");          // origin x, y, z, h, R
    const auto pts = load<double>("splat_points"), nrm = load<double>("splat_normals");
    if (meta.size() != 5) return;
    const long long R = (long long)meta[4], n = (long long)pts.size() / 3;
    std::vector<long long> cells(3 * n), addends(32 * n);
    std::vector<double> frac(3 * n);
    for (long long p = 0; p < n; ++p) {
        double u[3];
        for (int a = 0; a < 3; ++a) poisson_axis(pts[3 * p + a], meta[a], meta[3], R, &cells[3 * p + a], &frac[3 * p + a]);
        poisson_unit(&nrm[3 * p], u);
        for (int corner = 0; corner < 8; ++corner) {
            const double w = poisson_corner_weight(&frac[3 * p], corner);
            addends[32 * p + 4 * corner] = poisson_quantise(w);
            for (int a = 0; a < 3; ++a) addends[32 * p + 4 * corner + 1 + a] = poisson_quantise(w * u[a]);
        }
    }
    same("splat cells", cells, load<long long>("splat_cells"));
    same("splat fractions", frac, load<double>("splat_fractions"));
    same("splat addends", addends, load<long long>("splat_addends"));
    const auto sums = load<long long>("splat_sums");
    std::vector<double> fields(sums.size());
    for (size_t j = 0; j < sums.size(); ++j) fields[j] = poisson_unquantise(sums[j]);
    same("splat fields", fields, load<double>("splat_fields"));
}

static void check_stencils() {
    const auto meta = load<double>("grid_meta");           // M, h, h2
    if (meta.size() != 3) return;
    const long long M = (long long)meta[0], Mc = (M - 1) / 2 + 1, N = M * M * M;
    const double h = meta[1], h2 = meta[2];
    const auto V = load<double>("grid_v"), u = load<double>("grid_u"), f = load<double>("grid_f"), e = load<double>("grid_e");
    if ((long long)V.size() != 3 * N || (long long)u.size() != N || (long long)f.size() != N || (long long)e.size() != Mc * Mc * Mc) { ++g_bad; return; }
    std::vector<double> rhs(N), jac(N), res(N), fc(Mc * Mc * Mc), up(u);
    for (long long k = 0; k < M; ++k)
        for (long long j = 0; j < M; ++j)
            for (long long i = 0; i < M; ++i) {
                const long long at = poisson_node_index(i, j, k, M);
                const bool in = interior(M, i, j, k);
                rhs[at] = in ? poisson_divergence(V[at - 1], V[at + 1], V[N + at - M], V[N + at + M], V[2 * N + at - M * M], V[2 * N + at + M * M], 2.0 * h) : 0.0;
                jac[at] = in ? poisson_jacobi(u[at], sum6(u, at, M), f[at], h2) : u[at];
                res[at] = in ? poisson_residual(u[at], sum6(u, at, M), f[at], h2) : 0.0;
            }
    for (long long K = 0; K < Mc; ++K)
        for (long long J = 0; J < Mc; ++J)
            for (long long I = 0; I < Mc; ++I) {
                double v = 0.0;
                if (interior(Mc, I, J, K)) {
                    double z[3];
                    for (int c = 0; c < 3; ++c) {
                        double y[3];
                        for (int b = 0; b < 3; ++b) {
                            const long long at = poisson_node_index(2 * I, 2 * J + b - 1, 2 * K + c - 1, M);
                            y[b] = poisson_full_weight(res[at - 1], res[at], res[at + 1]);
                        }
                        z[c] = poisson_full_weight(y[0], y[1], y[2]);
                    }
                    v = poisson_full_weight(z[0], z[1], z[2]);
                }
                fc[poisson_node_index(I, J, K, Mc)] = v;
            }
    for (long long k = 1; k < M - 1; ++k)
        for (long long j = 1; j < M - 1; ++j)
            for (long long i = 1; i < M - 1; ++i) {
                const int nx = (int)(i & 1), ny = (int)(j & 1), nz = (int)(k & 1);
                double z[2];
                for (int c = 0; c <= nz; ++c) {
                    double y[2];
                    for (int b = 0; b <= ny; ++b) {
                        const long long at = poisson_node_index(i >> 1, (j >> 1) + b, (k >> 1) + c, Mc);
                        y[b] = nx ? poisson_midpoint(e[at], e[at + 1]) : e[at];
                    }
                    z[c] = ny ? poisson_midpoint(y[0], y[1]) : y[0];
                }
                const long long at = poisson_node_index(i, j, k, M);
                up[at] = up[at] + (nz ? poisson_midpoint(z[0], z[1]) : z[0]);
            }
    same("divergence", rhs, load<double>("grid_rhs"));
    same("jacobi sweep", jac, load<double>("grid_jacobi"));
    same("residual", res, load<double>("grid_residual"));
    same("restriction", fc, load<double>("grid_restricted"));
    same("prolongation", up, load<double>("grid_prolonged"));
    same("coarse solve", std::vector<double>{poisson_coarse(f[0], h2)}, load<double>("grid_coarse"));
}

static void check_edges() {
    const auto in = load<double>("edge_in");               // rows of fa, fb, iso, o, ia, step, h, wa, wb
    const long long n = (long long)in.size() / 9;
    std::vector<double> out(3 * n);
    std::vector<long long> inside(2 * n);
    for (long long r = 0; r < n; ++r) {
        const double* q = &in[9 * r];
        const double t = poisson_edge_t(q[0], q[1], q[2]);
        out[3 * r] = t;
        out[3 * r + 1] = poisson_edge_position(q[3], (long long)q[4], (int)q[5], q[6], t);
        out[3 * r + 2] = poisson_edge_blend(q[7], q[8], t);
        inside[2 * r] = poisson_inside(q[0], q[2]) ? 1 : 0;
        inside[2 * r + 1] = poisson_inside(q[1], q[2]) ? 1 : 0;
    }
    same("edge interpolation", out, load<double>("edge_out"));
    same("edge ends inside", inside, load<long long>("edge_inside"));
}

static void check_tetrahedra() {
    // per tetrahedron and case 17 ints: its four corners, the number of triangles, then lo, hi of the three edges of each (-1 where none)
    std::vector<int> got;
    for (int t = 0; t < 6; ++t)
        for (unsigned code = 0; code < 16; ++code) {
            int c[4];
            poisson_tet_corners(t, c);
            PoissonTri tr[2];
            const int nt = poisson_tet_triangles(c, code, tr);
            if (nt != poisson_tet_triangle_count(code)) { std::printf("DIFFERENT triangle count of case %u\n", code); ++g_bad; }
            for (int p = 0; p < 4; ++p) got.push_back(c[p]);
            got.push_back(nt);
            for (int q = 0; q < 2; ++q)
                for (int e = 0; e < 3; ++e) {
                    got.push_back(q < nt ? tr[q].lo[e] : -1);
                    got.push_back(q < nt ? tr[q].hi[e] : -1);
                }
        }
    same("tetrahedron cases and winding", got, load<int>("tet_cases"));
    std::vector<int> pop;
    for (unsigned m = 0; m < 128; ++m) pop.push_back(poisson_popcount7(m));
    same("mask bit counts", pop, load<int>("popcount"));
}

static void check_depth9() {
    // node (512, 512, 512), the last edge key, the last byte of four float64 fields, of the int32 vertex table, of the last corner offset
    const long long M = poisson_axis_nodes(POISSON_MAX_DEPTH), N = poisson_node_count(POISSON_MAX_DEPTH);
    const long long node = poisson_node_index(M - 1, M - 1, M - 1, M);
    std::vector<long long> got = {M, N, node, poisson_edge_key(node, 7), poisson_byte_offset(4 * N, 8), poisson_byte_offset(N, 4),
                                  poisson_node_index(M - 2, M - 2, M - 2, M) + poisson_corner_offset(7, M),
                                  (long long)PoissonScanScratch(N).bytes, POISSON_MAX_POINTS, POISSON_MIN_DEPTH, POISSON_MAX_DEPTH, POISSON_CHUNK};
    same("depth 9 keys, offsets and constants", got, load<long long>("depth9"));
}

int main(int argc, char** argv) {
    if (argc != 2) { std::printf("usage: poisson_host_harness DIR\n"); return 2; }
    g_dir = argv[1];
    check_splat();
    check_stencils();
    check_edges();
    check_tetrahedra();
    check_depth9();
    std::printf("%s\n", g_bad ? "FAILED" : "PASSED");
    return g_bad ? 1 : 0;
}
