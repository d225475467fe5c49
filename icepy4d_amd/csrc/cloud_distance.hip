// Distances between two clouds on the device: what the k-NN and the ball features ask of a cloud about its own points, asked of a target
// cloud at external queries, and M3C2's cylinder along a normal (Lague et al. 2013; CloudCompare's C2C and M3C2, Open3D's
// compute_point_cloud_distance). Neither tool is a dependency: every quantity has a definition of its own (cyl_point.h, ball_point.h,
// knn_point.h) and is pinned bit for bit against tests/cloud_distance_oracle.py. Parity with a binary of either is unpinned.
//
//   knn_gather_kernel    (knn_sorted.h) the target cloud in cell order, into the scratch im_knn_self uses
//   knn_cross_kernel     one wave per query: knn_list.h's ring search and best-k list, the query's cell clamped into the target's grid
//   ball_cross_kernel    one wave per query: the box of cells of ball_rings, walked by knn_box_walk; ten int64 sums of offsets from the query,
//                        merged, finished and stored by ball_wave.h as in ballfeat.hip
//   cyl_stats_kernel     one wave per query: the cylinder's axis-aligned box (cyl_extent) in cells, walked by knn_box_walk; three int64
//                        sums of quantised projections, each lane its own, one butterfly per query
//   m3c2_finish_kernel   one thread per core point: distance, level of detection, significance from two cylinders' sums
// The waves take the queries in the order d_qorder gives (the Python layer sorts them by the target's cell key so that neighbouring waves
// read the same cells); every output is addressed by the query's own index, and no result depends on the order. No LDS, no barrier, no atomics.
#include <cmath>

#include "common.h"
#include "ctx.h"
#include "stage_scratch.h"
#include "knn_sorted.h"
#include "knn_list.h"
#include "ball_point.h"
#include "ball_wave.h"
#include "cyl_point.h"

namespace im {
namespace {

constexpr int CROSS_REFUSED = -79;

// the external queries of a launch
struct CrossQueries {
    const double* q;            // [m][3]
    const long long* order;     // [m] or null
    long long m;
};

// The query of this wave: its index (an order entry outside 0..m-1 is clamped: meaningless then, but every access stays inside), its
// coordinates, its cell coordinates and its clamped cell in the target's grid. False for a wave beyond the queries.
__device__ __forceinline__ bool cross_query(const CrossQueries& Q, const KnnGrid& g, long long& qi, double (&p)[3], double (&t)[3], int (&c)[3]) {
    const long long w = (unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * KNN_WAVES + threadIdx.x / IM_WAVE));
    if (w >= Q.m) return false;
    qi = Q.order ? Q.order[w] : w;
    qi = qi < 0 ? 0 : (qi >= Q.m ? Q.m - 1 : qi);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        p[a] = Q.q[3 * qi + a];
        t[a] = knn_cell_coord(p[a], g.o[a], g.s);
        c[a] = knn_cell_of(t[a], g.n[a]);
    }
    return true;
}

__device__ __forceinline__ bool finite3(double x, double y, double z) { return isfinite(x) && isfinite(y) && isfinite(z); }

struct KnnCrossArgs : KnnSearch {
    CrossQueries Q;
    int* count; int* idx; double* d2; int* rings;
};

__global__ __launch_bounds__(IM_WAVE * KNN_WAVES) void knn_cross_kernel(KnnCrossArgs a) {
    const int lane = threadIdx.x & (IM_WAVE - 1);
    long long qi;
    double p[3], t[3];
    int c[3];
    if (!cross_query(a.Q, a.g, qi, p, t, c)) return;                  // the whole wave
    KnnList L{knn_inf(), KNN_NONE, knn_inf(), KNN_NONE};
    // a query with a non-finite coordinate has no neighbours and visits nothing
    const int rings = finite3(p[0], p[1], p[2]) ? knn_ring_search(a, L, lane, p[0], p[1], p[2], t, c) : 0;
    const bool held = L.idx != KNN_NONE;
    const int count = __popcll(__ballot(held));
    if (lane < a.k) {
        if (a.idx) a.idx[qi * a.k + lane] = held ? L.idx : -1;
        if (a.d2) a.d2[qi * a.k + lane] = held ? L.d2 : knn_inf();
    }
    if (lane == 0) {
        if (a.count) a.count[qi] = count;
        if (a.rings) a.rings[qi] = rings;
    }
}

struct BallCrossArgs {
    KnnGrid g;
    KnnSorted s;
    const int* start;
    int n;
    double r2, h, hh;
    CrossQueries Q;
    int* count; long long* sums; double* eig; double* normal; int* steps;
};

__global__ __launch_bounds__(IM_WAVE * KNN_WAVES) void ball_cross_kernel(BallCrossArgs a) {
    const int lane = threadIdx.x & (IM_WAVE - 1);
    long long qi;
    double p[3], t[3];
    int c[3];
    if (!cross_query(a.Q, a.g, qi, p, t, c)) return;
    BallSums S;
    ball_zero(S);
    int steps = 0;
    if (finite3(p[0], p[1], p[2])) {
        const int R = ball_rings(a.g, t, c, a.r2);                    // <= 2^24; the stop rule holds for a query outside the grid (knn_list.h)
        const int x0 = max(0, c[0] - R), x1 = min(a.g.n[0] - 1, c[0] + R);
        const int y0 = max(0, c[1] - R), y1 = min(a.g.n[1] - 1, c[1] + R);
        const int z0 = max(0, c[2] - R), z1 = min(a.g.n[2] - 1, c[2] + R);
        steps = knn_box_walk(a.g, a.start, a.n, lane, x0, x1, y0, y1, z0, z1, [&](int b, int e) {
            for (long long base = b; base < e; base += IM_WAVE) {
                const long long j = base + lane;
                if (j < e) ball_candidate(S, a.s.x[j], a.s.y[j], a.s.z[j], p[0], p[1], p[2], a.r2, a.h);
            }
        });
    }
    double eig[3], e3[3];
    ball_wave_finish(S, lane, qi, a.hh, steps, a.count, a.sums, a.eig, a.normal, a.steps, eig, e3);
}

struct CylArgs {
    KnnGrid g;
    KnnSorted s;
    const int* start;
    int n;
    double rho, rho2, L, h;
    CrossQueries Q;
    const double* nrm;          // [m][3]
    int* count; long long* sums; double* mean; double* std; int* steps;
};

__global__ __launch_bounds__(IM_WAVE * KNN_WAVES) void cyl_stats_kernel(CylArgs a) {
    const int lane = threadIdx.x & (IM_WAVE - 1);
    long long qi;
    double p[3], t[3];
    int c[3];
    if (!cross_query(a.Q, a.g, qi, p, t, c)) return;
    const double nx = a.nrm[3 * qi], ny = a.nrm[3 * qi + 1], nz = a.nrm[3 * qi + 2];
    CylSums S;
    cyl_zero(S);
    int steps = 0;
    if (finite3(p[0], p[1], p[2]) && finite3(nx, ny, nz)) {
        // The box of cells. Every inside candidate has |p_a - c_a| <= e[a] in real arithmetic (cyl_extent), so the double p_a lies between
        // the rounded corners fl(c_a - e[a]) and fl(c_a + e[a]) (rounding to nearest is monotone and p_a is its own rounding); the cell
        // coordinate and the cell are monotone in the coordinate (knn_point.h), so the candidate's cell lies between the corners' cells:
        // no inside point sits in a cell outside the box, and the margin of cyl_extent needs no padded cell on top.
        double e[3];
        cyl_extent(nx, ny, nz, a.rho, a.L, e);
        int lo[3], hi[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = knn_cell_of(knn_cell_coord(p[k] - e[k], a.g.o[k], a.g.s), a.g.n[k]);
            hi[k] = knn_cell_of(knn_cell_coord(p[k] + e[k], a.g.o[k], a.g.s), a.g.n[k]);
            hi[k] = hi[k] < lo[k] ? lo[k] : hi[k];                    // a NaN corner: cell 0
        }
        steps = knn_box_walk(a.g, a.start, a.n, lane, lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], [&](int b, int e2) {
            for (long long base = b; base < e2; base += IM_WAVE) {
                const long long j = base + lane;
                if (j < e2) cyl_candidate(S, a.s.x[j], a.s.y[j], a.s.z[j], p[0], p[1], p[2], nx, ny, nz, a.rho2, a.L, a.h);
            }
        });
    }
#pragma unroll
    for (int k = 0; k < CYL_SUMS; ++k)
#pragma unroll
        for (int o = IM_WAVE / 2; o > 0; o >>= 1) S.s[k] += __shfl_xor(S.s[k], o);
    double mean, sd;
    cyl_finish(S.s[0], S.s[1], S.s[2], a.h, mean, sd);
    if (lane == 0) {
        if (a.count) a.count[qi] = (int)S.s[0];
        if (a.steps) a.steps[qi] = steps;
        if (a.mean) a.mean[qi] = mean;
        if (a.std) a.std[qi] = sd;
    }
    if (a.sums && lane < 2) a.sums[2 * qi + lane] = lane == 0 ? S.s[1] : S.s[2];
}

struct M3c2Args {
    const int* count1; const long long* sums1; const int* count2; const long long* sums2;
    long long m;
    double h, reg_error;
    int min_points;
    double* dist; double* lod; unsigned char* sig;
};

__global__ __launch_bounds__(256) void m3c2_finish_kernel(M3c2Args a) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= a.m) return;
    double dist, lod;
    bool sig;
    cyl_m3c2(a.count1[i], a.sums1[2 * i], a.sums1[2 * i + 1], a.count2[i], a.sums2[2 * i], a.sums2[2 * i + 1], a.h, a.reg_error, a.min_points,
             dist, lod, sig);
    if (a.dist) a.dist[i] = dist;
    if (a.lod) a.lod[i] = lod;
    if (a.sig) a.sig[i] = sig ? 1 : 0;
}

static_assert(IM_WAVE * KNN_WAVES == 256, "the query kernels take the block of knn.hip: 256 threads, four waves");

// what the three query entry points refuse in common; nullptr when all is fine
const char* bad_cross(const double* d_pts, const long long* d_perm, const int32_t* d_start, long long n, const double* h_grid, int nx, int ny,
                      int nz, const double* d_q, long long m, KnnGrid& g) {
    if (!d_pts || !d_perm || !d_start || !d_q) return "null pointer";
    if (n < 0 || n > BALL_MAX_POINTS) return "n must be 0..2^26";
    if (m < 0 || m > BALL_MAX_POINTS) return "m must be 0..2^26";
    return bad_grid(h_grid, nx, ny, nz, g);
}

// the target cloud in cell order, in the context's scratch; 0, or the code the entry point returns
int cross_gather(im_ctx* ctx, const double* d_pts, const long long* d_perm, long long n, KnnSorted& out, hipStream_t s, const char* where) {
    const KnnSortedScratch lay(n);
    IM_GROW(ctx, ctx->grow(ctx->scratch.knn, lay.bytes, "knn_sorted"), -22, "%s: allocation failed", where);
    void* const base = ctx->scratch.knn.p;
    out.x = lay.x.at(base); out.y = lay.y.at(base); out.z = lay.z.at(base); out.idx = lay.idx.at(base);
    IM_LAUNCH(ctx, "knn_gather", s, launch(knn_gather_kernel, blocks_of(n, 256), 256, 0, s, d_pts, d_perm, n, out));
    return 0;
}

}  // namespace
}  // namespace im

using namespace im;

extern "C" {

int im_knn_cross(im_ctx* ctx, const double* d_pts, const long long* d_perm, const int32_t* d_start, long long n, const double* h_grid, int nx,
                 int ny, int nz, const double* d_q, const long long* d_qorder, long long m, int k, double radius2, int32_t* d_count,
                 int32_t* d_idx, double* d_d2, int32_t* d_rings, void* stream) {
    IM_CHECK_CTX(ctx);
    KnnCrossArgs a;
    if (const char* why = bad_cross(d_pts, d_perm, d_start, n, h_grid, nx, ny, nz, d_q, m, a.g)) return ctx->fail(CROSS_REFUSED, "im_knn_cross: %s", why);
    if (k < 1 || k > IM_WAVE) return ctx->fail(CROSS_REFUSED, "im_knn_cross: k must be 1..64");
    if (!(radius2 >= 0.0)) return ctx->fail(CROSS_REFUSED, "im_knn_cross: radius2 must be >= 0 (+inf: no radius)");
    if (n == 0 || m == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = cross_gather(ctx, d_pts, d_perm, n, a.s, s, "im_knn_cross")) return rc;
    a.start = d_start; a.n = (int)n; a.k = k; a.radius2 = radius2;
    a.Q = CrossQueries{d_q, d_qorder, m};
    a.count = d_count; a.idx = d_idx; a.d2 = d_d2; a.rings = d_rings;
    IM_LAUNCH(ctx, "knn_cross", s, launch(knn_cross_kernel, blocks_of(m, KNN_WAVES), IM_WAVE * KNN_WAVES, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_knn_cross");
    return 0;
}

int im_ball_cross(im_ctx* ctx, const double* d_pts, const long long* d_perm, const int32_t* d_start, long long n, const double* h_grid, int nx,
                  int ny, int nz, const double* d_q, const long long* d_qorder, long long m, double radius, int32_t* d_count, long long* d_sums,
                  double* d_eig, double* d_normal, int32_t* d_steps, void* stream) {
    IM_CHECK_CTX(ctx);
    BallCrossArgs a;
    if (const char* why = bad_cross(d_pts, d_perm, d_start, n, h_grid, nx, ny, nz, d_q, m, a.g)) return ctx->fail(CROSS_REFUSED, "im_ball_cross: %s", why);
    if (!(radius > 0.0) || !std::isfinite(radius) || !std::isnormal(radius * BALL_STEP))
        return ctx->fail(CROSS_REFUSED, "im_ball_cross: the radius must be finite and positive, and radius * 2^-18 a normal number");
    if (n == 0 || m == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = cross_gather(ctx, d_pts, d_perm, n, a.s, s, "im_ball_cross")) return rc;
    a.start = d_start; a.n = (int)n;
    a.h = radius * BALL_STEP; a.hh = a.h * a.h; a.r2 = radius * radius;
    a.Q = CrossQueries{d_q, d_qorder, m};
    a.count = d_count; a.sums = d_sums; a.eig = d_eig; a.normal = d_normal; a.steps = d_steps;
    IM_LAUNCH(ctx, "ball_cross", s, launch(ball_cross_kernel, blocks_of(m, KNN_WAVES), IM_WAVE * KNN_WAVES, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_ball_cross");
    return 0;
}

int im_cyl_stats(im_ctx* ctx, const double* d_pts, const long long* d_perm, const int32_t* d_start, long long n, const double* h_grid, int nx,
                 int ny, int nz, const double* d_q, const double* d_nrm, const long long* d_qorder, long long m, double radius,
                 double half_length, int32_t* d_count, long long* d_sums, double* d_mean, double* d_std, int32_t* d_steps, void* stream) {
    IM_CHECK_CTX(ctx);
    CylArgs a;
    if (const char* why = bad_cross(d_pts, d_perm, d_start, n, h_grid, nx, ny, nz, d_q, m, a.g)) return ctx->fail(CROSS_REFUSED, "im_cyl_stats: %s", why);
    if (!d_nrm) return ctx->fail(CROSS_REFUSED, "im_cyl_stats: null normals");
    if (!(radius > 0.0) || !std::isfinite(radius)) return ctx->fail(CROSS_REFUSED, "im_cyl_stats: the radius must be finite and positive");
    if (!(half_length > 0.0) || !std::isfinite(half_length) || !std::isnormal(half_length * BALL_STEP))
        return ctx->fail(CROSS_REFUSED, "im_cyl_stats: the half-length must be finite and positive, and half_length * 2^-18 a normal number");
    if (n == 0 || m == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (const int rc = cross_gather(ctx, d_pts, d_perm, n, a.s, s, "im_cyl_stats")) return rc;
    a.start = d_start; a.n = (int)n;
    a.rho = radius; a.rho2 = radius * radius; a.L = half_length; a.h = half_length * BALL_STEP;
    a.Q = CrossQueries{d_q, d_qorder, m};
    a.nrm = d_nrm;
    a.count = d_count; a.sums = d_sums; a.mean = d_mean; a.std = d_std; a.steps = d_steps;
    IM_LAUNCH(ctx, "cyl_stats", s, launch(cyl_stats_kernel, blocks_of(m, KNN_WAVES), IM_WAVE * KNN_WAVES, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_cyl_stats");
    return 0;
}

int im_m3c2_finish(im_ctx* ctx, const int32_t* d_count1, const long long* d_sums1, const int32_t* d_count2, const long long* d_sums2,
                   long long m, double half_length, double reg_error, int min_points, double* d_dist, double* d_lod, uint8_t* d_sig,
                   void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_count1 || !d_sums1 || !d_count2 || !d_sums2) return ctx->fail(CROSS_REFUSED, "im_m3c2_finish: null pointer");
    if (m < 0 || m > BALL_MAX_POINTS) return ctx->fail(CROSS_REFUSED, "im_m3c2_finish: m must be 0..2^26");
    if (!(half_length > 0.0) || !std::isfinite(half_length) || !std::isnormal(half_length * BALL_STEP))
        return ctx->fail(CROSS_REFUSED, "im_m3c2_finish: the half-length must be finite and positive, and half_length * 2^-18 a normal number");
    if (!(reg_error >= 0.0) || !std::isfinite(reg_error)) return ctx->fail(CROSS_REFUSED, "im_m3c2_finish: the registration error must be finite and >= 0");
    if (min_points < 2) return ctx->fail(CROSS_REFUSED, "im_m3c2_finish: min_points must be >= 2");
    if (m == 0) return 0;
    const M3c2Args a{d_count1, d_sums1, d_count2, d_sums2, m, half_length * BALL_STEP, reg_error, min_points, d_dist, d_lod, d_sig};
    hipStream_t s = (hipStream_t)stream;
    IM_LAUNCH(ctx, "m3c2_finish", s, launch(m3c2_finish_kernel, blocks_of(m, 256), 256, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_m3c2_finish");
    return 0;
}

}  // extern "C"
