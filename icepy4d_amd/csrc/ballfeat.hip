// Geometric features of the ball around every point of a cloud (`scripts/pcd_postprocessing/top_border.py`: CloudCompare's
// computeFeature(Linearity, 2.0) and computeFeature(Verticality, 0.15)), on the device. A ball of 2 m on a dense front holds hundreds to
// thousands of points, more than the 64-slot list of knn.hip: this kernel accumulates instead of selecting. The definition (ball_point.h,
// DESIGN §4) sums quantised offsets in int64, exactly, so the grid decides the speed, never the result; pinned bit for bit against
// tests/ball_oracle.py. Parity with a CloudCompare binary is unpinned.
//
//   knn_gather_kernel    (knn_sorted.h) the cloud in cell order, into the scratch im_knn_self uses
//   ball_features_kernel one wave per query, queries in cell order. The box of cells [c - R, c + R] (R = ball_rings, the k-NN's stop rule
//                        without a k-th distance) clipped to the grid is walked as rows (knn_list.h: knn_box_walk), each row one
//                        contiguous range of the sorted cloud: the lanes look up the ranges of 64 rows at a time, a ballot keeps those that hold points, and those are
//                        read 64 candidates at a time, coalesced. Each lane adds its own candidates to its own ten sums; one butterfly
//                        per query merges them. No LDS, no barrier, no atomics, no per-thread array. A box whose row lookups alone would
//                        cost more than knn_step_budget is given up for one scan of the whole sorted cloud before it starts.
#include <cmath>

#include "common.h"
#include "ctx.h"
#include "stage_scratch.h"
#include "knn_sorted.h"
#include "knn_list.h"
#include "ball_point.h"
#include "ball_wave.h"

namespace im {
namespace {

struct BallArgs {
    KnnGrid g;
    KnnSorted s;
    const int* start;       // [cells + 1]
    int n, n_kinds;
    double r2, h, hh;
    unsigned long long kinds;      // kind j in bits 4 j .. 4 j + 3
    int* count; long long* sums; double* eig; double* normal; double* feat; int* steps;
};

static_assert(IM_BALL_KINDS <= 16 && BALL_MAX_KINDS * 4 <= 64, "sixteen kinds of four bits each fill the packed word");
static_assert(BALL_MAX_KINDS <= IM_WAVE, "a row of features is stored by the first lanes of a wave");

// the candidates at sorted positions [b, e), each lane its own
__device__ __forceinline__ void ball_scan(const BallArgs& a, BallSums& S, int lane, double qx, double qy, double qz, int b, int e) {
    for (long long base = b; base < e; base += IM_WAVE) {
        const long long j = base + lane;
        if (j < e) ball_candidate(S, a.s.x[j], a.s.y[j], a.s.z[j], qx, qy, qz, a.r2, a.h);
    }
}

__global__ __launch_bounds__(IM_WAVE * KNN_WAVES) void ball_features_kernel(BallArgs a) {
    const int lane = threadIdx.x & (IM_WAVE - 1);
    const long long q = (unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * KNN_WAVES + threadIdx.x / IM_WAVE));
    if (q >= a.n) return;                                             // the whole wave
    const double qx = a.s.x[q], qy = a.s.y[q], qz = a.s.z[q];
    const int qi = a.s.idx[q];
    const double t[3] = {knn_cell_coord(qx, a.g.o[0], a.g.s), knn_cell_coord(qy, a.g.o[1], a.g.s), knn_cell_coord(qz, a.g.o[2], a.g.s)};
    const int c[3] = {knn_cell_of(t[0], a.g.n[0]), knn_cell_of(t[1], a.g.n[1]), knn_cell_of(t[2], a.g.n[2])};
    const int R = ball_rings(a.g, t, c, a.r2);                        // <= 2^24
    const int x0 = max(0, c[0] - R), x1 = min(a.g.n[0] - 1, c[0] + R);
    const int y0 = max(0, c[1] - R), y1 = min(a.g.n[1] - 1, c[1] + R);
    const int z0 = max(0, c[2] - R), z1 = min(a.g.n[2] - 1, c[2] + R);
    BallSums S;
    ball_zero(S);
    const int steps = knn_box_walk(a.g, a.start, a.n, lane, x0, x1, y0, y1, z0, z1, [&](int b, int e) { ball_scan(a, S, lane, qx, qy, qz, b, e); });
    double eig[3], e3[3];
    ball_wave_finish(S, lane, qi, a.hh, steps, a.count, a.sums, a.eig, a.normal, a.steps, eig, e3);
    if (a.feat && lane < a.n_kinds)
        a.feat[(long long)qi * a.n_kinds + lane] = ball_feature((int)((a.kinds >> (4 * lane)) & 15), eig, e3, S.s[0]);
}

}  // namespace
}  // namespace im

using namespace im;

extern "C" {

int im_ball_features(im_ctx* ctx, const double* d_pts, const long long* d_perm, const int32_t* d_start, long long n, const double* h_grid,
                     int nx, int ny, int nz, double radius, const int32_t* h_kinds, int n_kinds, int32_t* d_count, long long* d_sums,
                     double* d_eig, double* d_normal, double* d_feat, int32_t* d_steps, void* stream) {
    IM_CHECK_CTX(ctx);
    BallArgs a;
    if (!d_pts || !d_perm || !d_start) return ctx->fail(-75, "im_ball_features: null pointer");
    if (n < 0 || n > BALL_MAX_POINTS) return ctx->fail(-75, "im_ball_features: n must be 0..2^26");
    if (!(radius > 0.0) || !std::isfinite(radius) || !std::isnormal(radius * BALL_STEP))
        return ctx->fail(-75, "im_ball_features: the radius must be finite and positive, and radius * 2^-18 a normal number");
    if (const char* why = bad_grid(h_grid, nx, ny, nz, a.g)) return ctx->fail(-75, "im_ball_features: %s", why);
    if (n_kinds < 0 || n_kinds > BALL_MAX_KINDS) return ctx->fail(-75, "im_ball_features: n_kinds must be 0..16");
    if (n_kinds > 0 && !h_kinds) return ctx->fail(-75, "im_ball_features: null kinds");
    a.kinds = 0;
    for (int j = 0; j < n_kinds; ++j) {
        if (h_kinds[j] < 0 || h_kinds[j] >= IM_BALL_KINDS) return ctx->fail(-75, "im_ball_features: unknown kind %d", (int)h_kinds[j]);
        a.kinds |= (unsigned long long)h_kinds[j] << (4 * j);
    }
    if (n == 0) return 0;
    const KnnSortedScratch lay(n);
    IM_GROW(ctx, ctx->grow(ctx->scratch.knn, lay.bytes, "knn_sorted"), -22, "im_ball_features: allocation failed");
    void* const base = ctx->scratch.knn.p;
    a.s.x = lay.x.at(base); a.s.y = lay.y.at(base); a.s.z = lay.z.at(base); a.s.idx = lay.idx.at(base);
    a.start = d_start; a.n = (int)n; a.n_kinds = n_kinds;
    a.h = radius * BALL_STEP; a.hh = a.h * a.h; a.r2 = radius * radius;
    a.count = d_count; a.sums = d_sums; a.eig = d_eig; a.normal = d_normal; a.feat = d_feat; a.steps = d_steps;
    hipStream_t s = (hipStream_t)stream;
    IM_LAUNCH(ctx, "knn_gather", s, launch(knn_gather_kernel, blocks_of(n, 256), 256, 0, s, d_pts, d_perm, n, a.s));
    IM_LAUNCH(ctx, "ball_features", s, launch(ball_features_kernel, blocks_of(n, KNN_WAVES), IM_WAVE * KNN_WAVES, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_ball_features");
    return 0;
}

}  // extern "C"
