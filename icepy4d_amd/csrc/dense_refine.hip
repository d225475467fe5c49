// Slanted-window refinement of a dense-stereo depth map on the device: the slant of every kept pixel from the map itself, then a search of a
// few sub-plane candidates around the pixel's inverse depth whose window samples follow that slant (the sweep of dense.hip warps every
// sample of a window with the centre's inverse depth: fronto-parallel). Metashape's matcher is closed and is not reproduced: every quantity
// has a definition of this project's own (refine_pixel.h) and is pinned bit for bit against tests/refine_oracle.py. Parity with
// Metashape is unpinned by construction.
//
//   dense_slant_kernel    one block of 256 threads per 64 x 16 tile, one lane per column (the tile, the map from a thread to its pixels and the
//                         staging loop are dense_tile.h's, shared with the sweep). The inverse depths and the kept flags of the tile and
//                         its halo of R are staged in LDS once (a flag is 0 outside the map); each thread then owns the nine integer sums of
//                         its four pixels, one pixel after another, in registers (slant_pixel on the staged arrays).
//   dense_refine_kernel   the same tile. The ref bytes of the tile and its halo of r are staged in LDS; a thread reads the map and the slant of
//                         its own pixels from memory and runs refine_pixel on the staged bytes: candidates outside, samples inside, three
//                         integer sums and an invalid count per candidate, the running best with its two neighbours. The four src taps of a
//                         sample are gathered through the cache. A slanted window shares no sample with its neighbour's, so nothing is
//                         exchanged between threads behind the staging.
// All sums are integers: the order of execution does not matter. No atomics, no cost volume in memory. Enqueue only.
#include "common.h"
#include "ctx.h"
#include "refine_pixel.h"
#include "dense_tile.h"
#include "dense_host.h"

namespace im {
namespace {

constexpr int HALO = DENSE_MAX_RADIUS > REFINE_MAX_FIT_RADIUS ? DENSE_MAX_RADIUS : REFINE_MAX_FIT_RADIUS;
constexpr int RW = TW + 2 * HALO, RH = TH + 2 * HALO;                             // 78 x 30 with the largest halo

struct DenseSlantArgs {
    const int16_t* plane; const double* w;
    int h, wd, R, min_count;
    double w_step, max_diff;
    double* slant; uint8_t* fitted;
};

__global__ __launch_bounds__(TILE_BLOCK) void dense_slant_kernel(DenseSlantArgs a) {
    __shared__ double s_w[RH * RW];                   // inverse depths of tile + halo
    __shared__ uint8_t s_k[RH * RW];                  // 1: inside the map and kept
    const int R = a.R, hw = TW + 2 * R;
    tile_stage(tile_x0() - R, tile_y0() - R, hw, TH + 2 * R, a.h, a.wd, [&](int i, bool inside, long g, int, int) {
        const bool kept = inside && a.plane[g] >= 0;
        s_k[i] = kept ? 1 : 0;
        s_w[i] = kept ? a.w[g] : 0.0;
    });
    __syncthreads();
    for (int j = 0; j < PIX; ++j) {
        const TilePixel q = tile_pixel(j);
        if (!q.inside(a.h, a.wd)) continue;
        const int at = (q.row + R) * hw + q.c + R;
        double gu = 0.0, gv = 0.0;
        bool fit = false;
        if (s_k[at] != 0)
            fit = slant_pixel(s_w + at, s_k + at, hw, -min(R, q.u), min(R, a.wd - 1 - q.u), -min(R, q.v), min(R, a.h - 1 - q.v), a.w_step, a.max_diff,
                              a.min_count, gu, gv);
        const long i = q.at(a.wd);
        a.slant[2 * i] = gu; a.slant[2 * i + 1] = gv;
        a.fitted[i] = fit ? 1 : 0;
    }
}

struct DenseRefineArgs {
    const uint8_t* ref; const uint8_t* src;
    int h0, w0, h1, w1, r, span, sub;
    double A[9], B[9], w_step;
    long long min_var;
    const int16_t* plane; const double* w; const float* score; const double* slant;
    double* w_out; float* score_out; uint8_t* taken;
};

__global__ __launch_bounds__(TILE_BLOCK) void dense_refine_kernel(DenseRefineArgs a) {
    __shared__ uint8_t s_a[RH * RW];                  // ref bytes of tile + halo (0 outside ref)
    __shared__ double s_AB[18];                       // A and B: read per sample from LDS, 36 scalar registers less to hold
    const int t = threadIdx.x, r = a.r, hw = TW + 2 * r;
    tile_stage_bytes(s_a, a.ref, a.h0, a.w0, r);
    if (t < 9) { s_AB[t] = a.A[t]; s_AB[9 + t] = a.B[t]; }
    __syncthreads();
    for (int j = 0; j < PIX; ++j) {
        const TilePixel q = tile_pixel(j);
        if (!q.inside(a.h0, a.w0)) continue;
        const long i = q.at(a.w0);
        double w = a.w[i];
        float score = a.score[i];
        bool took = false;
        // refined: kept, and the window lies inside ref (so every byte it reads of s_a is a byte of ref)
        if (a.plane[i] >= 0 && window_inside(q.u, q.v, r, a.h0, a.w0))
            took = refine_pixel(s_a + (q.row + r) * hw + q.c + r, hw, a.src, a.h1, a.w1, s_AB, s_AB + 9, q.u, q.v, r, w, score, a.slant[2 * i],
                                a.slant[2 * i + 1], a.w_step, a.span, a.sub, a.min_var, w, score);
        a.w_out[i] = w; a.score_out[i] = score; a.taken[i] = took ? 1 : 0;
    }
}

}  // namespace
}  // namespace im

using namespace im;

extern "C" {

int im_dense_slant(im_ctx* ctx, const int16_t* d_plane, const double* d_w, int h, int w, double w_step, int fit_radius, double max_diff, int min_count,
                   double* d_slant, uint8_t* d_fitted, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_plane || !d_w || !d_slant || !d_fitted) return ctx->fail(DENSE_REFUSED, "im_dense_slant: null pointer");
    if (bad_side(h) || bad_side(w)) return ctx->fail(DENSE_REFUSED, "im_dense_slant: h and w must be 1..16384");
    if (bad_step(w_step)) return ctx->fail(DENSE_REFUSED, "im_dense_slant: w_step must be finite and not zero");
    if (fit_radius < 1 || fit_radius > REFINE_MAX_FIT_RADIUS) return ctx->fail(DENSE_REFUSED, "im_dense_slant: fit_radius must be 1..7");
    if (!(max_diff > 0.0 && max_diff <= REFINE_MAX_DIFF)) return ctx->fail(DENSE_REFUSED, "im_dense_slant: max_diff must be in (0, 64]");
    if (min_count < REFINE_MIN_COUNT || min_count > REFINE_MAX_COUNT) return ctx->fail(DENSE_REFUSED, "im_dense_slant: min_count must be 3..225");
    hipStream_t s = (hipStream_t)stream;
    DenseSlantArgs a{d_plane, d_w, h, w, fit_radius, min_count, w_step, max_diff, d_slant, d_fitted};
    IM_LAUNCH(ctx, "dense_slant", s, launch(dense_slant_kernel, dim3((unsigned)blocks_of(w, TW), (unsigned)blocks_of(h, TH)), TILE_BLOCK, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_dense_slant");
    return 0;
}

int im_dense_refine(im_ctx* ctx, const uint8_t* d_ref, int h0, int w0, const uint8_t* d_src, int h1, int w1, const double* h_A, const double* h_B,
                    const int16_t* d_plane, const double* d_w, const float* d_score, const double* d_slant, double w_step, int r, long long min_var, int span,
                    int sub, double* d_w_out, float* d_score_out, uint8_t* d_taken, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_ref || !d_src || !h_A || !h_B || !d_plane || !d_w || !d_score || !d_slant || !d_w_out || !d_score_out || !d_taken)
        return ctx->fail(DENSE_REFUSED, "im_dense_refine: null pointer");
    if (bad_side(h0) || bad_side(w0) || bad_side(h1) || bad_side(w1)) return ctx->fail(DENSE_REFUSED, "im_dense_refine: h and w must be 1..16384");
    if (bad_step(w_step)) return ctx->fail(DENSE_REFUSED, "im_dense_refine: w_step must be finite and not zero");
    if (r < 1 || r > DENSE_MAX_RADIUS) return ctx->fail(DENSE_REFUSED, "im_dense_refine: r must be 1..7");
    // n^2 min_var 2^20 must fit an int64 beside the sums, as in im_dense_sweep
    if (min_var < 0 || min_var > (1LL << 26)) return ctx->fail(DENSE_REFUSED, "im_dense_refine: min_var must be 0..2^26");
    if (span < 1 || span > REFINE_MAX_SPAN) return ctx->fail(DENSE_REFUSED, "im_dense_refine: span must be 1..4");
    if (sub < 1 || sub > REFINE_MAX_SUB) return ctx->fail(DENSE_REFUSED, "im_dense_refine: sub must be 1..8");
    hipStream_t s = (hipStream_t)stream;
    DenseRefineArgs a{d_ref, d_src, h0, w0, h1, w1, r, span, sub, {}, {}, w_step, min_var, d_plane, d_w, d_score, d_slant, d_w_out, d_score_out, d_taken};
    copy_matrices(h_A, h_B, a.A, a.B);
    IM_LAUNCH(ctx, "dense_refine", s, launch(dense_refine_kernel, dim3((unsigned)blocks_of(w0, TW), (unsigned)blocks_of(h0, TH)), TILE_BLOCK, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_dense_refine");
    return 0;
}

}  // extern "C"
