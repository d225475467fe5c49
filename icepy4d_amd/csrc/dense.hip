// Two-view dense stereo on the device: depth maps by a plane sweep, their mutual consistency, and the dense cloud of the kept pixels
// (what the reference gets from Metashape's buildDepthMaps / buildDenseCloud, `metashape.py:198-240`). Metashape's matcher is closed and
// is not reproduced: every quantity has a definition of this project's own (dense_pixel.h) and is pinned bit for bit against
// tests/dense_oracle.py. Parity with Metashape is unpinned by construction.
//
//   dense_sweep_kernel        one block of 256 threads per 64 x 16 tile of ref pixels (the tile, its staging and the scoring of one plane are
//                             dense_tile.h's, shared with dense_costs_kernel). The ref bytes of the tile and its halo of r are staged in
//                             LDS once; then, for every plane inside the kernel: (A) each thread warps its share of tile + halo into LDS,
//                             (B) the rows are box-summed over 2 r + 1 columns into 8-byte partials (sum b^2; sum b, the invalid count and
//                             sum a b packed in the other 8 bytes), rows of 64 consecutive entries, one per lane: ds_read_b64 / ds_write_b64
//                             without bank conflicts, (C) each thread sums 2 r + 1 rows of partials for its four pixels, scores them and
//                             keeps the running best, its predecessor and its successor in registers. No cost volume reaches memory.
//   dense_consistency_kernel  one thread per pixel of map 0
//   DenseCloudScan            mark = the keep byte, scan.h's three kernels, and the scan's write is the scatter of point, colour, normal, confidence
// The host checks shared with the other dense stages are dense_host.h's.
// All sums are integers: the order of execution does not matter. No atomics. Enqueue only.
#include "common.h"
#include "ctx.h"
#include "stage_scratch.h"
#include "dense_tile.h"
#include "dense_host.h"

namespace im {
namespace {

#include "scan.h"

struct DenseSweepArgs {
    const uint8_t* ref; const uint8_t* src;
    int h0, w0, h1, w1, D, r;
    double A[9], B[9], w_first, w_step, min_score;
    long long min_var;
    int16_t* plane; double* w; float* score;
};

__global__ __launch_bounds__(TILE_BLOCK) void dense_sweep_kernel(DenseSweepArgs a) {
    __shared__ PlaneLds L;                            // dense_tile.h: ref bytes, the plane's samples, the two rows of partials
    __shared__ double s_AB[18];                       // A and B
    const int t = threadIdx.x, r = a.r;

    int16_t* const o_plane = a.plane; double* const o_w = a.w; float* const o_score = a.score;
    // a tile none of whose pixels has its window inside ref: every pixel is invalid for every plane
    if (!tile_any_window_inside(a.h0, a.w0, r)) {
#pragma unroll
        for (int j = 0; j < PIX; ++j) {
            const TilePixel q = tile_pixel(j);
            if (q.inside(a.h0, a.w0)) {
                const long i = q.at(a.w0);
                o_plane[i] = -1; o_w[i] = 0.0; o_score[i] = 0.0f;
            }
        }
        return;
    }

    tile_stage_bytes(L.a, a.ref, a.h0, a.w0, r);
    if (t < 9) { s_AB[t] = a.A[t]; s_AB[9 + t] = a.B[t]; }      // read per plane from LDS: 36 scalar registers less to hold
    __syncthreads();

    PlaneRef R;
    plane_ref_sums(L, a.h0, a.w0, r, R);
    DenseBest best[PIX];
#pragma unroll
    for (int j = 0; j < PIX; ++j) dense_best_init(best[j]);

    for (int k = 0; k < a.D; ++k) {
        double H[9];
        dense_plane(s_AB, s_AB + 9, a.w_first, a.w_step, k, H);
        // the score of plane k at every pixel, and the running best of this thread's pixels
        plane_scores(L, R, a.src, a.h0, a.w0, a.h1, a.w1, r, a.min_var, H,
                     [&](int j, const TilePixel&, bool valid, double s) { dense_best_step(best[j], k, valid, s); });
    }

#pragma unroll
    for (int j = 0; j < PIX; ++j) {
        const TilePixel q = tile_pixel(j);
        if (q.inside(a.h0, a.w0)) {
            const long i = q.at(a.w0);
            int16_t plane; double w; float score;
            dense_best_finish(best[j], a.D, a.w_first, a.w_step, a.min_score, plane, w, score);
            o_plane[i] = plane; o_w[i] = w; o_score[i] = score;
        }
    }
}

struct DenseConsistencyArgs {
    const int16_t* plane0; const double* w0map; int h0, w0;
    const int16_t* plane1; const double* w1map; int h1, w1;
    DensePose P;
    double tol;
    int check;
    uint8_t* keep;
};

__global__ __launch_bounds__(256) void dense_consistency_kernel(DenseConsistencyArgs a) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= (long)a.h0 * a.w0) return;
    bool k = a.plane0[i] >= 0;
    if (k && a.check) k = dense_consistent(a.P, (int)(i % a.w0), (int)(i / a.w0), a.w0map[i], a.plane1, a.w1map, a.h1, a.w1, a.tol);
    a.keep[i] = k ? 1 : 0;
}

// the scan over the keep bytes whose write is the scatter: kept pixels in row-major order give the point order
struct DenseCloudScan {
    const uint8_t* keep; const double* wmap; const float* score; const uint8_t* img;
    int channels, h, w;
    long long capacity;
    DenseCam cam;
    double* xyz; uint8_t* rgb; double* nrm; float* conf;
    __device__ long long count(long long j) const { return j < (long long)h * w && keep[j] != 0 ? 1 : 0; }
    __device__ void write(long long j, long long pos) const {
        if (j >= (long long)h * w || keep[j] == 0 || pos >= capacity) return;
        const int u = (int)(j % w), v = (int)(j / w);
        double W[3], N[3];
        dense_point(cam, keep, wmap, h, w, u, v, W, N);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            xyz[3 * pos + c] = W[c];
            nrm[3 * pos + c] = N[c];
            rgb[3 * pos + c] = channels == 3 ? img[3 * j + c] : img[j];
        }
        conf[pos] = score[j];
    }
};

}  // namespace
}  // namespace im

using namespace im;

extern "C" {

int im_dense_tile_w(void) { return DENSE_TILE_W; }
int im_dense_tile_h(void) { return DENSE_TILE_H; }

int im_dense_sweep(im_ctx* ctx, const uint8_t* d_ref, int h0, int w0, const uint8_t* d_src, int h1, int w1, const double* h_A, const double* h_B,
                   double w_first, double w_step, int D, int r, long long min_var, double min_score, int16_t* d_plane, double* d_w, float* d_score,
                   void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_ref || !d_src || !h_A || !h_B || !d_plane || !d_w || !d_score) return ctx->fail(DENSE_REFUSED, "im_dense_sweep: null pointer");
    if (bad_side(h0) || bad_side(w0) || bad_side(h1) || bad_side(w1)) return ctx->fail(DENSE_REFUSED, "im_dense_sweep: h and w must be 1..16384");
    if (D < 1 || D > DENSE_MAX_PLANES) return ctx->fail(DENSE_REFUSED, "im_dense_sweep: D must be 1..4096");
    if (r < 1 || r > DENSE_MAX_RADIUS) return ctx->fail(DENSE_REFUSED, "im_dense_sweep: r must be 1..7");
    if (min_var < 0) return ctx->fail(DENSE_REFUSED, "im_dense_sweep: min_var must not be negative");
    // n^2 min_var 2^20 must fit an int64 beside the sums: 225^2 2^20 min_var < 2^63
    if (min_var > (1LL << 26)) return ctx->fail(DENSE_REFUSED, "im_dense_sweep: min_var must be at most 2^26");
    hipStream_t s = (hipStream_t)stream;
    DenseSweepArgs a{d_ref, d_src, h0, w0, h1, w1, D, r, {}, {}, w_first, w_step, min_score, min_var, d_plane, d_w, d_score};
    copy_matrices(h_A, h_B, a.A, a.B);
    IM_LAUNCH(ctx, "dense_sweep", s, launch(dense_sweep_kernel, dim3((unsigned)blocks_of(w0, TW), (unsigned)blocks_of(h0, TH)), TILE_BLOCK, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_dense_sweep");
    return 0;
}

int im_dense_consistency(im_ctx* ctx, const int16_t* d_plane0, const double* d_w0, int h0, int w0, const int16_t* d_plane1, const double* d_w1, int h1,
                         int w1, const double* h_pose, double tol, int check, uint8_t* d_keep, void* stream) {
    IM_CHECK_CTX(ctx);
    if (check != 0 && check != 1) return ctx->fail(DENSE_REFUSED, "im_dense_consistency: check must be 0 or 1");
    if (!d_plane0 || !d_w0 || !d_keep || (check && (!d_plane1 || !d_w1 || !h_pose))) return ctx->fail(DENSE_REFUSED, "im_dense_consistency: null pointer");
    if (bad_side(h0) || bad_side(w0) || (check && (bad_side(h1) || bad_side(w1)))) return ctx->fail(DENSE_REFUSED, "im_dense_consistency: h and w must be 1..16384");
    if (check && !(tol >= 0.0)) return ctx->fail(DENSE_REFUSED, "im_dense_consistency: the tolerance must not be negative");
    hipStream_t s = (hipStream_t)stream;
    DenseConsistencyArgs a{d_plane0, d_w0, h0, w0, d_plane1, d_w1, h1, w1, {}, tol, check, d_keep};
    if (check) __builtin_memcpy(&a.P, h_pose, sizeof(DensePose));
    IM_LAUNCH(ctx, "dense_consistency", s, launch(dense_consistency_kernel, blocks_of((long long)h0 * w0, 256), 256, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_dense_consistency");
    return 0;
}

int im_dense_cloud(im_ctx* ctx, const uint8_t* d_keep, const double* d_w, const float* d_score, const uint8_t* d_img, int channels, int h, int w,
                   const double* h_cam, long long capacity, double* d_xyz, uint8_t* d_rgb, double* d_nrm, float* d_conf, long long* d_count,
                   void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_keep || !d_w || !d_score || !d_img || !h_cam || !d_xyz || !d_rgb || !d_nrm || !d_conf || !d_count)
        return ctx->fail(DENSE_REFUSED, "im_dense_cloud: null pointer");
    if (bad_side(h) || bad_side(w)) return ctx->fail(DENSE_REFUSED, "im_dense_cloud: h and w must be 1..16384");
    if (channels != 1 && channels != 3) return ctx->fail(DENSE_REFUSED, "im_dense_cloud: 1 or 3 channels");
    if (capacity < 0) return ctx->fail(DENSE_REFUSED, "im_dense_cloud: the capacity must not be negative");
    if (!finite_all(h_cam, 21)) return ctx->fail(DENSE_REFUSED, "im_dense_cloud: the camera must be finite");
    hipStream_t s = (hipStream_t)stream;
    const long long n = (long long)h * w;
    const DenseCloudScratch lay(n);
    IM_GROW(ctx, ctx->grow(ctx->scratch.dense, lay.bytes, "dense.scratch"), -22, "im_dense_cloud: allocation failed");
    DenseCloudScan sc{d_keep, d_w, d_score, d_img, channels, h, w, capacity, {}, d_xyz, d_rgb, d_nrm, d_conf};
    __builtin_memcpy(&sc.cam, h_cam, sizeof(DenseCam));
    IM_LAUNCH(ctx, "dense_cloud", s, launch_scan(sc, n, lay.sums.at(ctx->scratch.dense.p), d_count, s));
    IM_GUARD_CHECK(ctx, s, "im_dense_cloud");
    return 0;
}

}  // extern "C"
