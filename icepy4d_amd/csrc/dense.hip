// Two-view dense stereo on the device: depth maps by a plane sweep, their mutual consistency, and the dense cloud of the kept pixels
// (what the reference gets from Metashape's buildDepthMaps / buildDenseCloud, `metashape.py:198-240`). Metashape's matcher is closed and
// is not reproduced: every quantity has a definition of this project's own (dense_pixel.h) and is pinned bit for bit against
// tests/dense_oracle.py. Parity with Metashape is unpinned by construction.
//
//   dense_sweep_kernel        one block of 256 threads per 64 x 16 tile of ref pixels. The ref bytes of the tile and its halo of r are staged in
//                             LDS once; then, for every plane inside the kernel: (A) each thread warps its share of tile + halo into LDS,
//                             (B) the rows are box-summed over 2 r + 1 columns into 8-byte partials (sum b^2; sum b, the invalid count and
//                             sum a b packed in the other 8 bytes), rows of 64 consecutive entries, one per lane: ds_read_b64 / ds_write_b64
//                             without bank conflicts, (C) each thread sums 2 r + 1 rows of partials for its four pixels, scores them and
//                             keeps the running best, its predecessor and its successor in registers. No cost volume reaches memory.
//   dense_consistency_kernel  one thread per pixel of map 0
//   DenseCloudScan            mark = the keep byte, scan.h's three kernels, and the scan's write is the scatter of point, colour, normal, confidence
// All sums are integers: the order of execution does not matter. No atomics. Enqueue only.
#include "common.h"
#include "ctx.h"
#include "stage_scratch.h"
#include "dense_pixel.h"

namespace im {
namespace {

constexpr int DENSE_REFUSED = -83;
constexpr int TW = DENSE_TILE_W, TH = DENSE_TILE_H, DENSE_BLOCK = 256;
constexpr int HW = TW + 2 * DENSE_MAX_RADIUS, HH = TH + 2 * DENSE_MAX_RADIUS;      // 78 x 30 with the largest halo
constexpr int PIX = TW * TH / DENSE_BLOCK;                                        // pixels of the tile per thread
constexpr unsigned INV_BIT = 1u << 31;
static_assert(TW == 64 && TW * TH % DENSE_BLOCK == 0, "a row of partials is one entry per lane; whole rounds of the block cover the tile");
// sum b over 15 samples < 2^22 and the invalid count <= 15 share 32 bits; sum a b over 15 samples < 2^30
static_assert(15LL * 261120 < (1LL << 22) && 15LL * 255 * 261120 < (1LL << 31), "the packed row partials");

#include "scan.h"

struct DenseSweepArgs {
    const uint8_t* ref; const uint8_t* src;
    int h0, w0, h1, w1, D, r;
    double A[9], B[9], w_first, w_step, min_score;
    long long min_var;
    int16_t* plane; double* w; float* score;
};

__global__ __launch_bounds__(DENSE_BLOCK) void dense_sweep_kernel(DenseSweepArgs a) {
    __shared__ uint8_t s_a[HH * HW];                  // ref bytes of tile + halo (0 outside ref)
    __shared__ unsigned s_b[HH * HW];                 // the plane's warped values, INV_BIT where invalid
    __shared__ unsigned long long s_bb[HH * TW];      // row partials: sum b^2
    __shared__ uint2 s_px[HH * TW];                   //               x = sum b | invalid count << 22, y = sum a b
    __shared__ double s_AB[18];                       // A and B
    const int t = threadIdx.x, r = a.r, side = 2 * r + 1;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int hw = TW + 2 * r, hh = TH + 2 * r;       // the halo region of this radius, rows of hw entries

    // pixels of this thread: p = t + 256 j -> column p % 64 (one per lane), row p / 64
    int16_t* const o_plane = a.plane; double* const o_w = a.w; float* const o_score = a.score;
    // a tile none of whose pixels has its window inside ref: every pixel is invalid for every plane
    const bool any = x0 + TW > r && x0 < a.w0 - r && y0 + TH > r && y0 < a.h0 - r;
    if (!any) {
#pragma unroll
        for (int j = 0; j < PIX; ++j) {
            const int p = t + DENSE_BLOCK * j, u = x0 + (p & (TW - 1)), v = y0 + p / TW;
            if (u < a.w0 && v < a.h0) {
                const long i = (long)v * a.w0 + u;
                o_plane[i] = -1; o_w[i] = 0.0; o_score[i] = 0.0f;
            }
        }
        return;
    }

    for (int i = t; i < hh * hw; i += DENSE_BLOCK) {
        const int u = x0 - r + i % hw, v = y0 - r + i / hw;
        s_a[i] = (u >= 0 && u < a.w0 && v >= 0 && v < a.h0) ? a.ref[(long)v * a.w0 + u] : (uint8_t)0;
    }
    if (t < 9) { s_AB[t] = a.A[t]; s_AB[9 + t] = a.B[t]; }      // read per plane from LDS: 36 scalar registers less to hold
    __syncthreads();

    const long long n = (long long)side * side;
    long long sa[PIX], saa[PIX];
    unsigned outside[PIX];              // 1: the window leaves ref; starts the count of invalid samples (a word, not a bool: see DenseBest)
    DenseBest best[PIX];
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
        const int p = t + DENSE_BLOCK * j, c = p & (TW - 1), row = p / TW, u = x0 + c, v = y0 + row;
        outside[j] = (u >= r && u < a.w0 - r && v >= r && v < a.h0 - r) ? 0u : 1u;
        dense_best_init(best[j]);
        long long s1 = 0, s2 = 0;
        if (!outside[j])
            for (int dy = 0; dy < side; ++dy)
                for (int dx = 0; dx < side; ++dx) {
                    const int av = s_a[(row + dy) * hw + c + dx];
                    s1 += av; s2 += av * av;
                }
        sa[j] = s1; saa[j] = s2;
    }

    for (int k = 0; k < a.D; ++k) {
        double H[9];
        dense_plane(s_AB, s_AB + 9, a.w_first, a.w_step, k, H);
        // (A) the samples of tile + halo
        for (int i = t; i < hh * hw; i += DENSE_BLOCK) {
            const int u = x0 - r + i % hw, v = y0 - r + i / hw;
            int b = 0;
            const bool ok = u >= 0 && u < a.w0 && v >= 0 && v < a.h0 && dense_sample(a.src, a.h1, a.w1, H, u, v, b);
            s_b[i] = ok ? (unsigned)b : INV_BIT;
        }
        __syncthreads();
        // (B) rows: 2 r + 1 columns
        for (int i = t; i < hh * TW; i += DENSE_BLOCK) {
            const int c = i & (TW - 1), row = i / TW;
            unsigned sb = 0, sab = 0, inv = 0;
            unsigned long long sbb = 0;
            for (int dx = 0; dx < side; ++dx) {
                const unsigned q = s_b[row * hw + c + dx];
                const unsigned b = q & ~INV_BIT;
                inv += q >> 31;
                sb += b; sab += b * s_a[row * hw + c + dx]; sbb += (unsigned long long)b * b;
            }
            s_bb[i] = sbb;
            s_px[i] = make_uint2(sb | (inv << 22), sab);
        }
        __syncthreads();
        // (C) columns: 2 r + 1 rows of partials, the score, the running best
#pragma unroll
        for (int j = 0; j < PIX; ++j) {
            const int p = t + DENSE_BLOCK * j, c = p & (TW - 1), row = p / TW;
            long long sb = 0, sbb = 0, sab = 0;
            unsigned inv = outside[j];
            for (int dy = 0; dy < side; ++dy) {
                const uint2 q = s_px[(row + dy) * TW + c];
                sb += q.x & ((1u << 22) - 1); inv += q.x >> 22; sab += q.y;
                sbb += (long long)s_bb[(row + dy) * TW + c];
            }
            double s = 0.0;
            const bool valid = inv == 0 && dense_score(n, sa[j], saa[j], sb, sbb, sab, a.min_var, s);
            dense_best_step(best[j], k, valid, s);
        }
        // the next plane's (A) writes s_b only, which (B) has finished reading; its barrier orders (C) before the next (B)
    }

#pragma unroll
    for (int j = 0; j < PIX; ++j) {
        const int p = t + DENSE_BLOCK * j, u = x0 + (p & (TW - 1)), v = y0 + p / TW;
        if (u < a.w0 && v < a.h0) {
            const long i = (long)v * a.w0 + u;
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

bool finite_all(const double* p, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}
bool bad_side(int v) { return v < 1 || v > DENSE_MAX_SIDE; }

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
    for (int i = 0; i < 9; ++i) { a.A[i] = h_A[i]; a.B[i] = h_B[i]; }
    IM_LAUNCH(ctx, "dense_sweep", s, launch(dense_sweep_kernel, dim3((unsigned)blocks_of(w0, TW), (unsigned)blocks_of(h0, TH)), DENSE_BLOCK, 0, s, a));
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
