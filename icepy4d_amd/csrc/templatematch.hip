// Feature tracking by template matching with orientation correlation (`src/icepy4d/matching/templatematch.py:160-340`, driven
// by `utils/track_targets.py`). The reference correlates each template with its search window through complex64 FFTs
// (`templatematch.py:234-255, 296-301`); what it keeps of the full correlation is the (S - T) x (S - T) block
//   C[i][j] = sum_{ty, tx < T} Ar[ty][tx] Br[i + ty][j + tx] + Ai[ty][tx] Bi[i + ty][j + tx]
// (A = template cut from forient(A), B = search window cut from conj(forient(B)) and conjugated again by the product), and
// that is what is computed here, directly, in fp32 on the vector ALUs: one template per pair makes it a matrix-vector
// contraction, so there is nothing for the matrix cores to take without multiplying the work.
//
//   forient_kernel   one thread per pixel: the 3 x 3 complex filter of `forient` (`:332-340`) and the division by the modulus
//   tm_corr_kernel   C of a tile of one pair: B rows of the tile and a chunk of template rows / columns staged in LDS (both
//                    channels in separate planes), each thread a 1 x 16 strip of C slid along the template columns from a
//                    32-value register window; template rows of a chunk split over `ks` thread groups, summed in a fixed order
//   tm_peak_kernel   one wave per pair: the scan of both windows for a NaN or an infinity, argmax (first maximum in row-major order),
//                    mean |C|, edge test and the sub-pixel centroid of `:303-325` with numpy's own summation order for the float32 /
//                    float64 sums of the window
// The arithmetic of a pair, the plan and the summation order of C are csrc/tm_pair.h, which a host program compiles too.
#include <cmath>

#include "common.h"
#include "ctx.h"
#include "tm_pair.h"

namespace im {
namespace {

static_assert(TM_WAVE == IM_WAVE, "tm_pair.h plans for the wave of common.h");

__global__ __launch_bounds__(256) void forient_kernel(const void* __restrict__ img, int dtype, int h, int w, float2* __restrict__ out) {
    const long n = blockIdx.y;
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.z;
    if (x >= w) return;
    const long base = n * (long)h * w;
    float re, im;
    forient_pixel(img, dtype, base, h, w, y, x, re, im);
    out[base + (long)y * w + x] = make_float2(re, im);
}

__global__ __launch_bounds__(TM_MAX_THREADS) void tm_corr_kernel(const float2* __restrict__ A, int ha, int wa, const float2* __restrict__ B,
                                                                int hb, int wb, const double* __restrict__ pairs,
                                                                const int32_t* __restrict__ bidx, int n_b, long pair0, int T, int S, float isign,
                                                                TmPlan p, float* __restrict__ C) {
    extern __shared__ float lds[];
    const int tiles = p.ny * p.nx;
    const long pl = blockIdx.x / tiles;
    const int tile = blockIdx.x - (int)(pl * tiles);
    const PairWin w = pair_window(pairs, bidx, n_b, pair0 + pl, T, S, ha, wa, hb, wb);
    if (!w.valid) return;
    const int oy0 = (tile / p.nx) * p.gy, ox0 = (tile % p.nx) * p.gx * TM_DX;
    const int tid = threadIdx.x;
    const int y = tid % p.gy, x = (tid / p.gy) % p.gx, k = tid / (p.gy * p.gx);
    const bool active = k < p.ks;
    float* sBr = lds;
    float* sBi = sBr + p.brows * p.pitch;
    float* sAr = sBi + p.brows * p.pitch;
    float* sAi = sAr + p.kt * p.kx;
    const float2* Bimg = B + (long)bidx[pair0 + pl] * hb * wb;
    float acc[TM_DX];
#pragma unroll
    for (int q = 0; q < TM_DX; ++q) acc[q] = 0.f;

    for (int cy = 0; cy < T; cy += p.kt) {
        for (int cx = 0; cx < T; cx += p.kx) {
            __syncthreads();
            // B rows oy0 + cy + r and columns ox0 + cx + c of the search window; zero outside it
            for (int e = tid; e < p.brows * p.pitch; e += blockDim.x) {
                const int r = e / p.pitch, c = e - r * p.pitch;
                const int sy = oy0 + cy + r, sx = ox0 + cx + c;
                float2 b = make_float2(0.f, 0.f);
                if (sy < S && sx < S) b = Bimg[(w.brow + sy) * wb + w.bcol + sx];
                sBr[e] = b.x;
                sBi[e] = b.y;
            }
            // template rows cy + r, columns cx + c; zero outside T x T
            for (int e = tid; e < p.kt * p.kx; e += blockDim.x) {
                const int r = e / p.kx, c = e - r * p.kx;
                float2 a = make_float2(0.f, 0.f);
                if (cy + r < T && cx + c < T) a = A[(w.arow + cy + r) * wa + w.acol + cx + c];
                sAr[e] = a.x;
                sAi[e] = isign * a.y;
            }
            __syncthreads();
            if (!active) continue;
            for (int r = k; r < p.kt; r += p.ks) {
#pragma unroll
                for (int ch = 0; ch < 2; ++ch) {
                    const float* brow = (ch ? sBi : sBr) + (y + r) * p.pitch + TM_DX * x;
                    const float* arow = (ch ? sAi : sAr) + r * p.kx;
                    f32x4 win[8];
#pragma unroll
                    for (int v = 0; v < 4; ++v) win[v] = *reinterpret_cast<const f32x4*>(brow + 4 * v);
                    for (int t0 = 0; t0 < p.kx; t0 += 16) {
#pragma unroll
                        for (int v = 0; v < 4; ++v) win[4 + v] = *reinterpret_cast<const f32x4*>(brow + t0 + 16 + 4 * v);
                        f32x4 a4[4];
#pragma unroll
                        for (int v = 0; v < 4; ++v) a4[v] = *reinterpret_cast<const f32x4*>(arow + t0 + 4 * v);
#pragma unroll
                        for (int tt = 0; tt < 16; ++tt) {
                            const float a = a4[tt >> 2][tt & 3];
#pragma unroll
                            for (int q = 0; q < TM_DX; ++q) acc[q] = fmaf(a, win[(q + tt) >> 2][(q + tt) & 3], acc[q]);
                        }
#pragma unroll
                        for (int v = 0; v < 4; ++v) win[v] = win[4 + v];
                    }
                }
            }
        }
    }

    float* Cp = C + pl * (long)p.R * p.R;
    if (p.ks == 1) {
        if (!active) return;
        const int i = oy0 + y;
#pragma unroll
        for (int q = 0; q < TM_DX; ++q) {
            const int j = ox0 + TM_DX * x + q;
            if (i < p.R && j < p.R) Cp[i * p.R + j] = acc[q];
        }
        return;
    }
    // the ks partial sums of every output, added in group order
    __syncthreads();
    const int per = p.gy * p.gx * TM_DX;
    if (active) {
#pragma unroll
        for (int q = 0; q < TM_DX; ++q) lds[k * per + (x * p.gy + y) * TM_DX + q] = acc[q];
    }
    __syncthreads();
    for (int o = tid; o < per; o += blockDim.x) {
        float s = lds[o];
        for (int kk = 1; kk < p.ks; ++kk) s += lds[kk * per + o];
        const int q = o % TM_DX, yx = o / TM_DX, yy = yx % p.gy, xx = yx / p.gy;
        const int i = oy0 + yy, j = ox0 + TM_DX * xx + q;
        if (i < p.R && j < p.R) Cp[i * p.R + j] = s;
    }
}

// one wave per pair: `templatematch.py:303-329`. A pair whose template or search window holds a NaN or an infinity keeps NaN in du, dv,
// peakCorr and meanAbsCorr, as the reference's FFT of such a window leaves them.
__global__ __launch_bounds__(256) void tm_peak_kernel(const float2* __restrict__ A, const float2* __restrict__ B, const double* __restrict__ pairs,
                                                      const int32_t* __restrict__ bidx, int n_b, long pair0, long n_batch, int T, int S, int ha, int wa,
                                                      int hb, int wb, const float* __restrict__ C, long n_pairs, double* __restrict__ out) {
    const long pl = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (pl >= n_batch) return;
    const long pi = pair0 + pl;
    const PairWin w = pair_window(pairs, bidx, n_b, pi, T, S, ha, wa, hb, wb);
    double* o_pu = out;
    double* o_pv = out + n_pairs;
    double* o_du = out + 2 * n_pairs;
    double* o_dv = out + 3 * n_pairs;
    double* o_pk = out + 4 * n_pairs;
    double* o_mc = out + 5 * n_pairs;
    if (lane == 0) {
        o_pu[pi] = w.pu; o_pv[pi] = w.pv;
        o_du[pi] = NAN; o_dv[pi] = NAN; o_pk[pi] = NAN; o_mc[pi] = NAN;
    }
    if (!w.valid) return;
    const float* Bimg = reinterpret_cast<const float*>(B + (long)bidx[pi] * hb * wb);
    const bool bad = tm_window_not_finite(reinterpret_cast<const float*>(A), w.arow, w.acol, wa, T, lane) ||
                     tm_window_not_finite(Bimg, w.brow, w.bcol, wb, S, lane);
    if (__any(bad)) return;
    const int R = S - T, n = R * R;
    const float* Cp = C + pl * (long)n;
    float best;
    int bi;
    double sabs;
    tm_lane_scan(Cp, n, lane, best, bi, sabs);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        tm_best_merge(best, bi, __shfl_xor(best, o), __shfl_xor(bi, o));
        sabs += __shfl_xor(sabs, o);
    }
    if (lane != 0) return;
    double r[4];
    tm_peak_tail(Cp, R, bi, best, sabs, w.initdu, w.initdv, r);
    o_du[pi] = r[0]; o_dv[pi] = r[1]; o_pk[pi] = r[2]; o_mc[pi] = r[3];
}

hipError_t launch_forient(const void* img, int dtype, int n, int h, int w, float* out, hipStream_t s) {
    hipLaunchKernelGGL(forient_kernel, dim3((unsigned)blocks_of(w, 256), n, h), dim3(256), 0, s, img, dtype, h, w, reinterpret_cast<float2*>(out));
    return hipGetLastError();
}

hipError_t launch_corr(const TmPlan& p, long blocks, const float2* A, int ha, int wa, const float2* B, int hb, int wb, const double* pairs,
                       const int32_t* bidx, int n_b, long pair0, int T, int S, float isign, float* C, hipStream_t s) {
    hipLaunchKernelGGL(tm_corr_kernel, dim3((unsigned)blocks), dim3(p.threads), p.lds_floats * sizeof(float), s, A, ha, wa, B, hb, wb, pairs,
                       bidx, n_b, pair0, T, S, isign, p, C);
    return hipGetLastError();
}

hipError_t launch_peak(const float2* A, const float2* B, const double* pairs, const int32_t* bidx, int n_b, long pair0, long nb, int T, int S, int ha, int wa, int hb, int wb,
                       const float* C, long n_pairs, double* out, hipStream_t s) {
    hipLaunchKernelGGL(tm_peak_kernel, dim3((unsigned)blocks_of(nb, 4)), dim3(256), 0, s, A, B, pairs, bidx, n_b, pair0, nb, T, S, ha, wa, hb,
                       wb, C, n_pairs, out);
    return hipGetLastError();
}

}  // namespace
}  // namespace im

using namespace im;

extern "C" int im_forient(im_ctx* ctx, const void* d_img, int dtype, int n_images, int h, int w, float* d_out, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_img || !d_out || (dtype != 0 && dtype != 1) || n_images < 0 || h < 0 || w < 0 || n_images > 65535 || h > 65535)
        return ctx->fail(-72, "im_forient: bad arguments");
    if (!n_images || !h || !w) return 0;
    hipStream_t s = (hipStream_t)stream;
    IM_LAUNCH(ctx, "forient", s, launch_forient(d_img, dtype, n_images, h, w, d_out, s));
    IM_GUARD_CHECK(ctx, s, "im_forient");
    return 0;
}

// what im_template_match_oc and im_template_match_corr refuse; 0 when the arguments are fine
static int tm_refuse(im_ctx* ctx, const char* who, const float* d_a, int ha, int wa, const float* d_b, int n_b, int hb, int wb, const double* d_pairs,
                     const int32_t* d_bidx, int n_pairs, int T, int S, const void* d_out) {
    if (!d_a || !d_b || !d_pairs || !d_bidx || !d_out || n_pairs < 0 || n_b < 1 || ha < 0 || wa < 0 || hb < 0 || wb < 0)
        return ctx->fail(-72, "%s: bad arguments", who);
    if (T < 1 || S <= T) return ctx->fail(-72, "%s: need 1 <= template width < search width (got %d, %d)", who, T, S);
    return 0;
}

extern "C" int im_template_match_oc(im_ctx* ctx, const float* d_a, int ha, int wa, const float* d_b, int n_b, int hb, int wb,
                                    const double* d_pairs, const int32_t* d_bidx, int n_pairs, int T, int S, int conj_b,
                                    double* d_out, void* stream) {
    IM_CHECK_CTX(ctx);
    if (const int rc = tm_refuse(ctx, "im_template_match_oc", d_a, ha, wa, d_b, n_b, hb, wb, d_pairs, d_bidx, n_pairs, T, S, d_out)) return rc;
    if (!n_pairs) return 0;
    hipStream_t s = (hipStream_t)stream;
    const TmPlan p = tm_plan(T, S);
    const long per_pair = (long)p.R * p.R;
    // C of one batch of pairs lives in a scratch buffer of at most 64 Mi floats (grown on demand)
    const long batch = std::max(1L, std::min((long)n_pairs, (64L << 20) / per_pair));
    const size_t need = (size_t)(batch * per_pair);
    IM_GROW(ctx, ctx->grow(ctx->scratch.tm, need * sizeof(float), "templatematch.C"), -71, "im_template_match_oc: out of device memory (%zu floats)", need);
    float* const C = ctx->scratch.tm.as<float>();
    const float2* A = reinterpret_cast<const float2*>(d_a);
    const float2* B = reinterpret_cast<const float2*>(d_b);
    const float isign = conj_b ? 1.f : -1.f;
    for (long p0 = 0; p0 < n_pairs; p0 += batch) {
        const long nb = std::min(batch, (long)n_pairs - p0);
        const long blocks = nb * p.ny * p.nx;
        if (blocks > 0x7fffffffL) return ctx->fail(-72, "im_template_match_oc: too many pairs per launch");
        IM_LAUNCH(ctx, "tm_corr", s, launch_corr(p, blocks, A, ha, wa, B, hb, wb, d_pairs, d_bidx, n_b, p0, T, S, isign, C, s));
        IM_LAUNCH(ctx, "tm_peak", s, launch_peak(A, B, d_pairs, d_bidx, n_b, p0, nb, T, S, ha, wa, hb, wb, C, (long)n_pairs, d_out, s));
    }
    IM_GUARD_CHECK(ctx, s, "im_template_match_oc");
    return 0;
}

extern "C" int im_template_match_corr(im_ctx* ctx, const float* d_a, int ha, int wa, const float* d_b, int n_b, int hb, int wb,
                                      const double* d_pairs, const int32_t* d_bidx, int n_pairs, int T, int S, int conj_b, float* d_c,
                                      void* stream) {
    IM_CHECK_CTX(ctx);
    if (const int rc = tm_refuse(ctx, "im_template_match_corr", d_a, ha, wa, d_b, n_b, hb, wb, d_pairs, d_bidx, n_pairs, T, S, d_c)) return rc;
    if (!n_pairs) return 0;
    hipStream_t s = (hipStream_t)stream;
    const TmPlan p = tm_plan(T, S);
    const long blocks = (long)n_pairs * p.ny * p.nx;
    if (blocks > 0x7fffffffL) return ctx->fail(-72, "im_template_match_corr: too many pairs per launch");
    IM_LAUNCH(ctx, "tm_corr", s, launch_corr(p, blocks, reinterpret_cast<const float2*>(d_a), ha, wa, reinterpret_cast<const float2*>(d_b), hb, wb,
                                             d_pairs, d_bidx, n_b, 0, T, S, conj_b ? 1.f : -1.f, d_c, s));
    IM_GUARD_CHECK(ctx, s, "im_template_match_corr");
    return 0;
}
