// Semi-global regularisation of a dense-stereo depth map on the device: the sweep's scores as an 8-bit cost volume, min-plus path costs
// summed over four or eight directions, and the choice of the plane of least sum (sgm_pixel.h), pinned bit for bit against
// tests/sgm_oracle.py. The sample, the box sums and the score are dense_pixel.h's, as in dense.hip. A definition of this project's own;
// it is not Metashape's depth filter.
//
//   dense_costs_kernel       one block of 256 threads per 64 x 16 tile of ref pixels, the plane loop of dense_sweep_kernel (samples of tile
//                            + halo into LDS, row partials, column sums, score: plane_scores of dense_tile.h, defined once for the two
//                            kernels); each score is quantised, four planes are packed into a word per pixel and sixteen planes are
//                            staged in LDS, then stored as runs: whole words where D is a multiple of four (a pixel's sixteen bytes from
//                            four neighbouring lanes), bytes in plane order otherwise.
//   dense_sgm_kernel         one wave per path line (a row, a column, a diagonal or an anti-diagonal), four lines per block. Lane l holds
//                            L(q, 4 l .. 4 l + 3) in registers; planes at or beyond D hold SGM_FAR, which never wins and is never stored.
//                            d - 1 and d + 1 across lanes come from __shfl_up / __shfl_down, m from the xor butterfly. The wave walks its
//                            line forwards and then backwards: one launch covers two opposite directions and no two waves touch one element
//                            of `sum`. The first walk of the first launch stores, every other adds. Costs and sums are fetched four pixels
//                            ahead of the recurrence, which is what bounds a line.
//   dense_sgm_choose_kernel  sixteen lanes per pixel: each takes every sixteenth plane, a butterfly over (S << 16 | k) keeps the least.
// Everything is an integer behind the score: the order of execution does not matter. No atomics. Enqueue only.
#include "common.h"
#include "ctx.h"
#include "dense_tile.h"
#include "dense_host.h"
#include "sgm_pixel.h"

namespace im {
namespace {

constexpr int GROUP = 16;                                // planes staged per tile before they are stored
static_assert(SGM_MAX_PLANES == 4 * IM_WAVE, "four planes per lane");

struct DenseCostArgs {
    const uint8_t* ref; const uint8_t* src;
    int h0, w0, h1, w1, D, r;
    double A[9], B[9], w_first, w_step;
    long long min_var;
    uint8_t* cost;
};

__global__ __launch_bounds__(TILE_BLOCK) void dense_costs_kernel(DenseCostArgs a) {
    __shared__ PlaneLds L;                            // dense_tile.h: ref bytes, the plane's samples, the two rows of partials
    __shared__ double s_AB[20];                       // A, B, w_first and w_step: read per plane from LDS, 40 scalar registers less to hold
    __shared__ unsigned s_c[TW * TH * GROUP / 4];     // GROUP planes of every pixel of the tile, planes contiguous
    const int t = threadIdx.x, r = a.r, D = a.D;
    uint8_t* const o_cost = a.cost;

    // a tile none of whose pixels has its window inside ref: every plane of every pixel is invalid. A row of the tile is one run of bytes
    if (!tile_any_window_inside(a.h0, a.w0, r)) {
        const int cols = min(TW, a.w0 - tile_x0());
        for (int row = 0; row < TH && tile_y0() + row < a.h0; ++row) {
            uint8_t* const run = o_cost + ((size_t)(tile_y0() + row) * a.w0 + tile_x0()) * D;
            for (int i = t; i < cols * D; i += TILE_BLOCK) run[i] = (uint8_t)SGM_INVALID;
        }
        return;
    }

    tile_stage_bytes(L.a, a.ref, a.h0, a.w0, r);
    if (t < 9) { s_AB[t] = a.A[t]; s_AB[9 + t] = a.B[t]; }
    if (t == 9) { s_AB[18] = a.w_first; s_AB[19] = a.w_step; }
    __syncthreads();

    PlaneRef R;
    plane_ref_sums(L, a.h0, a.w0, r, R);
    unsigned pack[PIX] = {};

    for (int k = 0; k < D; ++k) {
        double H[9];
        dense_plane(s_AB, s_AB + 9, s_AB[18], s_AB[19], k, H);
        // the score of plane k at every pixel, its cost into byte k % 4 of the pixel's word
        const bool word_done = (k & 3) == 3 || k == D - 1;
        plane_scores(L, R, a.src, a.h0, a.w0, a.h1, a.w1, r, a.min_var, H, [&](int j, const TilePixel& q, bool valid, double s) {
            pack[j] |= (unsigned)sgm_cost(valid, s) << (8 * (k & 3));
            if (word_done) { s_c[q.p * (GROUP / 4) + ((k / 4) & (GROUP / 4 - 1))] = pack[j]; pack[j] = 0; }
        });
        // the staged planes k0 .. k of every pixel, as runs. The next write into s_c lies behind the two barriers of a later plane.
        if ((k & (GROUP - 1)) == GROUP - 1 || k == D - 1) {
            __syncthreads();
            const int k0 = k & ~(GROUP - 1), cnt = k - k0 + 1;
            if ((D & 3) == 0 && (reinterpret_cast<unsigned long long>(o_cost) & 3) == 0) {      // whole aligned words
                for (int i = t; i < TW * TH * (GROUP / 4); i += TILE_BLOCK) {
                    const TilePixel q(i / (GROUP / 4));
                    const int j = i & (GROUP / 4 - 1);
                    if (4 * j < cnt && q.inside(a.h0, a.w0))
                        *reinterpret_cast<unsigned*>(o_cost + (size_t)q.at(a.w0) * D + k0 + 4 * j) = s_c[i];
                }
            } else {
                for (int i = t; i < TW * TH * GROUP; i += TILE_BLOCK) {
                    const TilePixel q(i / GROUP);
                    const int b = i & (GROUP - 1);
                    if (b < cnt && q.inside(a.h0, a.w0))
                        o_cost[(size_t)q.at(a.w0) * D + k0 + b] = (uint8_t)(s_c[i >> 2] >> (8 * (i & 3)));
                }
            }
        }
    }
}

// ---- aggregation -------------------------------------------------------------------------------------------------------------------------
enum { LINE_ROW = 0, LINE_COLUMN = 1, LINE_DIAGONAL = 2, LINE_ANTIDIAGONAL = 3 };
constexpr int SGM_BLOCK = 256, LINES_PER_BLOCK = SGM_BLOCK / IM_WAVE, AHEAD = 4;

struct SgmArgs {
    const uint8_t* cost; uint16_t* sum;
    int h0, w0, D, P1, P2, kind, first;
};

// The four cost bytes of planes d0 .. d0 + 3 of one pixel (`p` its plane 0) as one word. The lane that straddles D reads on into the next
// pixel's first planes (`whole`: the four elements lie inside the volume), whose values nobody uses: assembling single bytes would wait
// for each of them at once and undo the fetch ahead. Only at the volume's last pixel does that lane go byte by byte.
__device__ __forceinline__ unsigned sgm_cost4(const uint8_t* p, int d0, int D, bool whole) {
    unsigned v = 0xFFFFFFFFu;
    if (whole) {
        __builtin_memcpy(&v, p + d0, 4);
    } else {
        for (int j = 0; j < 4; ++j)
            if (d0 + j < D) v = (v & ~(0xFFu << (8 * j))) | ((unsigned)p[d0 + j] << (8 * j));
    }
    return v;
}
__device__ __forceinline__ uint2 sgm_sum4(const uint16_t* p, int d0, int D, bool whole) {
    uint2 v = make_uint2(0u, 0u);
    if (whole) {
        __builtin_memcpy(&v, p + d0, 8);
    } else {
        unsigned e[4] = {0u, 0u, 0u, 0u};
        for (int j = 0; j < 4; ++j)
            if (d0 + j < D) e[j] = p[d0 + j];
        v = make_uint2(e[0] | (e[1] << 16), e[2] | (e[3] << 16));
    }
    return v;
}
__device__ __forceinline__ void sgm_store4(uint16_t* p, int d0, int D, uint2 v) {
    if (d0 + 4 <= D) {
        __builtin_memcpy(p + d0, &v, 8);
    } else {
        const unsigned e[4] = {v.x & 0xFFFFu, v.x >> 16, v.y & 0xFFFFu, v.y >> 16};
        for (int j = 0; j < 4; ++j)
            if (d0 + j < D) p[d0 + j] = (uint16_t)e[j];
    }
}

struct SgmAhead { unsigned c[AHEAD]; uint2 s[AHEAD]; };

// One walk over the n pixels pix0, pix0 + stride, ... of a line: the path costs of the direction of the walk, stored into or added to `sum`
template <bool STORE>
__device__ __forceinline__ void sgm_walk(const SgmArgs& a, long long pix0, long long stride, int n, int lane) {
    const int d0 = 4 * lane, D = a.D;
    const bool mine = d0 < D;                         // lanes beyond the planes take part in the shuffles only
    const size_t total = (size_t)a.h0 * a.w0 * D;
    auto fetch = [&](int base, SgmAhead& f) {
#pragma unroll
        for (int j = 0; j < AHEAD; ++j) {
            f.c[j] = 0xFFFFFFFFu; f.s[j] = make_uint2(0u, 0u);
            if (mine && base + j < n) {
                const size_t e = (size_t)(pix0 + (base + j) * stride) * D;
                const bool whole = e + d0 + 4 <= total;
                f.c[j] = sgm_cost4(a.cost + e, d0, D, whole);
                if (!STORE) f.s[j] = sgm_sum4(a.sum + e, d0, D, whole);
            }
        }
    };
    int L[4] = {SGM_FAR, SGM_FAR, SGM_FAR, SGM_FAR};
    SgmAhead cur, nxt;
    fetch(0, cur);
    for (int base = 0; base < n; base += AHEAD) {
        fetch(base + AHEAD, nxt);
#pragma unroll
        for (int j = 0; j < AHEAD; ++j) {
            if (base + j < n) {                       // uniform over the wave
                int c[4], N[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) c[q] = (int)((cur.c[j] >> (8 * q)) & 0xFFu);
                if (base + j == 0) {                  // the pixel before lies outside the image
#pragma unroll
                    for (int q = 0; q < 4; ++q) N[q] = c[q];
                } else {
                    int below = __shfl_up(L[3], 1), above = __shfl_down(L[0], 1);
                    if (lane == 0) below = SGM_FAR;
                    if (lane == IM_WAVE - 1) above = SGM_FAR;
                    int m = min(min(L[0], L[1]), min(L[2], L[3]));
#pragma unroll
                    for (int o = IM_WAVE / 2; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o));
                    N[0] = sgm_step(c[0], L[0], below, L[1], m, a.P1, a.P2);
                    N[1] = sgm_step(c[1], L[1], L[0], L[2], m, a.P1, a.P2);
                    N[2] = sgm_step(c[2], L[2], L[1], L[3], m, a.P1, a.P2);
                    N[3] = sgm_step(c[3], L[3], L[2], above, m, a.P1, a.P2);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) L[q] = d0 + q < D ? N[q] : SGM_FAR;
                if (mine) {
                    // 16-bit halves never carry: every partial sum of at most eight L <= 4350 stays below 2^16, and a half at or beyond D is dropped
                    const uint2 v = make_uint2(cur.s[j].x + (((unsigned)N[0] & 0xFFFFu) | ((unsigned)N[1] << 16)),
                                               cur.s[j].y + (((unsigned)N[2] & 0xFFFFu) | ((unsigned)N[3] << 16)));
                    sgm_store4(a.sum + (size_t)(pix0 + (base + j) * stride) * D, d0, D, v);
                }
            }
        }
        cur = nxt;
    }
}

__global__ __launch_bounds__(SGM_BLOCK) void dense_sgm_kernel(SgmArgs a) {
    const int lane = threadIdx.x & (IM_WAVE - 1);
    const int line = blockIdx.x * LINES_PER_BLOCK + (int)(threadIdx.x / IM_WAVE);
    const int h0 = a.h0, w0 = a.w0;
    int ys = 0, xs = 0, n = 0;
    long long stride = 1;
    if (a.kind == LINE_ROW) {
        if (line >= h0) return;
        ys = line; n = w0;
    } else if (a.kind == LINE_COLUMN) {
        if (line >= w0) return;
        xs = line; n = h0; stride = w0;
    } else if (a.kind == LINE_DIAGONAL) {             // x - y = line - (h0 - 1), walked down and to the right
        if (line >= h0 + w0 - 1) return;
        const int c = line - (h0 - 1);
        ys = c < 0 ? -c : 0; xs = c > 0 ? c : 0;
        n = min(h0 - ys, w0 - xs); stride = (long long)w0 + 1;
    } else {                                          // x + y = line, walked down and to the left
        if (line >= h0 + w0 - 1) return;
        ys = max(0, line - (w0 - 1)); xs = line - ys;
        n = min(h0 - ys, xs + 1); stride = (long long)w0 - 1;
    }
    const long long pix0 = (long long)ys * w0 + xs;
    if (a.first) sgm_walk<true>(a, pix0, stride, n, lane);
    else sgm_walk<false>(a, pix0, stride, n, lane);
    sgm_walk<false>(a, pix0 + (n - 1) * stride, -stride, n, lane);
}

// ---- choice ------------------------------------------------------------------------------------------------------------------------------
constexpr int CHOOSE_BLOCK = 256, CHOOSE_LANES = 16;
static_assert(IM_WAVE % CHOOSE_LANES == 0, "the pixels of a wave are whole groups of lanes");

struct SgmChooseArgs {
    const uint8_t* cost; const uint16_t* sum;
    int h0, w0, D;
    double w_first, w_step, min_score;
    int16_t* plane; double* w; float* score;
};

__global__ __launch_bounds__(CHOOSE_BLOCK) void dense_sgm_choose_kernel(SgmChooseArgs a) {
    const long long pix = (long long)blockIdx.x * (CHOOSE_BLOCK / CHOOSE_LANES) + threadIdx.x / CHOOSE_LANES;
    const int sub = threadIdx.x & (CHOOSE_LANES - 1), D = a.D;
    const bool in = pix < (long long)a.h0 * a.w0;     // every lane stays for the butterfly
    const uint8_t* const c = a.cost + (size_t)(in ? pix : 0) * D;
    const uint16_t* const S = a.sum + (size_t)(in ? pix : 0) * D;
    unsigned key = SGM_NO_KEY;
    if (in)
        for (int k = sub; k < D; k += CHOOSE_LANES) key = min(key, sgm_key(c[k], S[k], k));
#pragma unroll
    for (int o = CHOOSE_LANES / 2; o > 0; o >>= 1) key = min(key, (unsigned)__shfl_xor((int)key, o));
    if (!in || sub != 0) return;
    int c0 = SGM_INVALID, cm = SGM_INVALID, cp = SGM_INVALID, Sm = 0, Sp = 0;
    if (key != SGM_NO_KEY) {
        const int k = (int)(key & 0xFFFFu);
        c0 = c[k];
        if (k >= 1 && k <= D - 2) { cm = c[k - 1]; cp = c[k + 1]; Sm = S[k - 1]; Sp = S[k + 1]; }
    }
    int16_t plane; double w; float score;
    sgm_finish(key, D, c0, cm, cp, Sm, Sp, a.w_first, a.w_step, a.min_score, plane, w, score);
    a.plane[pix] = plane; a.w[pix] = w; a.score[pix] = score;
}

bool bad_planes(int D) { return D < 1 || D > SGM_MAX_PLANES; }
bool too_large(int h0, int w0, int D) { return (long long)h0 * w0 * D > (1LL << 32); }

}  // namespace
}  // namespace im

using namespace im;

extern "C" {

int im_dense_sgm_max_planes(void) { return SGM_MAX_PLANES; }

int im_dense_costs(im_ctx* ctx, const uint8_t* d_ref, int h0, int w0, const uint8_t* d_src, int h1, int w1, const double* h_A, const double* h_B,
                   double w_first, double w_step, int D, int r, long long min_var, uint8_t* d_cost, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_ref || !d_src || !h_A || !h_B || !d_cost) return ctx->fail(DENSE_REFUSED, "im_dense_costs: null pointer");
    if (bad_side(h0) || bad_side(w0) || bad_side(h1) || bad_side(w1)) return ctx->fail(DENSE_REFUSED, "im_dense_costs: h and w must be 1..16384");
    if (bad_planes(D)) return ctx->fail(DENSE_REFUSED, "im_dense_costs: D must be 1..256");
    if (r < 1 || r > DENSE_MAX_RADIUS) return ctx->fail(DENSE_REFUSED, "im_dense_costs: r must be 1..7");
    if (min_var < 0 || min_var > (1LL << 26)) return ctx->fail(DENSE_REFUSED, "im_dense_costs: min_var must be 0..2^26");
    if (too_large(h0, w0, D)) return ctx->fail(DENSE_REFUSED, "im_dense_costs: h0 w0 D must be at most 2^32");
    hipStream_t s = (hipStream_t)stream;
    DenseCostArgs a{d_ref, d_src, h0, w0, h1, w1, D, r, {}, {}, w_first, w_step, min_var, d_cost};
    copy_matrices(h_A, h_B, a.A, a.B);
    IM_LAUNCH(ctx, "dense_costs", s, launch(dense_costs_kernel, dim3((unsigned)blocks_of(w0, TW), (unsigned)blocks_of(h0, TH)), TILE_BLOCK, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_dense_costs");
    return 0;
}

int im_dense_sgm(im_ctx* ctx, const uint8_t* d_cost, int h0, int w0, int D, int P1, int P2, int paths, uint16_t* d_sum, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_cost || !d_sum) return ctx->fail(DENSE_REFUSED, "im_dense_sgm: null pointer");
    if (bad_side(h0) || bad_side(w0)) return ctx->fail(DENSE_REFUSED, "im_dense_sgm: h and w must be 1..16384");
    if (bad_planes(D)) return ctx->fail(DENSE_REFUSED, "im_dense_sgm: D must be 1..256");
    if (P1 < 0 || P1 > P2 || P2 > SGM_MAX_PENALTY) return ctx->fail(DENSE_REFUSED, "im_dense_sgm: 0 <= P1 <= P2 <= 4095 is expected");
    if (paths != 4 && paths != 8) return ctx->fail(DENSE_REFUSED, "im_dense_sgm: paths must be 4 or 8");
    if (too_large(h0, w0, D)) return ctx->fail(DENSE_REFUSED, "im_dense_sgm: h0 w0 D must be at most 2^32");
    hipStream_t s = (hipStream_t)stream;
    // one launch per pair of opposite directions; the stream orders them, so the adds of one launch meet the finished sums of the one before
    for (int kind = 0; kind < paths / 2; ++kind) {
        const int lines = kind == LINE_ROW ? h0 : kind == LINE_COLUMN ? w0 : h0 + w0 - 1;
        SgmArgs a{d_cost, d_sum, h0, w0, D, P1, P2, kind, kind == 0 ? 1 : 0};
        IM_LAUNCH(ctx, "dense_sgm", s, launch(dense_sgm_kernel, (unsigned)blocks_of(lines, LINES_PER_BLOCK), SGM_BLOCK, 0, s, a));
    }
    IM_GUARD_CHECK(ctx, s, "im_dense_sgm");
    return 0;
}

int im_dense_sgm_choose(im_ctx* ctx, const uint8_t* d_cost, const uint16_t* d_sum, int h0, int w0, int D, double w_first, double w_step,
                        double min_score, int16_t* d_plane, double* d_w, float* d_score, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_cost || !d_sum || !d_plane || !d_w || !d_score) return ctx->fail(DENSE_REFUSED, "im_dense_sgm_choose: null pointer");
    if (bad_side(h0) || bad_side(w0)) return ctx->fail(DENSE_REFUSED, "im_dense_sgm_choose: h and w must be 1..16384");
    if (bad_planes(D)) return ctx->fail(DENSE_REFUSED, "im_dense_sgm_choose: D must be 1..256");
    if (too_large(h0, w0, D)) return ctx->fail(DENSE_REFUSED, "im_dense_sgm_choose: h0 w0 D must be at most 2^32");
    hipStream_t s = (hipStream_t)stream;
    SgmChooseArgs a{d_cost, d_sum, h0, w0, D, w_first, w_step, min_score, d_plane, d_w, d_score};
    IM_LAUNCH(ctx, "dense_sgm_choose", s,
              launch(dense_sgm_choose_kernel, (unsigned)blocks_of((long long)h0 * w0, CHOOSE_BLOCK / CHOOSE_LANES), CHOOSE_BLOCK, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_dense_sgm_choose");
    return 0;
}

}  // extern "C"
