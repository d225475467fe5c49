// What the tiled kernels of the dense stages share (dense.hip, dense_sgm.hip, dense_refine.hip, dense_flow.hip, depth_clean.hip): the tile of
// 64 x 16 pixels that a block of 256 threads owns and the map from a thread to its pixels, the staging of a rectangle of the image around
// the tile into LDS, and the scoring of one plane of the sweep over the tile (samples of tile + halo, packed row partials, column sums,
// dense_score), which dense_sweep_kernel and dense_costs_kernel end differently. The arithmetic is dense_pixel.h's. Kernel text only
// (threadIdx, __shared__, barriers): no host harness includes this header.
#pragma once
#include "dense_pixel.h"

namespace im {
namespace {

// ---- the tile -----------------------------------------------------------------------------------------------------------------------------
constexpr int TW = DENSE_TILE_W, TH = DENSE_TILE_H, TILE_BLOCK = 256;
constexpr int PIX = TW * TH / TILE_BLOCK;                                         // pixels of the tile per thread
static_assert(TW == 64 && TW * TH % TILE_BLOCK == 0, "a row of the tile is one entry per lane; whole rounds of the block cover the tile");

__device__ __forceinline__ int tile_x0() { return blockIdx.x * TW; }
__device__ __forceinline__ int tile_y0() { return blockIdx.y * TH; }

// Pixel p of the tile: column c = p % 64 (one per lane), row = p / 64, at (u, v) of the image
struct TilePixel {
    int p, c, row, u, v;
    __device__ __forceinline__ explicit TilePixel(int p_) : p(p_), c(p_ & (TW - 1)), row(p_ / TW), u(tile_x0() + c), v(tile_y0() + row) {}
    __device__ __forceinline__ bool inside(int h, int w) const { return u < w && v < h; }
    __device__ __forceinline__ long at(int w) const { return (long)v * w + u; }      // the linear index in an image of w columns
};
// pixel j of this thread, j < PIX: p = t + 256 j
__device__ __forceinline__ TilePixel tile_pixel(int j) { return TilePixel((int)threadIdx.x + TILE_BLOCK * j); }

// does any pixel of this tile have its window of radius r inside an image [h][w]?
__device__ __forceinline__ bool tile_any_window_inside(int h, int w, int r) {
    return tile_x0() + TW > r && tile_x0() < w - r && tile_y0() + TH > r && tile_y0() < h - r;
}

// ---- staging ------------------------------------------------------------------------------------------------------------------------------
// The block walks a rectangle of rw x rh entries, rows of rw, whose entry 0 is position (u0, v0) of an image [h][w]: f(i, inside, g, u, v)
// for entry i at position (u, v), g its linear index in the image, which is an address only where `inside`.
template <class F>
__device__ __forceinline__ void tile_stage(int u0, int v0, int rw, int rh, int h, int w, F&& f) {
    for (int i = threadIdx.x; i < rh * rw; i += TILE_BLOCK) {
        const int u = u0 + i % rw, v = v0 + i / rw;
        f(i, u >= 0 && u < w && v >= 0 && v < h, (long)v * w + u, u, v);
    }
}
// the bytes of tile + halo of `halo` pixels, rows of TW + 2 halo, 0 outside the image
__device__ __forceinline__ void tile_stage_bytes(uint8_t* s, const uint8_t* img, int h, int w, int halo) {
    tile_stage(tile_x0() - halo, tile_y0() - halo, TW + 2 * halo, TH + 2 * halo, h, w,
               [&](int i, bool inside, long g, int, int) { s[i] = inside ? img[g] : (uint8_t)0; });
}

// ---- one plane of the sweep over the tile -------------------------------------------------------------------------------------------------
constexpr int HW = TW + 2 * DENSE_MAX_RADIUS, HH = TH + 2 * DENSE_MAX_RADIUS;      // 78 x 30 with the largest halo
constexpr unsigned INV_BIT = 1u << 31;
// sum b over 15 samples < 2^22 and the invalid count <= 15 share 32 bits; sum a b over 15 samples < 2^30
static_assert(15LL * 261120 < (1LL << 22) && 15LL * 255 * 261120 < (1LL << 31), "the packed row partials");

// The LDS of the scoring, one object per block. With radius r the first hh = TH + 2 r rows are in use, rows of hw = TW + 2 r entries in a and b.
struct PlaneLds {
    uint8_t a[HH * HW];                     // ref bytes of tile + halo (0 outside ref)
    unsigned b[HH * HW];                    // the plane's warped values, INV_BIT where invalid
    unsigned long long bb[HH * TW];         // row partials: sum b^2
    uint2 px[HH * TW];                      //               x = sum b | invalid count << 22, y = sum a b
};

// What a thread keeps of ref for its pixels over all planes: the window's sum and sum of squares, and
// outside = 1: the window leaves ref; starts the count of invalid samples (a word, not a bool: see DenseBest)
struct PlaneRef { long long sa[PIX], saa[PIX]; unsigned outside[PIX]; };

// after the barrier behind the staging of L.a
__device__ __forceinline__ void plane_ref_sums(const PlaneLds& L, int h0, int w0, int r, PlaneRef& R) {
    const int hw = TW + 2 * r;
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
        const TilePixel q = tile_pixel(j);
        R.outside[j] = window_inside(q.u, q.v, r, h0, w0) ? 0u : 1u;
        long long s1 = 0, s2 = 0;
        if (!R.outside[j]) dense_window_sums(L.a + (q.row + r) * hw + q.c + r, hw, r, s1, s2);
        R.sa[j] = s1; R.saa[j] = s2;
    }
}

// The plane of homography H (dense_plane) scored at every pixel of the tile: f(j, q, valid, s) for pixel j of this thread, q its TilePixel;
// s is 0 where not valid. Two barriers inside; the caller's loop over the planes needs none of its own, see the end.
template <class F>
__device__ __forceinline__ void plane_scores(PlaneLds& L, const PlaneRef& R, const uint8_t* src, int h0, int w0, int h1, int w1, int r, long long min_var,
                                             const double* H, F&& f) {
    const int t = threadIdx.x, side = 2 * r + 1, hw = TW + 2 * r, hh = TH + 2 * r;
    const long long n = (long long)side * side;
    // (A) the samples of tile + halo
    tile_stage(tile_x0() - r, tile_y0() - r, hw, hh, h0, w0, [&](int i, bool inside, long, int u, int v) {
        int b = 0;
        const bool ok = inside && dense_sample(src, h1, w1, H, u, v, b);
        L.b[i] = ok ? (unsigned)b : INV_BIT;
    });
    __syncthreads();
    // (B) rows: 2 r + 1 columns
    for (int i = t; i < hh * TW; i += TILE_BLOCK) {
        const int c = i & (TW - 1), row = i / TW;
        unsigned sb = 0, sab = 0, inv = 0;
        unsigned long long sbb = 0;
        for (int dx = 0; dx < side; ++dx) {
            const unsigned q = L.b[row * hw + c + dx];
            const unsigned b = q & ~INV_BIT;
            inv += q >> 31;
            sb += b; sab += b * L.a[row * hw + c + dx]; sbb += (unsigned long long)b * b;
        }
        L.bb[i] = sbb;
        L.px[i] = make_uint2(sb | (inv << 22), sab);
    }
    __syncthreads();
    // (C) columns: 2 r + 1 rows of partials, the score
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
        const TilePixel q = tile_pixel(j);
        long long sb = 0, sbb = 0, sab = 0;
        unsigned inv = R.outside[j];
        for (int dy = 0; dy < side; ++dy) {
            const uint2 e = L.px[(q.row + dy) * TW + q.c];
            sb += e.x & ((1u << 22) - 1); inv += e.x >> 22; sab += e.y;
            sbb += (long long)L.bb[(q.row + dy) * TW + q.c];
        }
        double s = 0.0;
        const bool valid = inv == 0 && dense_score(n, R.sa[j], R.saa[j], sb, sbb, sab, min_var, s);
        f(j, q, valid, s);
    }
    // the next plane's (A) writes L.b only, which (B) has finished reading; its barrier orders (C) before the next (B)
}

}  // namespace
}  // namespace im
