// Depth-map clean-up on the device: the connected components of a depth map, the removal of small components (speckles) and the filling of
// small holes (depth_pixel.h), pinned bit for bit against tests/depth_oracle.py. A definition of this project's own; it is not
// OpenCV's filterSpeckles and not Metashape's depth filter.
//
// Labelling is a union-find over the label array itself, parent[i] <= i, in separate launches on one stream:
//   depth_tile_kernel      one block of 256 threads per 64 x 16 tile (the sweep's tile and its map from a thread to its pixels: dense_tile.h):
//                          planes, parents and counts of the tile in LDS (10 KB), every pixel linked with its left and upper
//                          neighbour inside the tile (depth_link on LDS) and counted on its local root, then every
//                          pixel's root written as a GLOBAL linear index and, on a root's slot of the scratch array, the pixels the tile
//                          holds of it (0 elsewhere). Local and global indices order the pixels of a tile alike, so the local root is the
//                          least global index.
//   depth_merge_kernel     one thread per pixel of a tile's first column or row (but the image's): the join across the tile edge by the lock-free
//                          depth_link on global memory. Parents are read by relaxed device-scope atomic loads; a stale one is still an ancestor.
//   depth_flatten_kernel   every root of a tile (the merge moves no other slot) finds its root, stores it as its label and adds its tile's
//                          count to the root's slot: one atomicAdd per tile and component, not per pixel.
//   depth_size_kernel      every pixel takes the label of its tile's root, which is the root by now, and size = the count there.
// No block ever waits for another block's store: the launch boundaries order the phases, every loop descends a chain of falling indices.
// The root of a finished component is its least index, which is the definition: nothing is renumbered.
//   depth_drop_kernel      plane = -1, w = 0, score = 0 where the component is smaller than min_size; one count per wave.
//   depth_rim_init_kernel / depth_rim_kernel / depth_fill_kernel   per hole (mode-1 labels and sizes are inputs): lo / hi of the planes around it
//                          by atomicMin / atomicMax and the border flag by atomicOr on the root's slots, then per pixel the decision, the four
//                          anchors (walks of at most max_hole pixels along the input maps) and the interpolation.
// Every atomic is an integer: the order of execution does not matter. Enqueue only.
#include "common.h"
#include "ctx.h"
#include "stage_scratch.h"
#include "depth_pixel.h"
#include "dense_tile.h"
#include "dense_host.h"

namespace im {
namespace {

// the labelling's tile is the sweep's (TW, TH, PIX and the map from a thread to its pixels are dense_tile.h's); so is the limit on a side
constexpr int DEPTH_BLOCK = TILE_BLOCK;
static_assert(DEPTH_TILE_W == TW && DEPTH_TILE_H == TH && DEPTH_MAX_SIDE == DENSE_MAX_SIDE, "im_depth_tile_w/h and bad_side speak of the shared tile");

struct DepthLabelArgs {
    const int16_t* plane;
    int h, w, mode, max_diff;
    int* label; int* cnt; int* size;
};

__global__ __launch_bounds__(DEPTH_BLOCK) void depth_tile_kernel(DepthLabelArgs a) {
    __shared__ int s_parent[TW * TH];
    __shared__ int s_count[TW * TH];
    __shared__ short s_plane[TW * TH];
    const short outside = a.mode == DEPTH_SURFACES ? (short)-1 : (short)0;      // no member in either mode
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
        const TilePixel q = tile_pixel(j);
        s_plane[q.p] = q.inside(a.h, a.w) ? a.plane[q.at(a.w)] : outside;
        s_parent[q.p] = q.p;
        s_count[q.p] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
        const TilePixel px = tile_pixel(j);
        const int p = px.p, lx = px.c, ly = px.row, q = s_plane[p];
        if (lx > 0 && depth_joined(q, s_plane[p - 1], a.mode, a.max_diff)) depth_link(s_parent, p, p - 1);
        if (ly > 0 && depth_joined(q, s_plane[p - TW], a.mode, a.max_diff)) depth_link(s_parent, p, p - TW);
    }
    __syncthreads();
    int root[PIX];
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
        const int p = tile_pixel(j).p;
        root[j] = depth_member(s_plane[p], a.mode) ? depth_find(s_parent, p) : -1;      // pixels beyond the image are no members
        if (root[j] >= 0) atomicAdd(s_count + root[j], 1);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
        const TilePixel q = tile_pixel(j);
        const int r = root[j];
        if (!q.inside(a.h, a.w)) continue;
        const long i = q.at(a.w);
        a.label[i] = r < 0 ? -1 : (int)TilePixel(r).at(a.w);
        a.cnt[i] = s_count[q.p];                       // not zero on the roots of the tile only
    }
}

// Pixel i of the seams: first the first columns of the tiles right of the first one (x = TW, 2 TW, ...; h pixels each), then the first rows
__global__ __launch_bounds__(DEPTH_BLOCK) void depth_merge_kernel(DepthLabelArgs a, int n_columns, int n_rows) {
    const long long i = blockIdx.x * (long long)DEPTH_BLOCK + threadIdx.x;
    const long long in_columns = (long long)n_columns * a.h;
    int x, y, other;
    if (i < in_columns) {
        x = ((int)(i / a.h) + 1) * TW; y = (int)(i % a.h);
        other = y * a.w + x - 1;
    } else {
        const long long j = i - in_columns;
        if (j >= (long long)n_rows * a.w) return;
        y = ((int)(j / a.w) + 1) * TH; x = (int)(j % a.w);
        other = (y - 1) * a.w + x;
    }
    const int self = y * a.w + x;
    if (depth_joined(a.plane[self], a.plane[other], a.mode, a.max_diff)) depth_link(a.label, self, other);
}

// The slots the merge has moved are roots of tiles, and those alone hold a count: they find the root and hand their count on. A slot that
// is the root keeps its own and receives the others'; nobody reads it in this launch.
__global__ __launch_bounds__(DEPTH_BLOCK) void depth_flatten_kernel(DepthLabelArgs a) {
    const long long i = blockIdx.x * (long long)DEPTH_BLOCK + threadIdx.x;
    if (i >= (long long)a.h * a.w) return;
    const int p = depth_load(a.label + i);
    if (p < 0 || p == i) return;                      // no member, or the root: its slot is written by nobody here, its count only added to
    const int c = a.cnt[i];                           // of a slot that is no root: written by nobody here
    if (c == 0) return;                               // no root of a tile: its label is one, and depth_size_kernel follows it
    const int r = depth_find(a.label, p);
    depth_store(a.label + i, r);
    atomicAdd(a.cnt + r, c);
}

__global__ __launch_bounds__(DEPTH_BLOCK) void depth_size_kernel(DepthLabelArgs a) {
    const long long i = blockIdx.x * (long long)DEPTH_BLOCK + threadIdx.x;
    if (i >= (long long)a.h * a.w) return;
    int r = depth_load(a.label + i);
    if (r >= 0) {
        r = depth_load(a.label + r);                  // the root of its tile points at the root, or is it
        depth_store(a.label + i, r);
    }
    a.size[i] = r >= 0 ? a.cnt[r] : 0;
}

// the number of lanes of the wave whose `hit` is set, added to *count once
__device__ __forceinline__ void depth_count(long long* count, bool hit) {
    const unsigned long long hits = __ballot(hit);
    if (hits != 0 && (threadIdx.x & (IM_WAVE - 1)) == __ffsll((long long)hits) - 1)
        atomicAdd(reinterpret_cast<unsigned long long*>(count), (unsigned long long)__popcll(hits));
}

struct DepthDropArgs {
    const int* size;
    int h, w, min_size;
    int16_t* plane; double* wmap; float* score; long long* count;
};

__global__ __launch_bounds__(DEPTH_BLOCK) void depth_drop_kernel(DepthDropArgs a) {
    const long long i = blockIdx.x * (long long)DEPTH_BLOCK + threadIdx.x;
    bool drop = false;
    if (i < (long long)a.h * a.w) {
        drop = a.plane[i] >= 0 && a.size[i] < a.min_size;
        if (drop) { a.plane[i] = -1; a.wmap[i] = 0.0; a.score[i] = 0.0f; }
    }
    depth_count(a.count, drop);
}

struct DepthFillArgs {
    const int16_t* plane; const double* wmap; const float* score; const int* label; const int* size;
    int h, w, max_hole, max_diff, D;
    double w_first, w_step;
    int* lo; int* hi;
    int16_t* plane_out; double* w_out; float* score_out; uint8_t* filled; long long* count;
};

// a label that can be a root's slot: uploaded labels are not trusted with an address
__device__ __forceinline__ bool depth_slot(int l, long long n) { return l >= 0 && l < n; }

__global__ __launch_bounds__(DEPTH_BLOCK) void depth_rim_init_kernel(DepthFillArgs a) {
    const long long i = blockIdx.x * (long long)DEPTH_BLOCK + threadIdx.x;
    if (i >= (long long)a.h * a.w || a.label[i] != i) return;
    a.lo[i] = DEPTH_NO_RIM;
    a.hi[i] = 0;
}

// holes larger than max_hole never qualify: their rims are not collected
__global__ __launch_bounds__(DEPTH_BLOCK) void depth_rim_kernel(DepthFillArgs a) {
    const long long i = blockIdx.x * (long long)DEPTH_BLOCK + threadIdx.x, n = (long long)a.h * a.w;
    if (i >= n) return;
    const int l = a.label[i];
    if (!depth_slot(l, n) || a.size[i] > a.max_hole) return;
    const int x = (int)(i % a.w), y = (int)(i / a.w);
    if (x == 0 || y == 0 || x == a.w - 1 || y == a.h - 1) { atomicOr(a.hi + l, DEPTH_BORDER); return; }
    const int q[4] = {a.plane[i - 1], a.plane[i + 1], a.plane[i - a.w], a.plane[i + a.w]};
    int lo = DEPTH_NO_RIM, hi = -1;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (q[k] >= 0) { lo = min(lo, q[k]); hi = max(hi, q[k]); }
    if (hi >= 0) { atomicMin(a.lo + l, lo); atomicMax(a.hi + l, hi); }
}

__global__ __launch_bounds__(DEPTH_BLOCK) void depth_fill_kernel(DepthFillArgs a) {
    const long long i = blockIdx.x * (long long)DEPTH_BLOCK + threadIdx.x, n = (long long)a.h * a.w;
    bool fill = false;
    if (i < n) {
        int16_t plane = a.plane[i];
        double wv = a.wmap[i];
        float score = a.score[i];
        const int l = a.label[i], x = (int)(i % a.w), y = (int)(i / a.w);
        if (plane < 0 && depth_slot(l, n) && x > 0 && y > 0 && x < a.w - 1 && y < a.h - 1 &&
            depth_hole_qualifies(a.size[i], a.lo[l], a.hi[l], a.max_hole, a.max_diff)) {
            // the anchors lie inside the image because the hole does not touch the border; a walk that leaves it (labels of another map) fills nothing
            const int16_t* const row = a.plane + (size_t)y * a.w;
            int xl = x - 1, xr = x + 1, yu = y - 1, yd = y + 1;
            while (xl >= 0 && row[xl] < 0) --xl;
            while (xr < a.w && row[xr] < 0) ++xr;
            while (yu >= 0 && a.plane[(size_t)yu * a.w + x] < 0) --yu;
            while (yd < a.h && a.plane[(size_t)yd * a.w + x] < 0) ++yd;
            if (xl >= 0 && xr < a.w && yu >= 0 && yd < a.h) {
                const double* const wrow = a.wmap + (size_t)y * a.w;
                const double across = depth_between(wrow[xl], wrow[xr], x, xl, xr);
                const double along = depth_between(a.wmap[(size_t)yu * a.w + x], a.wmap[(size_t)yd * a.w + x], y, yu, yd);
                wv = depth_fill(across, along);
                plane = (int16_t)depth_plane_of(wv, a.w_first, a.w_step, a.D);
                score = 0.0f;
                fill = true;
            }
        }
        a.plane_out[i] = plane; a.w_out[i] = wv; a.score_out[i] = score; a.filled[i] = fill ? 1 : 0;
    }
    depth_count(a.count, fill);
}

}  // namespace
}  // namespace im

using namespace im;

extern "C" {

int im_depth_tile_w(void) { return DEPTH_TILE_W; }
int im_depth_tile_h(void) { return DEPTH_TILE_H; }

int im_depth_components(im_ctx* ctx, const int16_t* d_plane, int h, int w, int mode, int max_diff, int* d_label, int* d_size, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_plane || !d_label || !d_size) return ctx->fail(DENSE_REFUSED, "im_depth_components: null pointer");
    if (bad_side(h) || bad_side(w)) return ctx->fail(DENSE_REFUSED, "im_depth_components: h and w must be 1..16384");
    if (mode != DEPTH_SURFACES && mode != DEPTH_HOLES) return ctx->fail(DENSE_REFUSED, "im_depth_components: mode must be 0 or 1");
    if (max_diff < 0 || max_diff > DEPTH_MAX_DIFF) return ctx->fail(DENSE_REFUSED, "im_depth_components: max_diff must be 0..4095");
    hipStream_t s = (hipStream_t)stream;
    const long long n = (long long)h * w;
    const DepthComponentsScratch lay(n);
    IM_GROW(ctx, ctx->grow(ctx->scratch.depth, lay.bytes, "depth.scratch"), -22, "im_depth_components: allocation failed");
    DepthLabelArgs a{d_plane, h, w, mode, max_diff, d_label, lay.cnt.at(ctx->scratch.depth.p), d_size};
    const int tiles_x = (int)blocks_of(w, TW), tiles_y = (int)blocks_of(h, TH);
    IM_LAUNCH(ctx, "depth_tile", s, launch(depth_tile_kernel, dim3((unsigned)tiles_x, (unsigned)tiles_y), DEPTH_BLOCK, 0, s, a));
    const long long seams = (long long)(tiles_x - 1) * h + (long long)(tiles_y - 1) * w;
    if (seams > 0)
        IM_LAUNCH(ctx, "depth_merge", s, launch(depth_merge_kernel, (unsigned)blocks_of(seams, DEPTH_BLOCK), DEPTH_BLOCK, 0, s, a, tiles_x - 1, tiles_y - 1));
    IM_LAUNCH(ctx, "depth_flatten", s, launch(depth_flatten_kernel, (unsigned)blocks_of(n, DEPTH_BLOCK), DEPTH_BLOCK, 0, s, a));
    IM_LAUNCH(ctx, "depth_size", s, launch(depth_size_kernel, (unsigned)blocks_of(n, DEPTH_BLOCK), DEPTH_BLOCK, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_depth_components");
    return 0;
}

int im_depth_drop_small(im_ctx* ctx, const int* d_size, int h, int w, int min_size, int16_t* d_plane, double* d_w, float* d_score, long long* d_count,
                        void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_size || !d_plane || !d_w || !d_score || !d_count) return ctx->fail(DENSE_REFUSED, "im_depth_drop_small: null pointer");
    if (bad_side(h) || bad_side(w)) return ctx->fail(DENSE_REFUSED, "im_depth_drop_small: h and w must be 1..16384");
    if (min_size < 1) return ctx->fail(DENSE_REFUSED, "im_depth_drop_small: min_size must be 1..2^31-1");
    hipStream_t s = (hipStream_t)stream;
    IM_HIP(ctx, hipMemsetAsync(d_count, 0, sizeof(long long), s));
    DepthDropArgs a{d_size, h, w, min_size, d_plane, d_w, d_score, d_count};
    IM_LAUNCH(ctx, "depth_drop", s, launch(depth_drop_kernel, (unsigned)blocks_of((long long)h * w, DEPTH_BLOCK), DEPTH_BLOCK, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_depth_drop_small");
    return 0;
}

int im_depth_fill_holes(im_ctx* ctx, const int16_t* d_plane, const double* d_w, const float* d_score, const int* d_label, const int* d_size, int h, int w,
                        int max_hole, int max_diff, double w_first, double w_step, int D, int16_t* d_plane_out, double* d_w_out, float* d_score_out,
                        uint8_t* d_filled, long long* d_count, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_plane || !d_w || !d_score || !d_label || !d_size || !d_plane_out || !d_w_out || !d_score_out || !d_filled || !d_count)
        return ctx->fail(DENSE_REFUSED, "im_depth_fill_holes: null pointer");
    // a filled pixel must never be read as a rim pixel or an anchor by another thread
    if ((const void*)d_plane_out == (const void*)d_plane || (const void*)d_w_out == (const void*)d_w || (const void*)d_score_out == (const void*)d_score)
        return ctx->fail(DENSE_REFUSED, "im_depth_fill_holes: the outputs must not be the inputs");
    if (bad_side(h) || bad_side(w)) return ctx->fail(DENSE_REFUSED, "im_depth_fill_holes: h and w must be 1..16384");
    if (max_hole < 1 || max_hole > DEPTH_MAX_HOLE) return ctx->fail(DENSE_REFUSED, "im_depth_fill_holes: max_hole must be 1..4096");
    if (max_diff < 0 || max_diff > DEPTH_MAX_DIFF) return ctx->fail(DENSE_REFUSED, "im_depth_fill_holes: max_diff must be 0..4095");
    if (D < 1 || D > DEPTH_MAX_PLANES) return ctx->fail(DENSE_REFUSED, "im_depth_fill_holes: D must be 1..4096");
    if (!std::isfinite(w_first) || !std::isfinite(w_step) || w_step == 0.0)
        return ctx->fail(DENSE_REFUSED, "im_depth_fill_holes: w_first must be finite, w_step finite and not zero");
    hipStream_t s = (hipStream_t)stream;
    const long long n = (long long)h * w;
    const DepthHolesScratch lay(n);
    IM_GROW(ctx, ctx->grow(ctx->scratch.depth, lay.bytes, "depth.scratch"), -22, "im_depth_fill_holes: allocation failed");
    IM_HIP(ctx, hipMemsetAsync(d_count, 0, sizeof(long long), s));
    DepthFillArgs a{d_plane, d_w, d_score, d_label, d_size, h, w, max_hole, max_diff, D, w_first, w_step,
                    lay.lo.at(ctx->scratch.depth.p), lay.hi.at(ctx->scratch.depth.p), d_plane_out, d_w_out, d_score_out, d_filled, d_count};
    const unsigned blocks = (unsigned)blocks_of(n, DEPTH_BLOCK);
    IM_LAUNCH(ctx, "depth_rim_init", s, launch(depth_rim_init_kernel, blocks, DEPTH_BLOCK, 0, s, a));
    IM_LAUNCH(ctx, "depth_rim", s, launch(depth_rim_kernel, blocks, DEPTH_BLOCK, 0, s, a));
    IM_LAUNCH(ctx, "depth_fill", s, launch(depth_fill_kernel, blocks, DEPTH_BLOCK, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_depth_fill_holes");
    return 0;
}

}  // extern "C"
