// Coarse-to-fine dense displacement on the device: the prior of every pixel of a level from the displacement field of the level above, and
// the match of every pixel around its own prior. With them dense_flow.py runs im_flow_match on the coarsest level of a Gaussian pyramid
// (im_pyr_down) and walks down to the images themselves; the reach grows with 2^levels and the candidates per pixel shrink to
// (2 fine_search + 1)^2. A definition of this project's own (flow_field_pixel.h, flow_pixel.h), pinned bit for bit against
// tests/pyrflow_oracle.py.
//
//   flow_prior_up_kernel     one thread per fine pixel: the lower median of up to 25 coarse displacements per axis, by ranks, in registers
//   flow_match_field_kernel  one block of 256 threads per 64 x 16 tile of pixels of a, as flow_match_kernel (dense_flow.hip), whose staging
//                            and row partials need one offset for the whole tile. Here every pixel has its own, so the block first folds
//                            the box [lo_u, hi_u] x [lo_v, hi_v] of the priors of its pixels that are to be matched (wanted, and with
//                            their window inside a). Then one of three paths, a pure function of the tile's inputs:
//                              0  no such pixel: zeros;
//                              1  tiled, where hi_u - lo_u <= E and hi_v - lo_v <= E, E = flow_field_spread(r, S) (8, less where the
//                                 LDS of a launch would not hold it): the region of b that the box with its halo of r + S needs is staged
//                                 once, the block walks the absolute offsets lo - S .. hi + S of the box with row partials and column
//                                 sums exactly as flow_match_kernel does, and a pixel scores an offset only where it lies within S of
//                                 its own prior. The parabola's neighbours come from the staged bytes;
//                              2  direct, where the box is wider: each thread runs flow_match_pixel, the definition itself, on global
//                                 memory for its pixels. Slow and right.
//                            Both paths sum integers: the same bits. LDS is sized per launch from r, S and E: 30.8 KB at r = 7, S = 2,
//                            E = 8; at most 64344 bytes (r = 14, S = 13 .. 16); 64168 at r = 15, S = 16, E = 1 (E = 0: 62800).
// No read-modify-write of memory anywhere; every output element is written; whatever the prior field holds, b is read only through the
// staging's own bounds test or flow_match_pixel's window test. Enqueue only.
#include "common.h"
#include "ctx.h"
#include "flow_field_pixel.h"
#include "dense_tile.h"
#include "dense_host.h"

namespace im {
namespace {

constexpr unsigned NO_WINDOW = 0xffffffffu;                                       // s_sb.x of a position whose window leaves b
static_assert(31LL * 255 * 255 < (1LL << 32), "the row partials");
constexpr int WAVE = 64, WAVES = TILE_BLOCK / WAVE;

// the four arrays of the tiled path behind one another for a box of priors spanning ex x ey: flow_field_lds_bytes, term by term
struct FieldLds {
    int aw, ah, bw, bh, pw, ph;
    size_t a, b, sb, row, bytes;
    __host__ __device__ FieldLds(int r, int S, int ex, int ey)
        : aw(TW + 2 * r), ah(TH + 2 * r), bw(TW + ex + 2 * (r + S)), bh(TH + ey + 2 * (r + S)), pw(TW + ex + 2 * S), ph(TH + ey + 2 * S) {
        a = 0;
        b = (size_t)flow_field_up8((long long)aw * ah);
        sb = b + (size_t)flow_field_up8((long long)bw * bh);
        row = sb + (size_t)pw * ph * sizeof(uint2);
        bytes = row + (size_t)ah * TW * sizeof(unsigned);
    }
};

struct FlowFieldArgs {
    const uint8_t* a; const uint8_t* b; const uint8_t* ask; const uint8_t* have;
    const int16_t* pu; const int16_t* pv;
    int h, w, r, S, E;
    long long min_var;
    double min_score;
    double* du; double* dv; float* score; uint8_t* valid; uint8_t* path;
};

__device__ __forceinline__ int wave_min(int v) {
    for (int o = WAVE / 2; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(TILE_BLOCK) void flow_match_field_kernel(FlowFieldArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ int s_box[WAVES][4];
    const int t = threadIdx.x, r = a.r, S = a.S, side = 2 * r + 1;
    const int x0 = tile_x0(), y0 = tile_y0();

    // what this thread's pixels ask for, and the box of their priors: lo_u, -hi_u, lo_v, -hi_v under one fold by min
    unsigned todo = 0;                      // bit j: pixel j is wanted and has its window inside a
    int prior[PIX];                         // pv << 16 | (pu & 0xffff) of such a pixel
    int box[4] = {FLOW_MAX_PRIOR + 1, FLOW_MAX_PRIOR + 1, FLOW_MAX_PRIOR + 1, FLOW_MAX_PRIOR + 1};
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
        const TilePixel q = tile_pixel(j);
        prior[j] = 0;
        if (!q.inside(a.h, a.w)) continue;
        const long i = q.at(a.w);
        const int pu = a.pu[i], pv = a.pv[i];
        if (!flow_field_wanted(a.have[i], a.ask == nullptr ? 1 : (int)a.ask[i], pu, pv) || !window_inside(q.u, q.v, r, a.h, a.w)) continue;
        todo |= 1u << j;
        prior[j] = (int)((unsigned)pv << 16 | ((unsigned)pu & 0xffffu));
        box[0] = min(box[0], pu); box[1] = min(box[1], -pu); box[2] = min(box[2], pv); box[3] = min(box[3], -pv);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int m = wave_min(box[k]);
        if ((t & (WAVE - 1)) == 0) s_box[t / WAVE][k] = m;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int m = s_box[0][k];
#pragma unroll
        for (int v = 1; v < WAVES; ++v) m = min(m, s_box[v][k]);
        box[k] = m;
    }
    const int lo_u = box[0], hi_u = -box[1], lo_v = box[2], hi_v = -box[3];
    const int path = lo_u > FLOW_MAX_PRIOR ? 0 : (hi_u - lo_u > a.E || hi_v - lo_v > a.E) ? 2 : 1;      // the same in every thread
    if (a.path != nullptr && t == 0) a.path[(long)blockIdx.y * gridDim.x + blockIdx.x] = (uint8_t)path;

    if (path != 1) {                        // nothing to do: zeros; or the direct path: the definition itself, pixel after pixel
#pragma unroll 1
        for (int j = 0; j < PIX; ++j) {
            const TilePixel q = tile_pixel(j);
            if (!q.inside(a.h, a.w)) continue;
            const long i = q.at(a.w);
            double du = 0.0, dv = 0.0;
            float score = 0.0f;
            bool ok = false;
            if (path == 2 && (todo >> j & 1))
                ok = flow_match_pixel(a.a, a.b, a.h, a.w, q.u, q.v, r, S, a.pu[i], a.pv[i], a.min_var, a.min_score, du, dv, score);
            a.du[i] = du; a.dv[i] = dv; a.score[i] = score; a.valid[i] = ok ? 1 : 0;
        }
        return;
    }

    // the tiled path: offsets lo - S .. hi + S on either axis; offset index (ox, oy) is the absolute displacement (ex0 + ox, ey0 + oy)
    const int ex0 = lo_u - S, ey0 = lo_v - S, nx = hi_u - lo_u + 2 * S + 1, ny = hi_v - lo_v + 2 * S + 1;
    const FieldLds L(r, S, hi_u - lo_u, hi_v - lo_v);      // within the launch's bytes: both spreads <= E
    uint8_t* const s_a = lds + L.a;
    uint8_t* const s_b = lds + L.b;
    uint2* const s_sb = reinterpret_cast<uint2*>(lds + L.sb);
    unsigned* const s_row = reinterpret_cast<unsigned*>(lds + L.row);
    const int bx0 = x0 + ex0 - r, by0 = y0 + ey0 - r;                             // the first byte of the staged region of b

    tile_stage_bytes(s_a, a.a, a.h, a.w, r);
    tile_stage(bx0, by0, L.bw, L.bh, a.h, a.w, [&](int i, bool inside, long g, int, int) { s_b[i] = inside ? a.b[g] : (uint8_t)0; });
    __syncthreads();
    // the sums of b at every position a candidate can be centred on: position (px, py) is byte (px + r, py + r) of the region
    tile_stage(bx0 + r, by0 + r, L.pw, L.ph, a.h, a.w, [&](int i, bool, long, int u, int v) {
        uint2 q = make_uint2(NO_WINDOW, 0u);
        if (window_inside(u, v, r, a.h, a.w)) {
            long long s1, s2;
            dense_window_sums(s_b + (v - by0) * L.bw + (u - bx0), L.bw, r, s1, s2);
            q = make_uint2((unsigned)s1, (unsigned)s2);
        }
        s_sb[i] = q;
    });

    const long long n = (long long)side * side;
    unsigned sa[PIX], saa[PIX];
    double s0[PIX];
    int best[PIX];                          // (dy + S) << 8 | (dx + S) of the best around the pixel's own prior, -1: none yet
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
        const TilePixel q = tile_pixel(j);
        long long s1 = 0, s2 = 0;
        if (todo >> j & 1) dense_window_sums(s_a + (q.row + r) * L.aw + q.c + r, L.aw, r, s1, s2);
        sa[j] = (unsigned)s1; saa[j] = (unsigned)s2;
        s0[j] = 0.0; best[j] = -1;
        // from here on the pixel's prior as its offset index: (pv - ey0) << 8 | (pu - ex0), each in S .. S + E
        prior[j] = (todo >> j & 1) ? (((prior[j] >> 16) - ey0) << 8) | ((int)(short)(prior[j] & 0xffff) - ex0) : 0;
    }
    __syncthreads();

    for (int k = 0; k < nx * ny; ++k) {
        const int ox = k % nx, oy = k / nx;
        // (B) rows of a * b: partial (row, c) sums a[row][c .. c + 2 r] * b[row + oy][c + ox ..] in the staged arrays
        for (int i = t; i < L.ah * TW; i += TILE_BLOCK) {
            const int c = i & (TW - 1), row = i / TW;
            const uint8_t* pa = s_a + row * L.aw + c;
            const uint8_t* pb = s_b + (row + oy) * L.bw + c + ox;
            unsigned ab = 0;
            for (int q = 0; q < side; ++q) ab += (unsigned)pa[q] * pb[q];
            s_row[i] = ab;
        }
        __syncthreads();
        // (C) columns, for the pixels whose own range holds this offset
#pragma unroll
        for (int j = 0; j < PIX; ++j) {
            const int dx = ox - (prior[j] & 255), dy = oy - (prior[j] >> 8);
            if (!(todo >> j & 1) || dx < -S || dx > S || dy < -S || dy > S) continue;
            const TilePixel px = tile_pixel(j);
            const uint2 q = s_sb[(px.row + oy) * L.pw + px.c + ox];
            if (q.x == NO_WINDOW) continue;
            unsigned ab = 0;
            for (int e = 0; e < side; ++e) ab += s_row[(px.row + e) * TW + px.c];
            double s;
            if (!dense_score(n, sa[j], saa[j], q.x, q.y, ab, a.min_var, s, 1)) continue;
            const bool take = flow_better(best[j] >= 0, s, dx, dy, s0[j], (best[j] & 255) - S, (best[j] >> 8) - S);      // -1 decodes to anything: not read
            s0[j] = take ? s : s0[j];
            best[j] = take ? ((dy + S) << 8 | (dx + S)) : best[j];
        }
        __syncthreads();                    // the next offset's (B) overwrites the partials
    }

    // the second phase: the four neighbours of each pixel's best, directly from the staged bytes
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
        const TilePixel px = tile_pixel(j);
        const int c = px.c, row = px.row;
        if (!px.inside(a.h, a.w)) continue;
        double du = 0.0, dv = 0.0;
        float score = 0.0f;
        bool ok = false;
        if ((todo >> j & 1) && best[j] >= 0 && !(s0[j] < a.min_score)) {
            const int dx = (best[j] & 255) - S, dy = (best[j] >> 8) - S;
            const int qx = prior[j] & 255, qy = prior[j] >> 8;                    // the prior's offset index
            const uint8_t* ca = s_a + (row + r) * L.aw + c + r;
            auto neighbour = [&](int ex, int ey, double& s) {
                s = 0.0;
                if (ex < -S || ex > S || ey < -S || ey > S) return false;
                const uint2 q = s_sb[(row + qy + ey) * L.pw + c + qx + ex];
                if (q.x == NO_WINDOW) return false;
                const long long ab = flow_window_ab(ca, L.aw, s_b + (row + qy + ey + r) * L.bw + c + qx + ex + r, L.bw, r);
                return dense_score(n, sa[j], saa[j], q.x, q.y, ab, a.min_var, s, 1);
            };
            double sm, sp;
            bool both = dx - 1 >= -S && dx + 1 <= S;
            both = both && neighbour(dx - 1, dy, sm);
            both = both && neighbour(dx + 1, dy, sp);
            du = (double)(ex0 + qx + dx) + flow_offset(both, sm, s0[j], sp);
            both = dy - 1 >= -S && dy + 1 <= S;
            both = both && neighbour(dx, dy - 1, sm);
            both = both && neighbour(dx, dy + 1, sp);
            dv = (double)(ey0 + qy + dy) + flow_offset(both, sm, s0[j], sp);
            score = (float)s0[j];
            ok = true;
        }
        const long i = px.at(a.w);
        a.du[i] = du; a.dv[i] = dv; a.score[i] = score; a.valid[i] = ok ? 1 : 0;
    }
}

struct FlowPriorArgs {
    const double* du; const double* dv; const uint8_t* valid;
    int hc, wc, h, w, min_count;
    int16_t* pu; int16_t* pv; uint8_t* have;
};

template <int M>
__global__ __launch_bounds__(256) void flow_prior_up_kernel(FlowPriorArgs a) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= (long)a.h * a.w) return;
    int pu, pv;
    const bool have = flow_prior_up_pixel<M>(a.du, a.dv, a.valid, a.hc, a.wc, (int)(i % a.w), (int)(i / a.w), a.min_count, pu, pv);
    a.pu[i] = (int16_t)pu; a.pv[i] = (int16_t)pv; a.have[i] = have ? 1 : 0;
}

}  // namespace
}  // namespace im

using namespace im;

extern "C" {

int im_flow_prior_up(im_ctx* ctx, const double* d_du_c, const double* d_dv_c, const uint8_t* d_valid_c, int hc, int wc, int h, int w, int median_radius,
                     int min_count, int16_t* d_pu, int16_t* d_pv, uint8_t* d_have, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_du_c || !d_dv_c || !d_valid_c || !d_pu || !d_pv || !d_have) return ctx->fail(DENSE_REFUSED, "im_flow_prior_up: null pointer");
    if (bad_side(h) || bad_side(w) || bad_side(hc) || bad_side(wc)) return ctx->fail(DENSE_REFUSED, "im_flow_prior_up: h and w must be 1..16384");
    if (hc != (h + 1) / 2 || wc != (w + 1) / 2) return ctx->fail(DENSE_REFUSED, "im_flow_prior_up: the coarse level must be (h + 1) / 2 x (w + 1) / 2");
    if (median_radius < 0 || median_radius > FLOW_MAX_MEDIAN_RADIUS) return ctx->fail(DENSE_REFUSED, "im_flow_prior_up: median_radius must be 0..2");
    const int side = 2 * median_radius + 1;
    if (min_count < 1 || min_count > side * side) return ctx->fail(DENSE_REFUSED, "im_flow_prior_up: min_count must be 1..(2 median_radius + 1)^2");
    hipStream_t s = (hipStream_t)stream;
    FlowPriorArgs a{d_du_c, d_dv_c, d_valid_c, hc, wc, h, w, min_count, d_pu, d_pv, d_have};
    const unsigned blocks = (unsigned)blocks_of((long long)h * w, 256);
    if (median_radius == 0) IM_LAUNCH(ctx, "flow_prior_up", s, launch(flow_prior_up_kernel<0>, blocks, 256, 0, s, a));
    else if (median_radius == 1) IM_LAUNCH(ctx, "flow_prior_up", s, launch(flow_prior_up_kernel<1>, blocks, 256, 0, s, a));
    else IM_LAUNCH(ctx, "flow_prior_up", s, launch(flow_prior_up_kernel<2>, blocks, 256, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_flow_prior_up");
    return 0;
}

int im_flow_match_field(im_ctx* ctx, const uint8_t* d_a, const uint8_t* d_b, int h, int w, int r, int search, const int16_t* d_pu, const int16_t* d_pv,
                        const uint8_t* d_have, long long min_var, double min_score, const uint8_t* d_ask, double* d_du, double* d_dv, float* d_score,
                        uint8_t* d_valid, uint8_t* d_tile_path, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_a || !d_b || !d_pu || !d_pv || !d_have || !d_du || !d_dv || !d_score || !d_valid) return ctx->fail(DENSE_REFUSED, "im_flow_match_field: null pointer");
    if (bad_side(h) || bad_side(w)) return ctx->fail(DENSE_REFUSED, "im_flow_match_field: h and w must be 1..16384");
    if (r < 1 || r > FLOW_MAX_RADIUS) return ctx->fail(DENSE_REFUSED, "im_flow_match_field: r must be 1..15");
    if (search < 0 || search > FLOW_MAX_SEARCH) return ctx->fail(DENSE_REFUSED, "im_flow_match_field: the search half-width must be 0..16");
    if (min_var < 0 || min_var > FLOW_MAX_MIN_VAR) return ctx->fail(DENSE_REFUSED, "im_flow_match_field: min_var must be 0..2^26");
    if (!std::isfinite(min_score)) return ctx->fail(DENSE_REFUSED, "im_flow_match_field: min_score must be finite");
    hipStream_t s = (hipStream_t)stream;
    const int E = flow_field_spread(TW, TH, r, search);
    FlowFieldArgs a{d_a, d_b, d_ask, d_have, d_pu, d_pv, h, w, r, search, E, min_var, min_score, d_du, d_dv, d_score, d_valid, d_tile_path};
    const FieldLds L(r, search, E, E);      // at most 64344 bytes: below the 64 KiB a launch may ask for without an attribute
    IM_LAUNCH(ctx, "flow_match_field", s, launch(flow_match_field_kernel, dim3((unsigned)blocks_of(w, TW), (unsigned)blocks_of(h, TH)), TILE_BLOCK, L.bytes, s, a));
    IM_GUARD_CHECK(ctx, s, "im_flow_match_field");
    return 0;
}

}  // extern "C"
