// Dense surface displacement between two epochs on the device: the match of every asked pixel of a camera's image at epoch A in the same
// camera's image at epoch B, the forward-backward check of two such fields, and the lift of both ends of a match to world points through
// each epoch's own depth map and pose. The reference has no such step: every quantity has a definition of this project's own
// (flow_pixel.h) and is pinned bit for bit against tests/flow_oracle.py. Parity with any image-correlation package is unpinned.
//
//   flow_match_kernel   one block of 256 threads per 64 x 16 tile of pixels of a (the sweep's block: the tile, the map from a thread to its
//                       pixels and the staging loop are dense_tile.h's; the score and the window sums dense_pixel.h's). Staged in LDS once:
//                       the bytes of the tile of a with its halo of r, the bytes of the region of b that the tile's candidates read (the tile moved by the prior,
//                       with a halo of r + S), and for every position of b at which a candidate's window can be centred its sum and sum
//                       of squares (or a mark that the window leaves b). A pixel's own sums of a live in registers. Then, per
//                       candidate (dx, dy): (B) the rows of a * b are box-summed over 2 r + 1 columns into 4-byte partials, rows of 64
//                       consecutive entries, one per lane; (C) each thread sums 2 r + 1 rows of partials for its four pixels, scores them
//                       and keeps the best. A short second phase scores the four neighbours of each pixel's best directly from LDS
//                       (they differ per pixel) for the parabola. The prior moves the staged region of b and costs nothing else.
//                       LDS is sized per launch from r and S: 34.8 KB at r = 7, S = 8, 62.8 KB at r = 15, S = 16.
//   flow_check_kernel, flow_lift_kernel   one thread per pixel
// All sums are integers: the order of execution does not matter. No atomics; every output element is written. Enqueue only.
#include "common.h"
#include "ctx.h"
#include "flow_pixel.h"
#include "dense_tile.h"
#include "dense_host.h"

namespace im {
namespace {

constexpr unsigned NO_WINDOW = 0xffffffffu;                                       // s_sb.x of a position whose window leaves b
// a row partial is the sum of 31 products of two bytes at the most
static_assert(31LL * 255 * 255 < (1LL << 32), "the row partials");

// the four arrays of the block behind one another, each starting at a multiple of 8 bytes
struct FlowLds {
    int aw, ah, bw, bh, pw, ph;             // a tile + halo r; b region: halo r + S; positions: halo S
    size_t a, b, sb, row, bytes;
    __host__ __device__ FlowLds(int r, int S)
        : aw(TW + 2 * r), ah(TH + 2 * r), bw(TW + 2 * (r + S)), bh(TH + 2 * (r + S)), pw(TW + 2 * S), ph(TH + 2 * S) {
        a = 0;
        b = up8((size_t)aw * ah);
        sb = b + up8((size_t)bw * bh);
        row = sb + (size_t)pw * ph * sizeof(uint2);
        bytes = row + (size_t)ah * TW * sizeof(unsigned);
    }
    __host__ __device__ static size_t up8(size_t v) { return (v + 7) & ~size_t(7); }
};

struct FlowMatchArgs {
    const uint8_t* a; const uint8_t* b; const uint8_t* ask;
    int h, w, r, S, pu, pv;
    long long min_var;
    double min_score;
    double* du; double* dv; float* score; uint8_t* valid;
};

__global__ __launch_bounds__(TILE_BLOCK) void flow_match_kernel(FlowMatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int t = threadIdx.x, r = a.r, S = a.S, side = 2 * r + 1;
    const FlowLds L(r, S);
    uint8_t* const s_a = lds + L.a;
    uint8_t* const s_b = lds + L.b;
    uint2* const s_sb = reinterpret_cast<uint2*>(lds + L.sb);
    unsigned* const s_row = reinterpret_cast<unsigned*>(lds + L.row);
    const int x0 = tile_x0(), y0 = tile_y0();
    const int bx0 = x0 + a.pu - S - r, by0 = y0 + a.pv - S - r;                    // the first byte of the staged region of b

    unsigned todo = 0;                      // bit j: pixel j lies in the image, is asked for and has its window inside a
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
        const TilePixel q = tile_pixel(j);
        if (q.inside(a.h, a.w) && (a.ask == nullptr || a.ask[q.at(a.w)] != 0) && window_inside(q.u, q.v, r, a.h, a.w)) todo |= 1u << j;
    }
    // no candidate of any pixel of the tile has its window inside b: the centres x0 + pu - S .. x0 + pu + S + 63 miss r .. w - 1 - r (or y)
    const bool some_b = x0 + a.pu + S + TW > r && x0 + a.pu - S < a.w - r && y0 + a.pv + S + TH > r && y0 + a.pv - S < a.h - r;
    const int work = __syncthreads_or(some_b && todo != 0);
    if (!work) {                            // nothing asked for (or nothing that can score): zeros, at once
#pragma unroll
        for (int j = 0; j < PIX; ++j) {
            const TilePixel q = tile_pixel(j);
            if (q.inside(a.h, a.w)) {
                const long i = q.at(a.w);
                a.du[i] = 0.0; a.dv[i] = 0.0; a.score[i] = 0.0f; a.valid[i] = 0;
            }
        }
        return;
    }

    tile_stage_bytes(s_a, a.a, a.h, a.w, r);
    tile_stage(bx0, by0, L.bw, L.bh, a.h, a.w, [&](int i, bool inside, long g, int, int) { s_b[i] = inside ? a.b[g] : (uint8_t)0; });
    __syncthreads();
    // the sums of b at every position a candidate can be centred on: position (px, py) is byte (px + r, py + r) of the region, which is
    // byte (u - bx0, v - by0) for the position's place (u, v) in b
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
    int best[PIX];                          // (dy + S) << 8 | (dx + S) of the best, -1: none yet
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
        const TilePixel q = tile_pixel(j);
        long long s1 = 0, s2 = 0;
        if (todo >> j & 1) dense_window_sums(s_a + (q.row + r) * L.aw + q.c + r, L.aw, r, s1, s2);
        sa[j] = (unsigned)s1; saa[j] = (unsigned)s2;
        s0[j] = 0.0; best[j] = -1;
    }
    __syncthreads();

    const int span = 2 * S + 1;
    for (int k = 0; k < span * span; ++k) {
        const int dx = k % span - S, dy = k / span - S;
        // (B) rows of a * b: partial (row, c) sums a[row][c .. c + 2 r] * b[row + S + dy][c + S + dx ..] in the staged arrays
        for (int i = t; i < L.ah * TW; i += TILE_BLOCK) {
            const int c = i & (TW - 1), row = i / TW;
            const uint8_t* pa = s_a + row * L.aw + c;
            const uint8_t* pb = s_b + (row + S + dy) * L.bw + c + S + dx;
            unsigned ab = 0;
            for (int q = 0; q < side; ++q) ab += (unsigned)pa[q] * pb[q];
            s_row[i] = ab;
        }
        __syncthreads();
        // (C) columns: 2 r + 1 rows of partials, the score, the running best
#pragma unroll
        for (int j = 0; j < PIX; ++j) {
            if (!(todo >> j & 1)) continue;
            const TilePixel px = tile_pixel(j);
            const uint2 q = s_sb[(px.row + S + dy) * L.pw + px.c + S + dx];
            if (q.x == NO_WINDOW) continue;
            unsigned ab = 0;
            for (int e = 0; e < side; ++e) ab += s_row[(px.row + e) * TW + px.c];
            double s;
            if (!dense_score(n, sa[j], saa[j], q.x, q.y, ab, a.min_var, s, 1)) continue;
            const bool take = flow_better(best[j] >= 0, s, dx, dy, s0[j], (best[j] & 255) - S, (best[j] >> 8) - S);      // -1 decodes to anything: not read
            s0[j] = take ? s : s0[j];
            best[j] = take ? ((dy + S) << 8 | (dx + S)) : best[j];
        }
        __syncthreads();                    // the next candidate's (B) overwrites the partials
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
            const uint8_t* ca = s_a + (row + r) * L.aw + c + r;
            auto neighbour = [&](int ex, int ey, double& s) {
                s = 0.0;
                if (ex < -S || ex > S || ey < -S || ey > S) return false;
                const uint2 q = s_sb[(row + S + ey) * L.pw + c + S + ex];
                if (q.x == NO_WINDOW) return false;
                const long long ab = flow_window_ab(ca, L.aw, s_b + (row + S + ey + r) * L.bw + c + S + ex + r, L.bw, r);
                return dense_score(n, sa[j], saa[j], q.x, q.y, ab, a.min_var, s, 1);
            };
            double sm, sp;
            bool both = dx - 1 >= -S && dx + 1 <= S;
            both = both && neighbour(dx - 1, dy, sm);
            both = both && neighbour(dx + 1, dy, sp);
            du = (double)(a.pu + dx) + flow_offset(both, sm, s0[j], sp);
            both = dy - 1 >= -S && dy + 1 <= S;
            both = both && neighbour(dx, dy - 1, sm);
            both = both && neighbour(dx, dy + 1, sp);
            dv = (double)(a.pv + dy) + flow_offset(both, sm, s0[j], sp);
            score = (float)s0[j];
            ok = true;
        }
        const long i = px.at(a.w);
        a.du[i] = du; a.dv[i] = dv; a.score[i] = score; a.valid[i] = ok ? 1 : 0;
    }
}

struct FlowCheckArgs {
    const double* du; const double* dv; const uint8_t* valid;
    const double* du_b; const double* dv_b; const uint8_t* valid_b;
    int h, w;
    double tol;
    uint8_t* keep;
};

__global__ __launch_bounds__(256) void flow_check_kernel(FlowCheckArgs a) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= (long)a.h * a.w) return;
    const bool k = a.valid[i] != 0 && flow_consistent((int)(i % a.w), (int)(i / a.w), a.du[i], a.dv[i], a.du_b, a.dv_b, a.valid_b, a.h, a.w, a.tol);
    a.keep[i] = k ? 1 : 0;
}

struct FlowLiftArgs {
    const double* du; const double* dv; const uint8_t* valid; const uint8_t* keep;
    const int16_t* plane_a; const double* w_a; int h, w;
    const int16_t* plane_b; const double* w_b; const uint8_t* keep_b; int hb, wb;
    DenseCam ca, cb;
    double span;
    double* P; double* D; uint8_t* ok;
};

__global__ __launch_bounds__(256) void flow_lift_kernel(FlowLiftArgs a) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= (long)a.h * a.w) return;
    double P[3] = {0.0, 0.0, 0.0}, D[3] = {0.0, 0.0, 0.0};
    bool ok = false;
    if (a.keep[i] != 0 && a.plane_a[i] >= 0 && a.valid[i] != 0)
        ok = flow_lift_pixel(a.ca, a.cb, (int)(i % a.w), (int)(i / a.w), a.w_a[i], a.du[i], a.dv[i], a.plane_b, a.w_b, a.keep_b, a.hb, a.wb, a.span, P, D);
#pragma unroll
    for (int c = 0; c < 3; ++c) { a.P[3 * i + c] = P[c]; a.D[3 * i + c] = D[c]; }
    a.ok[i] = ok ? 1 : 0;
}

}  // namespace
}  // namespace im

using namespace im;

extern "C" {

int im_flow_match(im_ctx* ctx, const uint8_t* d_a, const uint8_t* d_b, int h, int w, int r, int search, int prior_u, int prior_v, long long min_var,
                  double min_score, const uint8_t* d_ask, double* d_du, double* d_dv, float* d_score, uint8_t* d_valid, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_a || !d_b || !d_du || !d_dv || !d_score || !d_valid) return ctx->fail(DENSE_REFUSED, "im_flow_match: null pointer");
    if (bad_side(h) || bad_side(w)) return ctx->fail(DENSE_REFUSED, "im_flow_match: h and w must be 1..16384");
    if (r < 1 || r > FLOW_MAX_RADIUS) return ctx->fail(DENSE_REFUSED, "im_flow_match: r must be 1..15");
    if (search < 0 || search > FLOW_MAX_SEARCH) return ctx->fail(DENSE_REFUSED, "im_flow_match: the search half-width must be 0..16");
    if (prior_u < -FLOW_MAX_PRIOR || prior_u > FLOW_MAX_PRIOR || prior_v < -FLOW_MAX_PRIOR || prior_v > FLOW_MAX_PRIOR)
        return ctx->fail(DENSE_REFUSED, "im_flow_match: the prior must be -4096..4096");
    if (min_var < 0 || min_var > FLOW_MAX_MIN_VAR) return ctx->fail(DENSE_REFUSED, "im_flow_match: min_var must be 0..2^26");
    if (!std::isfinite(min_score)) return ctx->fail(DENSE_REFUSED, "im_flow_match: min_score must be finite");
    hipStream_t s = (hipStream_t)stream;
    FlowMatchArgs a{d_a, d_b, d_ask, h, w, r, search, prior_u, prior_v, min_var, min_score, d_du, d_dv, d_score, d_valid};
    const FlowLds L(r, search);             // at most 62800 bytes: below the 64 KiB a launch may ask for without an attribute
    IM_LAUNCH(ctx, "flow_match", s, launch(flow_match_kernel, dim3((unsigned)blocks_of(w, TW), (unsigned)blocks_of(h, TH)), TILE_BLOCK, L.bytes, s, a));
    IM_GUARD_CHECK(ctx, s, "im_flow_match");
    return 0;
}

int im_flow_check(im_ctx* ctx, const double* d_du, const double* d_dv, const uint8_t* d_valid, const double* d_du_b, const double* d_dv_b,
                  const uint8_t* d_valid_b, int h, int w, double tol, uint8_t* d_keep, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_du || !d_dv || !d_valid || !d_du_b || !d_dv_b || !d_valid_b || !d_keep) return ctx->fail(DENSE_REFUSED, "im_flow_check: null pointer");
    if (bad_side(h) || bad_side(w)) return ctx->fail(DENSE_REFUSED, "im_flow_check: h and w must be 1..16384");
    if (!positive(tol)) return ctx->fail(DENSE_REFUSED, "im_flow_check: tol must be finite and > 0");
    hipStream_t s = (hipStream_t)stream;
    FlowCheckArgs a{d_du, d_dv, d_valid, d_du_b, d_dv_b, d_valid_b, h, w, tol, d_keep};
    IM_LAUNCH(ctx, "flow_check", s, launch(flow_check_kernel, blocks_of((long long)h * w, 256), 256, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_flow_check");
    return 0;
}

int im_flow_lift(im_ctx* ctx, const double* d_du, const double* d_dv, const uint8_t* d_valid, const uint8_t* d_keep, const int16_t* d_plane_a,
                 const double* d_w_a, int h, int w, const double* h_cam_a, const int16_t* d_plane_b, const double* d_w_b, const uint8_t* d_keep_b, int hb,
                 int wb, const double* h_cam_b, double w_step_b, double max_diff, double* d_P, double* d_D, uint8_t* d_ok, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_du || !d_dv || !d_valid || !d_keep || !d_plane_a || !d_w_a || !h_cam_a || !d_plane_b || !d_w_b || !d_keep_b || !h_cam_b || !d_P || !d_D || !d_ok)
        return ctx->fail(DENSE_REFUSED, "im_flow_lift: null pointer");
    if (bad_side(h) || bad_side(w) || bad_side(hb) || bad_side(wb)) return ctx->fail(DENSE_REFUSED, "im_flow_lift: h and w must be 1..16384");
    if (!positive(max_diff)) return ctx->fail(DENSE_REFUSED, "im_flow_lift: max_diff must be finite and > 0");
    if (!positive(fabs(w_step_b))) return ctx->fail(DENSE_REFUSED, "im_flow_lift: w_step must be finite and not zero");
    hipStream_t s = (hipStream_t)stream;
    FlowLiftArgs a{d_du, d_dv, d_valid, d_keep, d_plane_a, d_w_a, h, w, d_plane_b, d_w_b, d_keep_b, hb, wb, {}, {}, max_diff * fabs(w_step_b), d_P, d_D, d_ok};
    __builtin_memcpy(&a.ca, h_cam_a, sizeof(DenseCam));
    __builtin_memcpy(&a.cb, h_cam_b, sizeof(DenseCam));
    IM_LAUNCH(ctx, "flow_lift", s, launch(flow_lift_kernel, blocks_of((long long)h * w, 256), 256, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_flow_lift");
    return 0;
}

}  // extern "C"
