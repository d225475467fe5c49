// Fusion of the two depth maps of a stereo pair on the device: one point per surface sample, placed by both views' measurements, with the
// number of views that saw it (what the reference gets from Metashape's buildDenseCloud(point_confidence=True), `metashape.py:198-240`).
// Metashape's merge is closed and is not reproduced: every quantity has a definition of this project's own (fuse_pixel.h) and
// is pinned bit for bit against tests/fuse_oracle.py. Parity with Metashape is unpinned by construction.
//
//   fuse_link_kernel   one thread per pixel of the base view a: its link into view b, the fused inverse depth and score, the view count, and
//                      claimed[link] = 1. Several pixels may claim the same target: they store the same byte, so the race is benign and
//                      needs no atomic; every pixel keeps its own point, so nothing depends on the order of the threads.
//   fuse_rest_kernel   one thread per pixel of view b: kept, unclaimed and without a link of its own into view a.
// Gather-bound float64 kernels with two or three divisions per pixel: nothing to tile, no LDS. The pose travels by value, as in
// dense_consistency_kernel. Every element of every output is written. Enqueue only.
#include <initializer_list>

#include "common.h"
#include "ctx.h"
#include "fuse_pixel.h"
#include "dense_host.h"

namespace im {
namespace {

static_assert(FUSE_MAX_SIDE == DENSE_MAX_SIDE, "bad_side of dense_host.h is the limit of a fused map's side");
constexpr int FUSE_BLOCK = 256;

struct FuseLinkArgs {
    const uint8_t* keep_a; const double* w_a; const float* score_a; int ha, wa;
    const uint8_t* keep_b; const double* w_b; const float* score_b; int hb, wb;
    DensePose P;
    double tol;
    int* link; double* w_out; float* score_out; uint8_t* views; uint8_t* claimed;
};

__global__ __launch_bounds__(FUSE_BLOCK) void fuse_link_kernel(FuseLinkArgs a) {
    const long i = blockIdx.x * (long)FUSE_BLOCK + threadIdx.x;
    if (i >= (long)a.ha * a.wa) return;
    const FusedPixel o = fuse_pixel(a.P, (int)(i % a.wa), (int)(i / a.wa), a.keep_a[i], a.w_a[i], a.score_a[i], a.keep_b, a.w_b, a.score_b, a.hb, a.wb, a.tol);
    a.link[i] = o.link; a.w_out[i] = o.w; a.score_out[i] = o.score; a.views[i] = o.views;
    if (o.link >= 0) a.claimed[o.link] = 1;           // 0 <= link < hb wb: fuse_link checked the pixel against both sides
}

struct FuseRestArgs {
    const uint8_t* keep_b; const double* w_b; int hb, wb;
    const uint8_t* keep_a; const double* w_a; int ha, wa;
    DensePose P;
    double tol;
    const uint8_t* claimed; uint8_t* rest;
};

__global__ __launch_bounds__(FUSE_BLOCK) void fuse_rest_kernel(FuseRestArgs a) {
    const long i = blockIdx.x * (long)FUSE_BLOCK + threadIdx.x;
    if (i >= (long)a.hb * a.wb) return;
    a.rest[i] = fuse_rest(a.P, (int)(i % a.wb), (int)(i / a.wb), a.keep_b[i], a.claimed[i], a.w_b[i], a.keep_a, a.w_a, a.ha, a.wa, a.tol) ? 1 : 0;
}

bool among(const void* out, std::initializer_list<const void*> ins) {
    for (const void* p : ins)
        if (p == out) return true;
    return false;
}

}  // namespace
}  // namespace im

using namespace im;

extern "C" {

int im_dense_fuse_link(im_ctx* ctx, const uint8_t* d_keep_a, const double* d_w_a, const float* d_score_a, int ha, int wa, const uint8_t* d_keep_b,
                       const double* d_w_b, const float* d_score_b, int hb, int wb, const double* h_pose, double tol, int* d_link, double* d_w_out,
                       float* d_score_out, uint8_t* d_views, uint8_t* d_claimed, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_keep_a || !d_w_a || !d_score_a || !d_keep_b || !d_w_b || !d_score_b || !h_pose || !d_link || !d_w_out || !d_score_out || !d_views || !d_claimed)
        return ctx->fail(DENSE_REFUSED, "im_dense_fuse_link: null pointer");
    if (bad_side(ha) || bad_side(wa) || bad_side(hb) || bad_side(wb)) return ctx->fail(DENSE_REFUSED, "im_dense_fuse_link: h and w must be 1..16384");
    if (!(tol >= 0.0)) return ctx->fail(DENSE_REFUSED, "im_dense_fuse_link: the tolerance must not be negative");
    // another thread reads what a thread writes if an output is an input: the result would depend on the order of the threads
    for (const void* out : {(const void*)d_link, (const void*)d_w_out, (const void*)d_score_out, (const void*)d_views, (const void*)d_claimed})
        if (among(out, {d_keep_a, d_w_a, d_score_a, d_keep_b, d_w_b, d_score_b}))
            return ctx->fail(DENSE_REFUSED, "im_dense_fuse_link: the outputs must not be the inputs");
    hipStream_t s = (hipStream_t)stream;
    FuseLinkArgs a{d_keep_a, d_w_a, d_score_a, ha, wa, d_keep_b, d_w_b, d_score_b, hb, wb, {}, tol, d_link, d_w_out, d_score_out, d_views, d_claimed};
    __builtin_memcpy(&a.P, h_pose, sizeof(DensePose));
    IM_HIP(ctx, hipMemsetAsync(d_claimed, 0, (size_t)hb * wb, s));
    IM_LAUNCH(ctx, "dense_fuse_link", s, launch(fuse_link_kernel, blocks_of((long long)ha * wa, FUSE_BLOCK), FUSE_BLOCK, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_dense_fuse_link");
    return 0;
}

int im_dense_fuse_rest(im_ctx* ctx, const uint8_t* d_keep_b, const double* d_w_b, int hb, int wb, const uint8_t* d_keep_a, const double* d_w_a, int ha,
                       int wa, const double* h_pose_ba, double tol_a, const uint8_t* d_claimed, uint8_t* d_rest, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_keep_b || !d_w_b || !d_keep_a || !d_w_a || !h_pose_ba || !d_claimed || !d_rest) return ctx->fail(DENSE_REFUSED, "im_dense_fuse_rest: null pointer");
    if (bad_side(ha) || bad_side(wa) || bad_side(hb) || bad_side(wb)) return ctx->fail(DENSE_REFUSED, "im_dense_fuse_rest: h and w must be 1..16384");
    if (!(tol_a >= 0.0)) return ctx->fail(DENSE_REFUSED, "im_dense_fuse_rest: the tolerance must not be negative");
    if (among(d_rest, {d_keep_b, d_w_b, d_keep_a, d_w_a, d_claimed})) return ctx->fail(DENSE_REFUSED, "im_dense_fuse_rest: the output must not be an input");
    hipStream_t s = (hipStream_t)stream;
    FuseRestArgs a{d_keep_b, d_w_b, hb, wb, d_keep_a, d_w_a, ha, wa, {}, tol_a, d_claimed, d_rest};
    __builtin_memcpy(&a.P, h_pose_ba, sizeof(DensePose));
    IM_LAUNCH(ctx, "dense_fuse_rest", s, launch(fuse_rest_kernel, blocks_of((long long)hb * wb, FUSE_BLOCK), FUSE_BLOCK, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_dense_fuse_rest");
    return 0;
}

}  // extern "C"
