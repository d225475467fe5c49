// SuperPoint forward (`lightglue/superpoint.py`): the convolution stack, detector and descriptor heads and the keypoint selection as a
// fixed sequence of kernel launches on one stream (no host synchronisation inside: keypoint counts live in device memory).
#include "ctx.h"
#include "sp_post.h"
#include "workspace.h"

using namespace im;

extern "C" {

int im_superpoint_forward(im_ctx* ctx, const uint8_t* d_img, int n_images, int h, int w, int channels, int nms_radius,
                          float threshold, int border, int max_kpts, int flavour, float* d_kpts, float* d_scores, float* d_desc,
                          int32_t* d_n, void* stream) {
    IM_CHECK_CTX(ctx);
    // flavour: both select the same candidate set (the border test commutes with the threshold for thr >= 0, tested); it
    // only picks the gray conversion of 3-channel input
    if (channels != 1 && channels != 3 && channels != 4)
        return ctx->fail(-44, "im_superpoint_forward: channels must be 1 (uint8 gray), 3 (uint8 RGB) or 4 (float32 gray), got %d", channels);
    if (!ctx->sp.ready) return ctx->fail(-40, "im_superpoint_forward: weights not finalized");
    Workspace* ws = ctx->ws;
    if (!ws || h > ctx->max_h || w > ctx->max_w || n_images > ctx->max_images)
        return ctx->fail(-41, "im_superpoint_forward: %d x %d x %d exceeds the reserved workspace", n_images, h, w);
    if (h < 8 || w < 8) return ctx->fail(-42, "im_superpoint_forward: image smaller than one cell");
    if (threshold < 0.f) return ctx->fail(-43, "im_superpoint_forward: negative detection threshold unsupported");
    hipStream_t s = (hipStream_t)stream;
    const SuperPointW& W = ctx->sp;
    const int B = n_images, K = ctx->max_kpts;
    // 3x3 layers run in Winograd F(2x2,3x3) form with the products on the bf16 matrix cores (conv_wino.hip BX, six bf16 products per fp32
    // product); IM_CONV_F32=1 selects the same form on the f32-input MFMA (rounds 2-5; read by launch_conv3x3_wino), IM_CONV_DIRECT=1 the direct
    // implicit GEMM (read per call, not cached: the parity tests run all forms in one process; a captured graph keeps the form it was captured with)
    const bool direct = env_is_1("IM_CONV_DIRECT");
    auto conv = [&](ConvArgs& a, int layer) {
        a.w = direct ? W.cw[layer] : W.cww[layer];
        a.wx = W.cwx[layer];
        a.clock = ctx->clock_of(1);
        return direct ? launch_conv3x3(a, s) : launch_conv3x3_wino(a, s);
    };
    // conv1a is fused into conv1b's patch producer: the full-resolution 64-channel activation never touches HBM
    float* src = nullptr;
    float* dst = ws->act1;
    int ch = h, cw_ = w;
    static const int pool_after[7] = {1, 0, 1, 0, 1, 0, 0};  // conv1b, 2a, 2b, 3a, 3b, 4a, 4b
    for (int i = 0; i < 7; ++i) {
        ConvArgs a;
        a.in = src; a.bias = W.cb[i]; a.out = dst; a.B = B; a.H = ch; a.W = cw_;
        a.Cin = SP_CIN[i]; a.Cout = SP_COUT[i]; a.pool = pool_after[i]; a.relu = 1;
        if (i == 0) { a.img = d_img; a.img_channels = channels; a.gray_mode = flavour == 1 ? 1 : 0; a.w1 = W.c1a_w; a.b1 = W.c1a_b; a.w1q = W.c1a_wq; }
        IM_LAUNCH(ctx, SP_CONV3[i], s, conv(a, i));
        if (pool_after[i]) { ch /= 2; cw_ /= 2; }
        src = dst;
        dst = (dst == ws->act1) ? ws->act0 : ws->act1;
    }
    dst = (src == ws->act1) ? ws->act0 : ws->act1;
    // src = feat [B][hc][wc][128] (in act1), dst = act0 free
    const int hc = ch, wc = cw_;
    const long cells = (long)B * hc * wc;
    float* feat = src;
    float* tmp = dst;
    {
        ConvArgs a;
        a.in = feat; a.bias = W.cb[7]; a.out = tmp; a.B = B; a.H = hc; a.W = wc; a.Cin = 128; a.Cout = 256;
        IM_LAUNCH(ctx, "convPa", s, conv(a, 7));
        GemmArgs g;
        g.A = tmp; g.lda = 256; g.W = W.pb_w; g.ldw = 256; g.bias = W.pb_b; g.N = 65; g.K = 256; g.m_max = (int)cells;
        g.C = ws->logits; g.ldc = 65; g.epi = EPI_BIAS;
        IM_LAUNCH(ctx, "convPb_gemm", s, launch_gemm(g, s));
        IM_LAUNCH(ctx, "det_softmax", s, launch_det_softmax(ws->logits, 65, ws->smap, B, hc, wc, s));
    }
    const int H8 = hc * 8, W8 = wc * 8;
    IM_LAUNCH(ctx, "nms_select", s, launch_nms_select(ws->smap, ws->nms, ws->mask, ws->supp, ws->rest, B, H8, W8, nms_radius, border,
                                                    threshold, max_kpts, K, ws->kpsel, d_kpts, d_scores, d_n, s));
    {
        ConvArgs a;
        a.in = feat; a.bias = W.cb[8]; a.out = tmp; a.B = B; a.H = hc; a.W = wc; a.Cin = 128; a.Cout = 256;
        IM_LAUNCH(ctx, "convDa", s, conv(a, 8));
        GemmArgs g;
        g.A = tmp; g.lda = 256; g.W = W.db_w; g.ldw = 256; g.bias = W.db_b; g.N = 256; g.K = 256; g.m_max = (int)cells;
        g.C = ws->dense; g.ldc = 256; g.epi = EPI_BIAS;
        IM_LAUNCH(ctx, "convDb_gemm", s, launch_gemm(g, s));
        IM_LAUNCH(ctx, "sample_desc", s, launch_sample_desc(ws->dense, B, hc, wc, d_kpts, d_n, K, d_desc, s));
    }
    IM_GUARD_CHECK(ctx, s, "im_superpoint_forward");
    return 0;
}

int im_superpoint_candidates(im_ctx* ctx, int n_images, int32_t* h_counts, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!ctx->ws || !h_counts || n_images < 1 || n_images > ctx->max_images) return ctx->fail(-41, "im_superpoint_candidates: bad arguments");
    IM_HIP(ctx, hipMemcpyAsync(h_counts, ctx->ws->kpsel.n_cand, sizeof(int32_t) * n_images, hipMemcpyDeviceToHost, (hipStream_t)stream));
    IM_HIP(ctx, hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

}  // extern "C"
