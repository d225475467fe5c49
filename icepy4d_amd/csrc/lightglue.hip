// LightGlue (`lightglue/lightglue.py`): one transformer block, the forward pass over pairs as a fixed sequence of kernel launches on
// one stream (no host synchronisation inside: early-stop and pruning state live in device memory), and the record packers.
#include "block.h"
#include "lg_misc.h"
#include "workspace.h"

using namespace im;

static constexpr int ST_INTS = (int)(sizeof(LGState) / sizeof(int));   // ints between the states of consecutive pairs

static int lg_block(im_ctx* ctx, hipStream_t s, int NI, int layer, bool cross, float* x, const float* cs, const float* sn) {
    Workspace* ws = ctx->ws;
    const LightGlueW& W = ctx->lg;
    const int K = ctx->max_kpts;
    const long xb = (long)K * 256;
    const int* n_ptr = ws->st->n;
    const int* active = &ws->st->active;
    GemmArgs base;
    base.m_max = K; base.m_ptr = n_ptr; base.active = active; base.pstride = ST_INTS; base.batch = NI; base.bx = 1;
    AttnArgs at;
    at.q = ws->q; at.k = cross ? ws->q : ws->k; at.v = ws->v; at.hstride = (long)K * 64; at.bstride = (long)K * 256;
    at.out = ws->att; at.out_bstride = xb; at.ldo = 256; at.n_ptr = n_ptr; at.pstride = ST_INTS; at.n_max = K; at.batch = NI; at.heads = 4;
    at.cross = cross ? 1 : 0; at.active = active; at.part = ws->attn_part; at.counters = ws->attn_cnt; at.planes = ws->attn_planes; at.clock = ctx->clock_of(0);
    bool planes_done = false;
    GemmArgs g = base;
    g.A = x; g.a_bstride = xb; g.lda = 256; g.ldw = 256; g.K = 256;
    g.q = ws->q; g.v = ws->v; g.head_bstride = (long)K * 256; g.head_stride = (long)K * 64; g.big_tile = NI >= 4;
    if (!cross) {
        g.W = W.qkv_w + (long)layer * 768 * 256; g.bias = W.qkv_b + (long)layer * 768; g.N = 768; g.epi = EPI_QKV_ROPE;
        g.k = ws->k; g.cs = cs; g.sn = sn; g.enc_bstride = (long)K * 32;
        if (int rc = launch_block_proj(ctx, s, "lg_qkv_rope_gemm", g, W.qkv_wp, layer, at, &planes_done)) return rc;
        at.scale = 0.125f;  // SDPA default 1/sqrt(64) (`lightglue.py:120-123`)
    } else {   // [to_qk ; to_v]
        g.W = W.cqv_w + (long)layer * 512 * 256; g.bias = W.cqv_b + (long)layer * 512; g.N = 512; g.epi = EPI_HEADS_QV;
        g.alpha = (float)0.35355339059327373;  // scale**0.5 = 64**-0.25 on to_qk (`lightglue.py:201`); to_v unscaled
        if (int rc = launch_block_proj(ctx, s, "lg_proj_gemm", g, W.cqv_wp, layer, at, &planes_done)) return rc;
        at.scale = 1.f;
    }
    // ffn.0 on cat([x, att]) (out_proj / to_out folded into the weights), LayerNorm, GELU, ffn.3, residual
    const LightGlueW::Ffn& F = cross ? W.cross_ffn : W.self_ffn;
    BlockFfn f;
    f.w0 = F.w0 + (long)layer * 512 * 512; f.w0p = F.w0p + (long)layer * 512 * 512 * 3 / 2; f.b0 = F.b0 + (long)layer * 512;
    f.ln_g = F.ln_g + (long)layer * 512; f.ln_b = F.ln_b + (long)layer * 512;
    f.w3 = F.w3 + (long)layer * 256 * 512; f.w3p = F.w3p + (long)layer * 256 * 512 * 3 / 2; f.b3 = F.b3 + (long)layer * 256;
    f.name_fused = "lg_ffn_fused"; f.name_ffn0 = "lg_ffn0_gemm"; f.name_ffn3 = "lg_ffn3_gemm";
    return launch_block_tail(ctx, s, at, planes_done, f, base, x);
}

static int lightglue_forward(im_ctx* ctx, int n_pairs, const float* d_kpts, const float* d_desc, const int32_t* d_n, const float* h_size,
                             const im_lightglue_conf* conf, int32_t* d_matches, float* d_mscores, int32_t* d_prune, int32_t* d_info,
                             void* stream) {
    IM_CHECK_CTX(ctx);
    if (!ctx->lg.ready) return ctx->fail(-50, "im_lightglue_forward: weights not finalized");
    Workspace* ws = ctx->ws;
    if (!ws) return ctx->fail(-51, "im_lightglue_forward: call im_ctx_reserve first");
    if (n_pairs < 1 || n_pairs > ws->n_pairs || n_pairs > 64)
        return ctx->fail(-53, "im_lightglue_forward: %d pairs, the workspace was reserved for %d (max_images / 2)", n_pairs, ws->n_pairs);
    hipStream_t s = (hipStream_t)stream;
    const LightGlueW& W = ctx->lg;
    const int K = ctx->max_kpts;
    const int L = conf->n_layers;
    const int NP = n_pairs, NI = 2 * n_pairs;
    if (L < 1 || L > 9) return ctx->fail(-52, "im_lightglue_forward: n_layers must be 1..9");
    const bool do_stop = conf->depth_confidence > 0, do_prune = conf->width_confidence > 0;
    const long xb = (long)K * 256, eb = (long)K * 32;
    LGState* st = ws->st;

    IM_HIP(ctx, launch_lg_init(st, NI, d_n, ws->ind[0], ws->prune, K, K, d_matches, d_mscores, K, s));
    IM_HIP(ctx, hipMemcpyAsync(ws->x[0], d_desc, sizeof(float) * NI * xb, hipMemcpyDeviceToDevice, s));
    IM_HIP(ctx, launch_posenc(d_kpts, (long)K * 2, st, NI, K, W.wr, h_size, ws->cs[0], ws->sn[0], eb, s));
    int cur = 0;
    for (int i = 0; i < L; ++i) {
        int rc = lg_block(ctx, s, NI, i, false, ws->x[cur], ws->cs[cur], ws->sn[cur]);
        if (rc) return rc;
        rc = lg_block(ctx, s, NI, i, true, ws->x[cur], ws->cs[cur], ws->sn[cur]);
        if (rc) return rc;
        if (i == L - 1) break;
        if (!do_stop && !do_prune) continue;
        IM_LAUNCH(ctx, "lg_adapt", s, launch_rowdot(ws->x[cur], xb, st, NI, K, do_stop ? W.tc_w + (long)i * 256 : nullptr, W.tc_b + i, 1,
                                  do_prune ? W.ma_w + (long)i * 256 : nullptr, W.ma_b + i, nullptr, ws->conf, ws->msc, K,
                                  W.thr[i], do_stop ? i : -1, 1, s));
        // keep threshold: `scores > (1 - width_confidence)` evaluated in double, compared in fp32 (`lightglue.py:566`)
        const float keep_thr = (float)(1.0 - (double)conf->width_confidence);
        IM_LAUNCH(ctx, "lg_adapt", s, launch_stop_prune(st, NP, i, do_stop, do_prune, (float)conf->depth_confidence, keep_thr, W.thr[i], ws->conf,
                                                      ws->msc, K, ws->ind[cur], ws->ind[1 - cur], ws->keep_idx, ws->prune, K,
                                                      conf->pruning_min_kpts, s));
        if (do_prune) {
            IM_LAUNCH(ctx, "lg_adapt", s, launch_gather_rows(st, NI, K, ws->keep_idx, K, ws->x[cur], ws->x[1 - cur], xb, ws->cs[cur], ws->cs[1 - cur],
                                                           ws->sn[cur], ws->sn[1 - cur], eb, do_stop ? i : -1, (float)conf->depth_confidence, s));
            cur = 1 - cur;
        }
    }
    ctx->dbg_cur = cur;
    // ---- assignment with log_assignment[last executed layer] (per pair: a device-side layer index)
    IM_HIP(ctx, launch_lg_select_layer(st, NP, L, ws->sel, d_info, s));
    {
        GemmArgs g;
        g.m_max = K; g.m_ptr = st->n; g.pstride = ST_INTS; g.batch = NI; g.bx = 1;
        g.A = ws->x[cur]; g.a_bstride = xb; g.lda = 256; g.W = W.fp_w; g.ldw = 256; g.bias = W.fp_b;
        g.sel = ws->sel; g.w_sel_stride = 65536; g.bias_sel_stride = 256; g.N = 256; g.K = 256;
        g.C = ws->md; g.c_bstride = xb; g.ldc = 256; g.alpha = 0.25f;  // / 256**0.25 (`lightglue.py:279`)
        g.epi = EPI_BIAS;
        IM_LAUNCH(ctx, "lg_proj_gemm", s, launch_gemm(g, s));
    }
    IM_HIP(ctx, launch_rowdot(ws->x[cur], xb, st, NI, K, W.ma_w, W.ma_b, 0, nullptr, nullptr, ws->sel, ws->z, nullptr, K, 0.f, -1, 0, s));
    IM_HIP(ctx, launch_logsig(ws->z, K, st, NI, K, ws->lz, s));
    {   // one score matrix per pair: md of image 2p against md of image 2p + 1
        GemmArgs g;
        g.m_max = K; g.m_ptr = &st->n[0]; g.n_ptr = &st->n[1]; g.pstride = ST_INTS; g.pair_batched = 1; g.batch = NP; g.bx = 1;
        g.A = ws->md; g.a_bstride = 2 * xb; g.lda = 256; g.W = ws->md + xb; g.w_bstride = 2 * xb; g.ldw = 256; g.N = K; g.K = 256;
        g.C = ws->sim; g.c_bstride = (long)ws->sim_ps; g.ldc = K; g.epi = EPI_BIAS; g.big_tile = 1;
        IM_LAUNCH(ctx, "score_gemm", s, launch_gemm(g, s));
    }
    AssignArgs a;
    a.sim = ws->sim; a.ld = K; a.m_ptr = &st->n[0]; a.n_ptr = &st->n[1]; a.m_max = K; a.n_max = K;
    a.lz0 = ws->lz; a.lz1 = ws->lz + K;
    a.rmax = ws->rmax; a.rlog = ws->rlog; a.cmax = ws->cmax; a.clog = ws->clog; a.part = ws->part;
    a.ridx = ws->ridx; a.rval = ws->rval; a.cbest = ws->cbest; a.threshold = (float)conf->filter_threshold;
    a.ind0 = ws->ind[cur]; a.ind1 = ws->ind[cur] + K;
    a.out_m0 = d_matches; a.out_m1 = d_matches + K; a.out_s0 = d_mscores; a.out_s1 = d_mscores + K;
    a.n_pairs = NP; a.sim_ps = (long)ws->sim_ps; a.vec_ps = (long)ws->vec_ps; a.part_ps = (long)ws->part_ps; a.lz_ps = 2L * K;
    a.out_ps = 2L * K; a.state_ps = ST_INTS;
    IM_LAUNCH(ctx, "assign", s, launch_assign(a, s));
    IM_HIP(ctx, hipMemcpyAsync(d_prune, ws->prune, sizeof(int) * NI * K, hipMemcpyDeviceToDevice, s));
    IM_GUARD_CHECK(ctx, s, "im_lightglue_forward");
    return 0;
}

extern "C" {

int im_lightglue_forward(im_ctx* ctx, const float* d_kpts, const float* d_desc, const int32_t* d_n, const float* h_size,
                         const im_lightglue_conf* conf, int32_t* d_matches, float* d_mscores, int32_t* d_prune,
                         int32_t* d_info, void* stream) {
    return lightglue_forward(ctx, 1, d_kpts, d_desc, d_n, h_size, conf, d_matches, d_mscores, d_prune, d_info, stream);
}

int im_lightglue_forward_pairs(im_ctx* ctx, int n_pairs, const float* d_kpts, const float* d_desc, const int32_t* d_n, const float* h_size,
                               const im_lightglue_conf* conf, int32_t* d_matches, float* d_mscores, int32_t* d_prune,
                               int32_t* d_info, void* stream) {
    return lightglue_forward(ctx, n_pairs, d_kpts, d_desc, d_n, h_size, conf, d_matches, d_mscores, d_prune, d_info, stream);
}

int im_pack_record(im_ctx* ctx, const int32_t* d_n, const int32_t* d_matches0, const float* d_mscores0, const int32_t* d_info,
                   int epoch, int32_t* d_record, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!ctx->ws) return ctx->fail(-51, "im_pack_record: call im_ctx_reserve first");
    IM_HIP(ctx, launch_pack_record(d_n, d_matches0, d_mscores0, d_info, epoch, ctx->max_kpts, d_record, 1, nullptr, (hipStream_t)stream));
    return 0;
}

int im_pack_records(im_ctx* ctx, int n_pairs, const int32_t* d_n, const int32_t* d_matches, const float* d_mscores, const int32_t* d_info,
                    int first_epoch, int32_t* d_records, const float* d_kpts, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!ctx->ws || n_pairs < 1) return ctx->fail(-51, "im_pack_records: call im_ctx_reserve first");
    IM_HIP(ctx, launch_pack_record(d_n, d_matches, d_mscores, d_info, first_epoch, ctx->max_kpts, d_records, n_pairs, d_kpts, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
