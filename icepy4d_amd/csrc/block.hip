// One attention block of the matchers as a launch sequence (block.h). Host code only.
#include "block.h"

#include "lg_misc.h"
#include "workspace.h"

namespace im {

int launch_block_proj(im_ctx* ctx, hipStream_t s, const char* name, const GemmArgs& g, const float* wp_layers, int layer, const AttnArgs& at,
                      bool* planes_done) {
    *planes_done = false;
    if (env_is_1("IM_PROJ_TILED")) {
        IM_LAUNCH(ctx, name, s, launch_gemm(g, s));
        return 0;
    }
    GemmArgs r = g;
    r.wp = reinterpret_cast<const unsigned char*>(wp_layers) + (size_t)layer * g.N * 256 * 6;   // three bf16 planes: 6 bytes per weight
    if (env_is_1("IM_PROJ_ROWS32") || !at.planes || attn_f32_form(at)) {
        IM_LAUNCH(ctx, name, s, launch_proj_rows(r, s));
        return 0;
    }
    IM_LAUNCH(ctx, name, s, launch_proj_planes(r, at.planes, s));
    *planes_done = true;
    return 0;
}

int launch_block_tail(im_ctx* ctx, hipStream_t s, const AttnArgs& at, bool planes_done, const BlockFfn& f, const GemmArgs& base, float* x) {
    Workspace* ws = ctx->ws;
    const long xb = (long)base.m_max * 256, hb = (long)base.m_max * 512;
    if (!planes_done) IM_LAUNCH(ctx, "attn_kv_planes", s, launch_attn_planes(at, s));
    IM_LAUNCH(ctx, at.cross ? "flash_attn_cross" : "flash_attn_self", s, launch_flash_attn(at, s));
    // A/B switch: IM_FFN_UNFUSED=1 keeps the launch-per-layer form
    static const bool unfused = env_is_1("IM_FFN_UNFUSED");
    if (!unfused) {   // first layer on cat([x, att]), LayerNorm + GELU or ReLU, second layer, residual: one kernel (ffn_fused.hip)
        FfnArgs a;
        a.act = f.act; a.x = x; a.x_bstride = xb; a.att = at.out; a.att_bstride = xb;
        a.w0p = f.w0p; a.b0 = f.b0; a.ln_g = f.ln_g; a.ln_b = f.ln_b; a.w3p = f.w3p; a.b3 = f.b3;
        a.m_max = base.m_max; a.batch = base.batch; a.m_ptr = base.m_ptr; a.active = base.active; a.pstride = base.pstride;
        IM_LAUNCH(ctx, f.name_fused, s, launch_ffn_fused(a, s));
        return 0;
    }
    {   // the second source of the first layer is the attention output itself: its output projection is folded into the weights
        GemmArgs g = base;
        g.A = x; g.a_bstride = xb; g.lda = 256; g.A1 = at.out; g.a1_bstride = xb; g.lda1 = 256; g.ksplit = 256;
        g.W = f.w0; g.ldw = 512; g.bias = f.b0; g.N = 512; g.K = 512;
        g.C = ws->h; g.c_bstride = hb; g.ldc = 512; g.epi = f.act == 1 ? EPI_BIAS_RELU : EPI_BIAS;
        IM_LAUNCH(ctx, f.name_ffn0, s, launch_gemm(g, s));
    }
    if (f.act == 0)
        IM_LAUNCH(ctx, "lg_layernorm_gelu", s, launch_layernorm_gelu(ws->h, hb, ws->st, base.batch, base.m_max, f.ln_g, f.ln_b, s));
    {   // x += second layer(h)
        GemmArgs g = base;
        g.A = ws->h; g.a_bstride = hb; g.lda = 512; g.W = f.w3; g.ldw = 512; g.bias = f.b3; g.N = 256; g.K = 512;
        g.C = x; g.c_bstride = xb; g.ldc = 256; g.R = x; g.r_bstride = xb; g.ldr = 256; g.epi = EPI_BIAS_RESID;
        IM_LAUNCH(ctx, f.name_ffn3, s, launch_gemm(g, s));
    }
    return 0;
}

}  // namespace im
