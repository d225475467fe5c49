// The launch sequence of one attention block of the matchers, shared by LightGlue (lightglue.hip) and SuperGlue (superglue.hip): the
// K = 256 projection, then K / V planes, attention and the feed-forward tail. Each model builds the projection's GemmArgs and the
// AttnArgs itself - that is where they differ; from there on a block is described by data only.
#pragma once
#include "ctx.h"

namespace im {

// Feed-forward weights of one block (pointers past the layer offset): first layer on [x | att] with the attention's output
// projection folded in (weights.hip), second layer with the residual
struct BlockFfn {
    int act = 0;                                                // FfnArgs::act: 0 = LayerNorm + GELU between the layers, 1 = ReLU
    const float* w0 = nullptr; const float* w0p = nullptr;      // [512][512] row-major / packed by pack_frag_weights
    const float* b0 = nullptr;                                  // [512]
    const float* ln_g = nullptr; const float* ln_b = nullptr;   // LayerNorm(512) pair; null with act = 1
    const float* w3 = nullptr; const float* w3p = nullptr;      // [256][512] row-major / packed
    const float* b3 = nullptr;                                  // [256]
    const char* name_fused = nullptr; const char* name_ffn0 = nullptr; const char* name_ffn3 = nullptr;   // profile names of the three launches
};

// g (N x 256, every field but wp set) as 64-row blocks over wp_layers + layer, the per-layer pack_frag_weights planes of g.W, that write q as
// fp32 and the K / V of `at` (the block's attention launch) straight into at.planes (proj_planes.hip): *planes_done = true, and launch_block_tail
// then skips the plane pass. The A/B and test switches (read per call; same bits): IM_PROJ_ROWS32=1, the 32-row blocks of gemm.hip that write
// fp32 q / k / v; IM_PROJ_TILED=1, the tiled GEMM. Both - and an attention launch without planes or in the f32 form, which reads fp32 K / V -
// leave *planes_done = false
int launch_block_proj(im_ctx* ctx, hipStream_t s, const char* name, const GemmArgs& g, const float* wp_layers, int layer, const AttnArgs& at,
                      bool* planes_done);

// attn_kv_planes (unless the projection wrote the planes), attention, then x += ffn(cat([x, at.out])) for the live rows: one fused kernel, or with IM_FFN_UNFUSED=1 (read once
// per process) GEMM (+ LayerNorm / GELU launch, or ReLU epilogue) + GEMM through ws->h. `base` carries the batch: m_max, m_ptr, active, pstride, batch, bx
int launch_block_tail(im_ctx* ctx, hipStream_t s, const AttnArgs& at, bool planes_done, const BlockFfn& f, const GemmArgs& base, float* x);

}  // namespace im
