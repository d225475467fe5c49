// The row-block form of the K = 256 projections, the part its kernels share (gemm.hip proj_rows_kernel: 32 rows per block, fp32 q / k / v;
// proj_planes.hip proj_rows64_kernel: 64 rows per block, K / V as the attention's bf16 planes): the LDS layout of the x planes, the weight
// fragment ring and the six products of one step. Macros, not functions: as calls the register numbering of proj_rows_kernel moves.
#pragma once
#include "bf16x3.h"
#include "common.h"
#include "kernels.h"

namespace im {
namespace pr {
constexpr int BM = 32, NT = 512;
constexpr int PS = 528;              // bytes per row of a plane: 256 x 2 + 16 (132 dwords = 4 mod 64: conflict-free 16-byte row reads)
constexpr int PLANE = BM * PS;       // 16,896
constexpr int LDS_BYTES = 3 * PLANE; // 50,688: the three planes of one 32-row group
constexpr unsigned TILE_BYTES = (256 / 16) * 3 * 1024;   // one packed 32-column tile at K = 256: 16 k chunks x 3 planes x 1 KiB
}  // namespace pr
}  // namespace im

// Weight steps (one 16-deep k chunk of one column tile = three 1 KB loads) run THREE steps ahead through four register buffers: the step index s = 16 j + kc
// walks this wave's tiles j * 8 + wave; steps past the last tile are out of the descriptor's range by their lane offset (zeros, no traffic, no branch).
// Reads rW (the descriptor of the packed weights), wave, lane and TILES of the kernel it is used in.
#define PR_LOAD(b_, s_)                                                                                                          \
    {                                                                                                                            \
        const bool in_ = (s_) < TILES * 16;                                                                                      \
        const unsigned so_ = in_ ? (unsigned)((((s_) >> 4) * 8 + wave)) * TILE_BYTES + (unsigned)(((s_) & 15) * 3) * 1024u : 0u;   \
        const unsigned vo_ = in_ ? lane * 16u : 0x80000000u;    /* out of range by the LANE offset: a scalar offset beyond num_records would wrap the range check */ \
        _Pragma("unroll") for (int g = 0; g < 3; ++g) b_[g] = __builtin_amdgcn_raw_buffer_load_b128(rW, vo_, so_ + (unsigned)g * 1024u, 0); \
    }

// acc_ += the x planes of the 32-row group at xs_ (LDS) times the weight fragment b_ of k chunk kc_: bf16x3.h's six(), spelled out (as a call two
// register quads of proj_rows_kernel swap names; not yet A/B-timed). Reads c and hh of the kernel it is used in.
#define PR_SIX(acc_, xs_, b_, kc_)                                                                                   \
    {                                                                                                                \
        const unsigned char* ap = (xs_) + c * PS + ((kc_) * 16 + hh * 8) * 2;                                        \
        const u32x4 ah = *reinterpret_cast<const u32x4*>(ap), am = *reinterpret_cast<const u32x4*>(ap + PLANE),   \
                     al = *reinterpret_cast<const u32x4*>(ap + 2 * PLANE);                                          \
        acc_ = mfma_bf(ah, b_[2], acc_);                                                                            \
        acc_ = mfma_bf(al, b_[0], acc_);                                                                            \
        acc_ = mfma_bf(am, b_[1], acc_);                                                                            \
        acc_ = mfma_bf(ah, b_[1], acc_);                                                                            \
        acc_ = mfma_bf(am, b_[0], acc_);                                                                            \
        acc_ = mfma_bf(ah, b_[0], acc_);                                                                            \
    }
