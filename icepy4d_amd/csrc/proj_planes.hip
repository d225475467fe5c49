// The K = 256 projections of a transformer block as 64-ROW blocks that write K and V as the attention's bf16 planes (round 10).
//
// proj_rows_kernel (gemm.hip) streams ALL weight planes of the projection (1.18 MB for q | k | v, 0.79 MB for qk | v) through the L1 -> register
// path of its CU once per 32 rows, and with three such blocks resident that one path carries three streams. Here a block owns G = 2 groups of 32
// rows (the x planes of both in LDS: 101 KB, one block per CU) and every weight fragment in registers feeds the six products of BOTH groups
// before it is released: twice the MFMAs per fragment, half the stream per row. Per group and accumulator the products and their order are those
// of proj_rows_kernel (proj_rows.h PR_SIX, k ascending), bias, rotary and scale are its statements: the same bits.
//
// The epilogue leaves out the round trip of K and V through HBM: proj_rows_kernel stored them as fp32 and kv_planes_kernel (attention_bx.hip) read
// them back to cut them into [K | V][image][head][row][plane][64] bf16, which is all the attention kernel reads. A lane holds ONE column of 16 rows
// after bias and rotary; the cut works on pairs of neighbouring columns packed into a dword, so the lanes of a column pair swap one value per two
// registers (the even lane then holds both columns of the even row, the odd lane those of the odd row), cut their pair with bf16x3.h's split2 -
// element by element what split8 does in kv_planes_kernel - and store one dword per plane. Rows at or past the live count are dropped by the
// range check of the descriptor, as the fp32 stores are. A 64-row block whose second group lies past the live rows multiplies zeros for it
// (x rows past the descriptor read as zero) and skips its epilogue: the tail is predication, not a second kernel.
#include "proj_rows.h"

namespace im {

// one 32 x 32 tile after the main loop: fp32 to a.q (the queries; of the cross block also the other image's keys, scaled by alpha) and / or the three planes
template <int EPI>
__device__ __forceinline__ void store_tile(const GemmArgs& a, unsigned char* planes, const f32x16& acc, int z, int M, unsigned row0, int tile, int c, int hh) {
    // ---- the values (gemm_nt_kernel's head-major branch): lane holds column colbase + c, rows row0 + 4 hh + (r & 3) + 8 (r >> 2)
    const int colbase = tile * 32;
    const int col = colbase + c;
    const float bv = a.bias ? a.bias[col] : 0.f;
    const unsigned rowl = row0 + 4 * hh;
    const int which = colbase >> 8, hd = colbase & 255;
    const int d = (hd & 63) + c;
    float scale = a.alpha;
    if constexpr (EPI == EPI_QKV_ROPE) scale = 1.f;
    if constexpr (EPI == EPI_HEADS_QV) scale = which ? 1.f : a.alpha;
    const bool rope = EPI == EPI_QKV_ROPE && which < 2 && a.cs;
    float val[16];
    if (rope) {
        const __amdgpu_buffer_rsrc_t rCs = make_rsrc(a.cs + (long)z * a.enc_bstride, (unsigned)M * 128u);
        const __amdgpu_buffer_rsrc_t rSn = make_rsrc(a.sn + (long)z * a.enc_bstride, (unsigned)M * 128u);
        const unsigned ve = (rowl * 32 + (d >> 1)) * 4u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned so = ((r & 3) + 8 * (r >> 2)) * 128u;
            const float cs = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rCs, ve, so, 0));
            const float sn = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rSn, ve, so, 0));
            const float v = acc[r] + bv;
            const float partner = __shfl_xor(v, 1);
            val[r] = (d & 1) ? (v * cs) + (partner * sn) : (v * cs) + ((-partner) * sn);
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) val[r] = scale * (acc[r] + bv);
    }
    // ---- fp32, head-major [head][row][64]: q only
    if (which == 0) {
        const __amdgpu_buffer_rsrc_t rD = make_rsrc(a.q + (long)z * a.head_bstride + (long)(hd >> 6) * a.head_stride, (unsigned)M * 256u);
        const unsigned vo = (rowl * 64 + d) * 4u;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(val[r]), rD, vo, ((r & 3) + 8 * (r >> 2)) * 256u, 0);
    }
    // ---- planes (kv_planes_kernel's layout: rid * 384 + plane * 128, rid = (z * heads + head) * n_max + row, the K half then the V half)
    const int half = EPI == EPI_QKV_ROPE ? which - 1 : which;       // 0: K (of the cross block: the scaled qk), 1: V
    if (half >= 0) {
        constexpr int HEADS = 4;
        const long rows_all = (long)a.batch * HEADS * a.m_max;
        unsigned char* pb = planes + ((long)half * rows_all + ((long)z * HEADS + (hd >> 6)) * a.m_max) * 384;
        const __amdgpu_buffer_rsrc_t rP = make_rsrc(pb, (unsigned)M * 384u);
        const int odd = c & 1;
        const unsigned vp = (rowl + odd) * 384u + (unsigned)(d & ~1) * 2u;      // even lanes store the row of register r, odd lanes that of r + 1
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            const float got = __shfl_xor(odd ? val[r] : val[r + 1], 1);
            const float lo = odd ? got : val[r], hi = odd ? val[r + 1] : got;    // columns d & ~1 and d | 1 of this lane's row
            unsigned h, m, l;
            split2(lo, hi, h, m, l);
            const unsigned so = ((r & 3) + 8 * (r >> 2)) * 384u;
            __builtin_amdgcn_raw_buffer_store_b32(h, rP, vp, so, 0);
            __builtin_amdgcn_raw_buffer_store_b32(m, rP, vp, so + 128u, 0);
            __builtin_amdgcn_raw_buffer_store_b32(l, rP, vp, so + 256u, 0);
        }
    }
}

// G = 2 row groups of 32 per block. With G = 1 (proj_rows_kernel's main loop, 50 KB of LDS, up to three blocks per CU) and this file's epilogue the two
// projections measured 212 / 149 us per launch of ten pairs against 202 / 139 us in this form (profiles/r10_proj_planes.txt): that form is not built
template <int EPI, int TILES>
__global__ __launch_bounds__(pr::NT, 2) void proj_rows64_kernel(GemmArgs a, unsigned char* planes) {
    using namespace pr;
    constexpr int G = 2;
    static_assert(EPI == EPI_QKV_ROPE || EPI == EPI_HEADS_QV, "the two projections of a LightGlue block");
    extern __shared__ __attribute__((aligned(16))) unsigned char psm[];
    const int z = blockIdx.y, pair = z >> 1;
    if (a.active && a.active[pair * a.pstride] == 0) return;
    const int M = min(a.m_ptr ? a.m_ptr[pair * a.pstride + (z & 1)] : a.m_max, a.m_max);
    const int m0 = blockIdx.x * (G * BM);
    if (m0 >= M) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, hh = lane >> 5;
    const __amdgpu_buffer_rsrc_t rX = make_rsrc(a.A + (long)z * a.a_bstride, (unsigned)M * 1024u);
    const __amdgpu_buffer_rsrc_t rW = make_rsrc(a.wp, (unsigned)a.N * 256u * 6u);

    u32x4 b0[3], b1[3], b2[3], b3[3];
    PR_LOAD(b0, 0)
    PR_LOAD(b1, 1)
    PR_LOAD(b2, 2)
    {   // G x 32 rows x 256 floats -> three planes per group: thread -> (row = idx >> 6, float4 idx & 63), 4 G float4 per thread; rows past M read as zero
        float4 v[4 * G];
#pragma unroll
        for (int i = 0; i < 4 * G; ++i) {
            const int idx = tid + i * NT;
            v[i] = buf_load4(rX, (unsigned)((m0 + (idx >> 6)) * 256 + (idx & 63) * 4) * 4u, 0);
        }
#pragma unroll
        for (int i = 0; i < 4 * G; ++i) {
            const int idx = tid + i * NT, row = idx >> 6;
            put4<PLANE>(psm + (row >> 5) * LDS_BYTES, (row & 31) * PS + (idx & 63) * 8, v[i]);
        }
    }
    __syncthreads();

#define PP_STEP(b_, kc_)                                                  \
    {                                                                     \
        PR_SIX(acc[0], psm, b_, kc_)                                      \
        PR_SIX(acc[1], psm + LDS_BYTES, b_, kc_)                          \
    }
#pragma unroll 1
    for (int j = 0; j < TILES; ++j) {
        const int tile = j * 8 + wave;                       // wave-uniform: columns [32 tile, 32 tile + 32)
        f32x16 acc[G];
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[g][r] = 0.f;
#pragma unroll 1
        for (int kc = 0; kc < 16; kc += 4) {
            const int s_ = j * 16 + kc;
            // a scheduling fence per step, as in proj_rows_kernel: left alone the machine scheduler sinks every load to its use
            PR_LOAD(b3, s_ + 3)
            __builtin_amdgcn_sched_barrier(0);
            PP_STEP(b0, kc)
            __builtin_amdgcn_sched_barrier(0);
            PR_LOAD(b0, s_ + 4)
            __builtin_amdgcn_sched_barrier(0);
            PP_STEP(b1, kc + 1)
            __builtin_amdgcn_sched_barrier(0);
            PR_LOAD(b1, s_ + 5)
            __builtin_amdgcn_sched_barrier(0);
            PP_STEP(b2, kc + 2)
            __builtin_amdgcn_sched_barrier(0);
            PR_LOAD(b2, s_ + 6)
            __builtin_amdgcn_sched_barrier(0);
            PP_STEP(b3, kc + 3)
            __builtin_amdgcn_sched_barrier(0);
        }
        store_tile<EPI>(a, planes, acc[0], z, M, m0, tile, c, hh);
        if (m0 + BM < M) store_tile<EPI>(a, planes, acc[1], z, M, m0 + BM, tile, c, hh);
    }
#undef PP_STEP
}

template <int EPI, int TILES>
static hipError_t launch_proj_planes_t(const GemmArgs& a, unsigned char* planes, hipStream_t s) {
    const dim3 grid((a.m_max + 2 * pr::BM - 1) / (2 * pr::BM), a.batch), block(pr::NT);    // 64 rows per block
    return launch_dyn_lds<proj_rows64_kernel<EPI, TILES>>(grid, block, 2 * pr::LDS_BYTES, s, a, planes);
}

// launch_proj_rows's arguments (a.k / a.v unused); planes = AttnArgs::planes of the attention launch that follows: attn_planes_bytes(a.m_max, a.batch, 4)
hipError_t launch_proj_planes(const GemmArgs& a, void* planes, hipStream_t s) {
    if (!planes || !a.wp || a.K != 256 || a.lda != 256 || a.A1 || a.sel || a.w_bstride || a.n_ptr || a.pair_batched) return hipErrorInvalidValue;
    if (a.m_max <= 0 || a.batch <= 0) return hipSuccess;
    unsigned char* p = static_cast<unsigned char*>(planes);
    if (a.epi == EPI_QKV_ROPE && a.N == 768) return launch_proj_planes_t<EPI_QKV_ROPE, 3>(a, p, s);
    if (a.epi == EPI_HEADS_QV && a.N == 512) return launch_proj_planes_t<EPI_HEADS_QV, 2>(a, p, s);
    return hipErrorInvalidValue;
}

}  // namespace im
