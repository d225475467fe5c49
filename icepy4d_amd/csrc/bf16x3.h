// fp32 products on the bf16 matrix cores at fp32 accuracy: the one definition of the arithmetic every large contraction of the library
// uses (gemm.hip BX / proj_rows, ffn_fused.hip, attention_bx.hip, the Winograd layers of conv_wino.hip / conv_wino_bx2.hip) and of the
// host cut of their weights (ffn_fused.hip::pack_frag_weights, weights.hip::pack_conv3x3_wino_bx).
//
// Why: gfx950's f32-input MFMA runs at the VECTOR rate (157 TFLOP/s, 1 / 16 of the bf16 matrix cores) and holds the vector issue port
// while it runs; the bf16 MFMA does neither. An fp32 value is the exact sum of three bf16 values (8 + 8 + 8 significant bits, each cut
// rounded to nearest even from the residual: x = h + m + l with |m| <= 2^-8 |x|, |l| <= 2^-17 |x|, nothing left; the subtractions that
// form the residuals are exact in fp32), a bf16 product is exact in the matrix core's fp32 accumulation, and of the nine products of two
// such triples the three that are dropped (m l, l m, l l) are worth at most 2^-24 |a b| - the rounding of ONE fp32 operation -, 2^-27.4
// in the root mean square (tests/test_host_cpu.py pins this arithmetic in numpy). The six that are kept are accumulated in fp32 small
// terms first: h l, l h, m m, h m, m h, h h. `tools/bf16x_probe.hip` measured the accumulation on the part
// (`profiles/r05_bf16x_probe.txt`): error against an f64 sum, in units of 2^-24 sum |a b|, rms 0.37-0.39 for six products against
// 0.45-0.47 for the f32 MFMA chain at K = 64 .. 4096 (the matrix core adds 16 products before it rounds once), nine products no
// better than six, three 4-30 x worse; and six `v_mfma_f32_32x32x16_bf16` per 16 k run at 2.2-2.35 PFLOP/s = 2.4-2.5 x the f32 MFMA,
// 1.8-2.15 x with four to five vector instructions between the MFMAs - the vector instructions of the cuts run BESIDE the matrix cores
// instead of in front of them.
//
// No timing-ablation switch lives here: a kernel file that has one wraps the shared function (attention_bx.hip, conv_wino.h).
#pragma once
#include <cstdint>
#include <cstring>

#include "common.h"

namespace im {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// v_mfma_f32_32x32x16_bf16: lane (c, hh) of A / B holds k = 8 hh .. 8 hh + 7 of row / column c as eight packed bf16
__device__ __forceinline__ f32x16 mfma_bf(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ unsigned cvt_pk(float a, float b) {            // v_cvt_pk_bf16_f32: a in the low half, round to nearest even
    const bf16x2 v = __builtin_convertvector(f32x2{a, b}, bf16x2);
    return __builtin_bit_cast(unsigned, v);
}
// (a, b) -> three packed bf16 pairs with a = h.lo + m.lo + l.lo and b = h.hi + m.hi + l.hi exactly
__device__ __forceinline__ void split2(float a, float b, unsigned& h, unsigned& m, unsigned& l) {
    h = cvt_pk(a, b);
    float ra = a - __uint_as_float(h << 16), rb = b - __uint_as_float(h & 0xffff0000u);
    m = cvt_pk(ra, rb);
    ra -= __uint_as_float(m << 16);
    rb -= __uint_as_float(m & 0xffff0000u);
    l = cvt_pk(ra, rb);
}
// eight consecutive k of one lane -> its 16 bytes of each plane (one MFMA operand per plane)
struct Planes { u32x4 h, m, l; };
__device__ __forceinline__ Planes split8(float x0, float x1, float x2, float x3, float x4, float x5, float x6, float x7) {
    unsigned h[4], m[4], l[4];
    split2(x0, x1, h[0], m[0], l[0]);
    split2(x2, x3, h[1], m[1], l[1]);
    split2(x4, x5, h[2], m[2], l[2]);
    split2(x6, x7, h[3], m[3], l[3]);
    return Planes{u32x4{h[0], h[1], h[2], h[3]}, u32x4{m[0], m[1], m[2], m[3]}, u32x4{l[0], l[1], l[2], l[3]}};
}
// four consecutive values of a row -> their 8 bytes in each of the three planes (plane p of the image starts at plane0 + p * PLANE_BYTES)
template <int PLANE_BYTES>
__device__ __forceinline__ void put4(unsigned char* plane0, int off, float4 x) {
    unsigned h0, m0, l0, h1, m1, l1;
    split2(x.x, x.y, h0, m0, l0);
    split2(x.z, x.w, h1, m1, l1);
    *reinterpret_cast<u32x2*>(plane0 + off) = u32x2{h0, h1};
    *reinterpret_cast<u32x2*>(plane0 + PLANE_BYTES + off) = u32x2{m0, m1};
    *reinterpret_cast<u32x2*>(plane0 + 2 * PLANE_BYTES + off) = u32x2{l0, l1};
}
// the six products of one 16-deep k chunk, small ones first: h l, l h, m m, h m, m h, h h
__device__ __forceinline__ f32x16 six(u32x4 ah, u32x4 am, u32x4 al, u32x4 bh, u32x4 bm, u32x4 bl, f32x16 acc) {
    acc = mfma_bf(ah, bl, acc);
    acc = mfma_bf(al, bh, acc);
    acc = mfma_bf(am, bm, acc);
    acc = mfma_bf(ah, bm, acc);
    acc = mfma_bf(am, bh, acc);
    acc = mfma_bf(ah, bh, acc);
    return acc;
}

// host: fp32 -> bf16, round to nearest even (what v_cvt_pk_bf16_f32 does; the weights are finite), and back
inline uint16_t bf16_rne(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline float bf16_to_float(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// host: the three planes of one weight, as split2 cuts them on the device
inline void cut3(float x, uint16_t& h, uint16_t& m, uint16_t& l) {
    h = bf16_rne(x);
    const float r1 = x - bf16_to_float(h);
    m = bf16_rne(r1);
    l = bf16_rne(r1 - bf16_to_float(m));
}

}  // namespace im
