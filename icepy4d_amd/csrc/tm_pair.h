// The arithmetic of one pair of csrc/templatematch.hip: the plan of the correlation kernel, the window rule of `OC`
// (`templatematch.py:268-294`), one pixel of `forient`, the definition of one element of C as the order of its fused multiply-adds, the
// wave's argmax and sum of |C| as lane 0 sees them, and the tail of the peak kernel (edge test, window, centroid, outputs). A header of its
// own, without the context or any launch code, like warp_pixel.h: a host program compiles the very text the kernels compile
// (tests/tm_host_harness.cpp, through a stub <hip/hip_runtime.h>) and is compared with the numpy restatement (tests/tm_oracle.py) bit for
// bit. Maps are complex64 as interleaved floats (re, im).
//
// The summation order of C[i][j] (tm_corr_element is the definition; tm_corr_kernel computes the same chains in its own layout): the
// template rows of a chunk are dealt over `ks` groups, group k takes the rows r = k, k + ks, ... of every chunk. Its partial sum is ONE
// fmaf chain from +0 over the chunks (cy outer, cx inner), its rows of the chunk, channel 0 (real) then channel 1 (imaginary, the
// template value multiplied by isign first), and the chunk's kx columns in order; rows and columns beyond T are zeros that are still
// multiplied, and so are B values beyond the S x S window. The ks partials are then added in group order, partial 0 first.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <math.h>

namespace im {
namespace {

constexpr int TM_DX = 16;                       // C columns per thread
constexpr int TM_MAX_THREADS = 256;
constexpr int TM_LDS_FLOATS = 16384;            // 64 KiB of LDS per block: two blocks of 256 threads per CU at least
constexpr int TM_WAVE = 64;

struct TmPlan {
    int R;            // S - T: C is R x R
    int gy, gx, ks;   // rows of C, 16-column strips of C and template-row groups per block
    int ny, nx;       // tiles of C per pair
    int kt, kx;       // template rows / columns staged per chunk (kt a multiple of ks, kx a multiple of 16)
    int pitch;        // floats per staged B row (== 4 mod 16: the 16 lanes of a ds_read_b128 group hit 16 different bank quads)
    int brows;        // gy + kt - 1
    int threads;
    int lds_floats;
};

inline int tm_stage_floats(const TmPlan& p) { return 2 * p.brows * p.pitch + 2 * p.kt * p.kx; }

inline TmPlan tm_plan(int T, int S) {
    TmPlan p;
    p.R = S - T;
    const int R = p.R;
    auto up = [](int a, int b) { return (a + b - 1) / b * b; };
    p.gy = R < 16 ? R : (up(R, 32) <= up(R, 16) ? 32 : 16);
    const int mx = (R + TM_DX - 1) / TM_DX;
    p.gx = std::min(mx, TM_MAX_THREADS / p.gy);
    p.nx = (mx + p.gx - 1) / p.gx;
    p.gx = (mx + p.nx - 1) / p.nx;
    p.ny = (R + p.gy - 1) / p.gy;
    p.ks = std::max(1, std::min(TM_MAX_THREADS / (p.gy * p.gx), T));
    p.kx = std::min(up(T, 16), 128);
    auto set_rows = [&](int kt) { p.kt = kt; p.brows = p.gy + kt - 1; p.pitch = TM_DX * p.gx + p.kx + 4; };
    set_rows(p.ks);
    while (tm_stage_floats(p) > TM_LDS_FLOATS && p.ks > 1) { p.ks /= 2; set_rows(p.ks); }
    while (tm_stage_floats(p) > TM_LDS_FLOATS && p.kx > 16) { p.kx -= 16; set_rows(p.ks); }
    // as many template rows per chunk as fit, in chunks of equal size
    int kt_max = p.ks;
    for (int kt = 2 * p.ks; kt <= up(T, p.ks); kt += p.ks) {
        set_rows(kt);
        if (tm_stage_floats(p) > TM_LDS_FLOATS) break;
        kt_max = kt;
    }
    const int nchunks = (T + kt_max - 1) / kt_max;
    set_rows(up((T + nchunks - 1) / nchunks, p.ks));
    p.threads = up(p.gy * p.gx * p.ks, TM_WAVE);
    p.lds_floats = std::max(tm_stage_floats(p), p.ks > 1 ? p.threads * TM_DX : 0);
    return p;
}

// Window of one pair (`templatematch.py:268-294`). `valid` = the reference correlates this pair.
struct PairWin {
    bool valid;
    long arow, acol, brow, bcol;
    double pu, pv, initdu, initdv;
};

__device__ PairWin pair_window(const double* __restrict__ pairs, const int32_t* __restrict__ bidx, int n_b, long i, int T, int S, int ha,
                               int wa, int hb, int wb) {
    const double u = pairs[4 * i], v = pairs[4 * i + 1], idu = pairs[4 * i + 2], idv = pairs[4 * i + 3];
    PairWin w;
    w.valid = false;
    w.arow = w.acol = w.brow = w.bcol = 0;
    w.initdu = w.initdv = NAN;
    w.pu = u;   // `:264-265`: a NaN u is skipped before anything is written back
    w.pv = v;
    if (isnan(u)) return w;
    const double th = (T & 1) ? 0.5 : 0.0, sh = (S & 1) ? 0.5 : 0.0;   // T / 2 % 1, S / 2 % 1
    const double acx = rint(u) - th, acy = rint(v) - th;                 // np.round: half to even, as rint
    const double bcx = rint(u + idu) - sh, bcy = rint(v + idv) - sh;
    w.pu = acx;
    w.pv = acy;
    w.initdu = bcx - acx;
    w.initdv = bcy - acy;
    if (isnan(u + v)) return w;
    // `.astype(int)` truncates toward zero; the reference skips a lower bound < 0 or an upper bound >= the image size
    const double b0 = trunc(bcy - S / 2.0), b1 = trunc(bcy + S / 2.0), c0 = trunc(bcx - S / 2.0), c1 = trunc(bcx + S / 2.0);
    const double a0 = trunc(acy - T / 2.0), a1 = trunc(acy + T / 2.0), d0 = trunc(acx - T / 2.0), d1 = trunc(acx + T / 2.0);
    if (!(b0 >= 0) || !(a0 >= 0) || !(c0 >= 0) || !(d0 >= 0)) return w;
    if (!(b1 < hb) || !(a1 < ha) || !(c1 < wb) || !(d1 < wa)) return w;
    w.valid = (unsigned)bidx[i] < (unsigned)n_b;      // a B-image index out of range leaves the pair's outputs NaN
    w.brow = (long)b0; w.bcol = (long)c0; w.arow = (long)a0; w.acol = (long)d0;
    return w;
}

// One pixel of forient: r = convolve2d(img, [[1, 0, i], [0, 0, 0], [-i, 0, -1]], "same"): Re = img[y+1][x+1] - img[y-1][x-1],
// Im = img[y+1][x-1] - img[y-1][x+1], divided by the modulus. `base` = the first pixel of the image in img.
__device__ __forceinline__ void forient_pixel(const void* __restrict__ img, int dtype, long base, int h, int w, int y, int x, float& ore, float& oim) {
    auto at = [&](int yy, int xx) -> float {
        if (yy < 0 || yy >= h || xx < 0 || xx >= w) return 0.f;          // convolve2d(mode="same"): zero padding
        const long k = base + (long)yy * w + xx;
        return dtype == 0 ? (float)static_cast<const uint8_t*>(img)[k] : static_cast<const float*>(img)[k];
    };
    const float re = at(y + 1, x + 1) - at(y - 1, x - 1);
    const float im = at(y + 1, x - 1) - at(y - 1, x + 1);
    const double m = sqrt((double)re * re + (double)im * im);           // np.abs; a modulus of 0 is set to 1
    ore = m == 0.0 ? re : (float)(re / m);
    oim = m == 0.0 ? im : (float)(im / m);
}

// The definition of C[i][j] of one pair (see the head of this file). Aw: the template's first value, a_pitch complex values per row; Bw: the
// search window's, b_pitch per row. Plain serial code: what tm_corr_kernel must equal bit for bit.
inline float tm_corr_element(const TmPlan& p, int T, int S, const float* Aw, long a_pitch, const float* Bw, long b_pitch, int i, int j,
                             float isign) {
    float s = 0.f;
    for (int k = 0; k < p.ks; ++k) {
        float acc = 0.f;
        for (int cy = 0; cy < T; cy += p.kt)
            for (int cx = 0; cx < T; cx += p.kx)
                for (int r = k; r < p.kt; r += p.ks)
                    for (int ch = 0; ch < 2; ++ch)
                        for (int t = 0; t < p.kx; ++t) {
                            const int ty = cy + r, tx = cx + t, sy = i + ty, sx = j + tx;
                            float a = 0.f, b = 0.f;
                            if (ty < T && tx < T) a = Aw[2 * ((long)ty * a_pitch + tx) + ch];
                            if (sy < S && sx < S) b = Bw[2 * ((long)sy * b_pitch + sx) + ch];
                            if (ch) a = isign * a;
                            acc = fmaf(a, b, acc);
                        }
        s = k ? s + acc : acc;
    }
    return s;
}

// NaN or an infinity
__device__ __forceinline__ bool tm_not_finite(float x) { return !(fabsf(x) <= 3.402823466e+38f); }

// This lane's share of a side x side window of a map (row0, col0 its first value, `pitch` complex values per map row): true when it holds
// a NaN or an infinity. The pair's outputs are NaN when any lane of the wave says so for either window.
__device__ __forceinline__ bool tm_window_not_finite(const float* __restrict__ map, long row0, long col0, long pitch, int side, int lane) {
    bool bad = false;
    for (int r = 0; r < side; ++r)
        for (int c = lane; c < side; c += TM_WAVE) {
            const float* v = map + 2 * ((row0 + r) * pitch + col0 + c);
            bad = bad || tm_not_finite(v[0]) || tm_not_finite(v[1]);
        }
    return bad;
}

// This lane's share of the n values of C: the first maximum in flat order among e = lane, lane + 64, ... and the sum of their moduli
__device__ __forceinline__ void tm_lane_scan(const float* __restrict__ Cp, int n, int lane, float& best, int& bi, double& sabs) {
    best = -INFINITY;
    bi = n;
    sabs = 0.0;
    for (int e = lane; e < n; e += TM_WAVE) {
        const float c = Cp[e];
        if (c > best || bi == n) { best = c; bi = e; }
        sabs += fabs((double)c);
    }
}

// One step of the xor butterfly: the other lane's maximum wins when it is larger, or equal at a lower flat index
__device__ __forceinline__ void tm_best_merge(float& best, int& bi, float ob, int oi) {
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
}

// The butterfly over all 64 lanes, strides 32 down to 1, as the wave performs it with __shfl_xor; lane 0 holds what tm_peak_tail takes.
// For the host build alone: the kernel's loop is its device form.
#ifndef __HIPCC__
inline void tm_wave_reduce(float* best, int* bi, double* sabs) {
    for (int o = 32; o > 0; o >>= 1) {
        float nb[TM_WAVE];
        int ni[TM_WAVE];
        double ns[TM_WAVE];
        for (int l = 0; l < TM_WAVE; ++l) {
            nb[l] = best[l];
            ni[l] = bi[l];
            tm_best_merge(nb[l], ni[l], best[l ^ o], bi[l ^ o]);
            ns[l] = sabs[l] + sabs[l ^ o];
        }
        for (int l = 0; l < TM_WAVE; ++l) { best[l] = nb[l]; bi[l] = ni[l]; sabs[l] = ns[l]; }
    }
}
#endif

__device__ __forceinline__ int tm_min(int a, int b) { return a < b ? a : b; }

// numpy's pairwise summation of n <= 128 values (`pairwise_sum` of umath loops), started from the reduction identity 0. Contraction is off
// here and in tm_peak_tail: numpy rounds every product before it adds it. The products of the centroid are exact in float64 (a coordinate
// of a few bits times a float32 weight), so fusing them into the sums would give the same bits today; the pragma keeps the order of
// roundings from depending on that.
template <typename T, typename F>
__device__ T np_sum_small(int n, F get) {
#pragma clang fp contract(off)
    if (n < 8) {
        T r = 0;
        for (int i = 0; i < n; ++i) r += get(i);
        return (T)0 + r;
    }
    T r[8];
    for (int j = 0; j < 8; ++j) r[j] = get(j);
    int i = 8;
    for (; i < n - n % 8; i += 8)
        for (int j = 0; j < 8; ++j) r[j] += get(i + j);
    T res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += get(i);
    return (T)0 + res;
}

// What lane 0 does with the wave's maximum (`templatematch.py:303-329`): out[0..3] = du, dv, peakCorr, meanAbsCorr of a pair whose C is Cp
// (R x R), whose first maximum `best` lies at flat index bi and whose moduli sum to sabs.
__device__ __forceinline__ void tm_peak_tail(const float* __restrict__ Cp, int R, int bi, float best, double sabs, double initdu, double initdv,
                                             double* out) {
#pragma clang fp contract(off)
    const int n = R * R;
    out[0] = out[1] = out[2] = NAN;
    out[3] = (double)(float)(sabs / n);       // np.mean of a float32 array is a float32
    const int mi = bi / R, mj = bi - mi * R;
    const int edge = tm_min(tm_min(mi, mj), tm_min(R - 1 - mi, R - 1 - mj));
    if (edge == 0) return;                    // a peak on the border of C is not trusted
    const int ww = tm_min(edge, 4), side = 2 * ww + 1, m = side * side;
    auto cw = [&](int e) { return Cp[(mi - ww + e / side) * R + mj - ww + e % side]; };
    const float mean_abs = np_sum_small<float>(m, [&](int e) { return fabsf(cw(e)); }) / (float)m;
    auto cpos = [&](int e) { const float c = cw(e) - mean_abs; return c < 0.f ? 0.f : c; };
    const float tot = np_sum_small<float>(m, cpos);
    const double wkeep = R / 2.0;             // C_uu = C_vv = arange(-wkeep, wkeep + 1)
    const double cv = np_sum_small<double>(m, [&](int e) { return (-wkeep + (mi - ww + e / side)) * (double)(cpos(e) / tot); });
    const double cu = np_sum_small<double>(m, [&](int e) { return (-wkeep + (mj - ww + e % side)) * (double)(cpos(e) / tot); });
    out[0] = cu + initdu;
    out[1] = cv + initdv;
    out[2] = (double)best;
}

}  // namespace
}  // namespace im
