// The arithmetic of one output pixel of csrc/warp.hip: the source coordinate of a perspective warp and of an undistortion, its rounding to
// 1/32 pixel and the four-tap sum of OpenCV's documented 8-bit INTER_LINEAR path with BORDER_CONSTANT 0 (`cv2.warpPerspective`,
// `cv2.undistort`), restated: a few IEEE float64 operations with contraction off, integers behind the rounding. A header of its own,
// without the context or any launch code, like sfm_point.h: a host program compiles the very text the kernels compile
// (tests/warp_host_harness.cpp, through a stub <hip/hip_runtime.h>) and is compared with the numpy restatement (tests/warp_oracle.py)
// bit for bit. The matrices arrive inverted (`inv3` on the host); nothing here inverts.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace im {
namespace {

// one camera of an undistortion: inv3(K) row-major, fx fy cx cy, k1 k2 p1 p2 k3 k4 k5 k6
struct UndistortCam { double ir[9]; double in[4]; double k[8]; };
static_assert(sizeof(UndistortCam) == 21 * sizeof(double), "h_cam of im_undistort_image is 21 doubles");

// v = a source coordinate times 32. false: not finite, the pixel lies outside. Otherwise the integer pixel (saturated to a short) and the
// 5-bit fraction of the coordinate rounded to 1/32 pixel, ties to even.
__device__ __forceinline__ bool fix_coord(double v, int& xi, int& f) {
#pragma clang fp contract(off)
    if (!(fabs(v) <= 1.7976931348623157e308)) return false;      // NaN and both infinities
    const double c = v < -2147483648.0 ? -2147483648.0 : (v > 2147483647.0 ? 2147483647.0 : v);
    const int X = (int)rint(c);
    const int q = X >> 5;                                         // arithmetic
    xi = q < -32768 ? -32768 : (q > 32767 ? 32767 : q);
    f = X & 31;
    return true;
}

// cv2.warpPerspective's coordinates of output pixel (x, y) times 32, M = inv3(H) row-major. xb is the start of OpenCV's 64-pixel block:
// the block's X0, Y0, W0 are formed first and the offset inside the block is added afterwards, which fixes the rounding.
__device__ __forceinline__ void warp_coords(const double* M, int x, int y, double& sx, double& sy) {
#pragma clang fp contract(off)
    const int xb = 64 * (x / 64), x1 = x - xb;
    const double X0 = (M[0] * xb + M[1] * y) + M[2];
    const double Y0 = (M[3] * xb + M[4] * y) + M[5];
    const double W0 = (M[6] * xb + M[7] * y) + M[8];
    const double W = W0 + M[6] * x1;
    const double Wi = W != 0.0 ? 32.0 / W : 0.0;
    sx = (X0 + M[0] * x1) * Wi;
    sy = (Y0 + M[3] * x1) * Wi;
}

// cv2.undistort(src, K, dist, None, K)'s coordinates of output pixel (row i, column j) times 32
__device__ __forceinline__ void undistort_coords(const UndistortCam& c, int i, int j, double& sx, double& sy) {
#pragma clang fp contract(off)
    const double* ir = c.ir;
    const double fx = c.in[0], fy = c.in[1], cx = c.in[2], cy = c.in[3];
    const double k1 = c.k[0], k2 = c.k[1], p1 = c.k[2], p2 = c.k[3], k3 = c.k[4], k4 = c.k[5], k5 = c.k[6], k6 = c.k[7];
    const double _x = j * ir[0] + (i * ir[1] + ir[2]);
    const double _y = j * ir[3] + (i * ir[4] + ir[5]);
    const double _w = j * ir[6] + (i * ir[7] + ir[8]);
    const double iw = 1.0 / _w;
    const double x = _x * iw, y = _y * iw;
    const double x2 = x * x, y2 = y * y;
    const double r2 = x2 + y2, _2xy = 2.0 * x * y;
    const double kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2);
    const double xd = (x * kr + p1 * _2xy) + p2 * (r2 + 2.0 * x2);
    const double yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * _2xy;
    const double u = fx * xd + cx;
    const double v = fy * yd + cy;
    sx = u * 32.0;
    sy = v * 32.0;
}

// the four-tap sum: int32 weights that add up to 32768
__device__ __forceinline__ uint8_t tap_sum(int p00, int p01, int p10, int p11, int fx, int fy) {
#pragma clang fp contract(off)
    const int w00 = 32 * (32 - fx) * (32 - fy), w01 = 32 * fx * (32 - fy), w10 = 32 * (32 - fx) * fy, w11 = 32 * fx * fy;
    return (uint8_t)((w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + 16384) >> 15);
}

// one output pixel of C interleaved channels from img [h][w][C] at the coordinates (sx, sy) (times 32); a tap outside the image is 0
template <int C>
__device__ __forceinline__ void remap_pixel(const uint8_t* img, int h, int w, double sx, double sy, uint8_t* out) {
#pragma clang fp contract(off)
    int xi = 0, yi = 0, fx = 0, fy = 0;
    const bool fin_x = fix_coord(sx, xi, fx), fin_y = fix_coord(sy, yi, fy);
    const bool ok = fin_x && fin_y;
    const bool x0 = ok && xi >= 0 && xi < w, x1 = ok && xi + 1 >= 0 && xi + 1 < w;
    const bool y0 = yi >= 0 && yi < h, y1 = yi + 1 >= 0 && yi + 1 < h;
    const long o0 = ((long)yi * w + xi) * C, o1 = o0 + (long)w * C;      // read only where the tap is inside
    if (x0 && x1 && y0 && y1) {
        // all four taps inside: the two taps of a row are 2 C adjacent bytes, read in one piece at any alignment (byte loads issue per
        // lane and byte, and twelve of them per pixel were what bounded the launch)
        uint8_t r0[2 * C], r1[2 * C];
        __builtin_memcpy(r0, img + o0, 2 * C);
        __builtin_memcpy(r1, img + o1, 2 * C);
#pragma unroll
        for (int ch = 0; ch < C; ++ch) out[ch] = tap_sum(r0[ch], r0[C + ch], r1[ch], r1[C + ch], fx, fy);
        return;
    }
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        const int p00 = x0 && y0 ? (int)img[o0 + ch] : 0, p01 = x1 && y0 ? (int)img[o0 + C + ch] : 0;
        const int p10 = x0 && y1 ? (int)img[o1 + ch] : 0, p11 = x1 && y1 ? (int)img[o1 + C + ch] : 0;
        out[ch] = tap_sum(p00, p01, p10, p11, fx, fy);
    }
}

}  // namespace
}  // namespace im
