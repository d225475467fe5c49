// Host build of the per-pixel arithmetic of csrc/warp.hip (csrc/warp_pixel.h) for tests/test_stabilise_cpu.py: the very text the kernels
// compile, as flat loops over the output pixels. Compiled with a stub <hip/hip_runtime.h> that defines __device__ and __forceinline__
// away; no arithmetic is written here.
#include <hip/hip_runtime.h>

#include "warp_pixel.h"

namespace {

template <int C>
void warp_host(const uint8_t* src, int n, int h, int w, const double* minv, int oh, int ow, uint8_t* dst) {
    for (int b = 0; b < n; ++b)
        for (int y = 0; y < oh; ++y)
            for (int x = 0; x < ow; ++x) {
                double sx, sy;
                im::warp_coords(minv + 9 * b, x, y, sx, sy);
                im::remap_pixel<C>(src + (long)b * h * w * C, h, w, sx, sy, dst + (((long)b * oh + y) * ow + x) * C);
            }
}

template <int C>
void undistort_host(const uint8_t* src, int n, int h, int w, const im::UndistortCam& cam, uint8_t* dst) {
    for (int b = 0; b < n; ++b)
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                double sx, sy;
                im::undistort_coords(cam, y, x, sx, sy);
                im::remap_pixel<C>(src + (long)b * h * w * C, h, w, sx, sy, dst + (((long)b * h + y) * w + x) * C);
            }
}

}  // namespace

// the arguments of im_warp_perspective, everything in host memory
extern "C" void warp_host_perspective(const uint8_t* src, int n, int h, int w, int c, const double* minv, int oh, int ow, uint8_t* dst) {
    switch (c) {
        case 1: warp_host<1>(src, n, h, w, minv, oh, ow, dst); break;
        case 2: warp_host<2>(src, n, h, w, minv, oh, ow, dst); break;
        case 3: warp_host<3>(src, n, h, w, minv, oh, ow, dst); break;
        default: warp_host<4>(src, n, h, w, minv, oh, ow, dst); break;
    }
}

// the arguments of im_undistort_image: cam = 9 ir, fx fy cx cy, 8 coefficients
extern "C" void warp_host_undistort(const uint8_t* src, int n, int h, int w, int c, const double* cam, uint8_t* dst) {
    im::UndistortCam u;
    for (int i = 0; i < 9; ++i) u.ir[i] = cam[i];
    for (int i = 0; i < 4; ++i) u.in[i] = cam[9 + i];
    for (int i = 0; i < 8; ++i) u.k[i] = cam[13 + i];
    switch (c) {
        case 1: undistort_host<1>(src, n, h, w, u, dst); break;
        case 2: undistort_host<2>(src, n, h, w, u, dst); break;
        case 3: undistort_host<3>(src, n, h, w, u, dst); break;
        default: undistort_host<4>(src, n, h, w, u, dst); break;
    }
}
