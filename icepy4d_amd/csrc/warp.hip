// Image stabilisation on 8-bit images, on the device: what the reference's driver calls through OpenCV for every epoch of the camera it
// warps (`cv2.undistort` in `sfm/geometry.py::undistort_image`, `cv2.warpPerspective` in `utils/homography.py::homography_warping`).
// OpenCV is an un-vendored dependency; the kernels restate its documented 8-bit INTER_LINEAR path with BORDER_CONSTANT 0 (parity with a
// particular OpenCV build is unpinned; pinned is bit identity with tests/warp_oracle.py): per output pixel a source coordinate in
// float64 (warp_pixel.h, contraction off), rounded to 1/32 pixel, four taps with integer weights that sum to 32768, (sum + 16384) >> 15.
// Byte traffic plus a few dozen float64 operations per pixel: one thread per output pixel, the 1..4 interleaved channels in a loop,
// consecutive lanes on consecutive pixels of an output row, no LDS: for the near-affine maps of this workload the taps of a wave fall into
// a few cache lines of two source rows. What bounds the launch is the number of tap reads, not the float64 chain and not the byte stores
// (profiles/r11_stabilise_ablations.txt): a pixel whose four taps are inside reads each row's two taps in one piece (warp_pixel.h).
#include "ctx.h"
#include "warp_pixel.h"

namespace im {

// minv [n_images][9]: inv3(H) of every image, row-major
template <int C>
__global__ __launch_bounds__(256) void warp_perspective_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                               const double* __restrict__ minv, int h, int w, int oh, int ow) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= ow) return;
    double sx, sy;
    warp_coords(minv + 9 * b, x, y, sx, sy);
    uint8_t px[C];
    remap_pixel<C>(src + (long)b * h * w * C, h, w, sx, sy, px);
    uint8_t* o = dst + (((long)b * oh + y) * ow + x) * C;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) o[ch] = px[ch];
}

template <int C>
__global__ __launch_bounds__(256) void undistort_image_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, UndistortCam cam, int h,
                                                              int w) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= w) return;
    double sx, sy;
    undistort_coords(cam, y, x, sx, sy);
    uint8_t px[C];
    remap_pixel<C>(src + (long)b * h * w * C, h, w, sx, sy, px);
    uint8_t* o = dst + (((long)b * h + y) * w + x) * C;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) o[ch] = px[ch];
}

// what both entry points refuse; nullptr when the arguments are fine
static const char* bad_images(const void* d_src, const void* d_dst, int n_images, int h, int w, int channels, int oh, int ow) {
    if (!d_src || !d_dst) return "null image pointer";
    if (channels < 1 || channels > 4) return "channels must be 1..4";
    if (h < 1 || h > 32766 || w < 1 || w > 32766 || oh < 1 || oh > 32766 || ow < 1 || ow > 32766) return "image sides must be 1..32766";
    if (n_images < 1 || n_images > 65535) return "n_images must be 1..65535";
    const uintptr_t s0 = (uintptr_t)d_src, s1 = s0 + (size_t)n_images * h * w * channels;
    const uintptr_t t0 = (uintptr_t)d_dst, t1 = t0 + (size_t)n_images * oh * ow * channels;
    if (s0 < t1 && t0 < s1) return "source and destination overlap";
    return nullptr;
}

// the instantiation for `channels` (1..4, checked by bad_images) out of the four: the one place that switches on the channel count
template <typename K> K by_channels(int channels, K k1, K k2, K k3, K k4) { return channels == 1 ? k1 : channels == 2 ? k2 : channels == 3 ? k3 : k4; }

}  // namespace im

using namespace im;

extern "C" {

int im_undistort_image(im_ctx* ctx, const uint8_t* d_src, int n_images, int h, int w, int channels, const double* h_cam, uint8_t* d_dst,
                       void* stream) {
    IM_CHECK_CTX(ctx);
    if (!h_cam) return ctx->fail(-74, "im_undistort_image: null camera");
    if (const char* why = bad_images(d_src, d_dst, n_images, h, w, channels, h, w)) return ctx->fail(-74, "im_undistort_image: %s", why);
    UndistortCam cam;
    for (int i = 0; i < 9; ++i) cam.ir[i] = h_cam[i];
    for (int i = 0; i < 4; ++i) cam.in[i] = h_cam[9 + i];
    for (int i = 0; i < 8; ++i) cam.k[i] = h_cam[13 + i];
    const dim3 grid((unsigned)blocks_of(w, 256), h, n_images);
    hipStream_t s = (hipStream_t)stream;
    const auto kernel = by_channels(channels, undistort_image_kernel<1>, undistort_image_kernel<2>, undistort_image_kernel<3>, undistort_image_kernel<4>);
    IM_LAUNCH(ctx, "undistort_image", s, launch(kernel, grid, 256, 0, s, d_src, d_dst, cam, h, w));
    IM_GUARD_CHECK(ctx, s, "im_undistort_image");
    return 0;
}

int im_warp_perspective(im_ctx* ctx, const uint8_t* d_src, int n_images, int h, int w, int channels, const double* d_minv, int oh, int ow,
                        uint8_t* d_dst, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_minv) return ctx->fail(-74, "im_warp_perspective: null matrices");
    if (const char* why = bad_images(d_src, d_dst, n_images, h, w, channels, oh, ow)) return ctx->fail(-74, "im_warp_perspective: %s", why);
    const dim3 grid((unsigned)blocks_of(ow, 256), oh, n_images);
    hipStream_t s = (hipStream_t)stream;
    const auto kernel = by_channels(channels, warp_perspective_kernel<1>, warp_perspective_kernel<2>, warp_perspective_kernel<3>, warp_perspective_kernel<4>);
    IM_LAUNCH(ctx, "warp_perspective", s, launch(kernel, grid, 256, 0, s, d_src, d_dst, d_minv, h, w, oh, ow));
    IM_GUARD_CHECK(ctx, s, "im_warp_perspective");
    return 0;
}

}  // extern "C"
