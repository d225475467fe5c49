// Reconstruction of matched points (`src/icepy4d/sfm/triangulation.py`: `Triangulate.triangulate_two_views`; `sfm/geometry.py`:
// `undistort_points`; `thirdparty/triangulation.py`: `iterative_LS_triangulation`, `linear_LS_triangulation`). The reference undistorts
// with cv2.undistortPoints and triangulates one point at a time in a Python loop with up to ten `cv2.solve(DECOMP_SVD)` calls per point.
// Here both are device kernels, one thread per point, float64, contraction off (tests/sfm_oracle.py restates them operation by operation):
//
//   undistort_points_kernel        cv2.undistortPoints(pts, K, dist, None, K) with the default criteria: five fixed-point iterations of the
//                                  Brown / rational model, OpenCV's icdist < 0 guard, float32 out
//   triangulate_iterative_kernel   n matched point pairs and ONE camera pair; optionally the undistortion fused in front (the float32
//                                  rounding of the undistorted points is kept, so the result equals the two calls in sequence)
//   table_offsets_kernel           one block: exclusive scan of max(n_matches, 0) over the records of a gathered match table
//   triangulate_table_kernel       one block per record of the table (`sequence.py`, int32 [8 + 6K] with the keypoint payload): the
//                                  matched keypoint-0 indices are compacted in ascending order into LDS (the reference's
//                                  `kpts0[matches0 > -1]` order), then the block's threads take the matched pairs densely
//
// The recurrence of the iterative triangulation (Hartley & Sturm 1997 as written in `thirdparty/triangulation.py:79-177`), kept with its
// three quirks: the re-weighting is cumulative (the rows already scaled by 1 / d are scaled again), the convergence test is absolute
// (|d_new - d| <= tolerance on both depths, d = 1 at the start, ten solves at most), and the status is
//   (d1 > 0 and d2 > 0) - (d1 <= 0) - 2 (d2 <= 0)   in {1, -1, -2, -3}
// because the loop index never reaches 10: the documented 0 ("outlier, but in front of both cameras") cannot occur for finite depths
// (a NaN depth fails all four comparisons and gives 0). max_solves = 1 is `linear_LS_triangulation`: one solve, status 1.
#include <climits>
#include <cmath>

#include "ctx.h"
#include "sfm_point.h"

namespace im {
namespace {

constexpr int SFM_THREADS = 256;
constexpr int SFM_MAX_K = 16384;         // 64 KB of LDS for the compacted indices of one record

// image points of one pair -> (undistorted points,) point and status at row `o` of the outputs
__device__ __forceinline__ void reconstruct_one(float a0, float a1, float b0, float b1, const CamPair& c, int undistort, double tol,
                                                int max_solves, long long o, double* __restrict__ X, int* __restrict__ status,
                                                float* __restrict__ und1, float* __restrict__ und2) {
    double u1x = a0, u1y = a1, u2x = b0, u2y = b1;
    if (undistort) {
        undistort_one(u1x, u1y, c.c[0], a0, a1);
        undistort_one(u2x, u2y, c.c[1], b0, b1);
        u1x = a0; u1y = a1; u2x = b0; u2y = b1;      // through float32, as the reference's `undistort_points` returns them
    }
    if (und1) { und1[2 * o] = a0; und1[2 * o + 1] = a1; }
    if (und2) { und2[2 * o] = b0; und2[2 * o + 1] = b1; }
    double x[3];
    const int st = triangulate_one(u1x, u1y, u2x, u2y, c.c[0].P, c.c[1].P, tol, max_solves, x);
    X[3 * o] = x[0]; X[3 * o + 1] = x[1]; X[3 * o + 2] = x[2];
    status[o] = st;
}

__global__ __launch_bounds__(SFM_THREADS) void undistort_points_kernel(const float* __restrict__ pts, long long n, CamParam c,
                                                                       float* __restrict__ out) {
    const long long i = blockIdx.x * (long long)SFM_THREADS + threadIdx.x;
    if (i >= n) return;
    float u, v;
    undistort_one((double)pts[2 * i], (double)pts[2 * i + 1], c, u, v);
    out[2 * i] = u;
    out[2 * i + 1] = v;
}

// T = float: image points as the matcher and `undistort_points` give them; T = double: points handed over in float64 (never undistorted here)
template <typename T>
__global__ __launch_bounds__(SFM_THREADS) void triangulate_iterative_kernel(const T* __restrict__ u1, const T* __restrict__ u2, long long n,
                                                                            CamPair c, int undistort, double tol, int max_solves,
                                                                            double* __restrict__ X, int* __restrict__ status,
                                                                            float* __restrict__ und1, float* __restrict__ und2) {
    const long long i = blockIdx.x * (long long)SFM_THREADS + threadIdx.x;
    if (i >= n) return;
    if constexpr (sizeof(T) == sizeof(float)) {
        reconstruct_one(u1[2 * i], u1[2 * i + 1], u2[2 * i], u2[2 * i + 1], c, undistort, tol, max_solves, i, X, status, und1, und2);
    } else {
        double x[3];
        const int st = triangulate_one(u1[2 * i], u1[2 * i + 1], u2[2 * i], u2[2 * i + 1], c.c[0].P, c.c[1].P, tol, max_solves, x);
        X[3 * i] = x[0]; X[3 * i + 1] = x[1]; X[3 * i + 2] = x[2];
        status[i] = st;
    }
}

// offsets[e] = sum over e' < e of max(n_matches[e'], 0); offsets[E] = the number of points. One block.
__global__ __launch_bounds__(SFM_THREADS) void table_offsets_kernel(const int* __restrict__ table, int E, long long W,
                                                                    long long* __restrict__ offsets) {
    __shared__ long long buf[SFM_THREADS];
    long long running = 0;
    for (int base = 0; base < E; base += SFM_THREADS) {
        const int e = base + (int)threadIdx.x;
        const long long v = e < E ? (long long)max(table[e * W + 3], 0) : 0;
        buf[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < SFM_THREADS; o <<= 1) {
            const long long add = (int)threadIdx.x >= o ? buf[threadIdx.x - o] : 0;
            __syncthreads();
            buf[threadIdx.x] += add;
            __syncthreads();
        }
        if (e < E) offsets[e] = running + buf[threadIdx.x] - v;
        running += buf[SFM_THREADS - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) offsets[E] = running;
}

// Record e: words [3] n_matches, [8 : 8 + K] matches0, [8 + 2K : 8 + 4K] keypoints0, [8 + 4K : 8 + 6K] keypoints1 (float32 bit patterns).
// Rows offsets[e] .. offsets[e] + n_matches - 1 of the outputs. A record whose matches0 holds fewer valid entries (0 <= m < K) than its
// header promises leaves the remaining rows NaN with status 0; surplus entries and rows >= m_cap are dropped: no write leaves the outputs.
__global__ __launch_bounds__(SFM_THREADS) void triangulate_table_kernel(const int* __restrict__ table, int K, const CamPair* __restrict__ cams,
                                                                        int n_cams, int undistort, double tol, int max_solves, long long m_cap,
                                                                        const long long* __restrict__ offsets, double* __restrict__ X,
                                                                        int* __restrict__ status, float* __restrict__ und1,
                                                                        float* __restrict__ und2) {
    extern __shared__ int matched[];             // [K] keypoint-0 indices with a match, ascending
    __shared__ int wave_cnt[SFM_THREADS / 64];
    const int e = blockIdx.x;
    const int* __restrict__ rec = table + (long long)e * (8 + 6LL * K);
    const int n_m = max(rec[3], 0);
    if (n_m == 0) return;                        // block-uniform
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int running = 0;
    for (int base = 0; base < K; base += SFM_THREADS) {
        const int i = base + (int)threadIdx.x;
        const int m = i < K ? rec[8 + i] : -1;
        const bool valid = m >= 0 && m < K;
        const unsigned long long bal = __ballot(valid);
        if (lane == 0) wave_cnt[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < SFM_THREADS / 64; ++w) {
            before += w < wave ? wave_cnt[w] : 0;
            total += wave_cnt[w];
        }
        if (valid) matched[running + before + __popcll(bal & ((1ull << lane) - 1ull))] = i;
        running += total;
        __syncthreads();
    }
    const CamPair& c = cams[n_cams == 1 ? 0 : e];   // by reference: 96 SGPRs of parameters are fetched where they are used
    const long long first = offsets[e];
    const int have = min(running, n_m);
    for (int r = threadIdx.x; r < have; r += SFM_THREADS) {
        const long long o = first + r;
        if (o >= m_cap) break;
        const int i = matched[r], m = rec[8 + i];
        const int* k0 = rec + 8 + 2LL * K + 2 * i;
        const int* k1 = rec + 8 + 4LL * K + 2 * m;
        reconstruct_one(__int_as_float(k0[0]), __int_as_float(k0[1]), __int_as_float(k1[0]), __int_as_float(k1[1]), c, undistort, tol,
                        max_solves, o, X, status, und1, und2);
    }
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int r = have + (int)threadIdx.x; r < n_m; r += SFM_THREADS) {
        const long long o = first + r;
        if (o >= m_cap) break;
        X[3 * o] = X[3 * o + 1] = X[3 * o + 2] = nan;
        status[o] = 0;
        if (und1) und1[2 * o] = und1[2 * o + 1] = (float)nan;
        if (und2) und2[2 * o] = und2[2 * o + 1] = (float)nan;
    }
}

void fill_cam(CamParam& c, const double* h_P, const double* h_cam) {
    for (int j = 0; j < 12; ++j) c.P[j] = h_P ? h_P[j] : 0.0;
    for (int j = 0; j < 4; ++j) c.in[j] = h_cam ? h_cam[j] : 1.0;
    for (int j = 0; j < 8; ++j) c.k[j] = h_cam ? h_cam[4 + j] : 0.0;
}

bool focal_ok(const double* h_cam) { return std::isfinite(h_cam[0]) && std::isfinite(h_cam[1]) && h_cam[0] != 0.0 && h_cam[1] != 0.0; }

}  // namespace
}  // namespace im

using namespace im;

extern "C" int im_undistort_points(im_ctx* ctx, const float* d_pts, long long n, const double* h_cam, float* d_out, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!h_cam || n < 0 || n >= INT_MAX) return ctx->fail(-73, "im_undistort_points: bad arguments");
    if (!focal_ok(h_cam)) return ctx->fail(-73, "im_undistort_points: the focal lengths must be finite and non-zero");
    if (!n) return 0;
    if (!d_pts || !d_out) return ctx->fail(-73, "im_undistort_points: null argument");
    CamParam c;
    fill_cam(c, nullptr, h_cam);
    hipStream_t s = (hipStream_t)stream;
    IM_LAUNCH(ctx, "undistort_points", s, launch(undistort_points_kernel, blocks_of(n, SFM_THREADS), SFM_THREADS, 0, s, d_pts, n, c, d_out));
    IM_GUARD_CHECK(ctx, s, "im_undistort_points");
    return 0;
}

extern "C" int im_triangulate_iterative(im_ctx* ctx, const void* d_u1, const void* d_u2, int f64, long long n, const double* h_P1,
                                        const double* h_P2, const double* h_cam1, const double* h_cam2, double tolerance, int max_solves,
                                        double* d_X, int32_t* d_status, float* d_und1, float* d_und2, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!h_P1 || !h_P2 || n < 0 || n >= INT_MAX) return ctx->fail(-73, "im_triangulate_iterative: bad arguments");
    if (max_solves < 1 || max_solves > 10 || !(tolerance >= 0.0))
        return ctx->fail(-73, "im_triangulate_iterative: 1 <= max_solves <= 10 and tolerance >= 0 (got %d, %g)", max_solves, tolerance);
    const bool undistort = h_cam1 || h_cam2;
    if (undistort && (!h_cam1 || !h_cam2 || f64)) return ctx->fail(-73, "im_triangulate_iterative: the fused undistortion takes two cameras and float32 points");
    if (undistort && (!focal_ok(h_cam1) || !focal_ok(h_cam2))) return ctx->fail(-73, "im_triangulate_iterative: the focal lengths must be finite and non-zero");
    if (f64 && (d_und1 || d_und2)) return ctx->fail(-73, "im_triangulate_iterative: float64 points have no float32 copy to return");
    if (!n) return 0;
    if (!d_u1 || !d_u2 || !d_X || !d_status) return ctx->fail(-73, "im_triangulate_iterative: null argument");
    CamPair c;
    fill_cam(c.c[0], h_P1, h_cam1);
    fill_cam(c.c[1], h_P2, h_cam2);
    hipStream_t s = (hipStream_t)stream;
    if (f64) {
        IM_LAUNCH(ctx, "triangulate_iterative", s, launch(triangulate_iterative_kernel<double>, blocks_of(n, SFM_THREADS), SFM_THREADS, 0, s, (const double*)d_u1,
                                                          (const double*)d_u2, n, c, 0, tolerance, max_solves, d_X, d_status,
                                                          (float*)nullptr, (float*)nullptr));
    } else {
        IM_LAUNCH(ctx, "triangulate_iterative", s, launch(triangulate_iterative_kernel<float>, blocks_of(n, SFM_THREADS), SFM_THREADS, 0, s, (const float*)d_u1,
                                                          (const float*)d_u2, n, c, undistort ? 1 : 0, tolerance, max_solves, d_X, d_status,
                                                          d_und1, d_und2));
    }
    IM_GUARD_CHECK(ctx, s, "im_triangulate_iterative");
    return 0;
}

extern "C" int im_triangulate_table(im_ctx* ctx, const int32_t* d_table, int n_records, int max_kpts, const double* d_cams, int n_cams,
                                    int undistort, double tolerance, int max_solves, long long m_cap, long long* d_offsets, double* d_X,
                                    int32_t* d_status, float* d_und0, float* d_und1, void* stream) {
    IM_CHECK_CTX(ctx);
    if (n_records < 0 || max_kpts < 1 || max_kpts > SFM_MAX_K || m_cap < 0 || m_cap >= INT_MAX || !d_offsets)
        return ctx->fail(-73, "im_triangulate_table: bad arguments (1 <= max_kpts <= %d)", SFM_MAX_K);
    if (n_cams != 1 && n_cams != n_records) return ctx->fail(-73, "im_triangulate_table: one camera pair, or one per record (got %d for %d)", n_cams, n_records);
    if (max_solves < 1 || max_solves > 10 || !(tolerance >= 0.0))
        return ctx->fail(-73, "im_triangulate_table: 1 <= max_solves <= 10 and tolerance >= 0 (got %d, %g)", max_solves, tolerance);
    if (n_records && (!d_table || !d_cams)) return ctx->fail(-73, "im_triangulate_table: null argument");
    if (m_cap && (!d_X || !d_status)) return ctx->fail(-73, "im_triangulate_table: null output");
    hipStream_t s = (hipStream_t)stream;
    const long long W = 8 + 6LL * max_kpts;
    IM_LAUNCH(ctx, "table_offsets", s, launch(table_offsets_kernel, 1, SFM_THREADS, 0, s, d_table, n_records, W, d_offsets));
    if (n_records && m_cap) {
        // K ints of dynamic LDS next to the 16 static bytes of wave_cnt: above 64 KB from K = 16381 on, hence the opt-in (kernels.h)
        IM_LAUNCH(ctx, "triangulate_table", s, launch_dyn_lds<triangulate_table_kernel>(
                                                   dim3((unsigned)n_records), dim3(SFM_THREADS), sizeof(int) * (size_t)max_kpts, s, d_table, max_kpts,
                                                   reinterpret_cast<const CamPair*>(d_cams), n_cams, undistort ? 1 : 0, tolerance, max_solves,
                                                   m_cap, (const long long*)d_offsets, d_X, d_status, d_und0, d_und1));
    }
    IM_GUARD_CHECK(ctx, s, "im_triangulate_table");
    return 0;
}
