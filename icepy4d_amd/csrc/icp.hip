// Co-registration of two clouds on the device: the rigid transform of a cloud and, per ICP iteration, the normal equations of the
// correspondences im_knn_cross found (k = 1, radius2 = d_max^2, on the transformed source), their solve and the next transform (Besl &
// McKay 1992; Chen & Medioni 1992; Open3D's registration_icp, CloudCompare's fine registration). Neither tool is a dependency: every
// quantity has a definition of its own (icp_point.h) and is pinned bit for bit against tests/icp_oracle.py. Parity with a
// binary of either is unpinned.
//
//   transform_points_kernel   one thread per point: icp_apply with the matrix read from device memory, in place allowed
//   icp_accumulate_kernel     one block of 256 threads per chunk of ICP_CHUNK source points: each thread adds its points' rows to 30 sums
//                             in registers (icp_point gathers q and n by index), the wave butterfly, the four waves through 1 KiB of LDS,
//                             one partial of 32 doubles per chunk
//   icp_finish_kernel         one block: the partials summed by the same scheme, then thread 0 solves, composes M_next and writes the record
// The order of every sum is fixed by the source index alone (icp_point.h). No atomics; the matrix never leaves the device between iterations.
#include "common.h"
#include "ctx.h"
#include "stage_scratch.h"
#include "icp_point.h"

namespace im {
namespace {

constexpr int ICP_REFUSED = -81;
constexpr long long ICP_MAX_POINTS = 1LL << 26;
constexpr int ICP_WAVES = ICP_BLOCK / IM_WAVE;

static_assert(ICP_PART == ICP_TERMS, "the scratch holds one partial of ICP_TERMS doubles per chunk");
static_assert(ICP_WAVES == 4 && ICP_CHUNK % ICP_BLOCK == 0, "icp_join_waves joins four waves; a chunk is whole rounds of the block");

__global__ __launch_bounds__(256) void transform_points_kernel(const double* __restrict__ M, const double* in, double* out, long long n, int as_vectors) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= n) return;
    double m[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = M[k];
    double p[3];
    icp_apply(m, in[3 * i], in[3 * i + 1], in[3 * i + 2], as_vectors != 0, p);
    out[3 * i] = p[0]; out[3 * i + 1] = p[1]; out[3 * i + 2] = p[2];
}

// The sums of the block's 256 threads, term by term: the butterfly inside each wave, then the four waves. Threads 0..31 return the block's
// sum of term threadIdx.x; what the others return is meaningless. sh: ICP_WAVES * ICP_TERMS doubles.
__device__ __forceinline__ double icp_block_sum(double (&S)[ICP_TERMS], double* sh) {
#pragma clang fp contract(off)
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < ICP_SUMS; ++k)
#pragma unroll
        for (int o = 1; o < IM_WAVE; o <<= 1) S[k] = S[k] + __shfl_xor(S[k], o);
    if ((t & (IM_WAVE - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < ICP_TERMS; ++k) sh[(t / IM_WAVE) * ICP_TERMS + k] = S[k];
    }
    __syncthreads();
    const int k = t & (ICP_TERMS - 1);
    return icp_join_waves(sh[k], sh[ICP_TERMS + k], sh[2 * ICP_TERMS + k], sh[3 * ICP_TERMS + k]);
}

struct IcpAccArgs {
    const double* src; const double* tgt; const double* nrm; const int* idx; const double* d2;
    long long n, n_tgt;
    double c[3];
    int method;
    double* parts;
};

__global__ __launch_bounds__(ICP_BLOCK) void icp_accumulate_kernel(IcpAccArgs a) {
    __shared__ double sh[ICP_WAVES * ICP_TERMS];
    const long long first = (long long)blockIdx.x * ICP_CHUNK;
    const long long end = min(first + ICP_CHUNK, a.n);
    const double c[3] = {a.c[0], a.c[1], a.c[2]};
    double S[ICP_TERMS];
    icp_zero(S);
    for (long long i = first + threadIdx.x; i < end; i += ICP_BLOCK)
        icp_point(S, a.src[3 * i], a.src[3 * i + 1], a.src[3 * i + 2], a.tgt, a.nrm, a.n_tgt, a.idx[i], a.d2[i], c, a.method);
    const double v = icp_block_sum(S, sh);
    if (threadIdx.x < ICP_TERMS) a.parts[(long long)blockIdx.x * ICP_TERMS + threadIdx.x] = v;
}

struct IcpFinishArgs {
    const double* parts; const double* M;
    long long n, n_chunks;
    double c[3];
    int solve;
    double* rec;
};

__global__ __launch_bounds__(ICP_BLOCK) void icp_finish_kernel(IcpFinishArgs a) {
    __shared__ double sh[ICP_WAVES * ICP_TERMS];
    __shared__ double tot[ICP_TERMS];
    double S[ICP_TERMS];
    icp_zero(S);
    for (long long ch = threadIdx.x; ch < a.n_chunks; ch += ICP_BLOCK) {
#pragma unroll
        for (int k = 0; k < ICP_SUMS; ++k) S[k] = S[k] + a.parts[ch * ICP_TERMS + k];
    }
    const double v = icp_block_sum(S, sh);
    if (threadIdx.x < ICP_TERMS) tot[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double c[3] = {a.c[0], a.c[1], a.c[2]};
        double T[ICP_TERMS];
#pragma unroll
        for (int k = 0; k < ICP_TERMS; ++k) T[k] = tot[k];
        icp_finish(T, a.M, c, a.n, a.solve != 0, a.rec);
    }
}

const char* bad_centre(const double* h_centre) {
    if (!h_centre) return "null pointer";
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(h_centre[a])) return "the centre must be finite";
    return nullptr;
}

}  // namespace
}  // namespace im

using namespace im;

extern "C" {

int im_icp_chunk(void) { return ICP_CHUNK; }

int im_transform_points(im_ctx* ctx, const double* d_M, const double* d_in, double* d_out, long long n, int as_vectors, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_M || !d_in || !d_out) return ctx->fail(ICP_REFUSED, "im_transform_points: null pointer");
    if (n < 0 || n > ICP_MAX_POINTS) return ctx->fail(ICP_REFUSED, "im_transform_points: n must be 0..2^26");
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    IM_LAUNCH(ctx, "transform_points", s, launch(transform_points_kernel, blocks_of(n, 256), 256, 0, s, d_M, d_in, d_out, n, as_vectors));
    IM_GUARD_CHECK(ctx, s, "im_transform_points");
    return 0;
}

int im_icp_accumulate(im_ctx* ctx, const double* d_src, long long n, const double* d_tgt, const double* d_nrm, long long n_tgt,
                      const int32_t* d_idx, const double* d_d2, const double* h_centre, int method, long long n_chunks, double* d_partials,
                      void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_src || !d_tgt || !d_idx || !d_d2) return ctx->fail(ICP_REFUSED, "im_icp_accumulate: null pointer");
    if (const char* why = bad_centre(h_centre)) return ctx->fail(ICP_REFUSED, "im_icp_accumulate: %s", why);
    if (method != ICP_POINT_TO_POINT && method != ICP_POINT_TO_PLANE) return ctx->fail(ICP_REFUSED, "im_icp_accumulate: method must be 0 (point to point) or 1 (point to plane)");
    if (method == ICP_POINT_TO_PLANE && !d_nrm) return ctx->fail(ICP_REFUSED, "im_icp_accumulate: point to plane needs the target's normals");
    if (n < 0 || n > ICP_MAX_POINTS) return ctx->fail(ICP_REFUSED, "im_icp_accumulate: n must be 0..2^26");
    if (n_tgt < 0 || n_tgt > ICP_MAX_POINTS) return ctx->fail(ICP_REFUSED, "im_icp_accumulate: n_tgt must be 0..2^26");
    if (n_chunks != blocks_of(n, ICP_CHUNK)) return ctx->fail(ICP_REFUSED, "im_icp_accumulate: n_chunks must be ceil(n / im_icp_chunk())");
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (!d_partials) {
        const IcpScratch lay(n_chunks);
        IM_GROW(ctx, ctx->grow(ctx->scratch.icp, lay.bytes, "icp.scratch"), -22, "im_icp_accumulate: allocation failed");
        d_partials = lay.parts.at(ctx->scratch.icp.p);
    }
    const IcpAccArgs a{d_src, d_tgt, d_nrm, d_idx, d_d2, n, n_tgt, {h_centre[0], h_centre[1], h_centre[2]}, method, d_partials};
    IM_LAUNCH(ctx, "icp_accumulate", s, launch(icp_accumulate_kernel, n_chunks, ICP_BLOCK, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_icp_accumulate");
    return 0;
}

int im_icp_finish(im_ctx* ctx, const double* d_partials, long long n, long long n_chunks, const double* d_M, const double* h_centre, int solve,
                  double* d_record, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_M || !d_record) return ctx->fail(ICP_REFUSED, "im_icp_finish: null pointer");
    if (const char* why = bad_centre(h_centre)) return ctx->fail(ICP_REFUSED, "im_icp_finish: %s", why);
    if (n < 0 || n > ICP_MAX_POINTS) return ctx->fail(ICP_REFUSED, "im_icp_finish: n must be 0..2^26");
    if (n_chunks != blocks_of(n, ICP_CHUNK)) return ctx->fail(ICP_REFUSED, "im_icp_finish: n_chunks must be ceil(n / im_icp_chunk())");
    if (solve != 0 && solve != 1) return ctx->fail(ICP_REFUSED, "im_icp_finish: solve must be 0 or 1");
    if (!d_partials && n_chunks > 0) {
        const IcpScratch lay(n_chunks);
        if (ctx->scratch.icp.bytes < lay.bytes) return ctx->fail(ICP_REFUSED, "im_icp_finish: the context holds no partials of %lld chunks", n_chunks);
        d_partials = lay.parts.at(ctx->scratch.icp.p);
    }
    hipStream_t s = (hipStream_t)stream;
    const IcpFinishArgs a{d_partials, d_M, n, n_chunks, {h_centre[0], h_centre[1], h_centre[2]}, solve, d_record};
    IM_LAUNCH(ctx, "icp_finish", s, launch(icp_finish_kernel, 1, ICP_BLOCK, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_icp_finish");
    return 0;
}

}  // extern "C"
