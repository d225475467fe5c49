// Two-view bundle adjustment with control points on the device: Levenberg-Marquardt with the points eliminated, batched over the epochs of
// a sequence (ba_point.h). A definition of its own, pinned bit for bit against tests/ba_oracle.py; parity with Metashape's
// optimizeCameras is unpinned.
//
//   ba_accumulate_kernel   grid (chunks, epochs), 256 threads. Per tile of BA_TILE = 32 points the first 32 threads write their point's
//                          factors (ba_point_factors: Jc, r, Y, z, L, D, cost, usable; 155 doubles) to LDS; then thread t owns sums t and
//                          t + 256 of the 448 and adds the tile's points in ascending order (ba_term). What the back-substitution needs
//                          (Y, z, L, D, cost, usable; 95 doubles) is KEPT per point in device memory, not recomputed. One partial of 448
//                          doubles per chunk.
//   ba_solve_kernel        one block per epoch: thread t adds the chunk partials of sums t and t + 256 in ascending chunk order; thread 0
//                          forms the reduced system in LDS (priors, damping, mask), solves it and writes the candidate cameras.
//   ba_step_points_kernel  grid (chunks, epochs), one thread per point: the back-substitution, the candidate point, its cost term; thread 0
//                          adds the chunk's 256 cost terms in ascending order.
//   ba_decide_kernel       one block per epoch: the candidate's cost, accept or reject, lambda, status, the iteration's record.
//   ba_residuals_kernel    one thread per point: the reprojection residuals of the current state.
// Cameras and points are double-buffered, [2][E][48] and [2][M][3]; an epoch's state row holds the parity of its current buffers and its done
// flag, so a run of max_iter iterations needs no read-back, and the blocks of a finished epoch return at once. No atomics.
#include "common.h"
#include "ctx.h"
#include "stage_scratch.h"
#include "ba_point.h"

namespace im {
namespace {

constexpr int BA_REFUSED = -82;
constexpr long long BA_MAX_POINTS = 1LL << 26;
constexpr int BA_MAX_EPOCHS = 65535;      // the grid's y

static_assert(BA_PART == BA_TERMS && BA_KEPT == BA_KEEP && BA_SLOT_POINTS == BA_CHUNK, "the scratch follows ba_point.h");
static_assert(BA_CHUNK == BA_BLOCK && BA_CHUNK % BA_TILE == 0 && BA_TERMS <= 2 * BA_BLOCK, "a thread per point of a chunk, two sums per thread");

struct BaArgs {
    const long long* off; int E; long long M;
    double* pts2; const double* obs; const double* sig; const double* prior;
    double* cams2; const double* cprior; double* state;
    double* parts; double* cparts; double* keep; double* sol;
    unsigned mask;
    double opts[BA_OPTS];
    double* history; long long hist_rows;
    double* res;
};

// the epoch of this block: false where it is finished or its offsets do not lie inside the arrays
__device__ __forceinline__ bool ba_epoch(const BaArgs& a, int e, bool any_state, long long& first, long long& n, int& parity) {
    const double* st = a.state + (long long)e * BA_STATE;
    if (!any_state && st[BA_ST_DONE] != 0.0) return false;
    first = a.off[e];
    n = a.off[e + 1] - first;
    parity = st[BA_ST_PARITY] != 0.0 ? 1 : 0;
    return first >= 0 && n >= 0 && first + n <= a.M;
}

__global__ __launch_bounds__(BA_BLOCK) void ba_accumulate_kernel(BaArgs a) {
    __shared__ double fac[BA_TILE * BA_FAC];
    const int e = blockIdx.y, t = threadIdx.x;
    long long first, n; int parity;
    if (!ba_epoch(a, e, false, first, n, parity)) return;
    const long long c0 = (long long)blockIdx.x * BA_CHUNK;
    if (c0 >= n) return;
    const double* cams = a.cams2 + ((long long)parity * a.E + e) * BA_EPOCH;
    const double* pts = a.pts2 + (long long)parity * a.M * 3;
    const double lambda = a.state[(long long)e * BA_STATE + BA_ST_LAMBDA];
    int k0, a0, b0, k1, a1, b1;
    ba_entry(t, k0, a0, b0);
    ba_entry(t + BA_BLOCK < BA_TERMS ? t + BA_BLOCK : BA_TERMS - 1, k1, a1, b1);
    double S0 = 0.0, S1 = 0.0;
    for (long long base = c0; base < n && base < c0 + BA_CHUNK; base += BA_TILE) {
        const int cnt = (int)(n - base < BA_TILE ? n - base : BA_TILE);
        if (t < cnt) {
            const long long i = first + base + t;
            const double X[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
            ba_point_factors(cams, X, a.obs + 4 * i, a.sig[i], a.prior + 6 * i, lambda, fac + t * BA_FAC);
        }
        __syncthreads();
        for (int p = 0; p < cnt; ++p) {
#pragma clang fp contract(off)
            S0 = S0 + ba_term(fac + p * BA_FAC, k0, a0, b0);
            S1 = S1 + ba_term(fac + p * BA_FAC, k1, a1, b1);
        }
        for (int j = t; j < cnt * BA_KEEP; j += BA_BLOCK)
            a.keep[(first + base) * BA_KEEP + j] = fac[(j / BA_KEEP) * BA_FAC + BA_F_Y + j % BA_KEEP];
        __syncthreads();
    }
    double* out = a.parts + (first / BA_CHUNK + e + blockIdx.x) * BA_TERMS;
    out[t] = S0;
    if (t + BA_BLOCK < BA_TERMS) out[t + BA_BLOCK] = S1;
}

__global__ __launch_bounds__(BA_BLOCK) void ba_solve_kernel(BaArgs a) {
    __shared__ double tot[BA_TERMS];
    __shared__ double A[BA_DIM * BA_DIM];
    __shared__ double wk[5 * BA_DIM];
    __shared__ double rec[BA_RECORD];
    const int e = blockIdx.x, t = threadIdx.x;
    long long first, n; int parity;
    if (!ba_epoch(a, e, false, first, n, parity)) return;
    const long long chunks = (n + BA_CHUNK - 1) / BA_CHUNK;
    const double* parts = a.parts + (first / BA_CHUNK + e) * BA_TERMS;
    double* sol = a.sol + (long long)e * BA_SOL;
    for (int k = t; k < BA_TERMS; k += BA_BLOCK) {
#pragma clang fp contract(off)
        double s = 0.0;
        for (long long ch = 0; ch < chunks; ++ch) s = s + parts[ch * BA_TERMS + k];
        tot[k] = s;
        sol[k] = s;
    }
    __syncthreads();
    if (t == 0) {
        const double* cams = a.cams2 + ((long long)parity * a.E + e) * BA_EPOCH;
        double* cand = a.cams2 + ((long long)(1 - parity) * a.E + e) * BA_EPOCH;
        ba_solve_epoch(tot, cams, a.cprior + 12LL * e, a.state[(long long)e * BA_STATE + BA_ST_LAMBDA], a.mask, A, wk, rec, cand);
    }
    __syncthreads();
    if (t < BA_RECORD) sol[BA_SOL_REC + t] = rec[t];
}

__global__ __launch_bounds__(BA_BLOCK) void ba_step_points_kernel(BaArgs a) {
    __shared__ double cost[BA_BLOCK];
    const int e = blockIdx.y, t = threadIdx.x;
    long long first, n; int parity;
    if (!ba_epoch(a, e, false, first, n, parity)) return;
    const long long c0 = (long long)blockIdx.x * BA_CHUNK;
    if (c0 >= n) return;
    const double* cand = a.cams2 + ((long long)(1 - parity) * a.E + e) * BA_EPOCH;
    const double* pts = a.pts2 + (long long)parity * a.M * 3;
    double* out = a.pts2 + (long long)(1 - parity) * a.M * 3;
    const double* x = a.sol + (long long)e * BA_SOL + BA_SOL_REC + BA_REC_X;
    double c = 0.0;
    if (c0 + t < n) {
        const long long i = first + c0 + t;
        const double* keep = a.keep + i * BA_KEEP;
        const double X[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
        double Y[3];
        ba_point_step(keep, x, X, Y);
        out[3 * i] = Y[0]; out[3 * i + 1] = Y[1]; out[3 * i + 2] = Y[2];
        c = ba_point_cost(cand, Y, a.obs + 4 * i, a.sig[i], a.prior + 6 * i, keep[BA_F_OK - BA_F_Y] != 0.0);
    }
    cost[t] = c;
    __syncthreads();
    if (t == 0) {
#pragma clang fp contract(off)
        double s = 0.0;
        for (int p = 0; p < BA_BLOCK; ++p) s = s + cost[p];
        a.cparts[first / BA_CHUNK + e + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(64) void ba_decide_kernel(BaArgs a) {
#pragma clang fp contract(off)
    __shared__ double dummy[BA_RECORD];
    const int e = blockIdx.x;
    long long first, n; int parity;
    if (threadIdx.x != 0 || !ba_epoch(a, e, false, first, n, parity)) return;
    const long long chunks = (n + BA_CHUNK - 1) / BA_CHUNK;
    const double* cparts = a.cparts + first / BA_CHUNK + e;
    double s = 0.0;
    for (long long ch = 0; ch < chunks; ++ch) s = s + cparts[ch];
    const double* cand = a.cams2 + ((long long)(1 - parity) * a.E + e) * BA_EPOCH;
    const double cost1 = s + ba_centre_cost(cand, a.cprior + 12LL * e);
    double* st = a.state + (long long)e * BA_STATE;
    const long long it = (long long)st[BA_ST_ITER];
    double* rec = it >= 0 && it < a.hist_rows ? a.history + (it * a.E + e) * BA_RECORD : dummy;
    ba_decide(a.sol + (long long)e * BA_SOL + BA_SOL_REC, cost1, a.opts, st, rec);
}

__global__ __launch_bounds__(BA_BLOCK) void ba_residuals_kernel(BaArgs a) {
    const int e = blockIdx.y;
    long long first, n; int parity;
    if (!ba_epoch(a, e, true, first, n, parity)) return;
    const long long j = (long long)blockIdx.x * BA_CHUNK + threadIdx.x;
    if (j >= n) return;
    const long long i = first + j;
    const double* cams = a.cams2 + ((long long)parity * a.E + e) * BA_EPOCH;
    const double* pts = a.pts2 + (long long)parity * a.M * 3;
    const double X[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    ba_point_residuals(cams, X, a.obs + 4 * i, a.res + 6 * i);
}

const char* bad_shape(int E, long long M, long long max_points) {
    if (E < 1 || E > BA_MAX_EPOCHS) return "E must be 1..65535";
    if (M < 0 || M > BA_MAX_POINTS) return "M must be 0..2^26";
    if (max_points < 0 || max_points > M) return "max_points must be 0..M";
    return nullptr;
}

// the context's scratch for what the caller did not bring; grow: im_ba_accumulate's call, the others find it there
int ba_scratch(im_ctx* ctx, const char* who, int E, long long M, bool grow, double** parts, double** cparts, double** keep) {
    const BaScratch lay(E, M);
    if (grow) IM_GROW(ctx, ctx->grow(ctx->scratch.ba, lay.bytes, "ba.scratch"), -22, "%s: allocation failed", who);
    else if (ctx->scratch.ba.bytes < lay.bytes) return ctx->fail(BA_REFUSED, "%s: the context holds no factors of %d epochs and %lld points", who, E, M);
    void* const sb = ctx->scratch.ba.p;
    if (parts && !*parts) *parts = lay.parts.at(sb);
    if (cparts && !*cparts) *cparts = lay.cparts.at(sb);
    if (keep) *keep = lay.keep.at(sb);
    return 0;
}

}  // namespace
}  // namespace im

using namespace im;

extern "C" {

int im_ba_chunk(void) { return BA_CHUNK; }

int im_ba_accumulate(im_ctx* ctx, const long long* d_off, int E, long long M, long long max_points, const double* d_pts2, const double* d_obs,
                     const double* d_sig, const double* d_prior, const double* d_cams2, const double* d_state, double* d_parts, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_off || !d_pts2 || !d_obs || !d_sig || !d_prior || !d_cams2 || !d_state) return ctx->fail(BA_REFUSED, "im_ba_accumulate: null pointer");
    if (const char* why = bad_shape(E, M, max_points)) return ctx->fail(BA_REFUSED, "im_ba_accumulate: %s", why);
    BaArgs a{};
    a.parts = d_parts;
    if (const int rc = ba_scratch(ctx, "im_ba_accumulate", E, M, true, &a.parts, nullptr, &a.keep)) return rc;
    if (max_points == 0) return 0;
    a.off = d_off; a.E = E; a.M = M; a.pts2 = const_cast<double*>(d_pts2); a.obs = d_obs; a.sig = d_sig; a.prior = d_prior;
    a.cams2 = const_cast<double*>(d_cams2); a.state = const_cast<double*>(d_state);
    hipStream_t s = (hipStream_t)stream;
    IM_LAUNCH(ctx, "ba_accumulate", s, launch(ba_accumulate_kernel, dim3((unsigned)blocks_of(max_points, BA_CHUNK), E), BA_BLOCK, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_ba_accumulate");
    return 0;
}

int im_ba_solve(im_ctx* ctx, const long long* d_off, int E, long long M, const double* d_parts, double* d_cams2, const double* d_cprior,
                const double* d_state, unsigned mask, double* d_sol, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_off || !d_cams2 || !d_cprior || !d_state || !d_sol) return ctx->fail(BA_REFUSED, "im_ba_solve: null pointer");
    if (const char* why = bad_shape(E, M, 0)) return ctx->fail(BA_REFUSED, "im_ba_solve: %s", why);
    if (mask >> BA_DIM) return ctx->fail(BA_REFUSED, "im_ba_solve: the mask has %d bits", BA_DIM);
    BaArgs a{};
    a.parts = const_cast<double*>(d_parts);
    if (!d_parts)
        if (const int rc = ba_scratch(ctx, "im_ba_solve", E, M, false, &a.parts, nullptr, nullptr)) return rc;
    a.off = d_off; a.E = E; a.M = M; a.cams2 = d_cams2; a.cprior = d_cprior; a.state = const_cast<double*>(d_state); a.mask = mask; a.sol = d_sol;
    hipStream_t s = (hipStream_t)stream;
    IM_LAUNCH(ctx, "ba_solve", s, launch(ba_solve_kernel, E, BA_BLOCK, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_ba_solve");
    return 0;
}

int im_ba_step_points(im_ctx* ctx, const long long* d_off, int E, long long M, long long max_points, double* d_pts2, const double* d_obs,
                      const double* d_sig, const double* d_prior, const double* d_cams2, const double* d_state, const double* d_sol,
                      double* d_cparts, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_off || !d_pts2 || !d_obs || !d_sig || !d_prior || !d_cams2 || !d_state || !d_sol) return ctx->fail(BA_REFUSED, "im_ba_step_points: null pointer");
    if (const char* why = bad_shape(E, M, max_points)) return ctx->fail(BA_REFUSED, "im_ba_step_points: %s", why);
    BaArgs a{};
    a.cparts = d_cparts;
    if (const int rc = ba_scratch(ctx, "im_ba_step_points", E, M, false, nullptr, &a.cparts, &a.keep)) return rc;
    if (max_points == 0) return 0;
    a.off = d_off; a.E = E; a.M = M; a.pts2 = d_pts2; a.obs = d_obs; a.sig = d_sig; a.prior = d_prior;
    a.cams2 = const_cast<double*>(d_cams2); a.state = const_cast<double*>(d_state); a.sol = const_cast<double*>(d_sol);
    hipStream_t s = (hipStream_t)stream;
    IM_LAUNCH(ctx, "ba_step_points", s, launch(ba_step_points_kernel, dim3((unsigned)blocks_of(max_points, BA_CHUNK), E), BA_BLOCK, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_ba_step_points");
    return 0;
}

int im_ba_decide(im_ctx* ctx, const long long* d_off, int E, long long M, const double* d_cparts, const double* d_cams2, const double* d_cprior,
                 double* d_state, const double* d_sol, const double* h_opts, double* d_history, long long hist_rows, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_off || !d_cams2 || !d_cprior || !d_state || !d_sol || !h_opts || !d_history) return ctx->fail(BA_REFUSED, "im_ba_decide: null pointer");
    if (const char* why = bad_shape(E, M, 0)) return ctx->fail(BA_REFUSED, "im_ba_decide: %s", why);
    if (!(h_opts[BA_OPT_LMIN] > 0.0) || !(h_opts[BA_OPT_LMAX] >= h_opts[BA_OPT_LMIN]) || !(h_opts[BA_OPT_FTOL] >= 0.0) ||
        !(h_opts[BA_OPT_MAX_ITER] >= 1.0) || !(h_opts[BA_OPT_MAX_ITER] <= (double)hist_rows) || !(h_opts[BA_OPT_CTOL] >= 0.0))
        return ctx->fail(BA_REFUSED, "im_ba_decide: options must be 0 < lambda_min <= lambda_max, ftol >= 0, 1 <= max_iter <= hist_rows, ctol >= 0");
    BaArgs a{};
    a.cparts = const_cast<double*>(d_cparts);
    if (!d_cparts)
        if (const int rc = ba_scratch(ctx, "im_ba_decide", E, M, false, nullptr, &a.cparts, nullptr)) return rc;
    a.off = d_off; a.E = E; a.M = M; a.cams2 = const_cast<double*>(d_cams2); a.cprior = d_cprior; a.state = d_state;
    a.sol = const_cast<double*>(d_sol); a.history = d_history; a.hist_rows = hist_rows;
    for (int k = 0; k < BA_OPTS; ++k) a.opts[k] = h_opts[k];
    hipStream_t s = (hipStream_t)stream;
    IM_LAUNCH(ctx, "ba_decide", s, launch(ba_decide_kernel, E, 64, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_ba_decide");
    return 0;
}

int im_ba_residuals(im_ctx* ctx, const long long* d_off, int E, long long M, long long max_points, const double* d_pts2, const double* d_obs,
                    const double* d_cams2, const double* d_state, double* d_res, void* stream) {
    IM_CHECK_CTX(ctx);
    if (!d_off || !d_pts2 || !d_obs || !d_cams2 || !d_state || !d_res) return ctx->fail(BA_REFUSED, "im_ba_residuals: null pointer");
    if (const char* why = bad_shape(E, M, max_points)) return ctx->fail(BA_REFUSED, "im_ba_residuals: %s", why);
    if (max_points == 0) return 0;
    BaArgs a{};
    a.off = d_off; a.E = E; a.M = M; a.pts2 = const_cast<double*>(d_pts2); a.obs = d_obs; a.cams2 = const_cast<double*>(d_cams2);
    a.state = const_cast<double*>(d_state); a.res = d_res;
    hipStream_t s = (hipStream_t)stream;
    IM_LAUNCH(ctx, "ba_residuals", s, launch(ba_residuals_kernel, dim3((unsigned)blocks_of(max_points, BA_CHUNK), E), BA_BLOCK, 0, s, a));
    IM_GUARD_CHECK(ctx, s, "im_ba_residuals");
    return 0;
}

}  // extern "C"
