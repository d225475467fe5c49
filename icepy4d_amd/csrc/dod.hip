// Volume variations on the device: the DEM of difference between the clouds of two epochs and the figures of CloudCompare's 2.5D volume
// (`scripts/pcd_postprocessing/volume_variations.py`; `post_processing/cloudcompare_fun.py`: `DemOfDifference.compute_volume` over
// `cc.ComputeVolume25D`), and the polygon crop that comes before it (`post_processing/open3d_fun.py`: `filter_pcd_by_polyline`).
// CloudComPy is an un-vendored dependency: the algorithm has a definition of its own and is pinned bit for bit against
// tests/dod_oracle.py. One call serves a batch of P pairs over E clouds that sit in one buffer; a cloud is rasterised once per pair it
// takes part in, into the grid of that pair's union box. An item is one (pair, side, point), sides in the order ground, ceil.
//
//   dod_bounds_kernel   per cloud the minimum and maximum of the kept points along the grid's two axes and the number of dropped points:
//                       a block reduction, then atomicMax on order-preserving integer keys (exact, order-free)
//   dod_keys_kernel     one thread per item: the key seg_base(pair, side) + j w + i of its cell (dod_cell.h), or the number of segments
//                       for a dropped point. The stable sort by key between this and the rest is torch's, plumbing: every (pair, side,
//                       cell) becomes a contiguous segment in input order
//   dod_hist_kernel     points per segment (integer atomics); scan_*_kernel (scan.h) turn them into segment starts
//   dod_cells_kernel    one thread per (pair, cell): the two sums in segment order = ascending input index, the means, H, which clouds
//                       fill the cell
//   dod_report_kernel   one block per chunk of DOD_CHUNK consecutive cells: H staged in LDS, the integer counts of the report (valid
//                       cells, filled cells, cells of one cloud only, valid neighbours in the 3 x 3 window), and the three chunk sums,
//                       each by one thread of a wave of its own in ascending cell index
//   dod_final_kernel    one block per pair: the chunk partials in ascending chunk index, then the report (dod_cell.h)
//   crop_polygon_kernel one thread per point, the polygon's vertices staged in LDS: the even-odd rule; a scan lists the kept indices
// float64 throughout, contraction off in dod_cell.h. The order of every floating-point sum is fixed by DOD_CHUNK alone: no launch
// geometry and no property of the device enters it.
#include <cmath>
#include <vector>

#include "common.h"
#include "ctx.h"
#include "stage_scratch.h"
#include "dod_cell.h"

namespace im {
namespace {

#include "scan.h"

constexpr long long DOD_MAX_CELLS = 1LL << 24;                  // per pair
constexpr long long DOD_MAX_BATCH_CELLS = 4 * DOD_MAX_CELLS;    // over the pairs of one call
constexpr int DOD_MAX_SETS = 65535;                             // clouds, and pairs, of one call
constexpr int DOD_BOUNDS_BLOCKS = 256;                          // blocks per cloud of dod_bounds_kernel at the most, of 1024 points or more each

// the tables of a call in device memory (DodScratch::table), q = 2 pair + side
struct DodTab {
    const long long* offsets;     // [E + 1] first point of every cloud
    const long long* item_base;   // [2 P + 1] first item of every side
    const long long* seg_base;    // [2 P + 1] first segment of every side; [2 P] = the number of segments
    const long long* pt_base;     // [2 P] first point of the side's cloud
    const double* gmin;           // [P][2] min_x, min_y
    const long long* gdim;        // [P][2] w, h
    const long long* chunk_base;  // [P + 1] first chunk of every pair
    int P;
};

// the last k in 0..n-1 with base[k] <= v (base ascending, base[0] <= v)
__device__ __forceinline__ int last_at_or_below(const long long* __restrict__ base, int n, long long v) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (base[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int o = IM_WAVE / 2; o > 0; o >>= 1) { const T u = __shfl_xor(v, o); v = u > v ? u : v; }
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = IM_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// bkeys [E][4]: the complement of the least key along X and along Y, the greatest key along X and along Y; 0 = no kept point
__global__ __launch_bounds__(256) void dod_bounds_kernel(const double* __restrict__ pts, const long long* __restrict__ offsets, int ax, int ay,
                                                         unsigned long long* __restrict__ bkeys, unsigned long long* __restrict__ dropped) {
    const int e = blockIdx.y;
    const long long p0 = offsets[e], p1 = offsets[e + 1];
    unsigned long long k[4] = {0, 0, 0, 0}, drop = 0;
    for (long long i = p0 + blockIdx.x * 256LL + threadIdx.x; i < p1; i += gridDim.x * 256LL) {
        const double c[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
        if (!dod_kept(c[0], c[1], c[2])) { ++drop; continue; }
        const unsigned long long kx = dod_order_key(c[ax]), ky = dod_order_key(c[ay]);
        k[0] = max(k[0], ~kx); k[1] = max(k[1], ~ky); k[2] = max(k[2], kx); k[3] = max(k[3], ky);
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) k[a] = wave_max(k[a]);
    drop = wave_sum(drop);
    __shared__ unsigned long long sk[256 / IM_WAVE][5];            // per wave: the four keys and the dropped count
    const int wv = threadIdx.x / IM_WAVE;
    if ((threadIdx.x & (IM_WAVE - 1)) == 0) {
#pragma unroll
        for (int a = 0; a < 4; ++a) sk[wv][a] = k[a];
        sk[wv][4] = drop;
    }
    __syncthreads();
    if (threadIdx.x < 5) {                                          // one atomic per block and quantity: they all meet at 5 E addresses
        const int a = threadIdx.x;
        unsigned long long m = 0;
        for (int v = 0; v < 256 / IM_WAVE; ++v) m = a < 4 ? max(m, sk[v][a]) : m + sk[v][a];
        if (m && a < 4) atomicMax(&bkeys[4 * e + a], m);
        if (m && a == 4) atomicAdd(&dropped[e], m);
    }
}

// min_x, min_y, max_x, max_y per cloud; +inf / -inf for a cloud without a kept point
__global__ __launch_bounds__(256) void dod_bounds_decode_kernel(const unsigned long long* __restrict__ bkeys, int n, double* __restrict__ bounds) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const unsigned long long k = bkeys[t];
    const bool is_min = (t & 3) < 2;
    bounds[t] = k ? dod_order_value(is_min ? ~k : k) : (is_min ? dod_inf() : -dod_inf());
}

__global__ __launch_bounds__(256) void dod_keys_kernel(DodTab T, const double* __restrict__ pts, long long items, int ax, int ay, double s,
                                                       long long* __restrict__ key) {
    const long long t = blockIdx.x * 256LL + threadIdx.x;
    if (t >= items) return;
    const int q = last_at_or_below(T.item_base, 2 * T.P, t), p = q >> 1;
    const long long i = T.pt_base[q] + (t - T.item_base[q]);
    const double c[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    long long cell = -1;
    if (dod_kept(c[0], c[1], c[2])) cell = dod_cell_of(c[ax], c[ay], T.gmin[2 * p], T.gmin[2 * p + 1], s, T.gdim[2 * p], T.gdim[2 * p + 1]);
    key[t] = cell < 0 ? T.seg_base[2 * T.P] : T.seg_base[q] + cell;
}

__global__ __launch_bounds__(256) void dod_hist_kernel(const long long* __restrict__ skey, long long n, long long n_seg, unsigned* __restrict__ counts) {
    const long long j = blockIdx.x * 256LL + threadIdx.x;
    if (j >= n) return;
    const long long k = skey[j];
    if (k >= 0 && k < n_seg) atomicAdd(&counts[k], 1u);
}

struct DodCountScan {         // points per segment -> first sorted position of each segment
    const unsigned* counts; long long n_seg; long long* starts;
    __device__ long long count(long long g) const { return g < n_seg ? counts[g] : 0; }
    __device__ void write(long long g, long long pos) const { if (g < n_seg) starts[g] = pos; }
};

// state: bit 0 the ground fills the cell, bit 1 the ceil does. An item index that is none (a permutation that is none) is clamped into
// its side: the result is then meaningless, but every access stays inside.
__global__ __launch_bounds__(256) void dod_cells_kernel(DodTab T, const double* __restrict__ pts, const long long* __restrict__ perm, long long items,
                                                        const long long* __restrict__ starts, long long cells, int d, double* __restrict__ H,
                                                        unsigned char* __restrict__ state) {
    const long long gc = blockIdx.x * 256LL + threadIdx.x;
    if (gc >= cells) return;
    int lo = 0, hi = T.P;                                  // the pair of cell gc: seg_base[2 p] = twice the pair's first cell
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (T.seg_base[2 * mid] <= 2 * gc) lo = mid; else hi = mid;
    }
    const int p = lo;
    const long long local = gc - T.seg_base[2 * p] / 2;
    double mean[2] = {0.0, 0.0};
    int st = 0;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const int q = 2 * p + side;
        const long long seg = T.seg_base[q] + local;
        long long j0 = starts[seg], j1 = starts[seg + 1];
        j0 = j0 < 0 ? 0 : j0;
        j1 = j1 > items ? items : j1;
        if (j1 <= j0) continue;
        const long long t0 = T.item_base[q], t1 = T.item_base[q + 1] - 1, base = T.pt_base[q];
        if (t1 < t0) continue;
        mean[side] = dod_mean([&](long long k) {
            long long t = perm[j0 + k];
            t = t < t0 ? t0 : (t > t1 ? t1 : t);
            return pts[3 * (base + (t - t0)) + d];
        }, j1 - j0);
        st |= 1 << side;
    }
    H[gc] = st == 3 ? dod_diff(mean[0], mean[1]) : dod_nan();
    state[gc] = (unsigned char)st;
}

__global__ __launch_bounds__(256) void dod_report_kernel(DodTab T, const double* __restrict__ H, const unsigned char* __restrict__ state,
                                                         double* __restrict__ parts, unsigned long long* __restrict__ ncnt) {
    __shared__ double sh[DOD_CHUNK];
    __shared__ unsigned cnt[DOD_N_COUNTS];
    const long long ch = blockIdx.x;
    const int p = last_at_or_below(T.chunk_base, T.P, ch), t = threadIdx.x;
    const long long w = T.gdim[2 * p], h = T.gdim[2 * p + 1], cells = w * h, first = T.seg_base[2 * p] / 2;
    const long long cell0 = (ch - T.chunk_base[p]) * DOD_CHUNK;
    const int n = (int)min((long long)DOD_CHUNK, cells - cell0);
    if (t < DOD_N_COUNTS) cnt[t] = 0;
    __syncthreads();
    unsigned c[DOD_N_COUNTS] = {0, 0, 0, 0, 0};
    const double* Hp = H + first;
    for (int k = t; k < DOD_CHUNK; k += 256) {
        double v = dod_nan();
        if (k < n) {
            const long long cell = cell0 + k;
            v = Hp[cell];
            const int st = state[first + cell];
            c[DOD_N_FILLED] += st != 0; c[DOD_N_GROUND_ONLY] += st == 1; c[DOD_N_CEIL_ONLY] += st == 2;
            if (dod_valid(v)) {
                ++c[DOD_N_VALID];
                c[DOD_N_NEIGHBOURS] += dod_neighbours([&](long long ii, long long jj) { return dod_valid(Hp[jj * w + ii]); }, cell % w, cell / w, w, h);
            }
        }
        sh[k] = v;
    }
#pragma unroll
    for (int a = 0; a < DOD_N_COUNTS; ++a) {
        const unsigned tot = wave_sum(c[a]);
        if ((t & (IM_WAVE - 1)) == 0 && tot) atomicAdd(&cnt[a], tot);
    }
    __syncthreads();
    if (t < DOD_N_COUNTS && cnt[t]) atomicAdd(&ncnt[DOD_N_COUNTS * p + t], (unsigned long long)cnt[t]);
    if ((t & (IM_WAVE - 1)) == 0 && t / IM_WAVE < 3) {
        const int which = t / IM_WAVE;             // DOD_VOLUME, DOD_ADDED, DOD_REMOVED
        parts[3 * ch + which] = dod_chunk_sum([&](long long k) { return sh[k]; }, n, which);
    }
}

__global__ __launch_bounds__(192) void dod_final_kernel(DodTab T, const double* __restrict__ parts, const unsigned long long* __restrict__ ncnt, double s,
                                                        double* __restrict__ report) {
    __shared__ double sums[3];
    const int p = blockIdx.x, t = threadIdx.x;
    const long long c0 = T.chunk_base[p], nc = T.chunk_base[p + 1] - c0;
    if ((t & (IM_WAVE - 1)) == 0) {
        const int which = t / IM_WAVE;
        sums[which] = dod_partial_sum([&](long long k) { return parts[3 * (c0 + k) + which]; }, nc);
    }
    __syncthreads();
    if (t == 0) dod_report(report + (long long)DOD_REPORT * p, sums, ncnt + DOD_N_COUNTS * p, s, T.gdim[2 * p], T.gdim[2 * p + 1], T.gmin[2 * p], T.gmin[2 * p + 1]);
}

static_assert(DOD_VOLUME == 0 && DOD_ADDED == 1 && DOD_REMOVED == 2, "the three sums are the report's first three slots");
static_assert(DOD_CHUNK % 256 == 0, "dod_report_kernel strides a chunk by its block");

__global__ __launch_bounds__(256) void crop_polygon_kernel(const double* __restrict__ pts, long long n, int ax, int ay, const double* __restrict__ poly, int nv,
                                                           int inside, unsigned char* __restrict__ mask) {
    __shared__ double sp[2 * DOD_MAX_VERTS];
    for (int k = threadIdx.x; k < 2 * nv; k += 256) sp[k] = poly[k];
    __syncthreads();
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= n) return;
    const bool in = dod_in_polygon([&](int k, double& x, double& y) { x = sp[2 * k]; y = sp[2 * k + 1]; }, nv, pts[3 * i + ax], pts[3 * i + ay]);
    mask[i] = in == (inside != 0) ? 1 : 0;
}

struct MaskScan {             // the kept indices in ascending order
    const unsigned char* mask; long long n; long long* index;
    __device__ long long count(long long j) const { return j < n && mask[j] ? 1 : 0; }
    __device__ void write(long long j, long long pos) const { if (count(j)) index[pos] = j; }
};

// ---- the host half: what a call refuses, the grids of its pairs, its tables ------------------------------------------------------------
struct DodPlan {
    std::vector<long long> table;
    std::vector<double> gmin;                                 // [P][2] min_x, min_y: a table of its own, as it is on the device
    size_t o_item, o_seg, o_pt, o_gdim, o_chunk;              // positions of the tables behind the cloud offsets
    long long items = 0, cells = 0, chunks = 0;
    DodTab tab(const long long* d, const double* d_gmin, int P) const {
        return DodTab{d, d + o_item, d + o_seg, d + o_pt, d_gmin, d + o_gdim, d + o_chunk, P};
    }
};

const char* bad_clouds(const long long* h_offsets, int E, int vert_dim) {
    if (!h_offsets) return "null offsets";
    if (E < 1 || E > DOD_MAX_SETS) return "the number of clouds must be 1..65535";
    if (vert_dim < 0 || vert_dim > 2) return "vertDim must be 0, 1 or 2";
    if (h_offsets[0] != 0) return "the first cloud must start at point 0";
    for (int e = 0; e < E; ++e)
        if (h_offsets[e + 1] < h_offsets[e]) return "a cloud with a negative number of points";
    if (h_offsets[E] >= (1LL << 31)) return "at most 2^31 - 1 points";
    return nullptr;
}

const char* dod_plan(const long long* h_offsets, int E, const int32_t* h_pairs, int P, int vert_dim, double step, const double* h_bounds, DodPlan& pl) {
    if (const char* why = bad_clouds(h_offsets, E, vert_dim)) return why;
    if (P < 0 || P > DOD_MAX_SETS) return "the number of pairs must be 0..65535";
    if (!(step > 0.0) || std::isinf(step)) return "the step must be finite and positive";
    if (P == 0) return nullptr;
    if (!h_pairs || !h_bounds) return "null pairs or bounds";
    for (int k = 0; k < 4 * E; ++k)
        if (std::isnan(h_bounds[k])) return "a bound is NaN";
    pl.o_item = E + 1; pl.o_seg = pl.o_item + 2 * P + 1; pl.o_pt = pl.o_seg + 2 * P + 1;
    pl.o_gdim = pl.o_pt + 2 * P + 1; pl.o_chunk = pl.o_gdim + 2 * P;
    pl.table.assign(pl.o_chunk + P + 1, 0);
    long long* t = pl.table.data();
    for (int e = 0; e <= E; ++e) t[e] = h_offsets[e];
    pl.gmin.assign(2 * P, 0.0);
    for (int p = 0; p < P; ++p) {
        const int g = h_pairs[2 * p], c = h_pairs[2 * p + 1];
        if (g < 0 || g >= E || c < 0 || c >= E) return "a pair names a cloud outside 0..E-1";
        double min_x, min_y, wd, hd;
        dod_pair_grid(h_bounds + 4 * g, h_bounds + 4 * c, step, min_x, min_y, wd, hd);
        if (!(wd * hd <= (double)DOD_MAX_CELLS) || !(wd >= 0.0) || !(hd >= 0.0)) return "a pair's grid holds more cells than im_dod_max_cells()";
        const long long w = (long long)wd, h = (long long)hd;
        pl.gmin[2 * p] = min_x; pl.gmin[2 * p + 1] = min_y;
        t[pl.o_gdim + 2 * p] = w; t[pl.o_gdim + 2 * p + 1] = h;
        const int cloud[2] = {g, c};
        for (int side = 0; side < 2; ++side) {
            const int q = 2 * p + side;
            t[pl.o_item + q] = pl.items; t[pl.o_seg + q] = 2 * pl.cells + side * w * h; t[pl.o_pt + q] = h_offsets[cloud[side]];
            pl.items += h_offsets[cloud[side] + 1] - h_offsets[cloud[side]];
        }
        t[pl.o_chunk + p] = pl.chunks;
        pl.cells += w * h;
        pl.chunks += blocks_of(w * h, DOD_CHUNK);
        if (pl.cells > DOD_MAX_BATCH_CELLS) return "the grids of the batch hold more than im_dod_max_batch_cells() cells: split the batch";
        if (pl.items >= (1LL << 31)) return "the pairs of the batch hold 2^31 points or more: split the batch";
    }
    t[pl.o_item + 2 * P] = pl.items; t[pl.o_seg + 2 * P] = 2 * pl.cells; t[pl.o_chunk + P] = pl.chunks;
    return nullptr;
}

}  // namespace
}  // namespace im

using namespace im;

extern "C" {

int im_dod_chunk(void) { return DOD_CHUNK; }
int im_dod_max_cells(void) { return (int)DOD_MAX_CELLS; }
int im_dod_max_batch_cells(void) { return (int)DOD_MAX_BATCH_CELLS; }

int im_dod_bounds(im_ctx* ctx, const double* d_pts, const long long* h_offsets, int n_clouds, int vert_dim, double* d_bounds, long long* d_dropped,
                  void* stream) {
    IM_CHECK_CTX(ctx);
    if (const char* why = bad_clouds(h_offsets, n_clouds, vert_dim)) return ctx->fail(-76, "im_dod_bounds: %s", why);
    if (!d_bounds || !d_dropped || (h_offsets[n_clouds] && !d_pts)) return ctx->fail(-76, "im_dod_bounds: null pointer");
    const int E = n_clouds;
    const DodScratch lay(E, 0, 0, 0, false);
    IM_GROW(ctx, ctx->grow(ctx->scratch.dod, lay.bytes, "dod.scratch"), -22, "im_dod_bounds: allocation failed");
    void* const base = ctx->scratch.dod.p;
    long long* d_offsets = lay.table.at(base);
    unsigned long long* bkeys = lay.bkeys.at(base);
    hipStream_t s = (hipStream_t)stream;
    IM_HIP(ctx, hipMemcpyAsync(d_offsets, h_offsets, (E + 1) * sizeof(long long), hipMemcpyHostToDevice, s));
    IM_HIP(ctx, hipStreamSynchronize(s));          // the source is host memory of this call
    IM_HIP(ctx, hipMemsetAsync(bkeys, 0, 4 * E * sizeof(unsigned long long), s));
    IM_HIP(ctx, hipMemsetAsync(d_dropped, 0, E * sizeof(long long), s));
    long long largest = 0;
    for (int e = 0; e < E; ++e) largest = std::max(largest, h_offsets[e + 1] - h_offsets[e]);
    if (largest) {
        const dim3 grid((unsigned)std::min<long long>(blocks_of(largest, 1024), DOD_BOUNDS_BLOCKS), (unsigned)E);
        IM_LAUNCH(ctx, "dod_bounds", s, launch(dod_bounds_kernel, grid, 256, 0, s, d_pts, (const long long*)d_offsets, dod_axis_x(vert_dim), dod_axis_y(vert_dim),
                                               bkeys, reinterpret_cast<unsigned long long*>(d_dropped)));
    }
    IM_LAUNCH(ctx, "dod_bounds_decode", s, launch(dod_bounds_decode_kernel, blocks_of(4 * E, 256), 256, 0, s, (const unsigned long long*)bkeys, 4 * E, d_bounds));
    IM_GUARD_CHECK(ctx, s, "im_dod_bounds");
    return 0;
}

int im_dod_keys(im_ctx* ctx, const double* d_pts, const long long* h_offsets, int n_clouds, const int32_t* h_pairs, int n_pairs, int vert_dim,
                double step, const double* h_bounds, double* h_grids, long long* d_key, void* stream) {
    IM_CHECK_CTX(ctx);
    DodPlan pl;
    if (const char* why = dod_plan(h_offsets, n_clouds, h_pairs, n_pairs, vert_dim, step, h_bounds, pl)) return ctx->fail(-76, "im_dod_keys: %s", why);
    if (n_pairs == 0) return 0;
    if (!h_grids || (pl.items && d_key && !d_pts)) return ctx->fail(-76, "im_dod_keys: null pointer");
    const int E = n_clouds, P = n_pairs;
    for (int p = 0; p < P; ++p) {
        h_grids[4 * p] = pl.gmin[2 * p]; h_grids[4 * p + 1] = pl.gmin[2 * p + 1];
        h_grids[4 * p + 2] = (double)pl.table[pl.o_gdim + 2 * p]; h_grids[4 * p + 3] = (double)pl.table[pl.o_gdim + 2 * p + 1];
    }
    if (!pl.items || !d_key) return 0;             // no key asked for: the grids alone
    const DodScratch lay(E, P, 0, 0, false);
    IM_GROW(ctx, ctx->grow(ctx->scratch.dod, lay.bytes, "dod.scratch"), -22, "im_dod_keys: allocation failed");
    long long* d_table = lay.table.at(ctx->scratch.dod.p);
    double* d_gmin = lay.gmin.at(ctx->scratch.dod.p);
    hipStream_t s = (hipStream_t)stream;
    IM_HIP(ctx, hipMemcpyAsync(d_table, pl.table.data(), pl.table.size() * sizeof(long long), hipMemcpyHostToDevice, s));
    IM_HIP(ctx, hipMemcpyAsync(d_gmin, pl.gmin.data(), pl.gmin.size() * sizeof(double), hipMemcpyHostToDevice, s));
    IM_HIP(ctx, hipStreamSynchronize(s));          // the source is host memory of this call
    IM_LAUNCH(ctx, "dod_keys", s, launch(dod_keys_kernel, blocks_of(pl.items, 256), 256, 0, s, pl.tab(d_table, d_gmin, P), d_pts, pl.items, dod_axis_x(vert_dim),
                                         dod_axis_y(vert_dim), step, d_key));
    IM_GUARD_CHECK(ctx, s, "im_dod_keys");
    return 0;
}

int im_dod_reduce(im_ctx* ctx, const double* d_pts, const long long* h_offsets, int n_clouds, const int32_t* h_pairs, int n_pairs, int vert_dim,
                  double step, const double* h_bounds, const long long* d_sorted_keys, const long long* d_perm, double* d_H, double* d_report,
                  void* stream) {
    IM_CHECK_CTX(ctx);
    DodPlan pl;
    if (const char* why = dod_plan(h_offsets, n_clouds, h_pairs, n_pairs, vert_dim, step, h_bounds, pl)) return ctx->fail(-76, "im_dod_reduce: %s", why);
    if (n_pairs == 0) return 0;
    if (!d_report || (pl.items && (!d_pts || !d_sorted_keys || !d_perm))) return ctx->fail(-76, "im_dod_reduce: null pointer");
    const int E = n_clouds, P = n_pairs;
    const long long n_seg = 2 * pl.cells;
    const DodScratch lay(E, P, pl.cells, pl.chunks, d_H == nullptr);
    IM_GROW(ctx, ctx->grow(ctx->scratch.dod, lay.bytes, "dod.scratch"), -22, "im_dod_reduce: allocation failed (%lld cells)", pl.cells);
    void* const base = ctx->scratch.dod.p;
    long long* d_table = lay.table.at(base);
    double* d_gmin = lay.gmin.at(base);
    unsigned* counts = lay.counts.at(base);
    long long* starts = lay.starts.at(base);
    double* parts = lay.parts.at(base);
    unsigned long long* ncnt = lay.ncnt.at(base);
    unsigned char* state = lay.state.at(base);
    double* H = d_H ? d_H : lay.H.at(base);
    const DodTab T = pl.tab(d_table, d_gmin, P);
    hipStream_t s = (hipStream_t)stream;
    IM_HIP(ctx, hipMemcpyAsync(d_table, pl.table.data(), pl.table.size() * sizeof(long long), hipMemcpyHostToDevice, s));
    IM_HIP(ctx, hipMemcpyAsync(d_gmin, pl.gmin.data(), pl.gmin.size() * sizeof(double), hipMemcpyHostToDevice, s));
    IM_HIP(ctx, hipStreamSynchronize(s));          // the source is host memory of this call
    IM_HIP(ctx, hipMemsetAsync(ncnt, 0, (size_t)DOD_N_COUNTS * P * sizeof(unsigned long long), s));
    if (pl.cells) {
        IM_HIP(ctx, hipMemsetAsync(counts, 0, n_seg * sizeof(unsigned), s));
        if (pl.items) IM_LAUNCH(ctx, "dod_hist", s, launch(dod_hist_kernel, blocks_of(pl.items, 256), 256, 0, s, d_sorted_keys, pl.items, n_seg, counts));
        const DodCountScan cs{counts, n_seg, starts};
        IM_LAUNCH(ctx, "dod_starts_scan", s, launch_scan(cs, n_seg, lay.sums.at(base), starts + n_seg, s));
        IM_LAUNCH(ctx, "dod_cells", s, launch(dod_cells_kernel, blocks_of(pl.cells, 256), 256, 0, s, T, d_pts, d_perm, pl.items, (const long long*)starts,
                                              pl.cells, vert_dim, H, state));
        IM_LAUNCH(ctx, "dod_report", s, launch(dod_report_kernel, pl.chunks, 256, 0, s, T, (const double*)H, (const unsigned char*)state, parts, ncnt));
    }
    IM_LAUNCH(ctx, "dod_final", s, launch(dod_final_kernel, P, 192, 0, s, T, (const double*)parts, (const unsigned long long*)ncnt, step, d_report));
    IM_GUARD_CHECK(ctx, s, "im_dod_reduce");
    return 0;
}

int im_crop_polygon(im_ctx* ctx, const double* d_pts, long long n, int axis_x, int axis_y, const double* h_poly, int n_verts, int inside,
                    unsigned char* d_mask, long long* d_index, long long* d_count, void* stream) {
    IM_CHECK_CTX(ctx);
    if (n < 0 || n >= (1LL << 31)) return ctx->fail(-76, "im_crop_polygon: n must be 0..2^31-1");
    if (axis_x < 0 || axis_x > 2 || axis_y < 0 || axis_y > 2 || axis_x == axis_y) return ctx->fail(-76, "im_crop_polygon: the axes must be two of 0, 1, 2");
    if (n_verts < 3 || n_verts > DOD_MAX_VERTS) return ctx->fail(-76, "im_crop_polygon: a polygon has 3..1024 vertices");
    if (!h_poly || !d_count || (n && (!d_pts || !d_mask || !d_index))) return ctx->fail(-76, "im_crop_polygon: null pointer");
    for (int k = 0; k < 2 * n_verts; ++k)
        if (!std::isfinite(h_poly[k])) return ctx->fail(-76, "im_crop_polygon: a vertex is not finite");
    hipStream_t s = (hipStream_t)stream;
    IM_HIP(ctx, hipMemsetAsync(d_count, 0, sizeof(long long), s));
    if (n == 0) return 0;
    const CropScratch lay(n);
    IM_GROW(ctx, ctx->grow(ctx->scratch.dod, lay.bytes, "dod.scratch"), -22, "im_crop_polygon: allocation failed");
    void* const base = ctx->scratch.dod.p;
    double* d_poly = lay.poly.at(base);
    IM_HIP(ctx, hipMemcpyAsync(d_poly, h_poly, 2 * n_verts * sizeof(double), hipMemcpyHostToDevice, s));
    IM_HIP(ctx, hipStreamSynchronize(s));          // the source is host memory of this call
    IM_LAUNCH(ctx, "crop_polygon", s, launch(crop_polygon_kernel, blocks_of(n, 256), 256, 0, s, d_pts, n, axis_x, axis_y, (const double*)d_poly, n_verts, inside, d_mask));
    const MaskScan ms{d_mask, n, d_index};
    IM_LAUNCH(ctx, "crop_index_scan", s, launch_scan(ms, n, lay.sums.at(base), d_count, s));
    IM_GUARD_CHECK(ctx, s, "im_crop_polygon");
    return 0;
}

}  // extern "C"
