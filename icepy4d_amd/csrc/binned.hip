// Velocity fields: binned statistics and the tracked-point table (`src/icepy4d/utils/binned_stats.py`: `compute_binned_stats2D / 3D`
// over `scipy.stats.binned_statistic_2d / _dd`; `utils/tracking_features_utils.py`: `tracked_points_time_series`, `tracked_dict_to_df`).
// The reference digitizes, then sums with np.bincount and takes medians from one lexsort of all points per value column. Here one stable
// sort of the points by (set, cell) - torch's, plumbing - makes every cell a contiguous segment in input order; everything else is below.
//
//   bin_cells_kernel        one thread per point: np.digitize per dimension (binary search over the edge doubles), scipy's
//                           rightmost-edge rule (np.around: multiply, rint, divide), the sort key set * cells + cell (outside: sets * cells)
//   bin_hist_kernel         points per cell (integer atomics: order-free); scan_*_kernel (scan.h) turn them into segment offsets and list
//                           the cells with more than BIN_GROUP points
//   bin_basic_kernel        one thread per (cell, column): count, sum, mean, std, min, max in segment order = np.bincount's order
//   bin_median_group_kernel a group of G lanes per (cell, column), G = 8 (several cells per wave) or 64: rank of every value by
//                           counting, the two middle ranks combined with a butterfly
//   bin_median_block_kernel one block per (cell, column) with more than 64 points: exact radix select (eight 8-bit passes, LDS histogram)
//                           over the keys staged in LDS (<= BIN_LDS_CAP points) or gathered from global memory (any size)
//   track_*                 ids sorted by (id, epoch): id starts by a scan, then per id the first / last epoch inside the volume, the
//                           velocities and the filters; a second scan compacts the kept rows in ascending id
// float64 throughout, contraction off wherever the reference's rounding is restated. Medians order keys as numbers (-0.0 == +0.0, NaN
// last) with ties to the lower input index, which is scipy's stable lexsort; only for a zero does the tie decide the result's bits.
#include <climits>
#include <cmath>

#include "common.h"
#include "ctx.h"
#include "stage_scratch.h"

namespace im {
namespace {

#include "scan.h"

constexpr int BIN_LDS_CAP = 4096;     // cells up to this size are selected from LDS (32 KB of keys), larger ones from global memory
constexpr unsigned long long KEY_ZERO = 0x8000000000000000ull, KEY_NAN = ~0ull;
enum { ST_COUNT, ST_SUM, ST_MEAN, ST_STD, ST_MIN, ST_MAX, ST_MEDIAN, ST_N };

struct BinGrid {
    const double* edges[3];   // device, ascending
    int ne[3];                // edges per dimension (bins + 1)
    double scale[3];          // 10 ** |decimal| of scipy's rounding
    int mode[3];              // sign of decimal: np.around multiplies first (> 0), divides first (< 0) or only rounds (0)
    int D;
};

__device__ __forceinline__ int digitize(const double* __restrict__ e, int n, double x) {   // np.digitize(x, e): edges <= x; NaN -> n
    if (x != x) return n;
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ double around(double x, double s, int mode) {
#pragma clang fp contract(off)
    if (mode == 0) return rint(x);
    return mode > 0 ? rint(x * s) / s : rint(x / s) * s;
}

__global__ __launch_bounds__(256) void bin_cells_kernel(BinGrid g, const double* __restrict__ pts, long long n, const long long* __restrict__ offsets,
                                                        int E, long long cells, long long* __restrict__ key) {
#pragma clang fp contract(off)
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool inside = true;
    long long cell = 0;
    for (int d = 0; d < g.D; ++d) {
        const double x = pts[i * g.D + d], last = g.edges[d][g.ne[d] - 1];
        int b = digitize(g.edges[d], g.ne[d], x);
        if (x >= last && around(x, g.scale[d], g.mode[d]) == around(last, g.scale[d], g.mode[d])) --b;
        inside = inside && b >= 1 && b <= g.ne[d] - 1;
        cell = cell * (g.ne[d] - 1) + (b - 1);
    }
    int lo = 0, hi = E;                      // the set of point i: offsets[set] <= i < offsets[set + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    key[i] = inside ? lo * cells + cell : E * cells;
}

__global__ __launch_bounds__(256) void bin_hist_kernel(const long long* __restrict__ skey, long long n, long long n_seg, unsigned* __restrict__ counts) {
    const long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (j < n && skey[j] < n_seg) atomicAdd(&counts[skey[j]], 1u);
}

struct CountScan {            // points per cell -> first sorted position of each cell
    const unsigned* counts; long long n_seg; long long* starts;
    __device__ long long count(long long g) const { return g < n_seg ? counts[g] : 0; }
    __device__ void write(long long g, long long pos) const { if (g < n_seg) starts[g] = pos; }
};
struct LargeScan {            // the cells that need more than one lane group
    const long long* starts; long long n_seg; long long* list;
    __device__ long long count(long long g) const { return g < n_seg && starts[g + 1] - starts[g] > BIN_GROUP ? 1 : 0; }
    __device__ void write(long long g, long long pos) const { if (count(g)) list[pos] = g; }
};

struct StatArgs {
    const long long* starts;  // [n_seg + 1]
    const long long* perm;    // [N] points in (set, cell) order
    const double* vals;       // [V][N]
    long long N, n_seg, C;
    int E, V;
    int slot[ST_N];           // plane of the output that receives the statistic, -1: not asked for
    double* out;              // [slots][E][V][C]
    __device__ double* at(int st, long long g, int v) const {
        const long long e = g / C;
        return out + ((((long long)slot[st] * E + e) * V + v) * C + (g - e * C));
    }
};

__device__ __forceinline__ double nan64() { return __longlong_as_double(0x7ff8000000000000ll); }

__global__ __launch_bounds__(256) void bin_basic_kernel(StatArgs a) {
#pragma clang fp contract(off)
    const long long it = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (it >= a.n_seg * a.V) return;
    const int v = (int)(it / a.n_seg);
    const long long g = it - v * a.n_seg, j0 = a.starts[g], j1 = a.starts[g + 1];
    const double* col = a.vals + v * a.N;
    const double cnt = (double)(j1 - j0);
    double s = 0.0, mn = nan64(), mx = nan64();
    bool any_nan = false;
    for (long long j = j0; j < j1; ++j) {            // np.bincount's order: the input order
        const double x = col[a.perm[j]];
        s += x;
        if (x != x) { any_nan = true; continue; }
        if (!(mn == mn) || x < mn) mn = x;
        if (!(mx == mx) || x > mx) mx = x;
    }
    if (a.slot[ST_COUNT] >= 0) *a.at(ST_COUNT, g, v) = cnt;
    if (a.slot[ST_SUM] >= 0) *a.at(ST_SUM, g, v) = s;
    if (a.slot[ST_MEAN] >= 0) *a.at(ST_MEAN, g, v) = j1 > j0 ? s / cnt : nan64();
    if (a.slot[ST_MIN] >= 0) *a.at(ST_MIN, g, v) = mn;
    if (a.slot[ST_MAX] >= 0) *a.at(ST_MAX, g, v) = any_nan ? nan64() : mx;   // scipy: argsort puts NaN last, the last write wins
    if (a.slot[ST_STD] >= 0) {
        const double mu = s / cnt;
        double q = 0.0;
        for (long long j = j0; j < j1; ++j) {
            const double x = col[a.perm[j]];
            q += (x - mu) * (x - mu);
        }
        *a.at(ST_STD, g, v) = j1 > j0 ? sqrt(q / cnt) : nan64();
    }
}

// ascending unsigned order == ascending value; -0.0 folded into +0.0, every NaN last (np.lexsort's order of a float64 key)
__device__ __forceinline__ unsigned long long med_key(double d) {
    if (d != d) return KEY_NAN;
    unsigned long long u = (unsigned long long)__double_as_longlong(d);
    if (u == KEY_ZERO) u = 0;
    return (u & KEY_ZERO) ? ~u : (u | KEY_ZERO);
}
__device__ __forceinline__ double key_value(unsigned long long k) {      // not for KEY_ZERO: its sign is the element's
    if (k == KEY_NAN) return nan64();
    return __longlong_as_double((long long)((k & KEY_ZERO) ? (k ^ KEY_ZERO) : ~k));
}
__device__ __forceinline__ double median_of(double lo, double hi) {
#pragma clang fp contract(off)
    return (lo + hi) / 2.0;
}

// G lanes per (cell, column). list == nullptr: every cell, those of 0 .. BIN_GROUP points are done (an empty one gets NaN);
// otherwise the listed cells, those of up to G points are done.
template <int G>
__global__ __launch_bounds__(256) void bin_median_group_kernel(StatArgs a, const long long* __restrict__ list, const long long* __restrict__ n_list) {
    const int l = threadIdx.x & (G - 1);
    const long long n_cells = list ? *n_list : a.n_seg, items = n_cells * a.V;
    const long long groups = (long long)gridDim.x * (256 / G);
    for (long long it = blockIdx.x * (long long)(256 / G) + threadIdx.x / G; it < items; it += groups) {
        const int v = (int)(it / n_cells);
        const long long c = it - v * n_cells, g = list ? list[c] : c;
        const long long j0 = a.starts[g];
        const int n = (int)min(a.starts[g + 1] - j0, (long long)(G + 1));
        if (n > G || (list && n <= BIN_GROUP)) continue;          // the whole group leaves together
        double x = 0.0;
        if (l < n) x = a.vals[v * a.N + a.perm[j0 + l]];
        const unsigned long long key = l < n ? med_key(x) : KEY_NAN;
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const unsigned long long o = __shfl(key, j, G);
            rank += (o < key || (o == key && j < l)) ? 1 : 0;
        }
        unsigned long long lo = (l < n && rank == (n - 1) / 2) ? (unsigned long long)__double_as_longlong(x) : 0;
        unsigned long long hi = (l < n && rank == n / 2) ? (unsigned long long)__double_as_longlong(x) : 0;
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) {
            lo |= __shfl_xor(lo, o, G);
            hi |= __shfl_xor(hi, o, G);
        }
        if (l == 0) *a.at(ST_MEDIAN, g, v) = n ? median_of(__longlong_as_double((long long)lo), __longlong_as_double((long long)hi)) : nan64();
    }
}

struct BlockSel {             // LDS of bin_median_block_kernel
    unsigned long long keys[BIN_LDS_CAP];
    unsigned hist[256];
    unsigned long long next;  // the smallest key above the selected one
    long long pos;
    int bin; unsigned below, equal;
};

// One block per listed (cell, column) of more than 64 points. Rank k1 = (n - 1) / 2 by radix select: per pass the histogram of the next
// eight key bits among the keys that share the prefix found so far. Rank k2 = n / 2 is the same key when the tie group reaches it, else
// the smallest key above. A zero key takes its sign from the element: the r-th zero of the segment in input order.
__global__ __launch_bounds__(256) void bin_median_block_kernel(StatArgs a, const long long* __restrict__ list, const long long* __restrict__ n_list) {
    __shared__ BlockSel sh;
    const int t = threadIdx.x;
    const long long n_cells = *n_list, items = n_cells * a.V;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int v = (int)(it / n_cells);
        const long long g = list[it - v * n_cells], j0 = a.starts[g], n = a.starts[g + 1] - j0;
        if (n <= IM_WAVE) continue;
        const double* col = a.vals + v * a.N;
        const long long* perm = a.perm + j0;
        const bool staged = n <= BIN_LDS_CAP;
        __syncthreads();                          // the previous item is done with the LDS
        if (staged)
            for (long long i = t; i < n; i += 256) sh.keys[i] = med_key(col[perm[i]]);
        auto key_at = [&](long long i) { return staged ? sh.keys[i] : med_key(col[perm[i]]); };
        unsigned long long prefix = 0;
        long long kk = (n - 1) / 2;
        unsigned equal = 0;
        for (int pass = 7; pass >= 0; --pass) {
            const int shift = 8 * pass;
            sh.hist[t] = 0;
            if (t == 0) sh.next = KEY_NAN;
            __syncthreads();
            for (long long i = t; i < n; i += 256) {
                const unsigned long long k = key_at(i);
                if (pass == 7 || (k >> (shift + 8)) == prefix) atomicAdd(&sh.hist[(k >> shift) & 255], 1u);
            }
            __syncthreads();
            if (t == 0) {
                unsigned cum = 0;
                int b = 0;
                for (; b < 255; ++b) {
                    if (kk < (long long)cum + sh.hist[b]) break;
                    cum += sh.hist[b];
                }
                sh.bin = b; sh.below = cum; sh.equal = sh.hist[b];
            }
            __syncthreads();
            prefix = (prefix << 8) | (unsigned)sh.bin;
            kk -= sh.below;
            equal = sh.equal;
            __syncthreads();
        }
        // prefix = the key of rank k1, kk = its rank among the `equal` elements with that key
        const unsigned long long K1 = prefix;
        const bool even = (n & 1) == 0, same = !even || kk + 1 < (long long)equal;
        if (!same) {
            for (long long i = t; i < n; i += 256) {
                const unsigned long long k = key_at(i);
                if (k > K1) atomicMin(&sh.next, k);
            }
            __syncthreads();
        }
        const unsigned long long K2 = same ? K1 : sh.next;
        const long long r1 = kk, r2 = !even ? kk : (same ? kk + 1 : 0);
        double val[2];
        for (int w = 0; w < 2; ++w) {
            const unsigned long long K = w ? K2 : K1;
            const long long r = w ? r2 : r1;
            if (K != KEY_ZERO) { val[w] = key_value(K); continue; }       // uniform over the block
            const long long chunk = (n + 255) / 256, i0 = min(n, t * chunk), i1 = min(n, i0 + chunk);
            unsigned c = 0;
            for (long long i = i0; i < i1; ++i) c += key_at(i) == KEY_ZERO;
            if (t == 0) sh.pos = 0;
            __syncthreads();
            sh.hist[t] = c;
            __syncthreads();
            long long before = 0;
            for (int u = 0; u < t; ++u) before += sh.hist[u];
            if (before <= r && r < before + c) {
                long long left = r - before;
                for (long long i = i0; i < i1; ++i)
                    if (key_at(i) == KEY_ZERO && left-- == 0) { sh.pos = i; break; }
            }
            __syncthreads();
            val[w] = col[perm[sh.pos]];
        }
        if (t == 0) *a.at(ST_MEDIAN, g, v) = median_of(val[0], val[1]);
    }
}

// ---- tracked-point table -----------------------------------------------------------------------------------------------------
struct TrackArgs {
    const long long* sid;      // [M] track ids, ascending (stable: rows of an id stay in epoch order)
    const long long* perm;     // [M] the row of the concatenated epochs behind every sorted position
    long long M;
    const long long* offsets;  // [E + 1] rows of every epoch
    int E;
    const double* xyz;         // [M][3]
    const long long* days;     // [E]
    int has_vol; double vol[6];                 // min x y z, max x y z (inclusive)
    long long min_eps;
    int has_min_dt; long long min_dt;
    int has_lim[3]; double lim[6];              // lo, hi per axis: lo <= v < hi
    const double* img; int n_cams;              // [n_cams][M][2]
    long long* starts; const long long* n_ids; long long* pre;   // scratch: id starts, number of ids, row index before the filters
    long long* oi; double* od;                  // [6][M], [13 + 4 n_cams][M]
    unsigned char* member;                      // [M] the row belongs to the series of a tracked id
};

struct IdScan {
    TrackArgs a;
    __device__ long long count(long long j) const { return j < a.M && (j == 0 || a.sid[j] != a.sid[j - 1]) ? 1 : 0; }
    __device__ void write(long long j, long long pos) const { if (count(j)) a.starts[pos] = j; }
};

struct Track { long long num, ini, fin, row_ini, row_fin; };

__device__ __forceinline__ int epoch_of(const TrackArgs& a, long long row) {
    int lo = 0, hi = a.E;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.offsets[mid] <= row) lo = mid; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ bool in_volume(const TrackArgs& a, long long row) {
    if (!a.has_vol) return true;
    const double* p = a.xyz + 3 * row;
    return a.vol[0] <= p[0] && p[0] <= a.vol[3] && a.vol[1] <= p[1] && p[1] <= a.vol[4] && a.vol[2] <= p[2] && p[2] <= a.vol[5];
}
// the epochs of id i inside the volume; true when the id is tracked (`len(epoch_list) >= min_tracked_epoches`)
__device__ bool track_of(const TrackArgs& a, long long i, Track& t, bool mark) {
    const long long j0 = a.starts[i], j1 = i + 1 < *a.n_ids ? a.starts[i + 1] : a.M;
    t.num = 0;
    for (long long j = j0; j < j1; ++j) {
        const long long row = a.perm[j];
        const int ep = epoch_of(a, row);
        if (!in_volume(a, row)) continue;
        if (!t.num) { t.ini = ep; t.row_ini = row; }
        t.fin = ep; t.row_fin = row;
        ++t.num;
    }
    const bool tracked = t.num >= 1 && t.num >= a.min_eps;
    if (mark && tracked)
        for (long long j = j0; j < j1; ++j)
            if (in_volume(a, a.perm[j])) a.member[a.perm[j]] = 1;
    return tracked;
}

struct TrackedScan {          // position of a tracked id among the tracked ids: the DataFrame's index before the filters
    TrackArgs a;
    __device__ long long count(long long i) const { Track t; return i < *a.n_ids && track_of(a, i, t, false) ? 1 : 0; }
    __device__ void write(long long i, long long pos) const { Track t; if (i < *a.n_ids && track_of(a, i, t, true)) a.pre[i] = pos; }
};

struct KeptRowScan {          // the rows that pass `tracked_dict_to_df`'s filters, compacted in ascending id
    TrackArgs a;
    __device__ bool row(long long i, Track& t, long long& dt, double* c) const {
#pragma clang fp contract(off)
        if (i >= *a.n_ids || !track_of(a, i, t, false)) return false;
        const double* p0 = a.xyz + 3 * t.row_ini;
        const double* p1 = a.xyz + 3 * t.row_fin;
        dt = a.days[t.fin] - a.days[t.ini];
        for (int k = 0; k < 3; ++k) {
            c[k] = p0[k]; c[3 + k] = p1[k];
            c[6 + k] = p1[k] - p0[k];
            c[9 + k] = c[6 + k] / (double)dt;
        }
        c[12] = sqrt((c[9] * c[9] + c[10] * c[10]) + c[11] * c[11]);      // np.linalg.norm(axis=1) of three columns
        bool keep = !a.has_min_dt || dt >= a.min_dt;
        for (int k = 0; k < 3; ++k)
            if (a.has_lim[k]) keep = keep && c[9 + k] >= a.lim[2 * k] && c[9 + k] < a.lim[2 * k + 1];
        return keep;
    }
    __device__ long long count(long long i) const { Track t; long long dt; double c[13]; return row(i, t, dt, c) ? 1 : 0; }
    __device__ void write(long long i, long long pos) const {
        Track t; long long dt; double c[13];
        if (!row(i, t, dt, c)) return;
        const long long M = a.M;
        a.oi[pos] = a.sid[a.starts[i]]; a.oi[M + pos] = t.num; a.oi[2 * M + pos] = t.ini; a.oi[3 * M + pos] = t.fin;
        a.oi[4 * M + pos] = dt; a.oi[5 * M + pos] = a.pre[i];
        for (int k = 0; k < 13; ++k) a.od[k * M + pos] = c[k];
        for (int cam = 0; cam < a.n_cams; ++cam) {
            const double* q0 = a.img + 2 * (cam * M + t.row_ini);
            const double* q1 = a.img + 2 * (cam * M + t.row_fin);
            double* o = a.od + (13 + 4 * cam) * M + pos;
            o[0] = q0[0]; o[M] = q0[1]; o[2 * M] = q1[0]; o[3 * M] = q1[1];
        }
    }
};

}  // namespace
}  // namespace im

using namespace im;

extern "C" int im_binned_lds_capacity(void) { return BIN_LDS_CAP; }

extern "C" int im_binned_cells(im_ctx* ctx, const double* d_pts, long long n, int dims, const double* d_edges, const int32_t* h_n_edges,
                               const double* h_scale, const int32_t* h_mode, const long long* d_offsets, int n_sets, long long* d_key,
                               void* stream) {
    IM_CHECK_CTX(ctx);
    if (dims < 1 || dims > 3 || !d_edges || !h_n_edges || !h_scale || !h_mode || !d_offsets || n_sets < 1 || n < 0 || n >= INT_MAX)
        return ctx->fail(-72, "im_binned_cells: bad arguments");
    BinGrid g{};
    g.D = dims;
    long long cells = 1;
    const double* e = d_edges;
    for (int d = 0; d < dims; ++d) {
        if (h_n_edges[d] < 2 || !(h_scale[d] > 0.0)) return ctx->fail(-72, "im_binned_cells: dimension %d needs two edges or more", d);
        g.edges[d] = e; g.ne[d] = h_n_edges[d]; g.scale[d] = h_scale[d]; g.mode[d] = h_mode[d];
        e += h_n_edges[d];
        cells *= h_n_edges[d] - 1;
        if (cells * n_sets >= (1LL << 40)) return ctx->fail(-72, "im_binned_cells: too many cells");
    }
    if (!n) return 0;
    if (!d_pts || !d_key) return ctx->fail(-72, "im_binned_cells: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    IM_LAUNCH(ctx, "bin_cells", s, launch(bin_cells_kernel, blocks_of(n, 256), 256, 0, s, g, d_pts, n, d_offsets, n_sets, cells, d_key));
    IM_GUARD_CHECK(ctx, s, "im_binned_cells");
    return 0;
}

extern "C" int im_binned_stats(im_ctx* ctx, const long long* d_sorted_key, const long long* d_perm, long long n, int n_sets, long long cells,
                               const double* d_values, int n_values, const int32_t* h_slots, double* d_out, void* stream) {
    IM_CHECK_CTX(ctx);
    if (n < 0 || n >= INT_MAX || n_sets < 1 || cells < 1 || n_values < 1 || !h_slots || !d_out || (n && (!d_sorted_key || !d_perm || !d_values)))
        return ctx->fail(-72, "im_binned_stats: bad arguments");
    const long long n_seg = cells * n_sets, items = n_seg * n_values;
    if (n_seg >= (1LL << 40) || blocks_of(items, 256 / BIN_GROUP) >= INT_MAX) return ctx->fail(-72, "im_binned_stats: too many cells");
    StatArgs a{};
    bool basic = false;
    int n_slots = 0;
    for (int k = 0; k < ST_N; ++k) {
        a.slot[k] = h_slots[k];
        if (h_slots[k] >= ST_N) return ctx->fail(-72, "im_binned_stats: bad output plane");
        if (h_slots[k] >= 0) { ++n_slots; basic = basic || k != ST_MEDIAN; }
    }
    if (!n_slots) return 0;
    hipStream_t s = (hipStream_t)stream;
    const BinnedStatsScratch lay(n, n_seg);
    IM_GROW(ctx, ctx->grow(ctx->scratch.binned, lay.bytes, "binned.scratch"), -71, "im_binned_stats: out of device memory (%lld cells)", n_seg);
    void* const sc = ctx->scratch.binned.p;
    unsigned* counts = lay.counts.at(sc);
    long long* starts = lay.starts.at(sc);
    long long* list = lay.list.at(sc);
    long long* sums = lay.sums.at(sc);
    long long* n_list = lay.n_list.at(sc);
    IM_HIP(ctx, hipMemsetAsync(counts, 0, n_seg * sizeof(unsigned), s));
    if (n) IM_LAUNCH(ctx, "bin_hist", s, launch(bin_hist_kernel, blocks_of(n, 256), 256, 0, s, d_sorted_key, n, n_seg, counts));
    const CountScan cs{counts, n_seg, starts};
    IM_LAUNCH(ctx, "bin_offsets_scan", s, launch_scan(cs, n_seg, sums, starts + n_seg, s));
    a.starts = starts; a.perm = d_perm; a.vals = d_values; a.N = n; a.n_seg = n_seg; a.C = cells; a.E = n_sets; a.V = n_values; a.out = d_out;
    if (basic) IM_LAUNCH(ctx, "bin_basic", s, launch(bin_basic_kernel, blocks_of(items, 256), 256, 0, s, a));
    if (a.slot[ST_MEDIAN] >= 0) {
        const LargeScan ls{starts, n_seg, list};
        IM_LAUNCH(ctx, "bin_large_scan", s, launch_scan(ls, n_seg, sums, n_list, s));
        int cus = 0;
        IM_HIP(ctx, device_cu_count(&cus));
        const long long n_large_max = n / (BIN_GROUP + 1);       // the listed cells hold more than BIN_GROUP points each
        IM_LAUNCH(ctx, "bin_median_8", s, launch(bin_median_group_kernel<BIN_GROUP>, std::min(blocks_of(items, 256 / BIN_GROUP), cus * 64LL), 256, 0, s, a,
                                                 (const long long*)nullptr, (const long long*)nullptr));
        if (n_large_max) {
            const long long large_items = n_large_max * n_values;
            IM_LAUNCH(ctx, "bin_median_64", s, launch(bin_median_group_kernel<IM_WAVE>, std::min(blocks_of(large_items, 256 / IM_WAVE), cus * 32LL), 256, 0, s, a,
                                                      (const long long*)list, (const long long*)n_list));
            if (n > IM_WAVE)
                IM_LAUNCH(ctx, "bin_median_block", s, launch(bin_median_block_kernel, std::min((n / (IM_WAVE + 1)) * n_values, cus * 8LL), 256, 0, s, a,
                                                             (const long long*)list, (const long long*)n_list));
        }
    }
    IM_GUARD_CHECK(ctx, s, "im_binned_stats");
    return 0;
}

extern "C" int im_tracked_points(im_ctx* ctx, const long long* d_sorted_ids, const long long* d_perm, long long n_rows, const long long* d_offsets,
                                 int n_epochs, const double* d_xyz, const long long* d_days, const double* h_volume, long long min_tracked_epochs,
                                 const long long* h_min_dt, const double* h_vlims, const double* d_image_points, int n_cams, long long* d_int_cols,
                                 double* d_f64_cols, unsigned char* d_member, long long* d_n_rows, void* stream) {
    IM_CHECK_CTX(ctx);
    if (n_rows < 0 || n_rows >= INT_MAX || n_epochs < 1 || !d_offsets || !d_days || !h_vlims || n_cams < 0 || (n_cams && !d_image_points) || !d_n_rows)
        return ctx->fail(-72, "im_tracked_points: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    IM_HIP(ctx, hipMemsetAsync(d_n_rows, 0, sizeof(long long), s));
    if (!n_rows) return 0;
    if (!d_sorted_ids || !d_perm || !d_xyz || !d_int_cols || !d_f64_cols || !d_member) return ctx->fail(-72, "im_tracked_points: bad arguments");
    const long long M = n_rows;
    const TrackedPointsScratch lay(M);
    IM_GROW(ctx, ctx->grow(ctx->scratch.binned, lay.bytes, "binned.scratch"), -71, "im_tracked_points: out of device memory");
    void* const sc = ctx->scratch.binned.p;
    TrackArgs a{};
    a.sid = d_sorted_ids; a.perm = d_perm; a.M = M; a.offsets = d_offsets; a.E = n_epochs; a.xyz = d_xyz; a.days = d_days;
    a.has_vol = h_volume != nullptr;
    for (int k = 0; k < 6 && h_volume; ++k) a.vol[k] = h_volume[k];
    a.min_eps = min_tracked_epochs;
    a.has_min_dt = h_min_dt != nullptr;
    a.min_dt = h_min_dt ? *h_min_dt : 0;
    for (int k = 0; k < 3; ++k) {                      // an axis without limits: lo = NaN
        a.has_lim[k] = h_vlims[2 * k] == h_vlims[2 * k];
        a.lim[2 * k] = h_vlims[2 * k]; a.lim[2 * k + 1] = h_vlims[2 * k + 1];
    }
    a.img = d_image_points; a.n_cams = n_cams;
    a.starts = lay.starts.at(sc);
    a.pre = lay.pre.at(sc);
    long long* sums = lay.sums.at(sc);
    long long* n_ids = lay.n_ids.at(sc);
    long long* n_tracked = n_ids + 1;
    a.n_ids = n_ids;
    a.oi = d_int_cols; a.od = d_f64_cols; a.member = d_member;
    IM_HIP(ctx, hipMemsetAsync(d_member, 0, M, s));
    IM_LAUNCH(ctx, "track_id_scan", s, launch_scan(IdScan{a}, M, sums, n_ids, s));
    IM_LAUNCH(ctx, "track_index_scan", s, launch_scan(TrackedScan{a}, M, sums, n_tracked, s));
    IM_LAUNCH(ctx, "track_row_scan", s, launch_scan(KeptRowScan{a}, M, sums, d_n_rows, s));
    IM_GUARD_CHECK(ctx, s, "im_tracked_points");
    return 0;
}
