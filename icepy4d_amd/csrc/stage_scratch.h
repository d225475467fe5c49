// What the stage entry points that carve one scratch buffer lay into it, apart from the kernels so that a host compiler reads it too:
// tests/test_stage_plumbing_cpu.py pins every total. Each is a Carve whose pieces are members; their order of declaration is the layout.
#pragma once
#include "carve.h"

namespace im {

constexpr int SCAN_THREADS = 256;     // the block of scan.h's kernels: a scan over n items keeps blocks_of(n, SCAN_THREADS) partial sums
constexpr int BIN_GROUP = 8;          // binned.hip: cells up to this size take eight lanes each, the larger ones are listed

struct DsmGroupScratch : Carve {      // im_dsm_group_mean, n > 0 points: sums [scan blocks], starts [n], first [2]
    Piece<long long> sums, starts; Piece<int> first;
    explicit DsmGroupScratch(long long n) : sums(take<long long>(blocks_of(n, SCAN_THREADS))), starts(take<long long>(n)), first(take<int>(2)) {}
};
struct DsmRasterScratch : Carve {     // im_dsm_rasterize, cells > 0, T >= 0 triangles: win [cells], offs [max(T, 1)], sums [scan blocks], total [1]
    Piece<int> win; Piece<long long> offs, sums, total;
    DsmRasterScratch(long long cells, long long T) : win(take<int>(cells)), offs(take<long long>(T > 0 ? T : 1)),
          sums(take<long long>(blocks_of(T > 0 ? T : 1, SCAN_THREADS))), total(take<long long>(1)) {}
};
struct BinnedStatsScratch : Carve {   // im_binned_stats, n >= 0 points, n_seg > 0 cells: counts [n_seg], starts [n_seg + 1], list [n / 8 + 1], sums, n_list [1]
    Piece<unsigned> counts; Piece<long long> starts, list, sums, n_list;
    BinnedStatsScratch(long long n, long long n_seg) : counts(take<unsigned>(n_seg)), starts(take<long long>(n_seg + 1)),
          list(take<long long>(n / BIN_GROUP + 1)), sums(take<long long>(blocks_of(n_seg, SCAN_THREADS))), n_list(take<long long>(1)) {}
};
struct TrackedPointsScratch : Carve { // im_tracked_points, M > 0 rows: starts [M], pre [M], sums [scan blocks], n_ids [2], then 256 bytes of slack no piece uses
    Piece<long long> starts, pre, sums, n_ids;
    explicit TrackedPointsScratch(long long M) : starts(take<long long>(M)), pre(take<long long>(M)),
          sums(take<long long>(blocks_of(M, SCAN_THREADS))), n_ids(take<long long>(2)) { bytes += 256; }
};
struct KnnSortedScratch : Carve {     // im_knn_self, n > 0 points: the cloud in cell order, x y z [n] each and the original indices [n]
    Piece<double> x, y, z; Piece<int> idx;
    explicit KnnSortedScratch(long long n) : x(take<double>(n)), y(take<double>(n)), z(take<double>(n)), idx(take<int>(n)) {}
};

}  // namespace im
