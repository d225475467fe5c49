// What the stage entry points that carve one scratch buffer lay into it, apart from the kernels so that a host compiler reads it too:
// tests/test_stage_plumbing_cpu.py pins every total (tests/test_dod_cpu.py those of dod.hip). Each is a Carve whose pieces are members; their order of declaration is the layout.
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
// im_dod_bounds (P = cells = chunks = 0), im_dod_keys and im_dod_reduce, E clouds, P pairs, `cells` cells and `chunks` chunks over the batch:
// table [E + 9 P + 5] (cloud offsets, per side the first item, segment and point, per pair w, h and the first chunk), gmin [2 P] (per pair
// min_x, min_y), bkeys [4 E],
// counts [2 cells], starts [2 cells + 1], sums [scan blocks], parts [3 chunks], ncnt [5 P], state [cells], H [own_h ? cells : 0]
struct DodScratch : Carve {
    Piece<long long> table; Piece<double> gmin; Piece<unsigned long long> bkeys; Piece<unsigned> counts; Piece<long long> starts, sums; Piece<double> parts;
    Piece<unsigned long long> ncnt; Piece<unsigned char> state; Piece<double> H;
    DodScratch(long long E, long long P, long long cells, long long chunks, bool own_h)
        : table(take<long long>(E + 9 * P + 5)), gmin(take<double>(2 * P)), bkeys(take<unsigned long long>(4 * E)), counts(take<unsigned>(2 * cells)),
          starts(take<long long>(2 * cells + 1)), sums(take<long long>(blocks_of(cells > 0 ? 2 * cells : 1, SCAN_THREADS))),
          parts(take<double>(3 * chunks)), ncnt(take<unsigned long long>(5 * P)), state(take<unsigned char>(cells)),
          H(take<double>(own_h ? cells : 0)) {}
};
struct CropScratch : Carve {          // im_crop_polygon, n > 0 points: the polygon [2 * 1024], sums [scan blocks]
    Piece<double> poly; Piece<long long> sums;
    explicit CropScratch(long long n) : poly(take<double>(2 * 1024)), sums(take<long long>(blocks_of(n, SCAN_THREADS))) {}
};

// im_voxel_bounds, im_voxel_keys and im_voxel_reduce, E clouds under G grids (1 or E), n points: table [2 (E + 1) + 3 G] (cloud offsets, the
// first key of every cloud, n_x n_y n_z per grid), grids [7 G], bkeys [6 E], seg [n + 1] (first sorted position of every voxel, then the end),
// sums [scan blocks of n + 1], total [1] (the number of voxels)
struct VoxelScratch : Carve {
    Piece<long long> table; Piece<double> grids; Piece<unsigned long long> bkeys; Piece<int> seg; Piece<long long> sums, total;
    VoxelScratch(long long E, long long G, long long n)
        : table(take<long long>(2 * (E + 1) + 3 * G)), grids(take<double>(7 * G)), bkeys(take<unsigned long long>(6 * E)), seg(take<int>(n + 1)),
          sums(take<long long>(blocks_of(n + 1, SCAN_THREADS))), total(take<long long>(1)) {}
};
// im_voxel_mesh, `items` = 8 V > 0 corner items: vstart [items + 1] (first sorted item of every vertex, then the end), vertex [items] (the
// vertex of local corner l of voxel v at 8 v + l), sums [scan blocks of items + 1]
struct VoxelMeshScratch : Carve {
    Piece<int> vstart, vertex; Piece<long long> sums;
    explicit VoxelMeshScratch(long long items) : vstart(take<int>(items + 1)), vertex(take<int>(items)), sums(take<long long>(blocks_of(items + 1, SCAN_THREADS))) {}
};

// im_mesh_select, V >= 0 vertices, T >= 0 triangles: tflag [T] (the triangle is kept), vflag [V] (the vertex is kept), ref [V] (a kept
// triangle references the vertex), sums [scan blocks of max(V, T, 1)]
struct MeshSelectScratch : Carve {
    Piece<unsigned char> tflag, vflag, ref; Piece<long long> sums;
    MeshSelectScratch(long long V, long long T)
        : tflag(take<unsigned char>(T)), vflag(take<unsigned char>(V)), ref(take<unsigned char>(V)),
          sums(take<long long>(blocks_of(V > T ? (V > 1 ? V : 1) : (T > 1 ? T : 1), SCAN_THREADS))) {}
};
// im_mesh_first_of_segment, n > 0 sorted items: head [n + 1] (the item at the first sorted position of every segment), segment [n] (the
// segment of every sorted position), sums [scan blocks of n], total [1]
struct MeshSegmentScratch : Carve {
    Piece<int> head, segment; Piece<long long> sums, total;
    explicit MeshSegmentScratch(long long n) : head(take<int>(n + 1)), segment(take<int>(n)), sums(take<long long>(blocks_of(n, SCAN_THREADS))), total(take<long long>(1)) {}
};
// im_mesh_in_hull, F > 0 facets: facets [4 F]
struct MeshHullScratch : Carve {
    Piece<double> facets;
    explicit MeshHullScratch(long long F) : facets(take<double>(4 * F)) {}
};
// im_mesh_sample_table, T > 0 triangles: area [T], cum [T] (inclusive cumulative quantised areas), sums [scan blocks of T], amax [1] (the
// bits of the largest area), total [1] (C)
struct MeshSampleScratch : Carve {
    Piece<double> area; Piece<long long> cum, sums; Piece<unsigned long long> amax; Piece<long long> total;
    explicit MeshSampleScratch(long long T) : area(take<double>(T)), cum(take<long long>(T)), sums(take<long long>(blocks_of(T, SCAN_THREADS))),
          amax(take<unsigned long long>(1)), total(take<long long>(1)) {}
};
// im_icp_accumulate and im_icp_finish, `chunks` >= 0 chunks of source points: parts [32 * max(chunks, 1)], one partial of 32 sums per chunk
constexpr int ICP_PART = 32;
struct IcpScratch : Carve {
    Piece<double> parts;
    explicit IcpScratch(long long chunks) : parts(take<double>(ICP_PART * (chunks > 0 ? chunks : 1))) {}
};
// im_ba_accumulate .. im_ba_decide, E >= 1 epochs of M >= 0 points in all: an epoch's chunks start at slot off[e] / BA_CHUNK + e, so
// slots = M / 256 + E + 1 hold every epoch's. parts [448 * slots], cparts [slots], keep [95 * max(M, 1)]
constexpr int BA_PART = 448, BA_KEPT = 95, BA_SLOT_POINTS = 256;
struct BaScratch : Carve {
    Piece<double> parts, cparts, keep;
    long long slots;
    BaScratch(long long E, long long M) : parts(take<double>(BA_PART * (M / BA_SLOT_POINTS + E + 1))), cparts(take<double>(M / BA_SLOT_POINTS + E + 1)),
          keep(take<double>(BA_KEPT * (M > 0 ? M : 1))), slots(M / BA_SLOT_POINTS + E + 1) {}
};
// im_dense_cloud, n = h w > 0 pixels: sums [scan blocks of n]
struct DenseCloudScratch : Carve {
    Piece<long long> sums;
    explicit DenseCloudScratch(long long n) : sums(take<long long>(blocks_of(n, SCAN_THREADS))) {}
};
// im_depth_components, n = h w > 0 pixels: cnt [n], the pixels of a component counted on its root's slot
struct DepthComponentsScratch : Carve {
    Piece<int> cnt;
    explicit DepthComponentsScratch(long long n) : cnt(take<int>(n)) {}
};
// im_depth_fill_holes, n = h w > 0 pixels: lo [n], hi [n], the least and the greatest plane around a hole on its root's slot (hi with the border flag)
struct DepthHolesScratch : Carve {
    Piece<int> lo, hi;
    explicit DepthHolesScratch(long long n) : lo(take<int>(n)), hi(take<int>(n)) {}
};

}  // namespace im
