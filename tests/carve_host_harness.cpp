// Host build of csrc/carve.h and csrc/stage_scratch.h for tests/test_stage_plumbing_cpu.py: the grid and alignment helpers, a Carve of n
// pieces, and the bytes each of the five carving entry points asks its context for.
#include "stage_scratch.h"

extern "C" long long carve_blocks_of(long long n, int per) { return im::blocks_of(n, per); }
extern "C" unsigned long long carve_up256(unsigned long long b) { return im::up256(b); }

// pieces of counts[i] elements of elem_bytes[i] (1, 4 or 8) bytes each, then `slack` bytes: offsets[i] out, the total returned
extern "C" unsigned long long carve_layout(int n, const unsigned long long* counts, const int* elem_bytes, unsigned long long slack,
                                           unsigned long long* offsets) {
    im::Carve c;
    for (int i = 0; i < n; ++i)
        offsets[i] = elem_bytes[i] == 1 ? c.take<char>(counts[i]).offset
                   : elem_bytes[i] == 4 ? c.take<int>(counts[i]).offset : c.take<long long>(counts[i]).offset;
    c.bytes += slack;
    return c.bytes;
}

// a piece's pointer is its offset behind the base
extern "C" long long carve_at(unsigned long long first_count, unsigned long long second_count) {
    im::Carve c;
    c.take<int>(first_count);
    const auto p = c.take<double>(second_count);
    char base[1];
    return reinterpret_cast<char*>(p.at(base)) - base;
}

extern "C" unsigned long long carve_dsm_group_mean(long long n) { return im::DsmGroupScratch(n).bytes; }
extern "C" unsigned long long carve_dsm_rasterize(long long cells, long long T) { return im::DsmRasterScratch(cells, T).bytes; }
extern "C" unsigned long long carve_binned_stats(long long n, long long n_seg) { return im::BinnedStatsScratch(n, n_seg).bytes; }
extern "C" unsigned long long carve_tracked_points(long long M) { return im::TrackedPointsScratch(M).bytes; }
extern "C" unsigned long long carve_knn_self(long long n) { return im::KnnSortedScratch(n).bytes; }
