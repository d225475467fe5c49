// What the entry points of csrc/poisson.hip lay into their scratch buffer (carve.h), apart from the kernels so that a host compiler reads
// it too (tests/poisson_host_harness.cpp). The fields themselves are the caller's memory.
#pragma once
#include "carve.h"
#include "stage_scratch.h"

namespace im {

// im_poisson_census and im_poisson_extract at `nodes` = (2^depth + 1)^3 nodes: sums [scan blocks of nodes] (the cells are fewer), total [1]
struct PoissonScanScratch : Carve {
    Piece<long long> sums, total;
    explicit PoissonScanScratch(long long nodes) : sums(take<long long>(blocks_of(nodes, SCAN_THREADS))), total(take<long long>(1)) {}
};

}  // namespace im
