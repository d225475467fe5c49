// Exclusive scans over per-item counts, shared by dsm.hip (group starts, row spans of the triangles) and binned.hip (cell offsets, large
// cells, track ids, row compaction). A scan is described by a small struct S with
//   __device__ long long count(long long j) const;          the count of item j (0 beyond the end)
//   __device__ void write(long long j, long long pos) const; receives the exclusive prefix of item j
// launch_scan runs three kernels: block sums, one block over them, block-local scan + write. Integer sums only: the result does not depend
// on the order of execution. Include inside `namespace im { namespace {` of the translation unit that instantiates the kernels, behind
// ctx.h and stage_scratch.h (SCAN_THREADS, and carve.h's blocks_of).
#pragma once

__device__ __forceinline__ long long block_excl_scan(long long v, long long& total) {
    __shared__ long long ws[SCAN_THREADS / IM_WAVE];
    const int lane = threadIdx.x & (IM_WAVE - 1), w = threadIdx.x / IM_WAVE;
    long long inc = v;
#pragma unroll
    for (int o = 1; o < IM_WAVE; o <<= 1) {
        const long long u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    if (lane == IM_WAVE - 1) ws[w] = inc;
    __syncthreads();
    long long off = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < SCAN_THREADS / IM_WAVE; ++k) {
        if (k < w) off += ws[k];
        tot += ws[k];
    }
    __syncthreads();
    total = tot;
    return off + inc - v;
}

template <typename S>
__global__ __launch_bounds__(SCAN_THREADS) void scan_sums_kernel(S s, long long* __restrict__ sums) {
    long long tot;
    block_excl_scan(s.count(blockIdx.x * (long long)SCAN_THREADS + threadIdx.x), tot);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

__global__ __launch_bounds__(SCAN_THREADS) void scan_top_kernel(long long* __restrict__ sums, long long nb, long long* __restrict__ total) {
    long long carry = 0;
    for (long long base = 0; base < nb; base += SCAN_THREADS) {
        const long long k = base + threadIdx.x;
        long long tot;
        const long long e = block_excl_scan(k < nb ? sums[k] : 0, tot);
        if (k < nb) sums[k] = carry + e;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

template <typename S>
__global__ __launch_bounds__(SCAN_THREADS) void scan_write_kernel(S s, const long long* __restrict__ sums) {
    const long long j = blockIdx.x * (long long)SCAN_THREADS + threadIdx.x;
    long long tot;
    const long long e = block_excl_scan(s.count(j), tot);
    s.write(j, sums[blockIdx.x] + e);
}

// sums: [max(1, blocks_of(n, SCAN_THREADS))] scratch; *total receives the sum of all counts
template <typename S>
hipError_t launch_scan(const S& s, long long n, long long* sums, long long* total, hipStream_t st) {
    const long long nb = std::max(1LL, blocks_of(n, SCAN_THREADS));
    hipLaunchKernelGGL(scan_sums_kernel<S>, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, st, s, sums);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, sums, nb, total);
    hipLaunchKernelGGL(scan_write_kernel<S>, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, st, s, (const long long*)sums);
    return hipGetLastError();
}
