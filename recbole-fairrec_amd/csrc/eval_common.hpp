// Device helpers shared by the evaluation kernels (metrics.hip, exposure.hip).
#pragma once
#include "common.hpp"

namespace fr {

__device__ __forceinline__ long long clamp_ll(long long x, long long lo, long long hi) { return x < lo ? lo : (x > hi ? hi : x); }

// group g's range [lo, hi) of positions, clamped into [0, U]: a malformed group_start gives unspecified values, never an
// address outside the arrays
__device__ __forceinline__ void group_range(const int64_t* __restrict__ group_start, long long g, long long U, long long& lo,
                                            long long& hi) {
    lo = clamp_ll(group_start[g], 0, U);
    hi = clamp_ll(group_start[g + 1], lo, U);
}

// Groups cut into chunks of consecutive positions (metrics.hip: group_chunk_scan_kernel writes chunk_start[g] = number of chunks
// of the groups before g).  The (group, chunk) of block b, or false: the last g with chunk_start[g] <= b (groups without a chunk
// share their successor's entry and are passed over)
__device__ __forceinline__ bool block_chunk(const long long* __restrict__ chunk_start, long long G, long long b, long long& g,
                                            long long& c) {
    if (b >= chunk_start[G]) return false;
    long long lo = 0, hi = G;            // invariant: chunk_start[lo] <= b < chunk_start[hi]
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (chunk_start[mid] <= b) lo = mid;
        else hi = mid;
    }
    g = lo;
    c = b - chunk_start[lo];
    return true;
}

}  // namespace fr
