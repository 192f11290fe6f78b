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

}  // namespace fr
