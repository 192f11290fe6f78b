// MT19937 (numpy's legacy RandomState, torch's CPU generator), stated once for the device kernels that walk its stream
// (sampler.hip, randperm.hip) and the host generator of focf_compose.hip: the recurrence word by word, the tempering, and the
// mask of numpy's bounded draws.  The state is numpy's layout throughout: key[MT_N] and the position of the next word.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fr {

static constexpr int MT_N = 624, MT_M = 397;
static constexpr int MT_H = MT_N - MT_M;      // 227: word k of a new block needs word k - 227 of it, or word k + 397 of the old one
static constexpr uint32_t MT_UPPER = 0x80000000u, MT_LOWER = 0x7fffffffu, MT_MATRIX_A = 0x9908b0dfu;
static constexpr uint32_t MT_TEMPER_B = 0x9d2c5680u, MT_TEMPER_C = 0xefc60000u;

__host__ __device__ __forceinline__ uint32_t mt_mix(uint32_t a, uint32_t b) {
    const uint32_t y = (b & MT_LOWER) | (a & MT_UPPER);
    return (y >> 1) ^ ((y & 1u) ? MT_MATRIX_A : 0u);
}

__host__ __device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
    y ^= y >> 11;
    y ^= (y << 7) & MT_TEMPER_B;
    y ^= (y << 15) & MT_TEMPER_C;
    y ^= y >> 18;
    return y;
}

// word k of the new block, from the old block and the part of the new block already formed (mt19937_gen's three loops):
// [0, 227) reads old words only, [227, 623) reads new[k - 227], word 623 reads new[396] and new[0]
__host__ __device__ __forceinline__ uint32_t mt_next_word(const uint32_t* old, const uint32_t* neu, int k) {
    if (k < MT_H) return old[k + MT_M] ^ mt_mix(old[k], old[k + 1]);
    if (k < MT_N - 1) return neu[k - MT_H] ^ mt_mix(old[k], old[k + 1]);
    return neu[MT_M - 1] ^ mt_mix(old[MT_N - 1], neu[0]);
}

// the smallest 2^b - 1 >= span: a bounded draw keeps `word & mask` when it is <= span (numpy's masked rejection)
__host__ __device__ __forceinline__ uint32_t bounded_mask(uint32_t span) {
    uint32_t mask = span;
    mask |= mask >> 1;
    mask |= mask >> 2;
    mask |= mask >> 4;
    mask |= mask >> 8;
    mask |= mask >> 16;
    return mask;
}

}  // namespace fr
