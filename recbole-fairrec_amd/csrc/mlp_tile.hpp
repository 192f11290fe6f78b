// The tile machine of the fused MLP inference kernels: mlp_infer.hip, pair_mlp.hip and dyn_neg_mlp.hip.  All three share
// the constants, the helpers, the planning of a split scorer's upper layers and the LDS-attribute helper below;
// dyn_neg_mlp.hip also runs its layers on mt_layer / mt_upper_layers.  mlp_infer.hip and pair_mlp.hip keep a layer loop of
// their own, the same code written out: built on the templates they compute the same bits and measured 1.2 % and 0.8 %
// slower, from a different register assignment and schedule around the same instructions (HISTORY.md).
//
// A workgroup of four waves holds 32 rows in LDS as [32][S], S = mt_stride(n): odd, so that the 32 lanes of one MFMA operand
// read hit 32 banks, and with one column of zeros behind an odd width, since the MFMA takes the input columns two at a time.
// Wave w multiplies the 32 rows with output columns 32w..32w+31 of a group of 128 on v_mfma_f32_32x32x2_f32; a lane then
// holds 16 rows (mt_row) of ONE output column, so a column's constants -- a bias, BatchNorm, a P cell -- are per-lane
// scalars.  The layer's weights are either resident in LDS as an image [round32(n_out)][mt_stride(n_in)], or go through LDS
// 128 output columns x 32 input columns at a time ([128][MT_WST]), one chunk fetched ahead into 16 registers.
//
// What a cell holds involves its row of the tile and the parameters only: the MFMA's cells do not mix rows; both weight
// paths run the same chain, ascending over the input column pairs from 0; and the cuts (32 rows, 128 output columns, 32
// staged input columns) are the same for every shape and do not enter a chain, so a row's bits do not depend on how many
// rows there are, on its place in the tile or on what the other rows hold.  What lies beyond a width is zero in LDS.  The
// streamed weights are fetched by conditional loads, not by loads on clamped indices with a select behind them: the select
// makes the compiler wait for each load where it is issued, ahead of the chain, and the fetch-ahead is gone (measured on
// fr_mlp_infer: 1.46x the kernel time).
#pragma once
#include "common.hpp"

namespace fr {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int MT_RT = 32;              // rows of a tile: one 32x32 MFMA tile
constexpr int MT_CG = 128;             // output columns of a step: 32 per wave
constexpr int MT_DK = 32;              // input columns of W staged in LDS at a time (streamed weights)
constexpr int MT_WST = MT_DK + 1;      // LDS row stride of the staged image (odd: the lanes of one read hit 32 banks)
constexpr int MT_UP = FR_PAIR_MLP_MAX_LINEARS - 1;      // linears above the split first one
constexpr size_t MT_LDS_MAX = 156 * 1024;               // resident weights: what a workgroup's LDS may come to with them

// LDS row stride of a tile of width n
__host__ __device__ __forceinline__ int mt_stride(int n) { return (n + 1) | 1; }

// relu that keeps a NaN (fmaxf would return the other operand)
__device__ __forceinline__ float mt_relu(float x) { return x < 0.f ? 0.f : x; }

// the tile row of cell r (0..15) of a lane's accumulator, h = lane >> 5
__device__ __forceinline__ int mt_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// the score of a one-output scorer's pre-activation: sigmoid(relu(z)), the sigmoid as the IEEE quotient over expf
__device__ __forceinline__ float mt_score(float z) { return __fdiv_rn(1.f, __fadd_rn(1.f, expf(-mt_relu(z)))); }

// One Linear of the 32-row tile `in` [32][s_in]: for every group of 128 output columns, pro(col) (the lane's loads for the
// epilogue, issued ahead of the chain), the ascending chain from 0 over the input column pairs, epi(col, acc).  `img`: the
// layer's resident image, or null -- then W (row stride ldw) goes through `stage` [128][MT_WST], one chunk fetched ahead.
// Called by all 256 threads; the resident chain wants a barrier behind the writes of `in` (the streamed one brings its own).
template <class Pro, class Epi>
__device__ __forceinline__ void mt_layer(const float* in, const int s_in, const int n_in, const float* __restrict__ W,
                                         const size_t ldw, const int n_out, const float* img, float* stage, const int tid,
                                         Pro&& pro, Epi&& epi) {
    const int lane = tid & 63, wave = uniform(tid >> 6), li = lane & 31, h = lane >> 5;
    float pre[16];
    auto fetch = [&](int col0, int c0) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int e = tid + 256 * j, col = col0 + (e >> 5), kc = c0 + (e & 31);
            pre[j] = (col < n_out && kc < n_in) ? W[(size_t)col * ldw + kc] : 0.f;
        }
    };
    if (!img) fetch(0, 0);
    for (int col0 = 0; col0 < n_out; col0 += MT_CG) {
        const int col = col0 + wave * 32 + li;
        pro(col);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        if (img) {
            if (wave * 32 < n_out - col0) {
                const int sw = mt_stride(n_in);
                const float* xp = in + li * s_in + h;
                const float* wp = img + (col0 + wave * 32 + li) * sw + h;
                const int steps = (n_in + 1) >> 1;
                for (int s = 0; s < steps; ++s)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xp[2 * s], wp[2 * s], acc, 0, 0, 0);
            }
        } else {
            for (int c0 = 0; c0 < n_in; c0 += MT_DK) {
                __syncthreads();      // the image is free; the layer's input is written
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int e = tid + 256 * j;
                    stage[(e >> 5) * MT_WST + (e & 31)] = pre[j];
                }
                __syncthreads();
                if (c0 + MT_DK < n_in) fetch(col0, c0 + MT_DK);
                else if (col0 + MT_CG < n_out) fetch(col0 + MT_CG, 0);
                if (wave * 32 < n_out - col0) {      // (a wave whose 32 columns lie beyond the layer only stages)
                    const int left = (n_in - c0 + 1) >> 1, steps = left < MT_DK / 2 ? left : MT_DK / 2;
                    const float* xp = in + li * s_in + c0 + h;
                    const float* wp = stage + (wave * 32 + li) * MT_WST + h;
                    for (int s = 0; s < steps; ++s)
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xp[2 * s], wp[2 * s], acc, 0, 0, 0);
                }
            }
        }
        epi(col, acc);
    }
}

// ---- the linears above a split first one (pair_mlp.hip, dyn_neg_mlp.hip): relu between them, one output at the end -----------
// Their kernels' argument blocks (`A` below) carry them as W[MT_UP], bias[MT_UP], n_out[MT_UP], w_off[MT_UP] (resident
// weights: the float offset of layer l's image), n_up and resident -- flat members: nested in a struct of their own they
// cost pair_mlp_kernel five more spilled SGPRs.

// the resident image [round32(n_out)][mt_stride(n_in)] of one layer's W [n_out][n_in]: zeros beyond either width
__device__ __forceinline__ void mt_stage_image(float* img, const float* W, const int n_in, const int n_out,
                                               const int tid) {
    const int s = mt_stride(n_in), rows = (n_out + 31) & ~31;
    for (int r = tid >> 5; r < rows; r += 8) {
        const int rc = r < n_out ? r : n_out - 1;
        for (int c = tid & 31; c < s; c += 32) {
            const float v = W[(size_t)rc * n_in + (c < n_in ? c : n_in - 1)];
            img[r * s + c] = (r < n_out && c < n_in) ? v : 0.f;
        }
    }
}

// The upper layers on the tile h1 = buf0 [32][s0]: layers 0, 2 write buf1 [32][s1], layers 1, 3 write buf0, and the last
// one leaves its 32 pre-activations in zs (n_out is 1: lanes 0 and 32 of wave 0 write them, so wave 0 may read them behind a
// wave barrier).  `imgs`: the resident images (`up.resident`), else null and the weights stream through `stage`.
template <class A>
__device__ __forceinline__ void mt_upper_layers(const A& up, const int n1, float* buf0, const int s0, float* buf1,
                                                const int s1, float* zs, const float* imgs, float* stage, const int tid) {
    const int h = (tid & 63) >> 5;
    int n_in = n1;
    for (int l = 0; l < up.n_up; ++l) {
        const int n_out = up.n_out[l];
        const bool last = l == up.n_up - 1;
        const float* in = (l & 1) ? buf1 : buf0;
        float* out = (l & 1) ? buf0 : buf1;
        const int s_in = (l & 1) ? s1 : s0, s_out = (l & 1) ? s0 : s1;
        float bias = 0.f;
        __syncthreads();      // the layer's input is written
        mt_layer(in, s_in, n_in, up.W[l], (size_t)n_in, n_out, imgs ? imgs + up.w_off[l] : nullptr, stage, tid,
                 [&](int col) { bias = up.bias[l][col < n_out ? col : n_out - 1]; },
                 [&](int col, const f32x16& acc) {
                     if (col < n_out) {
#pragma unroll
                         for (int r = 0; r < 16; ++r) {
                             const float z = __fadd_rn(acc[r], bias);
                             if (last) zs[mt_row(r, h)] = z;
                             else out[mt_row(r, h) * s_out + col] = mt_relu(z);
                         }
                     }
                 });
        if (!last && (n_out & 1) && tid < MT_RT) out[tid * s_out + n_out] = 0.f;
        n_in = n_out;
    }
}

// Host side: fills `up` but for `resident` from the caller's arrays (who names the entry in the refusals) and returns what
// the LDS layout and the accounting need.
struct MlpUpperPlan {
    int w0, w1;                        // the widest tile buf0 (h1 included) and buf1 hold
    size_t w_floats;                   // floats of all resident images
    double flop;                       // per row of a tile: the adds of h1 and the upper layers
};

template <class A>
inline int mt_plan_upper(const char* who, int n1, int n_linears, const float* const* W, const float* const* bias,
                         const int32_t* n_out, A& up, MlpUpperPlan& pl) {
    up.n_up = n_linears - 1;
    for (int l = 0; l < up.n_up; ++l) FR_CHECK_ARG(W[l] && bias[l], "%s: W[%d] or bias[%d] is null", who, l, l);
    pl = {n1, 1, 0, (double)n1};
    int n_in = n1;
    for (int l = 0; l < MT_UP; ++l) {
        const bool used = l < up.n_up;
        up.W[l] = used ? W[l] : nullptr;
        up.bias[l] = used ? bias[l] : nullptr;
        up.n_out[l] = used ? n_out[l] : 0;
        up.w_off[l] = (int)pl.w_floats;
        if (!used) continue;
        pl.w_floats += (size_t)((n_out[l] + 31) & ~31) * mt_stride(n_in);
        if (l < up.n_up - 1) {
            int& w = (l & 1) ? pl.w0 : pl.w1;
            w = n_out[l] > w ? n_out[l] : w;
        }
        pl.flop += 2.0 * n_in * n_out[l];
        n_in = n_out[l];
    }
    return FR_OK;
}

// do the images fit next to `fixed` bytes of a workgroup's LDS?
inline int mt_resident(size_t fixed, size_t w_floats) { return fixed + w_floats * sizeof(float) <= MT_LDS_MAX ? 1 : 0; }

// The dynamic LDS `Kernel` may ask for.  The attribute belongs to the current device, and a per-process cache of the largest
// size set would skip the second one: the cache is per device ordinal (set at every call, the attribute cost fr_mlp_infer
// about 1 us of host time in a 64 us call).  Not thread-safe, as the caches it replaces were not: the entries are called
// from one host thread per process.
template <auto Kernel>
inline hipError_t mt_allow_lds(size_t bytes) {
    constexpr int DEVICES = 64;        // (an ordinal beyond: set at every call)
    static size_t have[DEVICES] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess || (dev < DEVICES && bytes <= have[dev])) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess && dev < DEVICES) have[dev] = bytes;
    return e;
}

}  // namespace fr
