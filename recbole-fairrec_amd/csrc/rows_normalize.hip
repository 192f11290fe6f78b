// fr_rows_l2_normalize: every row of a matrix divided by max(its L2 norm, eps) -- the unit vectors whose dot product is the
// cosine of the rows (PFCN_DMF's tower outputs for the fused ranking kernels).  One wave per row, the row in registers
// (lane = column + 64 e), no workspace, no atomics, no LDS; the arithmetic of a row is the contract of fairrec_hip.h.
#include "table.hpp"

namespace fr {

constexpr int NORM_WAVES = 4;        // waves per workgroup
constexpr int NORM_MAX_BLOCKS = 2048;   // 256 CUs x 8 workgroups: rows beyond that are taken in further trips of the same waves

// Steps 1..3 of the contract on one row held by a wave; returns the unclamped norm (the same value in every lane).
template <int E>
__device__ __forceinline__ float normalize_frag(RowFrag<E>& f, float eps) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) s = fmaf(f.x[e], f.x[e], s);     // (columns >= D are loaded as 0: they add nothing)
    s = wave_sum(s);
    // round-to-nearest square root and quotient: sqrtf and `/` compile to the correctly rounded sequences (hipcc's default);
    // the header's __fsqrt_rn is the bare 1-ulp v_sqrt_f32 in this toolchain unless OCML_BASIC_ROUNDED_OPERATIONS is defined
    const float n = sqrtf(s);
    const float d = fmaxf(n, eps);
#pragma unroll
    for (int e = 0; e < E; ++e) f.x[e] = __fdiv_rn(f.x[e], d);
    return n;
}

// A wave takes the rows w, w + W, w + 2 W, ... (W = waves of the grid), two per trip: both rows are requested before either
// is reduced, since a row costs one memory round trip and little else.  A wave reads the whole of its rows before it writes
// them and no two waves share a row, so Y == X is safe.  X and Y carry no __restrict__ for that reason.
template <int E>
__global__ __launch_bounds__(NORM_WAVES * 64) void rows_l2_normalize_kernel(const float* X, long long M, int D, long long ldx,
                                                                            float eps, float* Y, long long ldy,
                                                                            float* norm_out) {
    const int lane = threadIdx.x & 63;
    const long long W = (long long)gridDim.x * NORM_WAVES;
    for (long long r0 = (long long)blockIdx.x * NORM_WAVES + uniform(threadIdx.x >> 6); r0 < M; r0 += 2 * W) {
        const long long r1 = r0 + W;
        const bool two = r1 < M;      // wave-uniform
        RowFrag<E> a, b;
        load_row<E>(a, X + r0 * ldx, D, lane);
        if (two) load_row<E>(b, X + r1 * ldx, D, lane);
        const float na = normalize_frag<E>(a, eps);
        store_row<E>(a, Y + r0 * ldy, D, lane);
        if (norm_out && lane == 0) norm_out[r0] = na;
        if (two) {
            const float nb = normalize_frag<E>(b, eps);
            store_row<E>(b, Y + r1 * ldy, D, lane);
            if (norm_out && lane == 0) norm_out[r1] = nb;
        }
    }
}

}  // namespace fr

using namespace fr;

extern "C" int fr_rows_l2_normalize(const float* X, int64_t M, int32_t D, int64_t ldx, float eps, float* Y, int64_t ldy,
                                    float* norm_out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    FR_CHECK_ARG(M >= 0, "fr_rows_l2_normalize: M = %lld is negative", (long long)M);
    FR_CHECK_ARG(D >= 1 && D <= 256, "fr_rows_l2_normalize: D = %d not in 1..256", (int)D);
    FR_CHECK_ARG(ldx >= D && ldy >= D, "fr_rows_l2_normalize: row strides ldx = %lld, ldy = %lld below D = %d", (long long)ldx,
                 (long long)ldy, (int)D);
    FR_CHECK_ARG(eps >= 0.f, "fr_rows_l2_normalize: eps = %g is negative or NaN", (double)eps);
    if (M == 0) return FR_OK;
    FR_CHECK_ARG(X && Y, "fr_rows_l2_normalize: null X or Y");
    const long long blocks = (M + NORM_WAVES - 1) / NORM_WAVES;
    const dim3 grid((unsigned)(blocks < NORM_MAX_BLOCKS ? blocks : NORM_MAX_BLOCKS));
    ProfScope prof(K_ROWS_NORMALIZE, stream);
    FR_DISPATCH_E(D, FR_LAUNCH(prof, rows_l2_normalize_kernel<E>, grid, dim3(NORM_WAVES * 64), 0, stream, X, (long long)M,
                               (int)D, (long long)ldx, eps, Y, (long long)ldy, norm_out));
    FR_CHECK_LAUNCH();
    return FR_OK;
}
