// fr_dyn_neg_mlp_select / fr_dyn_neg_mlp_scores: dynamic negative sampling for an MLP scorer over cat(user, item) (NFCF,
// PFCN_MLP), candidates scored and the pick taken in one launch.
//
// The first Linear is split as in pair_mlp.hip, z1 = (W1[:, :D] x_u + b1) + W1[:, D:] w_c = P[i] + q(c): the caller forms P
// once over the n batch rows; everything per candidate happens here -- the candidate's item row is read as of the table's
// step (row_at_step: the replay fr_table_gather and fr_dyn_neg_dot_select do), q(c) and the upper layers run on
// v_mfma_f32_32x32x2_f32, and the running pick of a column stays in one lane's registers across the M rounds.  No gathered-row
// buffer, no concatenation, no score array.
//
// A workgroup of four waves owns 32 consecutive output columns c = j*n + i and walks their M candidates round by round; for
// a fixed round r the 32 candidates are 32 consecutive entries of cand.  Per round: each wave brings 8 caught-up rows into
// LDS [32][S], S odd (the 32 lanes of one MFMA operand read hit 32 banks); the item half of W1 (n1 x D floats: it does not
// fit LDS next to the upper layers) goes through LDS 128 output columns x 32 input columns at a time, one chunk fetched
// ahead, as mlp_infer.hip streams its weights; h1 = relu(P[i] + q) is built in LDS and the upper layers run as the layer
// loop of pair_mlp.hip does -- wave w takes output columns 32w..32w+31 of a group of 128, a lane holds 16 rows of ONE
// column, the rows being the 32 candidates -- from weights resident in LDS when they fit, streamed otherwise.  The layer
// loop is a copy of pair_mlp.hip's, not shared with it: that kernel's bits stay what its tests pin.
//
// A score's arithmetic (include/fairrec_hip.h states it as the contract) involves the candidate's row, its P row and the
// parameters only: the MFMA's cells do not mix rows, both weight paths run the same ascending chain, and the cuts (32
// columns, the rounds) do not enter a chain.  Loads are unconditional on clamped indices; what lies beyond a width or the
// column count is replaced by zero after the load or never stored.
#include "common.hpp"
#include "kernels.hpp"
#include "table.hpp"

namespace fr {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int DM_CT = 32;              // columns (candidates of a round) of a workgroup: the rows of one 32x32 MFMA tile
constexpr int DM_CG = 128;             // output columns of a step: 32 per wave
constexpr int DM_DK = 32;              // input columns of W staged in LDS at a time
constexpr int DM_WST = DM_DK + 1;
constexpr int DM_UP = FR_PAIR_MLP_MAX_LINEARS - 1;      // linears above the first
constexpr int DM_NR = 4;               // candidate rows in flight per wave
constexpr size_t DM_LDS_MAX = 156 * 1024;

struct DynMlpK {
    const float *P, *W1i;
    const float* W[DM_UP];
    const float* bias[DM_UP];
    const int64_t* cand;
    int64_t* out;
    float* scores;
    uint32_t* err;
    long long ldp, ldw1, n, cols;
    int M, n1, n_up, resident;
    int sx, s0, s1;                    // row strides (floats): the candidates' rows; h1 / outputs of upper layers 1, 3; of 0, 2
    int x_floats;                      // floats of the region the rows share with the outputs of upper layers 0, 2
    int n_out[DM_UP];
    int w_off[DM_UP];                  // resident weights: float offset of layer l's image [round32(n_out)][dm_stride(n_in)]
};

// LDS row stride of a tile of width n: odd, with one column of zeros behind an odd width (the MFMA takes columns in pairs)
__host__ __device__ __forceinline__ int dm_stride(int n) { return (n + 1) | 1; }

// relu that keeps a NaN (fmaxf would return the other operand)
__device__ __forceinline__ float dm_relu(float x) { return x < 0.f ? 0.f : x; }

// running pick over r = 0, 1, ...: replace only by a strictly greater value or by the first NaN (dyn_neg.hip)
__device__ __forceinline__ bool dm_takes(float x, float best) { return !(best != best) && (x != x || x > best); }

// One Linear of the 32-row tile `in` [32][s_in]: for every group of 128 output columns, pro(col) (the lane's loads for the
// epilogue, issued ahead of the chain), the ascending chain from 0 over the input column pairs, epi(col, acc).  `img`: the
// layer's resident image [round32(n_out)][dm_stride(n_in)], or null -- then W (row stride ldw) goes through `stage`
// [128][DM_WST], one chunk fetched ahead.  Called by all 256 threads after a barrier behind the writes of `in`.
template <class Pro, class Epi>
__device__ __forceinline__ void dm_layer(const float* in, const int s_in, const int n_in, const float* __restrict__ W,
                                         const size_t ldw, const int n_out, const float* img, float* stage, const int tid,
                                         Pro&& pro, Epi&& epi) {
    const int lane = tid & 63, wave = uniform(tid >> 6), li = lane & 31, h = lane >> 5;
    float pre[16];
    auto fetch = [&](int col0, int c0) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int e = tid + 256 * j, col = col0 + (e >> 5), kc = c0 + (e & 31);
            const float v = W[(size_t)(col < n_out ? col : n_out - 1) * ldw + (kc < n_in ? kc : n_in - 1)];
            pre[j] = (col < n_out && kc < n_in) ? v : 0.f;
        }
    };
    if (!img) fetch(0, 0);
    for (int col0 = 0; col0 < n_out; col0 += DM_CG) {
        const int col = col0 + wave * 32 + li;
        pro(col);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        if (img) {
            if (wave * 32 < n_out - col0) {
                const int sw = dm_stride(n_in);
                const float* xp = in + li * s_in + h;
                const float* wp = img + (col0 + wave * 32 + li) * sw + h;
                const int steps = (n_in + 1) >> 1;
                for (int s = 0; s < steps; ++s)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xp[2 * s], wp[2 * s], acc, 0, 0, 0);
            }
        } else {
            for (int c0 = 0; c0 < n_in; c0 += DM_DK) {
                __syncthreads();      // the image is free
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int e = tid + 256 * j;
                    stage[(e >> 5) * DM_WST + (e & 31)] = pre[j];
                }
                __syncthreads();
                if (c0 + DM_DK < n_in) fetch(col0, c0 + DM_DK);
                else if (col0 + DM_CG < n_out) fetch(col0 + DM_CG, 0);
                if (wave * 32 < n_out - col0) {
                    const int left = (n_in - c0 + 1) >> 1, steps = left < DM_DK / 2 ? left : DM_DK / 2;
                    const float* xp = in + li * s_in + c0 + h;
                    const float* wp = stage + (wave * 32 + li) * DM_WST + h;
                    for (int s = 0; s < steps; ++s)
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xp[2 * s], wp[2 * s], acc, 0, 0, 0);
                }
            }
        }
        epi(col, acc);
    }
}

template <class L, int E>
__global__ __launch_bounds__(256, 2) void dyn_neg_mlp_kernel(TableV It_, AdamC ci, DynMlpK a) {
    extern __shared__ __align__(16) float dm_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
    const int h = lane >> 5;
    const TableV It = resolved(It_);
    const int D = It.D, n1 = a.n1;
    float* X = dm_smem;                                     // [32][sx]: the candidates' rows; then outputs of upper layers 0, 2
    float* buf0 = X + a.x_floats;                           // [32][s0]: h1; outputs of upper layers 1, 3
    float* zs = buf0 + DM_CT * a.s0;                        // [32]: the last layer's pre-activations
    int* prow = reinterpret_cast<int*>(zs + DM_CT);         // [32]: the P row of each column of the tile
    float* stage = reinterpret_cast<float*>(prow + DM_CT);  // [128][DM_WST]: the streamed weights' chunk
    float* Ws = stage + DM_CG * DM_WST;                     // the upper layers' resident images
    const long long c0 = (long long)blockIdx.x * DM_CT;
    const int c32 = tid & 31, r8 = tid >> 5;                // a thread's column (+ 32 j) and row (+ 8 i) of a [32][S] tile

    if (tid < DM_CT) {
        const long long c = c0 + tid < a.cols ? c0 + tid : a.cols - 1;
        prow[tid] = (int)(c % a.n);
    }
    if (a.resident) {
        int n_in = n1;
        for (int l = 0; l < a.n_up; ++l) {
            const int n_out = a.n_out[l], s = dm_stride(n_in), rows = (n_out + 31) & ~31;
            float* img = Ws + a.w_off[l];
            const float* W = a.W[l];
            for (int r = r8; r < rows; r += 8) {
                const int rc = r < n_out ? r : n_out - 1;
                for (int c = c32; c < s; c += 32) {
                    const float v = W[(size_t)rc * n_in + (c < n_in ? c : n_in - 1)];
                    img[r * s + c] = (r < n_out && c < n_in) ? v : 0.f;
                }
            }
            n_in = n_out;
        }
    }

    // the running pick of column c0 + lane: lanes 0..31 of wave 0
    const long long my_c = c0 + (lane & 31) < a.cols ? c0 + (lane & 31) : a.cols - 1;
    float best = 0.f;
    int64_t pick = 0;

    for (int r = 0; r < a.M; ++r) {
        const int64_t* cr = a.cand + (size_t)r * a.cols;
        const int64_t my_id = cr[my_c];
        __syncthreads();          // the round before has read its last activations (and prow, the images are written)
        // wave w brings rows 8w .. 8w+7 of the tile, DM_NR in flight
#pragma unroll
        for (int q0 = 0; q0 < DM_CT / 4; q0 += DM_NR) {
            int64_t id[DM_NR];
            RowFrag<E> p[DM_NR];
#pragma unroll
            for (int q = 0; q < DM_NR; ++q) {
                const long long c = c0 + wave * 8 + q0 + q;
                id[q] = cr[c < a.cols ? c : a.cols - 1];
            }
#pragma unroll
            for (int q = 0; q < DM_NR; ++q) row_at_step<E, L>(It, ci, id[q], p[q], a.err, lane);
#pragma unroll
            for (int q = 0; q < DM_NR; ++q) {
                float* xr = X + (wave * 8 + q0 + q) * a.sx;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const int d = lane + 64 * e;
                    if (d < a.sx) xr[d] = d < D ? p[q].x[e] : 0.f;
                }
                if (E * 64 < a.sx && lane == 0) xr[E * 64] = 0.f;      // (D = 64 E: the one column behind it)
            }
        }
        __syncthreads();          // the rows are written

        // q = W1[:, D:] w on the MFMA, h1 = relu(P[i] + q) into buf0
        float pv[16];
        dm_layer(X, a.sx, D, a.W1i, (size_t)a.ldw1, n1, nullptr, stage, tid,
                 [&](int col) {
                     const int cc = col < n1 ? col : n1 - 1;
#pragma unroll
                     for (int k = 0; k < 16; ++k) {
                         const int row = (k & 3) + 8 * (k >> 2) + 4 * h;
                         pv[k] = a.P[(size_t)prow[row] * a.ldp + cc];
                     }
                 },
                 [&](int col, const f32x16& acc) {
                     if (col < n1) {
#pragma unroll
                         for (int k = 0; k < 16; ++k) {
                             const int row = (k & 3) + 8 * (k >> 2) + 4 * h;
                             buf0[row * a.s0 + col] = dm_relu(__fadd_rn(pv[k], acc[k]));
                         }
                     }
                 });
        if ((n1 & 1) && tid < DM_CT) buf0[tid * a.s0 + n1] = 0.f;

        int n_in = n1;
        for (int l = 0; l < a.n_up; ++l) {
            const int n_out = a.n_out[l];
            const bool last = l == a.n_up - 1;
            const float* in = (l & 1) ? X : buf0;
            float* out = (l & 1) ? buf0 : X;
            const int s_in = (l & 1) ? a.s1 : a.s0, s_out = (l & 1) ? a.s0 : a.s1;
            float bias = 0.f;
            __syncthreads();      // the layer's input is written
            dm_layer(in, s_in, n_in, a.W[l], (size_t)n_in, n_out, a.resident ? Ws + a.w_off[l] : nullptr, stage, tid,
                     [&](int col) { bias = a.bias[l][col < n_out ? col : n_out - 1]; },
                     [&](int col, const f32x16& acc) {
                         if (col < n_out) {
#pragma unroll
                             for (int k = 0; k < 16; ++k) {
                                 const int row = (k & 3) + 8 * (k >> 2) + 4 * h;
                                 const float z = __fadd_rn(acc[k], bias);
                                 if (last) zs[row] = z;          // (n_out is 1: lanes 0 and 32 of wave 0)
                                 else out[row * s_out + col] = dm_relu(z);
                             }
                         }
                     });
            if (!last && (n_out & 1) && tid < DM_CT) out[tid * s_out + n_out] = 0.f;
            n_in = n_out;
        }
        // (LDS operations of a wave execute in order: zs was written by this wave)
        if (wave == 0) {
            __builtin_amdgcn_wave_barrier();
            if (lane < DM_CT && c0 + lane < a.cols) {
                const float y = dm_relu(zs[lane]);
                const float x = __fdiv_rn(1.f, __fadd_rn(1.f, expf(-y)));
                if (a.scores) a.scores[(size_t)r * a.cols + c0 + lane] = x;
                if (r == 0 || dm_takes(x, best)) { best = x; pick = my_id; }
            }
        }
    }
    if (a.out && wave == 0 && lane < DM_CT && c0 + lane < a.cols) a.out[c0 + lane] = pick;
}

}  // namespace fr

using namespace fr;

static int dyn_neg_mlp(const char* who, const fr_dyn_neg_mlp_args* a, int64_t* out, float* scores, uint32_t* err_flag,
                       void* stream_) {
    FR_CHECK_ARG(a, "%s: null argument struct", who);
    if (!fr_pair_mlp_supported(a->n1, a->n_linears, a->n_out, a->act)) {
        char why[256];       // (fr_pair_mlp_supported has named the argument)
        snprintf(why, sizeof(why), "%s", fr_last_error());
        FR_CHECK_ARG(false, "%s: the scorer's shape is not served (%s)", who, why);
    }
    FR_CHECK_ARG(a->item_t, "%s: item_t is null", who);
    FR_CHECK_ARG(a->item_optim, "%s: item_optim is null", who);
    FR_CHECK_ARG(a->item_t->dim >= 1 && a->item_t->dim <= 256, "%s: item_t->dim (D) %d not in 1..256", who, a->item_t->dim);
    int rc;
    if ((rc = check_table_for(a->item_t, a->item_optim, who))) return rc == FR_EUNSUPPORTED ? FR_EINVAL : rc;
    FR_CHECK_ARG(a->P, "%s: P is null", who);
    FR_CHECK_ARG(a->W1_item, "%s: W1_item is null", who);
    const int n_up = a->n_linears - 1;
    for (int l = 0; l < n_up; ++l) FR_CHECK_ARG(a->W[l] && a->bias[l], "%s: W[%d] or bias[%d] is null", who, l, l);
    FR_CHECK_ARG(a->cand, "%s: cand is null", who);
    FR_CHECK_ARG(out || scores, "%s: the output pointer is null", who);
    FR_CHECK_ARG(err_flag, "%s: err_flag is null", who);
    FR_CHECK_ARG(a->ldp >= a->n1, "%s: ldp %lld < n1 %d", who, (long long)a->ldp, a->n1);
    FR_CHECK_ARG(a->ldw1 >= a->item_t->dim, "%s: ldw1 %lld < D %d", who, (long long)a->ldw1, a->item_t->dim);
    FR_CHECK_ARG(a->n >= 0 && a->n <= 0x7fffffffLL, "%s: n %lld out of range", who, (long long)a->n);
    FR_CHECK_ARG(a->num >= 1, "%s: num %d < 1", who, a->num);
    FR_CHECK_ARG(a->M >= 1, "%s: M %d < 1", who, a->M);
    const long long cols = (long long)a->n * a->num;
    FR_CHECK_ARG((cols + DM_CT - 1) / DM_CT <= 0x7fffffffLL, "%s: n * num = %lld columns are too many", who, cols);
    if (a->n == 0) return FR_OK;

    const int D = a->item_t->dim;
    DynMlpK p;
    p.P = a->P;
    p.W1i = a->W1_item;
    p.cand = a->cand;
    p.out = out;
    p.scores = scores;
    p.err = err_flag;
    p.ldp = a->ldp;
    p.ldw1 = a->ldw1;
    p.n = a->n;
    p.cols = cols;
    p.M = a->M;
    p.n1 = a->n1;
    p.n_up = n_up;
    int w0 = a->n1, w1 = 1, n_in = a->n1;
    size_t w_floats = 0;
    double flop = 2.0 * D * a->n1 + a->n1;
    for (int l = 0; l < DM_UP; ++l) {
        p.W[l] = l < n_up ? a->W[l] : nullptr;
        p.bias[l] = l < n_up ? a->bias[l] : nullptr;
        p.n_out[l] = l < n_up ? a->n_out[l] : 0;
        p.w_off[l] = (int)w_floats;
        if (l >= n_up) continue;
        w_floats += (size_t)((a->n_out[l] + 31) & ~31) * dm_stride(n_in);
        if (l < n_up - 1) {
            int& w = (l & 1) ? w0 : w1;
            w = a->n_out[l] > w ? a->n_out[l] : w;
        }
        flop += 2.0 * n_in * a->n_out[l];
        n_in = a->n_out[l];
    }
    p.sx = dm_stride(D);
    p.s0 = dm_stride(w0);
    p.s1 = dm_stride(w1);
    p.x_floats = DM_CT * (p.sx > p.s1 ? p.sx : p.s1);
    const size_t fixed = ((size_t)p.x_floats + (size_t)DM_CT * p.s0 + 2 * DM_CT + (size_t)DM_CG * DM_WST) * sizeof(float);
    p.resident = fixed + w_floats * sizeof(float) <= DM_LDS_MAX ? 1 : 0;
    const size_t ldsb = fixed + (p.resident ? w_floats : 0) * sizeof(float);
    const unsigned tiles = (unsigned)((cols + DM_CT - 1) / DM_CT);
    hipStream_t stream = (hipStream_t)stream_;
    const AdamC ci = make_adamc(a->item_optim);
    const TableV It = view(a->item_t);
    ProfScope prof(K_DYN_NEG_MLP, stream);
    prof_work(K_DYN_NEG_MLP, flop * (double)cols * (double)a->M);
    // (the attribute is set at every call: it belongs to the current device, and a per-process cache would skip the second one)
    FR_DISPATCH_L(a->item_optim->learner, FR_DISPATCH_E(D, {
                      FR_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(dyn_neg_mlp_kernel<L, E>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsb));
                      FR_LAUNCH(prof, (dyn_neg_mlp_kernel<L, E>), dim3(tiles), dim3(256), ldsb, stream, It, ci, p);
                  }));
    FR_CHECK_LAUNCH();
    return FR_OK;
}

extern "C" int fr_dyn_neg_mlp_select(const fr_dyn_neg_mlp_args* a, int64_t* out, uint32_t* err_flag, void* stream) {
    FR_CHECK_ARG(out, "fr_dyn_neg_mlp_select: out is null");
    return dyn_neg_mlp("fr_dyn_neg_mlp_select", a, out, nullptr, err_flag, stream);
}

extern "C" int fr_dyn_neg_mlp_scores(const fr_dyn_neg_mlp_args* a, float* scores, uint32_t* err_flag, void* stream) {
    FR_CHECK_ARG(scores, "fr_dyn_neg_mlp_scores: scores is null");
    return dyn_neg_mlp("fr_dyn_neg_mlp_scores", a, nullptr, scores, err_flag, stream);
}
