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
// LDS [32][S]; the item half of W1 (n1 x D floats: it does not fit LDS next to the upper layers) is streamed, read in place
// by its row stride; h1 = relu(P[i] + q) is built in LDS and the upper layers run from weights resident in LDS when they
// fit, streamed otherwise -- all on the tile machine of mlp_tile.hpp, the 32 rows being the 32 candidates.
//
// A score's arithmetic (include/fairrec_hip.h states it as the contract) involves the candidate's row, its P row and the
// parameters only: the cuts (32 columns, the rounds) do not enter a chain (mlp_tile.hpp has the rest of the argument), and
// what lies beyond the column count is never stored.
#include "common.hpp"
#include "kernels.hpp"
#include "mlp_tile.hpp"
#include "table.hpp"

namespace fr {

constexpr int DM_CT = MT_RT;           // columns (candidates of a round) of a workgroup: the rows of a tile
constexpr int DM_NR = 4;               // candidate rows in flight per wave

struct DynMlpK {
    const float *P, *W1i;
    const int64_t* cand;
    int64_t* out;
    float* scores;
    uint32_t* err;
    long long ldp, ldw1, n, cols;
    int M, n1, n_up, resident;
    int sx, s0, s1;                    // row strides (floats): the candidates' rows; h1 / outputs of upper layers 1, 3; of 0, 2
    int x_floats;                      // floats of the region the rows share with the outputs of upper layers 0, 2
    const float* W[MT_UP];
    const float* bias[MT_UP];
    int n_out[MT_UP];
    int w_off[MT_UP];                  // resident weights: float offset of layer l's image
};

// running pick over r = 0, 1, ...: replace only by a strictly greater value or by the first NaN (dyn_neg.hip)
__device__ __forceinline__ bool dm_takes(float x, float best) { return !(best != best) && (x != x || x > best); }

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
    float* stage = reinterpret_cast<float*>(prow + DM_CT);  // [128][MT_WST]: the streamed weights' chunk
    float* Ws = stage + MT_CG * MT_WST;                     // the upper layers' resident images
    const long long c0 = (long long)blockIdx.x * DM_CT;

    if (tid < DM_CT) {
        const long long c = c0 + tid < a.cols ? c0 + tid : a.cols - 1;
        prow[tid] = (int)(c % a.n);
    }
    if (a.resident) {
        int n_in = n1;
        for (int l = 0; l < a.n_up; ++l) {
            mt_stage_image(Ws + a.w_off[l], a.W[l], n_in, a.n_out[l], tid);
            n_in = a.n_out[l];
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
        mt_layer(X, a.sx, D, a.W1i, (size_t)a.ldw1, n1, nullptr, stage, tid,
                 [&](int col) {
                     const int cc = col < n1 ? col : n1 - 1;
#pragma unroll
                     for (int k = 0; k < 16; ++k) pv[k] = a.P[(size_t)prow[mt_row(k, h)] * a.ldp + cc];
                 },
                 [&](int col, const f32x16& acc) {
                     if (col < n1) {
#pragma unroll
                         for (int k = 0; k < 16; ++k) buf0[mt_row(k, h) * a.s0 + col] = mt_relu(__fadd_rn(pv[k], acc[k]));
                     }
                 });
        if ((n1 & 1) && tid < DM_CT) buf0[tid * a.s0 + n1] = 0.f;

        mt_upper_layers(a, n1, buf0, a.s0, X, a.s1, zs, a.resident ? Ws : nullptr, stage, tid);
        // (LDS operations of a wave execute in order: zs was written by this wave)
        if (wave == 0) {
            __builtin_amdgcn_wave_barrier();
            if (lane < DM_CT && c0 + lane < a.cols) {
                const float x = mt_score(zs[lane]);
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
    DynMlpK p;
    MlpUpperPlan pl;
    if ((rc = mt_plan_upper(who, a->n1, a->n_linears, a->W, a->bias, a->n_out, p, pl))) return rc;
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
    p.sx = mt_stride(D);
    p.s0 = mt_stride(pl.w0);
    p.s1 = mt_stride(pl.w1);
    p.x_floats = DM_CT * (p.sx > p.s1 ? p.sx : p.s1);
    const size_t fixed = ((size_t)p.x_floats + (size_t)DM_CT * p.s0 + 2 * DM_CT + (size_t)MT_CG * MT_WST) * sizeof(float);
    p.resident = mt_resident(fixed, pl.w_floats);
    const size_t ldsb = fixed + (p.resident ? pl.w_floats : 0) * sizeof(float);
    const unsigned tiles = (unsigned)((cols + DM_CT - 1) / DM_CT);
    hipStream_t stream = (hipStream_t)stream_;
    const AdamC ci = make_adamc(a->item_optim);
    const TableV It = view(a->item_t);
    ProfScope prof(K_DYN_NEG_MLP, stream);
    prof_work(K_DYN_NEG_MLP, (2.0 * D * a->n1 + pl.flop) * (double)cols * (double)a->M);
    FR_DISPATCH_L(a->item_optim->learner, FR_DISPATCH_E(D, {
                      FR_CHECK_HIP((mt_allow_lds<dyn_neg_mlp_kernel<L, E>>(ldsb)));
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
