// Dynamic negative sampling (`neg_sampling: {uniform: 1, dynamic: M}`): of M candidate negatives per slot keep the one the
// model scores highest.
//
// Replaces the selection of abstract_dataloader.py `_neg_sampling` (dynamic branch):
//     scores = model.predict(interaction).reshape(M, -1)
//     indices = torch.max(scores, dim=0)[1]
//     neg_item_ids = neg_candidate_ids.reshape(M, -1)[indices, range(cols)]
// fr_dyn_neg_select is that selection on scores a caller computed (every model); fr_dyn_neg_dot_select also computes the
// scores of a dot-product model (PFCN_PMF / PFCN_BiasedMF predict) without materialising the candidates' rows.
//
// The pick follows torch.max(dim=0): the first maximum wins ties, a NaN beats every number and the first NaN wins.
#include "common.hpp"
#include "kernels.hpp"
#include "table.hpp"

namespace fr {

// running pick over r = 0, 1, ...: replace only by a strictly greater value or by the first NaN
__device__ __forceinline__ bool dyn_neg_takes(float x, float best) {
    return !(best != best) && (x != x || x > best);
}

// one thread per column
__global__ __launch_bounds__(256) void dyn_neg_select_kernel(const float* __restrict__ scores,
                                                             const int64_t* __restrict__ cand, long long cols, int M,
                                                             int64_t* __restrict__ out) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= cols) return;
    float best = scores[c];
    int pick = 0;
    for (int r = 1; r < M; ++r) {
        const float x = scores[(size_t)r * cols + c];
        if (dyn_neg_takes(x, best)) { best = x; pick = r; }
    }
    out[c] = cand[(size_t)pick * cols + c];
}

// Fused scorer + pick of a dot-product model.  One wave per output column c = j*n + i (user row i, negative slot j); its
// M candidates are cand[(r*num + j)*n + i].  Per candidate:
//     x = sigmoid(((dot(user_rows[i], item row) + user_bias[i]) + item bias) + global_bias)
// with the item rows read as of the table's step (row_at_step: the replay fr_table_gather does), the dot in
// rowdot_fwd_kernel's order (fmaf over d = lane, lane+64, ..., then wave_sum) and the sums in predict()'s order -- the fp32
// values PFCNBase.predict returns.  Candidates are processed NR at a time so that NR rows are in flight per wave.
constexpr int DYN_NR = 4;

template <class L, int E>
__global__ __launch_bounds__(256) void dyn_neg_dot_select_kernel(TableV It_, AdamC ci, TableV Bt_, AdamC cb, bool has_ib,
                                                                 const float* __restrict__ user_rows,
                                                                 const float* __restrict__ user_bias,
                                                                 const float* __restrict__ global_bias,
                                                                 const int64_t* __restrict__ cand, long long n, int num,
                                                                 int M, int64_t* __restrict__ out, uint32_t* err) {
    const int lane = threadIdx.x & 63;
    const long long c = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long cols = n * num;
    if (c >= cols) return;
    const TableV It = resolved(It_);
    const long long i = c % n, j = c / n;
    const int D = It.D;
    RowFrag<E> u;
    load_row<E>(u, user_rows + (size_t)i * D, D, lane);
    const float ub = user_bias ? user_bias[i] : 0.f;
    const float gb = global_bias ? *global_bias : 0.f;
    float best = 0.f;
    int64_t pick = 0;
    for (int r0 = 0; r0 < M; r0 += DYN_NR) {
        int64_t id[DYN_NR];
        RowFrag<E> p[DYN_NR];
#pragma unroll
        for (int q = 0; q < DYN_NR; ++q)
            id[q] = r0 + q < M ? cand[((size_t)(r0 + q) * num + j) * n + i] : -1;
#pragma unroll
        for (int q = 0; q < DYN_NR; ++q)
            if (r0 + q < M) row_at_step<E, L>(It, ci, id[q], p[q], err, lane);
#pragma unroll
        for (int q = 0; q < DYN_NR; ++q) {
            if (r0 + q >= M) break;
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < E; ++e)
                if (lane + 64 * e < D) s = fmaf(u.x[e], p[q].x[e], s);
            float x = wave_sum(s);
            if (user_bias) x = x + ub;
            if (has_ib) {
                const TableV Bt = resolved(Bt_);
                RowFrag<1> b;
                row_at_step<1, L>(Bt, cb, id[q], b, err, lane);
                x = x + __shfl(b.x[0], 0, 64);
            }
            if (global_bias) x = x + gb;
            x = 1.0f / (1.0f + expf(-x));
            if (r0 + q == 0 || dyn_neg_takes(x, best)) { best = x; pick = id[q]; }
        }
    }
    if (lane == 0) out[c] = pick;
}

// The scores alone (the values the kernel above picks from), for the tests that pin them to torch.sigmoid.
template <class L, int E>
__global__ __launch_bounds__(256) void dyn_neg_dot_scores_kernel(TableV It_, AdamC ci, TableV Bt_, AdamC cb, bool has_ib,
                                                                 const float* __restrict__ user_rows,
                                                                 const float* __restrict__ user_bias,
                                                                 const float* __restrict__ global_bias,
                                                                 const int64_t* __restrict__ cand, long long n, int num,
                                                                 int M, float* __restrict__ scores, uint32_t* err) {
    const int lane = threadIdx.x & 63;
    const long long k = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);     // k = (r*num + j)*n + i
    if (k >= n * num * M) return;
    const TableV It = resolved(It_);
    const long long i = k % n;
    const int D = It.D;
    RowFrag<E> u, p;
    load_row<E>(u, user_rows + (size_t)i * D, D, lane);
    const int64_t id = cand[k];
    row_at_step<E, L>(It, ci, id, p, err, lane);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e)
        if (lane + 64 * e < D) s = fmaf(u.x[e], p.x[e], s);
    float x = wave_sum(s);
    if (user_bias) x = x + user_bias[i];
    if (has_ib) {
        const TableV Bt = resolved(Bt_);
        RowFrag<1> b;
        row_at_step<1, L>(Bt, cb, id, b, err, lane);
        x = x + __shfl(b.x[0], 0, 64);
    }
    if (global_bias) x = x + *global_bias;
    x = 1.0f / (1.0f + expf(-x));
    if (lane == 0) scores[k] = x;
}

}  // namespace fr

using namespace fr;

extern "C" int fr_dyn_neg_select(const float* scores, const int64_t* cand, int64_t cols, int32_t M, int64_t* out,
                                 void* stream_) {
    FR_CHECK_ARG(scores && cand && out && cols >= 0 && M >= 1, "fr_dyn_neg_select: bad argument");
    if (cols == 0) return FR_OK;
    hipStream_t stream = (hipStream_t)stream_;
    ProfScope prof(K_DYN_NEG_SELECT, stream);
    FR_LAUNCH(prof, dyn_neg_select_kernel, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, stream, scores, cand,
              (long long)cols, (int)M, out);
    FR_CHECK_LAUNCH();
    return FR_OK;
}

static int dyn_neg_dot(const char* who, const fr_table* item_t, const fr_adam* item_adam, const fr_table* item_bias_t,
                       const fr_adam* item_bias_adam, const float* user_rows, const float* user_bias,
                       const float* global_bias, const int64_t* cand, int64_t n, int32_t num, int32_t M, int64_t* out,
                       float* scores, uint32_t* err_flag, void* stream_) {
    int rc;
    if ((rc = check_table_for(item_t, item_adam, who))) return rc;
    if (item_bias_t) {
        if ((rc = check_table_for(item_bias_t, item_bias_adam, who))) return rc;
        FR_CHECK_ARG(item_bias_t->dim == 1, "%s: the item bias table must have one column", who);
        FR_CHECK_ARG(item_bias_adam->learner == item_adam->learner, "%s: the item and item bias tables have different learners",
                     who);
    }
    FR_CHECK_ARG(user_rows && cand && (out || scores) && n >= 0 && num >= 1 && M >= 1, "%s: bad argument", who);
    FR_CHECK_ARG(n * num <= 0x7fffffffLL * 4, "%s: too many columns", who);
    if (n == 0) return FR_OK;
    hipStream_t stream = (hipStream_t)stream_;
    const AdamC ci = make_adamc(item_adam);
    const TableV It = view(item_t);
    const bool has_ib = item_bias_t != nullptr;
    const AdamC cb = has_ib ? make_adamc(item_bias_adam) : ci;
    const TableV Bt = has_ib ? view(item_bias_t) : It;
    ProfScope prof(K_DYN_NEG_DOT_SELECT, stream);
    if (out) {
        const long long cols = (long long)n * num;
        FR_DISPATCH_L(item_adam->learner,
                      FR_DISPATCH_E(item_t->dim, FR_LAUNCH(prof, (dyn_neg_dot_select_kernel<L, E>), dim3((unsigned)((cols + 3) / 4)),
                                                           dim3(256), 0, stream, It, ci, Bt, cb, has_ib, user_rows, user_bias,
                                                           global_bias, cand, (long long)n, (int)num, (int)M, out, err_flag)));
    } else {
        const long long k = (long long)n * num * M;
        FR_CHECK_ARG(k <= 0x7fffffffLL * 4, "%s: too many candidates", who);
        FR_DISPATCH_L(item_adam->learner,
                      FR_DISPATCH_E(item_t->dim, FR_LAUNCH(prof, (dyn_neg_dot_scores_kernel<L, E>), dim3((unsigned)((k + 3) / 4)),
                                                           dim3(256), 0, stream, It, ci, Bt, cb, has_ib, user_rows, user_bias,
                                                           global_bias, cand, (long long)n, (int)num, (int)M, scores, err_flag)));
    }
    FR_CHECK_LAUNCH();
    return FR_OK;
}

extern "C" int fr_dyn_neg_dot_select(const fr_table* item_t, const fr_adam* item_adam, const fr_table* item_bias_t,
                                     const fr_adam* item_bias_adam, const float* user_rows, const float* user_bias,
                                     const float* global_bias, const int64_t* cand, int64_t n, int32_t num, int32_t M,
                                     int64_t* out, uint32_t* err_flag, void* stream) {
    FR_CHECK_ARG(out, "fr_dyn_neg_dot_select: bad argument");
    return dyn_neg_dot("fr_dyn_neg_dot_select", item_t, item_adam, item_bias_t, item_bias_adam, user_rows, user_bias,
                       global_bias, cand, n, num, M, out, nullptr, err_flag, stream);
}

extern "C" int fr_dyn_neg_dot_scores(const fr_table* item_t, const fr_adam* item_adam, const fr_table* item_bias_t,
                                     const fr_adam* item_bias_adam, const float* user_rows, const float* user_bias,
                                     const float* global_bias, const int64_t* cand, int64_t n, int32_t num, int32_t M,
                                     float* scores, uint32_t* err_flag, void* stream) {
    FR_CHECK_ARG(scores, "fr_dyn_neg_dot_scores: bad argument");
    return dyn_neg_dot("fr_dyn_neg_dot_scores", item_t, item_adam, item_bias_t, item_bias_adam, user_rows, user_bias,
                       global_bias, cand, n, num, M, nullptr, scores, err_flag, stream);
}
