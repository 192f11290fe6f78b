// fr_pair_mlp_scores: every (user, item) score of an MLP scorer over cat(user, item), with the first layer split.
//
// The first Linear is linear in the concatenation, z1(u, i) = (W1[:, :D] x_u + b1) + W1[:, D:] w_i = P[u] + Q[i]: the caller
// forms P once per request and Q once per item table (two fr_linear_fwd products), and what is left per pair is n1 adds and
// the narrow upper layers.  This kernel does that part and writes the dense masked [n_users, ld] matrix.
//
// A workgroup of four waves owns a tile of 32 users and a slice of the items, which it walks 32 items at a time.  A tile of
// Q goes to LDS once and serves the 32 users in turn: h1 = act(P[u] + Q[tile]) is built in LDS as [32][S] and the upper
// layers run on the tile machine mlp_tile.hpp describes, the 32 rows being the 32 items.  The upper layers' weights stay in
// LDS for the whole launch when they fit (the usual scorer); otherwise they are streamed per user and tile (correct, and
// slow: the wide shapes are served, not tuned).  The one-output layer is the same MFMA chain with one live column; its 32
// pre-activations pass through LDS so that 32 lanes do the epilogue and one 128-byte store.  No atomics, no workspace.
//
// A cell's arithmetic (include/fairrec_hip.h states it as the contract) involves P[u], Q[i] and the parameters only: rows
// beyond the slice are zeros in LDS and are never stored, and the cuts (32 users, 32 items, the slices) do not enter a chain
// (mlp_tile.hpp has the rest of the argument).
//
// The staging of the resident images and the layer loop are this kernel's own copy of mt_stage_image / mt_upper_layers
// (mlp_tile.hpp): built on them it computed the same bits and measured 0.8 % slower.  The copy still fetches the streamed
// weights by a load on clamped indices with a select behind it, the slow form mlp_tile.hpp names; the streamed path is not
// tuned, and changing the fetch moves the resident path's code as well.
#include "common.hpp"
#include "kernels.hpp"
#include "mlp_tile.hpp"

namespace fr {

constexpr int PM_UT = 32;              // users of a workgroup
constexpr int PM_IT = MT_RT;           // items of a step: the rows of a tile
constexpr int PM_PC = (FR_PAIR_MLP_MAX_WIDTH + 2 + 31) / 32;      // columns of a [32][S] tile per thread: S <= 257
constexpr int PM_WG_WANT = 1024;       // workgroups that fill the chip: the items are cut into slices until there are as many

struct PairK {
    const float *P, *Q;
    const float* W[MT_UP];
    const float* bias[MT_UP];
    float* scores;
    long long U, N, ld, slice_len;
    int n1, n_up, resident;
    int s0, s1;                        // row strides (floats) of the two activation buffers
    int n_out[MT_UP];
    int w_off[MT_UP];                  // resident weights: float offset of layer l's image [round32(n_out)][mt_stride(n_in)]
};

__global__ __launch_bounds__(256) void pair_mlp_kernel(PairK a) {
    extern __shared__ __align__(16) float pm_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
    const int li = lane & 31, h = lane >> 5;
    const int n1 = a.n1, sq = mt_stride(n1);
    float* Qs = pm_smem;                                    // [32][sq]: the item tile's rows of Q
    float* buf0 = Qs + PM_IT * sq;                          // [32][s0]: h1; outputs of upper layers 1, 3
    float* buf1 = buf0 + PM_IT * a.s0;                      // [32][s1]: outputs of upper layers 0, 2
    float* zs = buf1 + PM_IT * a.s1;                        // [32]: the last layer's pre-activations
    float* Ws = zs + PM_IT;                                 // resident images, or the [128][MT_WST] staging image
    const long long u0 = (long long)blockIdx.x * PM_UT;
    const long long lo = (long long)blockIdx.y * a.slice_len;
    const long long hi = lo + a.slice_len < a.N ? lo + a.slice_len : a.N;
    const int nu = (int)(a.U - u0 < PM_UT ? a.U - u0 : PM_UT);
    const int c32 = tid & 31, r8 = tid >> 5;                // a thread's column (+ 32 j) and row (+ 8 i) of a [32][S] tile

    if (a.resident) {
        int n_in = n1;
        for (int l = 0; l < a.n_up; ++l) {
            const int n_out = a.n_out[l], s = mt_stride(n_in), rows = (n_out + 31) & ~31;
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

    for (long long i0 = lo; i0 < hi; i0 += PM_IT) {
        __syncthreads();          // the tile before is done with Qs
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r8 + 8 * i;
            const long long it = i0 + r;
            const float* qp = a.Q + (size_t)(it < hi ? it : hi - 1) * n1;
            for (int c = c32; c < sq; c += 32) {
                const float v = qp[c < n1 ? c : n1 - 1];
                Qs[r * sq + c] = (it < hi && c < n1) ? v : 0.f;
            }
        }
        float pv[PM_PC];          // this thread's columns of P[u], fetched one user ahead
        auto fetch_p = [&](int uu) {
            const float* pp = a.P + (size_t)(u0 + uu) * n1;
#pragma unroll
            for (int j = 0; j < PM_PC; ++j) {
                const int c = c32 + 32 * j;
                pv[j] = pp[c < n1 ? c : n1 - 1];
            }
        };
        fetch_p(0);
        for (int uu = 0; uu < nu; ++uu) {
            __syncthreads();      // Qs is written; the user before has read its last activations
#pragma unroll
            for (int j = 0; j < PM_PC; ++j) {
                const int c = c32 + 32 * j;
                if (c < sq) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int r = r8 + 8 * i;
                        buf0[r * a.s0 + c] = c < n1 ? mt_relu(__fadd_rn(pv[j], Qs[r * sq + c])) : 0.f;
                    }
                }
            }
            fetch_p(uu + 1 < nu ? uu + 1 : uu);
            int n_in = n1;
            for (int l = 0; l < a.n_up; ++l) {
                const int n_out = a.n_out[l];
                const bool last = l == a.n_up - 1;
                const float* in = (l & 1) ? buf1 : buf0;
                float* out = (l & 1) ? buf0 : buf1;
                const int s_in = (l & 1) ? a.s1 : a.s0, s_out = (l & 1) ? a.s0 : a.s1;
                const int sw = mt_stride(n_in);
                const float* W = a.W[l];
                __syncthreads();  // the layer's input is written
                float pre[16];
                auto fetch = [&](int col0, int c0) {
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const int e = tid + 256 * j, col = col0 + (e >> 5), kc = c0 + (e & 31);
                        const float v = W[(size_t)(col < n_out ? col : n_out - 1) * n_in + (kc < n_in ? kc : n_in - 1)];
                        pre[j] = (col < n_out && kc < n_in) ? v : 0.f;
                    }
                };
                if (!a.resident) fetch(0, 0);
                for (int col0 = 0; col0 < n_out; col0 += MT_CG) {
                    const int col = col0 + wave * 32 + li;
                    const bool ok = col < n_out;
                    const float bias = a.bias[l][ok ? col : n_out - 1];
                    f32x16 acc;
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
                    if (a.resident) {
                        if (wave * 32 < n_out - col0) {
                            const float* xp = in + li * s_in + h;
                            const float* wp = Ws + a.w_off[l] + (col0 + wave * 32 + li) * sw + h;
                            const int steps = (n_in + 1) >> 1;
                            for (int s = 0; s < steps; ++s)
                                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xp[2 * s], wp[2 * s], acc, 0, 0, 0);
                        }
                    } else {
                        for (int c0 = 0; c0 < n_in; c0 += MT_DK) {
                            __syncthreads();      // the image is free
#pragma unroll
                            for (int j = 0; j < 16; ++j) {
                                const int e = tid + 256 * j;
                                Ws[(e >> 5) * MT_WST + (e & 31)] = pre[j];
                            }
                            __syncthreads();
                            if (c0 + MT_DK < n_in) fetch(col0, c0 + MT_DK);
                            else if (col0 + MT_CG < n_out) fetch(col0 + MT_CG, 0);
                            if (wave * 32 < n_out - col0) {
                                const int left = (n_in - c0 + 1) >> 1, steps = left < MT_DK / 2 ? left : MT_DK / 2;
                                const float* xp = in + li * s_in + c0 + h;
                                const float* wp = Ws + (wave * 32 + li) * MT_WST + h;
                                for (int s = 0; s < steps; ++s)
                                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xp[2 * s], wp[2 * s], acc, 0, 0, 0);
                            }
                        }
                    }
                    if (ok) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int row = mt_row(r, h);
                            const float z = __fadd_rn(acc[r], bias);
                            if (last) zs[row] = z;          // (n_out is 1: lanes 0 and 32 of wave 0)
                            else out[row * s_out + col] = mt_relu(z);
                        }
                    }
                }
                if (!last && (n_out & 1) && tid < PM_IT) out[tid * s_out + n_out] = 0.f;
                n_in = n_out;
            }
            // (LDS operations of a wave execute in order: zs was written by this wave)
            if (wave == 0) {
                __builtin_amdgcn_wave_barrier();
                if (lane < PM_IT && i0 + lane < hi) a.scores[(size_t)(u0 + uu) * a.ld + i0 + lane] = mt_score(zs[lane]);
            }
        }
    }
}

// widths, layer count and activation of a scorer this entry serves
static int pm_shape_check(int32_t n1, int32_t n_linears, const int32_t* n_out, int32_t act, const char* who) {
    FR_CHECK_ARG(n_linears >= 2 && n_linears <= FR_PAIR_MLP_MAX_LINEARS, "%s: n_linears %d not in 2..%d", who, n_linears,
                 FR_PAIR_MLP_MAX_LINEARS);
    FR_CHECK_ARG(n1 >= 1 && n1 <= FR_PAIR_MLP_MAX_WIDTH, "%s: n1 %d not in 1..%d", who, n1, FR_PAIR_MLP_MAX_WIDTH);
    FR_CHECK_ARG(n_out, "%s: n_out is null", who);
    for (int l = 0; l < n_linears - 1; ++l)
        FR_CHECK_ARG(n_out[l] >= 1 && n_out[l] <= FR_PAIR_MLP_MAX_WIDTH, "%s: n_out[%d] %d not in 1..%d", who, l, n_out[l],
                     FR_PAIR_MLP_MAX_WIDTH);
    FR_CHECK_ARG(n_out[n_linears - 2] == 1, "%s: the last layer has n_out[%d] = %d outputs, not 1", who, n_linears - 2,
                 n_out[n_linears - 2]);
    FR_CHECK_ARG(act == 1, "%s: act %d: only relu (1) is served", who, act);
    return FR_OK;
}

}  // namespace fr

using namespace fr;

extern "C" int fr_pair_mlp_supported(int32_t n1, int32_t n_linears, const int32_t* n_out, int32_t act) {
    return pm_shape_check(n1, n_linears, n_out, act, "fr_pair_mlp_supported") == FR_OK ? 1 : 0;
}

extern "C" int fr_pair_mlp_scores(const fr_pair_mlp_args* a, void* stream_) {
    const char* who = "fr_pair_mlp_scores";
    FR_CHECK_ARG(a, "%s: null argument struct", who);
    int rc;
    if ((rc = pm_shape_check(a->n1, a->n_linears, a->n_out, a->act, who))) return rc;
    FR_CHECK_ARG(a->P, "%s: P is null", who);
    FR_CHECK_ARG(a->Q, "%s: Q is null", who);
    PairK p;
    MlpUpperPlan pl;
    if ((rc = mt_plan_upper(who, a->n1, a->n_linears, a->W, a->bias, a->n_out, p, pl))) return rc;
    FR_CHECK_ARG(a->scores_out, "%s: scores_out is null", who);
    FR_CHECK_ARG(a->n_users >= 0 && (a->n_users + PM_UT - 1) / PM_UT <= 0x7fffffffLL, "%s: n_users %lld out of range", who,
                 (long long)a->n_users);
    FR_CHECK_ARG(a->n_items >= 0 && a->n_items <= 0x7fffffffLL, "%s: n_items %lld out of range", who, (long long)a->n_items);
    FR_CHECK_ARG(a->ld >= a->n_items, "%s: ld %lld < n_items %lld", who, (long long)a->ld, (long long)a->n_items);
    if ((rc = check_hist_csr(a->hist_indptr, a->hist_items, a->hist_len, a->hist_sorted, who))) return rc;
    if (a->n_users == 0 || a->n_items == 0) return FR_OK;

    p.P = a->P;
    p.Q = a->Q;
    p.scores = a->scores_out;
    p.U = a->n_users;
    p.N = a->n_items;
    p.ld = a->ld;
    p.n1 = a->n1;
    p.s0 = mt_stride(pl.w0);
    p.s1 = mt_stride(pl.w1);
    const size_t fixed = ((size_t)PM_IT * (mt_stride(a->n1) + p.s0 + p.s1) + PM_IT) * sizeof(float);
    p.resident = mt_resident(fixed, pl.w_floats);
    const size_t ldsb = fixed + (p.resident ? pl.w_floats : (size_t)MT_CG * MT_WST) * sizeof(float);
    FR_CHECK_HIP(mt_allow_lds<pair_mlp_kernel>(ldsb));
    const long long tiles = (a->n_users + PM_UT - 1) / PM_UT, steps = (a->n_items + PM_IT - 1) / PM_IT;
    long long S = PM_WG_WANT / tiles;
    S = S < 1 ? 1 : (S > steps ? steps : S);
    S = S > 65535 ? 65535 : S;
    p.slice_len = (steps + S - 1) / S * PM_IT;
    S = (a->n_items + p.slice_len - 1) / p.slice_len;
    hipStream_t stream = (hipStream_t)stream_;
    ProfScope prof(K_PAIR_MLP, stream);
    prof_work(K_PAIR_MLP, pl.flop * (double)a->n_users * (double)a->n_items);
    FR_LAUNCH(prof, pair_mlp_kernel, dim3((unsigned)tiles, (unsigned)S), dim3(256), ldsb, stream, p);
    FR_CHECK_LAUNCH();
    if (a->mask_pad || a->hist_indptr)      // (accounted under K_TOPK_ROWS: K_PAIR_MLP times the scorer alone)
        return launch_score_mask(a->scores_out, a->n_users, a->n_items, a->ld, reinterpret_cast<const long long*>(a->hist_indptr),
                                 reinterpret_cast<const long long*>(a->hist_items), a->hist_len, a->mask_pad, stream);
    return FR_OK;
}
