// Recommendation: the k best items per user, without the [users, n_items] score matrix.
//
// Replaces the composition behind recbole.utils.case_study.full_sort_topk,
//     scores = model.full_sort_predict(...); scores[:, 0] = -inf; scores[hist_u, hist_i] = -inf; torch.topk(scores, k)
// fr_recommend_topk scores a tile of 32 users against a slice of the item table on the fp32 MFMA and keeps, per user, only
// the cells that beat the user's current k-th best; fr_topk_rows selects from a dense matrix a caller computed (the models
// whose scorer is not a dot product).  Both rank by ONE total order, so a result does not depend on how the work was cut:
//     higher score first, NaN above +inf, and among equal scores (-0 == +0, all NaNs equal) the lower id first.
// The order is carried by a 64-bit key, (monotone image of the score) << 32 | (2^32 - 1 - id): a greater key is a better
// cell, and keys of distinct cells differ.  Selection is exact whatever the thresholds were at the time a cell was seen: a
// threshold is always the k-th best key of cells already seen, so no cell of the final list is ever dropped.
#include <stdlib.h>

#include "common.hpp"
#include "kernels.hpp"

namespace fr {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned long long u64;

constexpr int REC_UT = 32;            // users of a workgroup: the rows of one 32x32 MFMA tile
constexpr int REC_IB = 128;           // items of a step: 32 per wave
constexpr int REC_DK = 32;            // columns of W staged in LDS at a time
constexpr int REC_WST = REC_DK + 1;   // LDS row stride of the W image (odd: lanes of one read hit 32 banks)
constexpr int REC_Q = 8;              // a wave compacts up to 64 * REC_Q keys ...
constexpr int REC_CAP_MAX = 64 * REC_Q;   // ... the longest per-user list
constexpr int REC_LDS_MAX = 156 * 1024;
constexpr int REC_STG = 512;          // a wave stages the candidates of 8 accumulator registers (8 x 64 cells) at a time
constexpr int TR_STEP = 256;          // fr_topk_rows: cells of a sub-step (one per thread) ...
constexpr int TR_LOADS = 8;           // ... and loads in flight per thread
constexpr int TR_Q = 3;               // the workgroup compacts up to 256 * TR_Q = FR_TOPK_MAX + 2 * TR_STEP keys
constexpr int REC_SLICES_MAX = 64;
constexpr int MERGE_KEYS_MAX = 8192;  // S * k keys of one user in the merge kernel's LDS (64 KiB)

__device__ __forceinline__ uint32_t order_bits(float x) {
    if (x != x) return 0xffffffffu;                 // every NaN: above +inf (0xff800000)
    const uint32_t b = __float_as_uint(x);
    if ((b << 1) == 0) return 0x80000000u;          // -0 ties with +0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ u64 make_key(float x, uint32_t id) {
    return ((u64)order_bits(x) << 32) | (u64)(0xffffffffu - id);
}

__device__ __forceinline__ uint32_t key_id(u64 key) { return 0xffffffffu - (uint32_t)key; }

// the score a key was made of (a NaN comes back as the canonical quiet NaN, a zero as +0)
__device__ __forceinline__ float key_value(u64 key) {
    const uint32_t f = (uint32_t)(key >> 32);
    if (f == 0xffffffffu) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((f & 0x80000000u) ? (f & 0x7fffffffu) : ~f);
}

// The epilogues.  `exact` is the score that is ranked and returned.  `approx` is a cheap stand-in that decides only whether
// a cell is worth the exact arithmetic: a cell is dropped unseen when approx(x) < limit_of(threshold score), and limit_of
// leaves room for the most the two can differ --
//   epilogue 1: y * (1 / scale) against the IEEE quotient: two roundings of 2^-24 each against one, < 2^-22 relative;
//   epilogue 2: e = v_exp_f32(-x * log2(e)): the product's rounding moves e by |x| 2^-24 relative, the instruction by 2^-22;
//               f = 1 / (1 + e) moves by f (1 - f) times that, and |x| f (1 - f) <= 0.2245 for every x: 1.4e-8 + 6e-8; the add
//               and v_rcp_f32 add f (2^-23 + 2^-22) <= 3.6e-7; expf (2 ulp) and the IEEE division on the exact side 1.8e-7:
//               < 6.2e-7 absolute in all --
// with a margin of at least 2x (2^-21 relative plus 1e-37 for subnormal quotients; 1.5e-6 absolute).  A NaN on either side never drops a cell.
__device__ __forceinline__ float epilogue_exact(float x, int epi, float scale) {
    if (epi == 1) {
        const float y = x < 0.f ? 0.f : (x > scale ? scale : x);      // a NaN stays a NaN, as torch.clamp keeps it
        x = __fdiv_rn(y, scale);
    } else if (epi == 2) {
        x = 1.0f / (1.0f + expf(-x));
    }
    return x + 0.0f;                                                   // -0 -> +0: one zero in the order and in the output
}

__device__ __forceinline__ float epilogue_approx(float x, int epi, float scale, float inv_scale) {
    if (epi == 1) {
        const float y = x < 0.f ? 0.f : (x > scale ? scale : x);
        return y * inv_scale;
    }
    if (epi == 2) return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.44269504088896341f));
    return x;
}

__device__ __forceinline__ float limit_of(float tv, int epi) {
    if (epi == 1) return tv - 4.76837158203125e-7f * fabsf(tv) - 1e-37f;   // 2^-21 |tv| (and a floor for a subnormal tv); an infinite tv
                                                                        // gives NaN: nothing is dropped
    if (epi == 2) return tv - 1.5e-6f;
    return tv;
}

// One wave keeps the best min(c, k) of the c <= 64 * REC_Q distinct keys of `b`, in descending order, by counting for every
// key the keys above it.  b[0..kp) is the sorted list the compaction before left, b[kp..c) the keys pushed since: every key
// is compared with the new keys only; an old key adds its position, a new one the old keys above it (binary search).
// LDS operations of a wave execute in order, so every read below is done before the first write.
__device__ __forceinline__ void wave_compact(u64* b, int kp, int c, int k, u64* thr, float* lim, int* cnt, int* kept, int epi,
                                             int lane) {
    u64 mine[REC_Q];
    int rank[REC_Q];
    const int nq = (c + 63) >> 6;
#pragma unroll
    for (int q = 0; q < REC_Q; ++q) {
        const int i = lane + 64 * q;
        mine[q] = i < c ? b[i] : 0ull;
        rank[q] = i < kp ? i : 0;
    }
    for (int j = kp; j < c; ++j) {
        const u64 kj = b[j];
#pragma unroll
        for (int q = 0; q < REC_Q; ++q)
            if (q < nq) rank[q] += kj > mine[q] ? 1 : 0;
    }
#pragma unroll
    for (int q = 0; q < REC_Q; ++q) {
        const int i = lane + 64 * q;
        if (q < nq && i >= kp && i < c) {
            int lo = 0, hi = kp;
            while (lo < hi) {
                const int m = (lo + hi) >> 1;
                if (b[m] > mine[q]) lo = m + 1;
                else hi = m;
            }
            rank[q] += lo;
        }
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int q = 0; q < REC_Q; ++q) {
        if (lane + 64 * q < c && rank[q] < k) {
            b[rank[q]] = mine[q];
            if (rank[q] == k - 1) {
                *thr = mine[q];
                *lim = limit_of(key_value(mine[q]), epi);
            }
        }
    }
    if (lane == 0) *cnt = *kept = c < k ? c : k;
}

// ---- the score tile: what recommend_kernel, recommend_cells_kernel and recommend_meanrank_kernel share -----------------------
// A cell (user, item) has one score, whichever kernel computes it and however the work was cut: the fp32 MFMA chain over the
// column pairs, ascending from 0 (rec_link), then cell_score.  The two tiled kernels run the chain in RecTile::step, on the
// users rec_load_users put in LDS; the cells kernel feeds rec_link from memory, the same ceil(D / 2) links.  Every piece below
// is defined once, so that an edit to the tile is an edit to all three.

// the arguments of an fr_rec_args that every kernel reads (rec_fill); RecK, CellK and MrK add their own
struct RecArgs {
    const float* X;
    const float* W;
    const float* ub;
    const float* ib;
    const long long* indptr;
    const long long* hist;
    long long U, N, hist_len;
    int D, epi, mask_pad;
    float bias0, scale;
};

// one link of a cell's chain: A = X (lane l: user l & 31, column 2s + (l >> 5)), B = W^T (item l & 31, the same column) ...
__device__ __forceinline__ f32x16 rec_link(float x, float w, f32x16 acc) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(x, w, acc, 0, 0, 0);
}

// ... after which accumulator register r of a lane, h = l >> 5, holds (user rec_user_of(r, h), item l & 31)
__device__ __forceinline__ int rec_user_of(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// What the chain's sum becomes before the epilogue: the bias adds in this order.  ubv / ibv are read only under a.ub / a.ib.
__device__ __forceinline__ float cell_sum(const RecArgs& a, float acc, float ubv, float ibv) {
    float x = acc;
    if (a.ub) x = x + ubv;
    if (a.ib) x = x + ibv;
    return x + a.bias0;
}

// The score of a cell.  (recommend_kernel without scores_out stages cell_sum and applies epilogue_exact to the staged sums
// that may enter a list: the same two halves, in the same order.)
__device__ __forceinline__ float cell_score(const RecArgs& a, float acc, float ubv, float ibv) {
    return epilogue_exact(cell_sum(a, acc, ubv, ibv), a.epi, a.scale);
}

// user u's range of the history CSR, clamped to the items array
__device__ __forceinline__ void hist_range(const long long* __restrict__ indptr, long long hist_len, long long u, long long& p,
                                           long long& q) {
    p = indptr[u];
    q = indptr[u + 1];
    p = p < 0 ? 0 : p;
    q = q > hist_len ? hist_len : q;
}

// is `item` among the ascending hist[p..q)?
__device__ __forceinline__ bool hist_has(const long long* __restrict__ hist, long long p, long long q, long long item) {
    while (p < q) {
        const long long m = (p + q) >> 1;
        const long long v = hist[m];
        if (v == item) return true;
        if (v < item) p = m + 1;
        else q = m;
    }
    return false;
}

// the first position of user u's history that holds an item >= bound (0 without a history, or beyond the last user)
__device__ __forceinline__ long long hist_lower_bound(const RecArgs& a, long long u, long long bound) {
    long long p = 0, q = 0;
    if (a.indptr && u < a.U) {
        hist_range(a.indptr, a.hist_len, u, p, q);
        while (p < q) {
            const long long m = (p + q) >> 1;
            if (a.hist[m] < bound) p = m + 1;
            else q = m;
        }
    }
    return p;
}

// [hp[u], hq[u]): the history of user u0 + u inside the slice [lo, hi) of the items (threads 0..63)
__device__ __forceinline__ void rec_slice_history(const RecArgs& a, long long u0, long long lo, long long hi, long long* hp,
                                                  long long* hq, int tid) {
    if (tid < 2 * REC_UT) ((tid & 1) ? hq : hp)[tid >> 1] = hist_lower_bound(a, u0 + (tid >> 1), (tid & 1) ? hi : lo);
}

// the tile's users: Xs [32][(D + 1) | 1], zero beyond column D and beyond user U, and their biases ubs [32]
__device__ __forceinline__ void rec_load_users(const RecArgs& a, long long u0, float* Xs, float* ubs, int tid) {
    const int D = a.D, Dx = (D + 1) | 1;
    for (int e = tid; e < REC_UT * Dx; e += 256) {
        const int u = e / Dx, c = e - u * Dx;
        Xs[e] = (c < D && u0 + u < a.U) ? a.X[(size_t)(u0 + u) * D + c] : 0.f;
    }
    if (tid < REC_UT) ubs[tid] = (a.ub && u0 + tid < a.U) ? a.ub[u0 + tid] : 0.f;
}

// The slice's rows of W go through LDS 128 items x 32 columns at a time (Ws [128][REC_WST]), fetched into registers one
// chunk ahead: the caller fetches (lo, 0) before its first step, and a step requests what the next one stages.
struct RecTile {
    float pre[16];      // element tid + 256 j of the chunk [128][32]

    __device__ __forceinline__ void fetch(const RecArgs& a, long long i0, long long hi, int c0, int tid) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int e = tid + 256 * j, item = e >> 5, col = e & 31;
            const long long it = i0 + item;
            pre[j] = (it < hi && c0 + col < a.D) ? a.W[(size_t)it * a.D + c0 + col] : 0.f;
        }
    }

    // The 32 users x items i0 + 32 wave .. + 31 of the slice [.., hi): per chunk, the image is staged between two barriers
    // (the first one also ends whatever the caller did with LDS since the step before), the next chunk is requested, and the
    // chain goes on.  In the first chunk staged() runs before the second barrier and fetched() behind the request.
    template <class Staged, class Fetched>
    __device__ __forceinline__ f32x16 step(const RecArgs& a, const float* Xs, float* Ws, long long i0, long long hi, int tid,
                                           Staged&& staged, Fetched&& fetched) {
        const int lane = tid & 63, wave = uniform(tid >> 6), li = lane & 31, h = lane >> 5;
        const int D = a.D, Dx = (D + 1) | 1;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int c0 = 0; c0 < D; c0 += REC_DK) {
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int e = tid + 256 * j;
                Ws[(e >> 5) * REC_WST + (e & 31)] = pre[j];
            }
            if (c0 == 0) staged();
            __syncthreads();
            if (c0 + REC_DK < D) fetch(a, i0, hi, c0 + REC_DK, tid);
            else if (i0 + REC_IB < hi) fetch(a, i0 + REC_IB, hi, 0, tid);
            if (c0 == 0) fetched();
            const int left = (D - c0 + 1) >> 1, steps = left < REC_DK / 2 ? left : REC_DK / 2;
            const float* xp = Xs + li * Dx + c0 + h;
            const float* wp = Ws + (wave * 32 + li) * REC_WST + h;
            for (int s = 0; s < steps; ++s) acc = rec_link(xp[2 * s], wp[2 * s], acc);
        }
        return acc;
    }
};

struct RecK : RecArgs {
    float* scores;
    u64* ws;
    long long slice_len;
    int k, S, cap;
    float inv_scale;
};

// A staged candidate: the exact key against the threshold, the mask test, then the push.
__device__ __forceinline__ void rec_push(const RecK& a, u64* buf, int* cnt, int ur, long long item, float score, u64 t,
                                         long long p, long long q) {
    u64 key = make_key(score, (uint32_t)item);
    if (!(key > t)) return;
    // [p, q): the user's history inside this slice (empty for most users of most slices)
    if ((a.mask_pad && item == 0) || hist_has(a.hist, p, q, item)) {
        key = make_key(-INFINITY, (uint32_t)item);
        if (!(key > t)) return;
    }
    const int pos = atomicAdd(&cnt[ur], 1);
    if (pos < a.cap) buf[(size_t)ur * a.cap + pos] = key;
}

// Workgroup (tile of 32 users, slice of the items).  The users' rows stay in LDS for the whole launch; the slice's rows of W go
// through the score tile above: wave w multiplies the 32 users with items 32w..32w+31 of the step, and the chain over the
// columns is one ascending fmaf chain from 0 (v_mfma_f32_32x32x2_f32).  A cell that may beat its user's threshold
// (epilogue_approx against the user's limit; with scores_out every cell's exact score is computed anyway) is staged in the
// wave's LDS list, eight registers' worth at a time, and the staged cells then get their exact score and key side by side on
// the lanes (one divergent pass per 512 cells instead of one per register); one above the threshold is pushed into the user's
// LDS list after the mask test (pad item; binary search in the part of the user's history that lies in the slice, found once
// per launch).  A list that could overflow in the next step is compacted to its best k, and threshold and limit rise.  A list
// holds up to cap - 128 >= k keys between steps, about 2k where LDS allows: rank counting costs (k + slack)^2 per slack
// survivors.  Each slice's sorted list goes to the workspace.
__global__ __launch_bounds__(256) void recommend_kernel(RecK a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
    const int li = lane & 31, h = lane >> 5;
    const int Dx = (a.D + 1) | 1, cap = a.cap, k = a.k, epi = a.epi;
    const bool dense = a.scores != nullptr;
    u64* buf = reinterpret_cast<u64*>(smem);              // [32][cap]
    u64* thr = buf + (size_t)REC_UT * cap;                // [32]
    long long* hp = reinterpret_cast<long long*>(thr + REC_UT);   // [32], [32]: the users' history inside the slice
    long long* hq = hp + REC_UT;
    int* cnt = reinterpret_cast<int*>(hq + REC_UT);       // [32]
    int* kept = cnt + REC_UT;                             // [32] length of the sorted part of a list
    float* lim = reinterpret_cast<float*>(kept + REC_UT); // [32]
    float* ubs = lim + REC_UT;                            // [32]
    float* Xs = ubs + REC_UT;                             // [32][Dx], zero beyond column D and beyond user U
    float* Ws = Xs + REC_UT * Dx;                         // [128][REC_WST]
    float* stg_x = Ws + REC_IB * REC_WST + wave * REC_STG;                                       // [4][REC_STG] scores ...
    unsigned short* stg_c = reinterpret_cast<unsigned short*>(Ws + REC_IB * REC_WST + 4 * REC_STG) + wave * REC_STG;   // ... cells
    const long long u0 = (long long)blockIdx.x * REC_UT;
    const long long lo = (long long)blockIdx.y * a.slice_len;
    const long long hi = lo + a.slice_len < a.N ? lo + a.slice_len : a.N;

    rec_load_users(a, u0, Xs, ubs, tid);
    if (tid < REC_UT) {
        thr[tid] = 0ull;
        lim[tid] = -INFINITY;
        cnt[tid] = 0;
        kept[tid] = 0;
    }
    rec_slice_history(a, u0, lo, hi, hp, hq, tid);

    RecTile tile;
    if (lo < hi) tile.fetch(a, lo, hi, 0, tid);
    for (long long i0 = lo; i0 < hi; i0 += REC_IB) {
        const long long item = i0 + wave * 32 + li;
        const bool ok = item < hi;
        const float ibv = (a.ib && ok) ? a.ib[item] : 0.f;
        // (the step's first barrier: the compaction of the step before is done as well)
        const f32x16 acc = tile.step(a, Xs, Ws, i0, hi, tid, [] {}, [] {});
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            int nst = 0;      // staged cells of this wave (uniform)
#pragma unroll
            for (int rr = 0; rr < 8; ++rr) {
                const int r = half * 8 + rr;
                const int ur = rec_user_of(r, h);
                const bool live = ok && u0 + ur < a.U;
                float x, rough;
                if (dense) {
                    x = rough = cell_score(a, acc[r], ubs[ur], ibv);
                    if (live) a.scores[(size_t)(u0 + ur) * a.N + item] = x;
                } else {
                    x = cell_sum(a, acc[r], ubs[ur], ibv);
                    rough = epilogue_approx(x, epi, a.scale, a.inv_scale);
                }
                const bool cand = live && !(rough < lim[ur]);
                const u64 m = __ballot(cand);
                if (m) {
                    if (cand) {
                        const int pos = nst + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
                        stg_x[pos] = x;
                        stg_c[pos] = (unsigned short)((ur << 5) | li);
                    }
                    nst += __popcll(m);
                }
            }
            __builtin_amdgcn_wave_barrier();
            for (int e = lane; e < nst; e += 64) {      // (LDS operations of a wave execute in order: the staged cells are there)
                const int code = stg_c[e], ur = code >> 5;
                const float sc = dense ? stg_x[e] : epilogue_exact(stg_x[e], epi, a.scale);
                rec_push(a, buf, cnt, ur, i0 + wave * 32 + (code & 31), sc, thr[ur], hp[ur], hq[ur]);
            }
        }
        __syncthreads();
        const bool last = i0 + REC_IB >= hi;
        for (int uu = wave; uu < REC_UT; uu += 4) {
            const int c = uniform(cnt[uu]);
            if (c > cap - REC_IB || (last && c > 0))
                wave_compact(buf + (size_t)uu * cap, uniform(kept[uu]), c, k, thr + uu, lim + uu, cnt + uu, kept + uu, epi, lane);
        }
    }
    __syncthreads();
    for (int uu = wave; uu < REC_UT; uu += 4) {
        if (u0 + uu >= a.U) break;
        const int c = cnt[uu];
        u64* out = a.ws + ((size_t)(u0 + uu) * a.S + blockIdx.y) * k;
        for (int p = lane; p < k; p += 64) out[p] = p < c ? buf[(size_t)uu * cap + p] : 0ull;
    }
}

// A dense [U, ld] score matrix (scores_out of fr_recommend_topk, fr_pair_mlp_scores): the pad column and the history cells
// become -inf (a wave per user)
__global__ __launch_bounds__(256) void recommend_mask_kernel(float* __restrict__ scores, const long long* __restrict__ indptr,
                                                             const long long* __restrict__ hist, long long hist_len,
                                                             long long U, long long N, long long ld, int mask_pad) {
    const int lane = threadIdx.x & 63;
    const long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= U) return;
    float* row = scores + (size_t)u * ld;
    if (mask_pad && lane == 0) row[0] = -INFINITY;
    if (!indptr) return;
    long long p, q;
    hist_range(indptr, hist_len, u, p, q);
    for (long long j = p + lane; j < q; j += 64) {
        const long long it = hist[j];
        if (it >= 0 && it < N) row[it] = -INFINITY;
    }
}

// Workgroup (row, slice of the columns) of a dense matrix: 8 loads in flight per thread, 256 cells tested per sub-step
// against the threshold, survivors pushed into one LDS list that the workgroup compacts when the next sub-step could
// overflow it.  The list's fill is tracked in a register (the barrier's own count), so every thread takes the same branch.
__global__ __launch_bounds__(256) void topk_rows_kernel(const float* __restrict__ mat, long long n_cols, long long ld, int k,
                                                        long long slice_len, int S, int cap, u64* __restrict__ ws) {
    extern __shared__ __align__(16) unsigned char smem[];
    u64* buf = reinterpret_cast<u64*>(smem);      // [cap]
    __shared__ u64 thr_s;
    __shared__ int cnt_s;
    const int tid = threadIdx.x;
    const long long row = blockIdx.x;
    const long long lo = (long long)blockIdx.y * slice_len;
    const long long hi = lo + slice_len < n_cols ? lo + slice_len : n_cols;
    const float* rp = mat + (size_t)row * ld;
    if (tid == 0) {
        thr_s = 0ull;
        cnt_s = 0;
    }
    __syncthreads();
    int c = 0;
    u64 t = 0ull;
    auto compact = [&]() {      // every thread calls it with the same c
        u64 mine[TR_Q];
        int rank[TR_Q];
        const int nq = (c + 255) >> 8;
#pragma unroll
        for (int q = 0; q < TR_Q; ++q) {
            const int i = tid + 256 * q;
            mine[q] = i < c ? buf[i] : 0ull;
            rank[q] = 0;
        }
        for (int j = 0; j < c; ++j) {
            const u64 kj = buf[j];
#pragma unroll
            for (int q = 0; q < TR_Q; ++q)
                if (q < nq) rank[q] += kj > mine[q] ? 1 : 0;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < TR_Q; ++q) {
            if (tid + 256 * q < c && rank[q] < k) {
                buf[rank[q]] = mine[q];
                if (rank[q] == k - 1) thr_s = mine[q];
            }
        }
        c = c < k ? c : k;
        if (tid == 0) cnt_s = c;
        __syncthreads();
        t = thr_s;
    };
    for (long long c0 = lo; c0 < hi; c0 += TR_STEP * TR_LOADS) {
        float v[TR_LOADS];
#pragma unroll
        for (int j = 0; j < TR_LOADS; ++j) {
            const long long col = c0 + j * TR_STEP + tid;
            v[j] = col < hi ? rp[col] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < TR_LOADS; ++j) {
            if (c0 + j * TR_STEP >= hi) break;
            const long long col = c0 + j * TR_STEP + tid;
            const u64 key = make_key(v[j], (uint32_t)col);
            const bool pass = col < hi && key > t;
            if (pass) {
                const int pos = atomicAdd(&cnt_s, 1);
                if (pos < cap) buf[pos] = key;
            }
            c += __syncthreads_count(pass);
            if (c > cap - TR_STEP) compact();
        }
    }
    compact();
    u64* out = ws + ((size_t)row * S + blockIdx.y) * k;
    for (int p = tid; p < k; p += 256) out[p] = p < c ? buf[p] : 0ull;
}

// The S sorted lists of a user -> its k best, in order: the rank of a key is its position in its own list plus, from every
// other list, the number of keys above it (binary search).  Padding keys (0) rank below every cell.  Values are read back
// from `mat` (fr_topk_rows: the cell's own bits) or rebuilt from the key.
__global__ __launch_bounds__(256) void topk_merge_kernel(const u64* __restrict__ ws, int S, int k, const float* __restrict__ mat,
                                                         long long ld, float* __restrict__ val, long long* __restrict__ idx) {
    extern __shared__ __align__(16) unsigned char smem[];
    u64* L = reinterpret_cast<u64*>(smem);
    const long long u = blockIdx.x;
    const int n = S * k;
    for (int e = threadIdx.x; e < n; e += 256) L[e] = ws[(size_t)u * n + e];
    __syncthreads();
    for (int e = threadIdx.x; e < n; e += 256) {
        const u64 key = L[e];
        if (!key) continue;
        const int s = e / k;
        int rank = e - s * k;
        for (int s2 = 0; s2 < S && rank < k; ++s2) {
            if (s2 == s) continue;
            const u64* l = L + s2 * k;
            int p = 0, q = k;
            while (p < q) {
                const int m = (p + q) >> 1;
                if (l[m] > key) p = m + 1;
                else q = m;
            }
            rank += p;
        }
        if (rank < k) {
            const uint32_t id = key_id(key);
            idx[(size_t)u * k + rank] = (long long)id;
            val[(size_t)u * k + rank] = mat ? mat[(size_t)u * ld + id] : key_value(key);
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
// Slices of a range of n cells ranked for `groups` workgroup rows: as many workgroups as fill the chip once (`want`), no slice
// shorter than min_len, a length that is a multiple of gran, and S * k keys that fit the merge kernel's LDS.  forced > 0
// (the caller's argument, else FAIRREC_REC_SLICES) replaces the first two rules.  Returns 0 for a forced count out of range.
static int plan_slices(long long n, int k, long long groups, long long want, long long min_len, long long gran, int forced,
                       long long* slice_len) {
    const int s_max = MERGE_KEYS_MAX / k < REC_SLICES_MAX ? MERGE_KEYS_MAX / k : REC_SLICES_MAX;
    if (forced <= 0) {
        const char* e = getenv("FAIRREC_REC_SLICES");
        if (e && *e) forced = atoi(e);
    }
    long long S;
    if (forced > 0) {
        if (forced > s_max) return 0;
        S = forced;
    } else {
        S = want / groups;
        const long long by_len = n / min_len;
        if (S > by_len) S = by_len;
        if (S > s_max) S = s_max;
        if (S < 1) S = 1;
    }
    long long len = (n + S - 1) / S;
    len = (len + gran - 1) / gran * gran;
    *slice_len = len;
    return (int)((n + len - 1) / len);
}

// The arguments every entry reads of an fr_rec_args (k, slices and scores_out are fr_recommend_topk's alone).  Every launch
// puts n_users, or its tiles, into a grid dimension.
static int eval_check(const fr_rec_args* a, const char* who) {
    FR_CHECK_ARG(a, "%s: null argument struct", who);
    FR_CHECK_ARG(a->X && a->W, "%s: null X or W", who);
    FR_CHECK_ARG(a->n_users >= 0 && a->n_users <= 0x7fffffffLL && a->n_items >= 1 && a->n_items <= 0x7fffffffLL,
                 "%s: bad n_users / n_items", who);
    FR_CHECK_ARG(a->dim >= 1 && a->dim <= 256, "%s: dim %d not in 1..256", who, a->dim);
    FR_CHECK_ARG(a->epilogue >= 0 && a->epilogue <= 2, "%s: unknown epilogue %d", who, a->epilogue);
    FR_CHECK_ARG(a->epilogue != 1 || a->scale > 0.f, "%s: epilogue 1 needs scale > 0", who);
    return check_hist_csr(a->hist_indptr, a->hist_items, a->hist_len, a->hist_sorted, who);
}

static int rec_check(const fr_rec_args* a, const char* who) {
    int rc;
    if ((rc = eval_check(a, who))) return rc;
    FR_CHECK_ARG(a->k >= 1 && a->k <= FR_TOPK_MAX && a->k <= a->n_items, "%s: k %d not in 1..min(%d, n_items)", who, a->k,
                 FR_TOPK_MAX);
    FR_CHECK_ARG(a->slices >= 0, "%s: slices < 0", who);
    return FR_OK;
}

// the kernels' share of the arguments
static void rec_fill(RecArgs& p, const fr_rec_args* a) {
    p.X = a->X;
    p.W = a->W;
    p.ub = a->user_bias;
    p.ib = a->item_bias;
    p.indptr = reinterpret_cast<const long long*>(a->hist_indptr);
    p.hist = reinterpret_cast<const long long*>(a->hist_items);
    p.U = a->n_users;
    p.N = a->n_items;
    p.hist_len = a->hist_indptr ? a->hist_len : 0;
    p.D = a->dim;
    p.epi = a->epilogue;
    p.mask_pad = a->mask_pad ? 1 : 0;
    p.bias0 = a->bias0;
    p.scale = a->scale;
}

static int rec_plan(const fr_rec_args* a, long long* slice_len) {
    const long long tiles = (a->n_users + REC_UT - 1) / REC_UT;
    return plan_slices(a->n_items, a->k, tiles < 1 ? 1 : tiles, 2 * 256, 1024, REC_IB, a->slices, slice_len);
}

static size_t rec_lds_bytes(int D, int cap) {
    const int Dx = (D + 1) | 1;
    return (size_t)REC_UT * cap * 8 + REC_UT * (8 + 8 + 8 + 4 + 4 + 4 + 4) + (size_t)REC_UT * Dx * 4 + (size_t)REC_IB * REC_WST * 4 +
           4 * REC_STG * (4 + 2);
}

// Length of a user's LDS list: k + 128 at least (a step pushes up to 128 keys), 2k + 128 where it fits (rank counting costs
// (k + slack)^2 per slack survivors: slack = k is the cheapest), shortened to keep two workgroups on a CU when half of that
// slack or more remains.
static int rec_cap(int D, int k) {
    const int lo = k + REC_IB;
    int cap = 2 * k + REC_IB < REC_CAP_MAX ? 2 * k + REC_IB : REC_CAP_MAX;
    const size_t fixed = rec_lds_bytes(D, 0);
    const int fit1 = (int)((REC_LDS_MAX - fixed) / (REC_UT * 8)), fit2 = (int)((REC_LDS_MAX / 2 - fixed) / (REC_UT * 8));
    if (cap > fit2 && fit2 >= lo + (k + 1) / 2) cap = fit2;
    if (cap > fit1) cap = fit1;
    return cap < lo ? lo : cap;
}

// ---- full-sort evaluation without the matrix: single cells of it, and the rank sums of GAUC ------------------------------
constexpr int MR_C = 128;                    // thresholds of a user in LDS per pass over its slice
constexpr uint32_t MR_SKIP = 0xffffffffu;    // a key that is no positive (listed twice, or outside the matrix): above every cell
constexpr uint32_t MR_NAN = 0xfffffffeu;     // a NaN positive: above every cell as well, and counted

struct CellK : RecArgs {
    const long long* cu;      // the cells: (cu[c], ci[c]) -> score[c] ...
    const long long* ci;
    const long long* keys;    // ... or the sorted keys user * N + item -> tb[c] = the score's image in the order (MR_SKIP, MR_NAN)
    float* score;
    uint32_t* tb;
    uint32_t* err;
    long long n;
};

// A wave scores 32 cells: the chain of the score tile over the cells' 32 user rows and 32 item rows, read from memory as they
// lie (column 2s + (l >> 5) of link s, zero beyond D: the same ceil(D / 2) links), of which cell c is the diagonal element
// (c, c) -- the register r of lane c or c + 32 with rec_user_of(r, h) = c.  cell_score and the mask (as recommend_mask_kernel
// applies it) follow.
__global__ __launch_bounds__(256) void recommend_cells_kernel(CellK a) {
    const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
    const long long c = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32 + li;
    const bool in = c < a.n;
    long long u = 0, it = 0;
    bool skip = false;
    if (in) {
        if (a.keys) {
            const long long key = a.keys[c];
            skip = key < 0 || key >= a.U * a.N || (c > 0 && a.keys[c - 1] == key);
            if (!skip) {
                u = key / a.N;
                it = key - u * a.N;
            }
        } else {
            u = a.cu[c];
            it = a.ci[c];
            if (u < 0 || u >= a.U || it < 0 || it >= a.N) {
                skip = true;
                u = it = 0;      // (its loads stay on row 0)
                if (h == 0) atomicOr(a.err, FR_DEV_ERR_INDEX_RANGE);
            }
        }
    }
    const float* xr = a.X + (size_t)u * a.D;
    const float* wr = a.W + (size_t)it * a.D;
    const int D = a.D, steps = (D + 1) >> 1;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int s0 = 0; s0 < steps; s0 += 8) {
        float xa[8], wb[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int col = 2 * (s0 + j) + h;
            xa[j] = col < D ? xr[col] : 0.f;
            wb[j] = col < D ? wr[col] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (s0 + j < steps) acc = rec_link(xa[j], wb[j], acc);
    }
    float x = 0.f;
    bool diag = false;      // one lane of each pair (l, l + 32) holds the diagonal
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if (rec_user_of(r, h) == li) {
            x = acc[r];
            diag = true;
        }
    }
    if (!in || !diag) return;
    if (skip) {
        if (a.keys) a.tb[c] = MR_SKIP;
        else a.score[c] = __uint_as_float(0x7fc00000u);
        return;
    }
    x = cell_score(a, x, a.ub ? a.ub[u] : 0.f, a.ib ? a.ib[it] : 0.f);
    bool masked = a.mask_pad && it == 0;
    if (!masked && a.indptr) {
        long long p, q;
        hist_range(a.indptr, a.hist_len, u, p, q);
        masked = hist_has(a.hist, p, q, it);
    }
    if (masked) x = -INFINITY;
    if (a.keys) a.tb[c] = x != x ? MR_NAN : order_bits(x);
    else a.score[c] = x;
}

struct MrK : RecArgs {
    const long long* keys;
    const uint32_t* tb;
    u64* out;
    long long slice_len, n_pos;
};

// out[u] = { positives, 0, positives } of user u (a thread each): the `+ 1` of every positive's rank, and pos_len
__global__ __launch_bounds__(256) void recommend_meanrank_init_kernel(const long long* __restrict__ keys, const uint32_t* __restrict__ tb,
                                                                      long long n_pos, long long U, long long N, u64* __restrict__ out) {
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    if (u >= U) return;
    long long b[2];
    for (int e = 0; e < 2; ++e) {
        long long p = 0, q = n_pos;
        while (p < q) {
            const long long m = (p + q) >> 1;
            if (keys[m] < (u + e) * N) p = m + 1;
            else q = m;
        }
        b[e] = p;
    }
    u64 n = 0;
    for (long long p = b[0]; p < b[1]; ++p) n += tb[p] != MR_SKIP ? 1 : 0;
    out[u * 3 + 0] = n;
    out[u * 3 + 1] = 0;
    out[u * 3 + 2] = n;
}

// Workgroup (tile of 32 users, slice of the items) on the score tile of recommend_kernel: a cell counted here is the cell
// ranked there.  Every cell gets its exact score (cell_score) and the mask: the pad item, and a bit per (user,
// item of the step) set from the users' ascending histories, which 8 threads per user walk along with the steps (the next 8
// entries of a user wait in registers; a step without history loads nothing).  A live cell (not masked, above -inf) adds 1 to
// user_len.  The scores of the user's positives (recommend_cells_kernel's images in the order) are its thresholds, up to MR_C
// of them sorted in LDS: a live cell at or above the lowest one is staged, and adds lb + ub to the user's sum, lb (ub) = the
// thresholds below (not above) it -- 2 for every positive it beats and 1 for every positive it ties with, which is what
// 2 * pos_rank_sum counts beyond the positives themselves.  A tile whose longest list has more than MR_C thresholds goes over
// its slice once per MR_C of them.  Integer LDS and global atomics only: the same result on every call.
__global__ __launch_bounds__(256, 2) void recommend_meanrank_kernel(MrK a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
    const int li = lane & 31, h = lane >> 5;
    const int Dx = (a.D + 1) | 1;
    u64* sum = reinterpret_cast<u64*>(smem);                      // [32]
    long long* hp = reinterpret_cast<long long*>(sum + REC_UT);   // [32], [32]: the users' history inside the slice
    long long* hq = hp + REC_UT;
    long long* pp = hq + REC_UT;                                  // [32], [32]: the users' keys
    long long* pq = pp + REC_UT;
    uint32_t* thr = reinterpret_cast<uint32_t*>(pq + REC_UT);     // [32][MR_C] ascending
    uint32_t* low = thr + REC_UT * MR_C;                          // [32] the lowest threshold of the pass
    int* nt = reinterpret_cast<int*>(low + REC_UT);               // [32] thresholds of the pass
    int* ulen = nt + REC_UT;                                      // [32]
    uint32_t* mbits = reinterpret_cast<uint32_t*>(ulen + REC_UT); // [32][4] history bits of the step's 128 items
    float* ubs = reinterpret_cast<float*>(mbits + REC_UT * 4);    // [32]
    float* Xs = ubs + REC_UT;                                     // [32][Dx]
    float* Ws = Xs + REC_UT * Dx;                                 // [128][REC_WST]
    uint32_t* stg_x = reinterpret_cast<uint32_t*>(Ws + REC_IB * REC_WST) + wave * REC_STG;      // [4][REC_STG] images ...
    unsigned short* stg_c = reinterpret_cast<unsigned short*>(Ws + REC_IB * REC_WST + 4 * REC_STG) + wave * REC_STG;   // ... users
    const long long u0 = (long long)blockIdx.x * REC_UT;
    const long long lo = (long long)blockIdx.y * a.slice_len;
    const long long hi = lo + a.slice_len < a.N ? lo + a.slice_len : a.N;
    const bool hist = a.indptr != nullptr;

    rec_load_users(a, u0, Xs, ubs, tid);
    if (tid < REC_UT) {
        sum[tid] = 0ull;
        ulen[tid] = 0;
    }
    rec_slice_history(a, u0, lo, hi, hp, hq, tid);
    if (tid >= 2 * REC_UT && tid < 4 * REC_UT) {      // the users' ranges of the sorted keys
        const int u = (tid - 2 * REC_UT) >> 1;
        long long p = 0, q = 0;
        if (u0 + u < a.U) {
            const long long bound = (u0 + u + (tid & 1)) * a.N;
            q = a.n_pos;
            while (p < q) {
                const long long m = (p + q) >> 1;
                if (a.keys[m] < bound) p = m + 1;
                else q = m;
            }
        }
        ((tid & 1) ? pq : pp)[u] = p;
    }
    __syncthreads();
    long long longest = 0;
    for (int u = 0; u < REC_UT; ++u) longest = pq[u] - pp[u] > longest ? pq[u] - pp[u] : longest;
    const long long npass = longest > MR_C ? (longest + MR_C - 1) / MR_C : 1;
    const int gu = tid >> 3, sub = tid & 7;      // history walk: 8 threads per user
    const long long hqg = hq[gu];

    RecTile tile;
    for (long long pass = 0; pass < npass; ++pass) {
        for (int uu = wave; uu < REC_UT; uu += 4) {      // a wave sorts a user's thresholds of this pass by counting
            const long long base = pp[uu] + pass * MR_C, left = pq[uu] - base;
            const int n = left < 0 ? 0 : (left > MR_C ? MR_C : (int)left);
            uint32_t* t = thr + uu * MR_C;
            uint32_t mine[MR_C / 64];
            int rank[MR_C / 64];
#pragma unroll
            for (int q = 0; q < MR_C / 64; ++q) {
                const int i = lane + 64 * q;
                mine[q] = i < n ? a.tb[base + i] : MR_SKIP;
                t[i] = mine[q];
                rank[q] = 0;
            }
            __builtin_amdgcn_wave_barrier();
            for (int j = 0; j < n; ++j) {      // (LDS operations of a wave execute in order)
                const uint32_t v = t[j];
#pragma unroll
                for (int q = 0; q < MR_C / 64; ++q) rank[q] += (v < mine[q] || (v == mine[q] && j < lane + 64 * q)) ? 1 : 0;
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int q = 0; q < MR_C / 64; ++q) {
                if (lane + 64 * q < n) {
                    t[rank[q]] = mine[q];
                    if (rank[q] == 0) low[uu] = mine[q];
                }
            }
            if (lane == 0) {
                nt[uu] = n;
                if (n == 0) low[uu] = MR_SKIP;
            }
        }
        long long cur = hp[gu];
        long long hv = (hist && cur + sub < hqg) ? a.hist[cur + sub] : 0x7fffffffffffffffLL;
        if (lo < hi) tile.fetch(a, lo, hi, 0, tid);
        __syncthreads();
        for (long long i0 = lo; i0 < hi; i0 += REC_IB) {
            const long long item = i0 + wave * 32 + li;
            const bool ok = item < hi;
            const float ibv = (a.ib && ok) ? a.ib[item] : 0.f;
            const f32x16 acc = tile.step(
                a, Xs, Ws, i0, hi, tid,
                [&] {      // (behind the step's first barrier the history bits of the step before are free)
                    if (hist && tid < REC_UT * 4) mbits[tid] = 0u;
                },
                [&] {      // the users' history entries inside [i0, i0 + 128): ascending, so a prefix of the 8 waiting
                    if (!hist) return;
                    const long long end = i0 + REC_IB;
                    for (;;) {
                        const bool hit = hv < end;
                        const u64 m = __ballot(hit);
                        if (!m) break;
                        if (hit && hv >= i0) atomicOr(&mbits[gu * 4 + (int)((hv - i0) >> 5)], 1u << (int)((hv - i0) & 31));
                        const int nh = __popcll((m >> (lane & 56)) & 0xffull);
                        if (nh) {
                            cur += nh;
                            hv = cur + sub < hqg ? a.hist[cur + sub] : 0x7fffffffffffffffLL;
                        }
                    }
                });
            if (hist) __syncthreads();      // the history bits are set
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                int nst = 0;      // staged cells of this wave (uniform)
#pragma unroll
                for (int rr = 0; rr < 8; ++rr) {
                    const int r = half * 8 + rr;
                    const int ur = rec_user_of(r, h);
                    const float x = cell_score(a, acc[r], ubs[ur], ibv);
                    bool alive = ok && u0 + ur < a.U && x > -INFINITY;      // (a NaN is no live cell)
                    if (a.mask_pad && item == 0) alive = false;
                    if (hist && ((mbits[ur * 4 + wave] >> li) & 1u)) alive = false;
                    if (pass == 0) {      // user_len: the live cells of the two users of this register
                        const u64 am = __ballot(alive);
                        const int na = __popc((uint32_t)(h ? am >> 32 : am));
                        if (li == 0 && na) atomicAdd(&ulen[ur], na);
                    }
                    const uint32_t ob = order_bits(x);
                    const bool cand = alive && ob >= low[ur];
                    const u64 m = __ballot(cand);
                    if (m) {
                        if (cand) {
                            const int pos = nst + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
                            stg_x[pos] = ob;
                            stg_c[pos] = (unsigned short)ur;
                        }
                        nst += __popcll(m);
                    }
                }
                __builtin_amdgcn_wave_barrier();
                for (int e = lane; e < nst; e += 64) {      // (LDS operations of a wave execute in order: the staged cells are there)
                    const int ur = stg_c[e];
                    const uint32_t ob = stg_x[e];
                    const uint32_t* t = thr + ur * MR_C;
                    const int n = nt[ur];
                    int p = 0, q = n;
                    while (p < q) {
                        const int m = (p + q) >> 1;
                        if (t[m] < ob) p = m + 1;
                        else q = m;
                    }
                    const int lb = p;
                    q = n;
                    while (p < q) {
                        const int m = (p + q) >> 1;
                        if (t[m] <= ob) p = m + 1;
                        else q = m;
                    }
                    atomicAdd(&sum[ur], (u64)(lb + p));
                }
            }
        }
        __syncthreads();      // every staged cell is counted before the next pass's thresholds come in
    }
    if (tid < REC_UT && u0 + tid < a.U) {
        atomicAdd(&a.out[(u0 + tid) * 3 + 0], sum[tid]);
        atomicAdd(&a.out[(u0 + tid) * 3 + 1], (u64)ulen[tid]);
    }
}

static size_t mr_lds_bytes(int D) {
    const int Dx = (D + 1) | 1;
    return (size_t)REC_UT * (5 * 8 + MR_C * 4 + 4 + 4 + 4 + 16 + 4) + (size_t)REC_UT * Dx * 4 + (size_t)REC_IB * REC_WST * 4 +
           4 * REC_STG * (4 + 2);
}

static int launch_cells(const fr_rec_args* a, const long long* cu, const long long* ci, const long long* keys, long long n,
                        float* score, uint32_t* tb, uint32_t* err, hipStream_t stream) {
    CellK p;
    rec_fill(p, a);
    p.cu = cu;
    p.ci = ci;
    p.keys = keys;
    p.score = score;
    p.tb = tb;
    p.err = err;
    p.n = n;
    ProfScope prof(K_REC_CELLS, stream);
    FR_LAUNCH(prof, recommend_cells_kernel, dim3((unsigned)((n + 127) / 128)), dim3(256), 0, stream, p);
    FR_CHECK_LAUNCH();
    return FR_OK;
}

int launch_score_mask(float* scores, long long U, long long N, long long ld, const long long* indptr, const long long* hist,
                      long long hist_len, int mask_pad, hipStream_t stream) {
    ProfScope prof(K_TOPK_ROWS, stream);
    FR_LAUNCH(prof, recommend_mask_kernel, dim3((unsigned)((U + 3) / 4)), dim3(256), 0, stream, scores, indptr, hist,
              indptr ? hist_len : 0LL, U, N, ld, mask_pad ? 1 : 0);
    FR_CHECK_LAUNCH();
    return FR_OK;
}

}  // namespace fr

using namespace fr;

extern "C" size_t fr_recommend_topk_workspace_bytes(const fr_rec_args* a) {
    if (rec_check(a, "fr_recommend_topk_workspace_bytes")) return 0;
    long long len;
    const int S = rec_plan(a, &len);
    return (size_t)a->n_users * S * a->k * sizeof(u64);
}

extern "C" int fr_recommend_topk(const fr_rec_args* a, float* val_out, int64_t* idx_out, void* ws, size_t ws_bytes,
                                 void* stream_) {
    int rc;
    if ((rc = rec_check(a, "fr_recommend_topk"))) return rc;
    FR_CHECK_ARG(val_out && idx_out, "fr_recommend_topk: null output");
    long long len;
    const int S = rec_plan(a, &len);
    FR_CHECK_ARG(S >= 1, "fr_recommend_topk: slice count out of range (at most %d slices, and slices * k <= %d)", REC_SLICES_MAX,
                 MERGE_KEYS_MAX);
    const size_t need = (size_t)a->n_users * S * a->k * sizeof(u64);
    FR_CHECK_ARG(need == 0 || (ws && ws_bytes >= need && ((uintptr_t)ws & 7) == 0),
                 "fr_recommend_topk: workspace too small or misaligned (%zu < %zu bytes)", ws_bytes, need);
    if (a->n_users == 0) return FR_OK;
    hipStream_t stream = (hipStream_t)stream_;
    RecK p;
    rec_fill(p, a);
    p.scores = a->scores_out;
    p.ws = static_cast<u64*>(ws);
    p.slice_len = len;
    p.k = a->k;
    p.S = S;
    p.cap = rec_cap(a->dim, a->k);
    p.inv_scale = a->epilogue == 1 ? 1.0f / a->scale : 1.0f;
    const size_t ldsb = rec_lds_bytes(p.D, p.cap);
    static size_t have = 0;
    if (ldsb > have) {
        FR_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(recommend_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsb));
        have = ldsb;
    }
    const long long tiles = (a->n_users + REC_UT - 1) / REC_UT;
    FR_CHECK_ARG(tiles <= 0x7fffffffLL, "fr_recommend_topk: too many users");
    ProfScope prof(K_RECOMMEND, stream);
    prof_work(K_RECOMMEND, 2.0 * (double)a->n_users * (double)a->n_items * a->dim);
    FR_LAUNCH(prof, recommend_kernel, dim3((unsigned)tiles, (unsigned)S), dim3(256), ldsb, stream, p);
    FR_CHECK_LAUNCH();
    if (a->scores_out && (a->mask_pad || a->hist_indptr) &&
        (rc = launch_score_mask(a->scores_out, p.U, p.N, p.N, p.indptr, p.hist, p.hist_len, p.mask_pad, stream)))
        return rc;
    ProfScope prof2(K_TOPK_ROWS, stream);
    FR_LAUNCH(prof2, topk_merge_kernel, dim3((unsigned)a->n_users), dim3(256), (size_t)S * a->k * sizeof(u64), stream,
              (const u64*)p.ws, S, (int)a->k, (const float*)nullptr, 0LL, val_out, reinterpret_cast<long long*>(idx_out));
    FR_CHECK_LAUNCH();
    return FR_OK;
}

extern "C" int fr_recommend_cells(const fr_rec_args* a, const int64_t* cell_user, const int64_t* cell_item, int64_t n_cells,
                                  float* score_out, uint32_t* err_flag, void* stream_) {
    int rc;
    if ((rc = eval_check(a, "fr_recommend_cells"))) return rc;
    FR_CHECK_ARG(n_cells >= 0 && n_cells <= (0x7fffffffLL << 7), "fr_recommend_cells: n_cells out of range");
    FR_CHECK_ARG(err_flag && (n_cells == 0 || (cell_user && cell_item && score_out)), "fr_recommend_cells: null pointer");
    FR_CHECK_ARG(n_cells == 0 || a->n_users >= 1, "fr_recommend_cells: cells of an empty set of users");
    if (n_cells == 0) return FR_OK;
    return launch_cells(a, reinterpret_cast<const long long*>(cell_user), reinterpret_cast<const long long*>(cell_item), nullptr,
                        n_cells, score_out, nullptr, err_flag, (hipStream_t)stream_);
}

extern "C" size_t fr_recommend_meanrank_workspace_bytes(const fr_rec_args* a, int64_t n_pos) {
    if (eval_check(a, "fr_recommend_meanrank_workspace_bytes") || n_pos < 0) return 0;
    return (size_t)n_pos * sizeof(uint32_t);
}

extern "C" int fr_recommend_meanrank(const fr_rec_args* a, const int64_t* pos_keys, int64_t n_pos, int64_t* out, void* ws,
                                     size_t ws_bytes, uint32_t* err_flag, void* stream_) {
    int rc;
    if ((rc = eval_check(a, "fr_recommend_meanrank"))) return rc;
    FR_CHECK_ARG(n_pos >= 0 && n_pos <= (0x7fffffffLL << 7), "fr_recommend_meanrank: n_pos out of range");
    FR_CHECK_ARG(out && err_flag && (n_pos == 0 || pos_keys), "fr_recommend_meanrank: null pointer");
    const size_t need = (size_t)n_pos * sizeof(uint32_t);
    FR_CHECK_ARG(need == 0 || (ws && ws_bytes >= need && ((uintptr_t)ws & 3) == 0),
                 "fr_recommend_meanrank: workspace too small or misaligned (%zu < %zu bytes)", ws_bytes, need);
    const long long tiles = (a->n_users + REC_UT - 1) / REC_UT;
    long long len;
    const int S = plan_slices(a->n_items, 1, tiles < 1 ? 1 : tiles, 2 * 256, 1024, REC_IB, 0, &len);
    FR_CHECK_ARG(S >= 1, "fr_recommend_meanrank: FAIRREC_REC_SLICES out of range (at most %d)", REC_SLICES_MAX);
    if (a->n_users == 0) return FR_OK;
    hipStream_t stream = (hipStream_t)stream_;
    uint32_t* tb = static_cast<uint32_t*>(ws);
    const long long* keys = reinterpret_cast<const long long*>(pos_keys);
    if (n_pos > 0 && (rc = launch_cells(a, nullptr, nullptr, keys, n_pos, nullptr, tb, err_flag, stream))) return rc;
    MrK p;
    rec_fill(p, a);
    p.keys = keys;
    p.tb = tb;
    p.out = reinterpret_cast<u64*>(out);
    p.slice_len = len;
    p.n_pos = n_pos;
    const size_t ldsb = mr_lds_bytes(p.D);
    static size_t have = 0;
    if (ldsb > have) {
        FR_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(recommend_meanrank_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsb));
        have = ldsb;
    }
    ProfScope prof(K_REC_MEANRANK, stream);
    prof_work(K_REC_MEANRANK, 2.0 * (double)a->n_users * (double)a->n_items * a->dim);
    FR_LAUNCH(prof, recommend_meanrank_init_kernel, dim3((unsigned)((a->n_users + 255) / 256)), dim3(256), 0, stream, keys,
              (const uint32_t*)tb, (long long)n_pos, p.U, p.N, p.out);
    FR_CHECK_LAUNCH();
    FR_LAUNCH(prof, recommend_meanrank_kernel, dim3((unsigned)tiles, (unsigned)S), dim3(256), ldsb, stream, p);
    FR_CHECK_LAUNCH();
    return FR_OK;
}

static int rows_check(int64_t n_rows, int64_t n_cols, int32_t k, int32_t slices, const char* who) {
    FR_CHECK_ARG(n_rows >= 0 && n_rows <= 0x7fffffffLL && n_cols >= 1 && n_cols <= 0x7fffffffLL, "%s: bad shape", who);
    FR_CHECK_ARG(k >= 1 && k <= FR_TOPK_MAX && k <= n_cols, "%s: k %d not in 1..min(%d, n_cols)", who, k, FR_TOPK_MAX);
    FR_CHECK_ARG(slices >= 0, "%s: slices < 0", who);
    return FR_OK;
}

static int rows_plan(int64_t n_rows, int64_t n_cols, int32_t k, int32_t slices, long long* len) {
    return plan_slices(n_cols, k, n_rows < 1 ? 1 : n_rows, 8 * 256, 4096, TR_STEP, slices, len);
}

extern "C" size_t fr_topk_rows_workspace_bytes(int64_t n_rows, int64_t n_cols, int32_t k, int32_t slices) {
    if (rows_check(n_rows, n_cols, k, slices, "fr_topk_rows_workspace_bytes")) return 0;
    long long len;
    const int S = rows_plan(n_rows, n_cols, k, slices, &len);
    return (size_t)n_rows * S * k * sizeof(u64);
}

extern "C" int fr_topk_rows(const float* scores, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t k, int32_t slices,
                            float* val_out, int64_t* idx_out, void* ws, size_t ws_bytes, void* stream_) {
    int rc;
    if ((rc = rows_check(n_rows, n_cols, k, slices, "fr_topk_rows"))) return rc;
    FR_CHECK_ARG(scores && val_out && idx_out, "fr_topk_rows: null pointer");
    FR_CHECK_ARG(ld >= n_cols, "fr_topk_rows: ld < n_cols");
    long long len;
    const int S = rows_plan(n_rows, n_cols, k, slices, &len);
    FR_CHECK_ARG(S >= 1, "fr_topk_rows: slice count out of range (at most %d slices, and slices * k <= %d)", REC_SLICES_MAX,
                 MERGE_KEYS_MAX);
    const size_t need = (size_t)n_rows * S * k * sizeof(u64);
    FR_CHECK_ARG(need == 0 || (ws && ws_bytes >= need && ((uintptr_t)ws & 7) == 0),
                 "fr_topk_rows: workspace too small or misaligned (%zu < %zu bytes)", ws_bytes, need);
    if (n_rows == 0) return FR_OK;
    hipStream_t stream = (hipStream_t)stream_;
    const int cap = k + 2 * TR_STEP;
    ProfScope prof(K_TOPK_ROWS, stream);
    FR_LAUNCH(prof, topk_rows_kernel, dim3((unsigned)n_rows, (unsigned)S), dim3(256), (size_t)cap * sizeof(u64), stream, scores,
              (long long)n_cols, (long long)ld, (int)k, len, S, cap, static_cast<u64*>(ws));
    FR_CHECK_LAUNCH();
    FR_LAUNCH(prof, topk_merge_kernel, dim3((unsigned)n_rows), dim3(256), (size_t)S * k * sizeof(u64), stream,
              (const u64*)ws, S, (int)k, scores, (long long)ld, val_out, reinterpret_cast<long long*>(idx_out));
    FR_CHECK_LAUNCH();
    return FR_OK;
}
