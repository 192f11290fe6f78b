// Evaluation metrics on the device: the reductions of recbole/evaluator/metrics.py without the host
// round trip and without the reference's Python loops over interactions (:950-960) or over items x groups (:1331-1335).
//
//   topk_metrics_kernel      Hit / MRR / NDCG / Recall / Precision / MAP @ 1..K from the `rec.topk` matrix (:40-232)
//   topk_grouped_kernel      the same six metrics per group of users (groups as segments of a permutation), and
//   gauc_grouped_kernel      GAUC's two sums per group from `rec.meanrank`: a wave per chunk of 64 members, any number of groups
//   topk_user_terms_kernel   every row's own terms of chosen (metric, cut-off) pairs, and
//   gauc_user_terms_kernel   every user's GAUC term and weight: the columns fr_bootstrap_group_sums (bootstrap.hip) resamples
//   group_sums_kernel        per (item segment, group): sum of scores, count, count of positives -- the tables every
//                            fairness metric starts from (:948-970, :1322-1335); same segment machinery as the FOCF
//                            fairness term (16 lanes per segment, fixed order)
//   fair_from_stats_kernel   Value / Absolute / Under / Over unfairness (:972-979 and siblings) and DifferentialFairness
//                            (:1337-1342, float32 tables like the reference) as means over the items
//   df_cells_kernel          DifferentialFairness for any number of groups from the members sorted by (item, group): the
//                            same table entries and the same epsilon, without the [items, groups] table
// All sums are double precision in a fixed order (bit-reproducible).
//
// Edges the reference leaves to chance, as they are pinned here (tests/test_metrics_kernels_hip.py, DESIGN.md "Evaluation
// quirks"):
//   * a `rec.topk` row with zero positives: its NDCG@k is 0 (the reference's idcg index min(k, 0) - 1 wraps to the last
//     rank, so it divides by the ideal DCG of all K ranks), its MAP@k is 0, its Recall@k is 0 / 0 = NaN as in the
//     reference -- and so is every Recall@k of that evaluation;
//   * fr_eval_hits: a list entry outside [0, n_items) is never a hit (its key would lie in another row's range);
//   * fr_group_sums: a member whose group index is outside [0, n_groups) is counted in no cell;
//   * DifferentialFairness: a pair of table entries one of whose float32 logarithms is NaN (a non-positive entry, from a
//     negative score sum) does not enter the item's maximum, and the result stays finite; numpy's maximum in the
//     reference's formula would return NaN there (oracle.metrics.differential_fairness does).
#include "eval_common.hpp"
#include "kernels.hpp"

namespace fr {

// A block of four waves adds up through LDS: every wave leaves its total in red4[wave] (wave_sum_to_lds), and after the
// caller's barrier block_sum4 folds the four in wave order, ((w0 + w1) + w2) + w3 -- the one association every block sum here has.
template <class T>
__device__ __forceinline__ void wave_sum_to_lds(T v, T* __restrict__ red4) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
}

template <class T>
__device__ __forceinline__ T block_sum4(const T* __restrict__ red4) {
    return ((red4[0] + red4[1]) + red4[2]) + red4[3];
}

// The per-row arithmetic of the six top-k metrics: topk_row_begin reads the row's head, topk_row_step(k) advances to rank k
// (k = 0, 1, .. in order) and leaves the row's terms at cut-off k + 1 in v[m], m = hit, mrr, ndcg, recall, precision, map.
// !ok: a lane without a row, every term 0.  A row with zero positives: NDCG 0 (divided by the ideal DCG of all K ranks, the
// reference's wrapped index), MAP 0, Recall NaN (0 / 0, as the reference).  The one place these terms are computed: the wave
// sums below (fr_topk_metrics, fr_topk_metrics_grouped) and fr_topk_user_terms read them from here, the same bits.
struct TopkRow {
    const int32_t* row;
    bool ok;
    int pos_len, ilen, csum;
    double first_rr, dcg, idcg, sum_pre;
    double idcg_all;             // ilen <= 0 only: the ideal DCG of all K ranks
};

__device__ __forceinline__ TopkRow topk_row_begin(const int32_t* __restrict__ rec_topk, long long u, bool ok, int K) {
    TopkRow s;
    s.row = rec_topk + (ok ? u : 0) * (long long)(K + 1);
    s.ok = ok;
    s.pos_len = ok ? s.row[K] : 1;
    s.ilen = s.pos_len < K ? s.pos_len : K;
    s.csum = 0;
    s.first_rr = 0.0, s.dcg = 0.0, s.idcg = 0.0, s.sum_pre = 0.0;
    s.idcg_all = 0.0;
    if (ok && s.ilen <= 0)
        for (int k = 0; k < K; ++k) s.idcg_all += 1.0 / log2((double)(k + 2));
    return s;
}

__device__ __forceinline__ void topk_row_step(TopkRow& s, int k, double (&v)[6]) {
    const bool ok = s.ok;
    const bool hit = ok && s.row[k] != 0;
    const double disc = 1.0 / log2((double)(k + 2));
    if (hit && s.csum == 0) s.first_rr = 1.0 / (double)(k + 1);
    s.csum += hit ? 1 : 0;
    if (hit) s.dcg += disc;
    if (k < s.ilen) s.idcg += disc;
    v[0] = ok && s.csum > 0 ? 1.0 : 0.0;
    v[1] = ok ? s.first_rr : 0.0;
    v[2] = ok ? s.dcg / (s.ilen > 0 ? s.idcg : s.idcg_all) : 0.0;
    v[3] = ok ? (double)s.csum / (double)s.pos_len : 0.0;
    v[4] = ok ? (double)s.csum / (double)(k + 1) : 0.0;
    // MAP (metrics.py:100-139): sum over the hits so far of Precision@j, over min(k + 1, min(positives, K))
    if (hit) s.sum_pre += (double)s.csum / (double)(k + 1);
    v[5] = ok && s.ilen > 0 ? s.sum_pre / (double)(k + 1 < s.ilen ? k + 1 : s.ilen) : 0.0;
}

// The terms of one wave of 64 rows and their butterfly sums: lane = one row of `rec_topk` (row u; !ok: a lane without a row),
// out[m][k] = wave sum.  Shared by topk_metrics_kernel (lane = user of the block) and topk_grouped_kernel (lane = member of a
// group's chunk): the same terms, the same bits.
__device__ __forceinline__ void topk_wave_terms(const int32_t* __restrict__ rec_topk, long long u, bool ok, int K, int lane,
                                                double* __restrict__ out) {
    TopkRow s = topk_row_begin(rec_topk, u, ok, K);
    for (int k = 0; k < K; ++k) {
        double v[6];
        topk_row_step(s, k, v);
        const double s0 = wave_sum(v[0]), s1 = wave_sum(v[1]), s2 = wave_sum(v[2]), s3 = wave_sum(v[3]),
                     s4 = wave_sum(v[4]), s5 = wave_sum(v[5]);
        if (lane == 0) {
            out[0 * K + k] = s0;
            out[1 * K + k] = s1;
            out[2 * K + k] = s2;
            out[3 * K + k] = s3;
            out[4 * K + k] = s4;
            out[5 * K + k] = s5;
        }
    }
}

// out[u][j] = row u's term of metric cols.metric[j] at cut-off cols.cut[j]: one thread per row, the steps of topk_row_step
// up to the largest cut-off
struct TopkCols {
    int n, kmax;
    int metric[FR_USER_TERMS_MAX_COLS], cut[FR_USER_TERMS_MAX_COLS];
};

__global__ __launch_bounds__(256) void topk_user_terms_kernel(const int32_t* __restrict__ rec_topk, long long U, int K,
                                                              TopkCols cols, double* __restrict__ out) {
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    if (u >= U) return;
    TopkRow s = topk_row_begin(rec_topk, u, true, K);
    for (int k = 0; k < cols.kmax; ++k) {
        double v[6];
        topk_row_step(s, k, v);
        for (int j = 0; j < cols.n; ++j) {
            if (cols.cut[j] != k + 1) continue;
            const int m = cols.metric[j];
            out[u * cols.n + j] = m == 0 ? v[0] : m == 1 ? v[1] : m == 2 ? v[2] : m == 3 ? v[3] : m == 4 ? v[4] : v[5];
        }
    }
}

// one wave per 64 users (lane = user); part[block][m][k]
__global__ __launch_bounds__(64) void topk_metrics_kernel(const int32_t* __restrict__ rec_topk, long long U, int K,
                                                          double* __restrict__ part) {
    const int lane = threadIdx.x;
    const long long u = (long long)blockIdx.x * 64 + lane;
    topk_wave_terms(rec_topk, u, u < U, K, lane, part + (size_t)blockIdx.x * 6 * K);
}

// ---- the same metrics (and GAUC's sums) per group of users: groups as segments -----------------------------------------------
// Group g's members are the rows perm[group_start[g] .. group_start[g+1]) (perm NULL: identity).  Its range is cut into chunks
// of 64 consecutive positions; chunk_start[g] = number of chunks of the groups before g, so chunk c of group g is block
// chunk_start[g] + c of the main grid, which has ceil(U / 64) + G blocks -- at least as many as there are chunks -- and finds
// its (group, chunk) by binary search.  Everything read from group_start (group_range, eval_common.hpp) and perm is clamped into
// [0, U]: a malformed table gives unspecified values, never an address outside the inputs or the workspace (chunk_start is clamped
// to the grid as well).
static constexpr int CS_THREADS = 256;

// chunk_start[0 .. G]: the exclusive scan of ceil(n_g / chunk_len), by ONE block (a thread scans a contiguous run of groups);
// chunk_len = 64 for the wave-per-chunk kernels here, fr_bootstrap_group_sums passes its own
__global__ __launch_bounds__(CS_THREADS) void group_chunk_scan_kernel(const int64_t* __restrict__ group_start, long long G,
                                                                      long long U, long long chunk_len, long long max_chunks,
                                                                      long long* __restrict__ chunk_start) {
    __shared__ long long tot[CS_THREADS];
    const int t = threadIdx.x;
    const long long per = (G + CS_THREADS - 1) / CS_THREADS;
    const long long g0 = t * per < G ? t * per : G, g1 = g0 + per < G ? g0 + per : G;
    long long mine = 0;
    for (long long g = g0; g < g1; ++g) {
        long long lo, hi;
        group_range(group_start, g, U, lo, hi);
        mine += (hi - lo + chunk_len - 1) / chunk_len;
    }
    tot[t] = mine;
    __syncthreads();
    long long run = 0;
    for (int s = 0; s < t; ++s) run += tot[s];
    for (long long g = g0; g < g1; ++g) {
        long long lo, hi;
        group_range(group_start, g, U, lo, hi);
        chunk_start[g] = run < max_chunks ? run : max_chunks;
        run += (hi - lo + chunk_len - 1) / chunk_len;
    }
    if (t == CS_THREADS - 1) chunk_start[G] = run < max_chunks ? run : max_chunks;
}

// the row of lane `lane` of block b, or ok = false
__device__ __forceinline__ long long chunk_member(const int64_t* __restrict__ perm, const int64_t* __restrict__ group_start,
                                                  long long U, long long g, long long c, int lane, bool& ok) {
    long long lo, hi;
    group_range(group_start, g, U, lo, hi);
    const long long j = lo + c * 64 + lane;
    ok = j < hi;
    if (!ok) return 0;
    return perm ? clamp_ll(perm[j], 0, U - 1) : j;
}

// one wave per chunk (lane = position within the chunk); part[block][m][k] as topk_metrics_kernel
__global__ __launch_bounds__(64) void topk_grouped_kernel(const int32_t* __restrict__ rec_topk,
                                                          const int64_t* __restrict__ perm,
                                                          const int64_t* __restrict__ group_start, long long U, int K,
                                                          long long G, const long long* __restrict__ chunk_start,
                                                          double* __restrict__ part) {
    long long g, c;
    if (!block_chunk(chunk_start, G, blockIdx.x, g, c)) return;
    bool ok;
    const long long u = chunk_member(perm, group_start, U, g, c, threadIdx.x, ok);
    topk_wave_terms(rec_topk, u, ok, K, threadIdx.x, part + (size_t)blockIdx.x * 6 * K);
}

// out[g][j] = (sum over group g's chunks, in chunk order, of part[chunk][j]) * (1 / n_g)    j < n; an empty group: NaN
__global__ __launch_bounds__(256) void group_fold_kernel(const double* __restrict__ part,
                                                         const long long* __restrict__ chunk_start,
                                                         const int64_t* __restrict__ group_start, long long U, long long G,
                                                         int n, bool mean, double* __restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= G * n) return;
    const long long g = t / n;
    const int j = (int)(t % n);
    long long lo, hi;
    group_range(group_start, g, U, lo, hi);
    double a = 0.0;
    for (long long b = chunk_start[g]; b < chunk_start[g + 1]; ++b) a += part[b * n + j];
    if (mean) a = hi > lo ? a * (1.0 / (double)(hi - lo)) : __longlong_as_double(0x7ff8000000000000LL);
    out[t] = a;
}

// One user's GAUC term from its `rec.meanrank` triple: kept (a positive and a negative) -> term = auc_u * pos_len, weight =
// pos_len; dropped (no_pos / no_neg) or !ok -> 0, 0.  Shared by gauc_grouped_kernel and fr_gauc_user_terms: the same bits.
__device__ __forceinline__ bool gauc_user_term(const int64_t* __restrict__ meanrank, long long u, bool ok, double& term,
                                               double& weight, bool& no_pos, bool& no_neg) {
    const long long two_rank = ok ? meanrank[u * 3] : 0, user_len = ok ? meanrank[u * 3 + 1] : 0,
                    pos_len = ok ? meanrank[u * 3 + 2] : 0;
    no_pos = ok && pos_len == 0;
    no_neg = ok && pos_len != 0 && user_len == pos_len;
    const bool keep = ok && !no_pos && !no_neg;
    term = 0.0, weight = 0.0;
    if (keep) {
        const long long pair2 = 2 * (user_len + 1) * pos_len - pos_len * (pos_len + 1) - two_rank;
        const double auc_u = (double)pair2 / (double)(2 * (user_len - pos_len) * pos_len);
        weight = (double)pos_len;
        term = auc_u * weight;
    }
    return keep;
}

__global__ __launch_bounds__(256) void gauc_user_terms_kernel(const int64_t* __restrict__ meanrank, long long U,
                                                              double* __restrict__ out) {
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    if (u >= U) return;
    bool no_pos, no_neg;
    double term, weight;
    gauc_user_term(meanrank, u, true, term, weight, no_pos, no_neg);
    out[u * 2] = term;
    out[u * 2 + 1] = weight;
}

// GAUC's sums per chunk from the `rec.meanrank` triples { 2 * pos_rank_sum, user_len, pos_len }: a user with a positive and a
// negative adds auc_u * pos_len and pos_len, auc_u = pair / ((user_len - pos_len) * pos_len) with pair = (user_len + 1) *
// pos_len - pos_len * (pos_len + 1) / 2 - pos_rank_sum (evaluator.gauc); numerator and denominator are integers (both doubled),
// so the one division rounds once.  part_d[block][2]; part_i[block][3] = users kept, without a positive, without a negative.
__global__ __launch_bounds__(64) void gauc_grouped_kernel(const int64_t* __restrict__ meanrank,
                                                          const int64_t* __restrict__ perm,
                                                          const int64_t* __restrict__ group_start, long long U, long long G,
                                                          const long long* __restrict__ chunk_start,
                                                          double* __restrict__ part_d, long long* __restrict__ part_i) {
    long long g, c;
    if (!block_chunk(chunk_start, G, blockIdx.x, g, c)) return;
    const int lane = threadIdx.x;
    bool ok;
    const long long u = chunk_member(perm, group_start, U, g, c, lane, ok);
    bool no_pos, no_neg;
    double term, weight;
    const bool keep = gauc_user_term(meanrank, u, ok, term, weight, no_pos, no_neg);
    const double s0 = wave_sum(term), s1 = wave_sum(weight);
    const int n0 = wave_sum(keep ? 1 : 0), n1 = wave_sum(no_pos ? 1 : 0), n2 = wave_sum(no_neg ? 1 : 0);
    if (lane == 0) {
        part_d[(size_t)blockIdx.x * 2] = s0;
        part_d[(size_t)blockIdx.x * 2 + 1] = s1;
        part_i[(size_t)blockIdx.x * 3] = n0;
        part_i[(size_t)blockIdx.x * 3 + 1] = n1;
        part_i[(size_t)blockIdx.x * 3 + 2] = n2;
    }
}

// kept[g][q] = sum over group g's chunks of part_i[chunk][q]
__global__ __launch_bounds__(256) void group_fold_counts_kernel(const long long* __restrict__ part_i,
                                                                const long long* __restrict__ chunk_start, long long G,
                                                                int64_t* __restrict__ kept) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= G * 3) return;
    const long long g = t / 3;
    const int q = (int)(t % 3);
    long long a = 0;
    for (long long b = chunk_start[g]; b < chunk_start[g + 1]; ++b) a += part_i[b * 3 + q];
    kept[t] = a;
}

// rec_topk[u][k] = 1 if the k-th ranked item of row u is one of its positives, rec_topk[u][K] = number of positives of
// row u (collector.py:146-154 without the dense [users, items] 0/1 matrix): the positives arrive as the SORTED keys
// row * n_items + item; membership and the per-row count are binary searches.  A list entry outside [0, n_items) is never
// a hit: its key would fall into another row's range.
__device__ __forceinline__ long long lower_bound_ll(const int64_t* __restrict__ a, long long n, long long key) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void eval_hits_kernel(const int64_t* __restrict__ topk_idx, long long U, int K,
                                                        long long n_items, const int64_t* __restrict__ pos_keys,
                                                        long long n_pos, int32_t* __restrict__ rec_topk) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= U * (K + 1)) return;
    const long long u = t / (K + 1);
    const int k = (int)(t % (K + 1));
    if (k == K) {
        rec_topk[t] = (int32_t)(lower_bound_ll(pos_keys, n_pos, (u + 1) * n_items) - lower_bound_ll(pos_keys, n_pos, u * n_items));
    } else {
        const long long item = topk_idx[u * K + k];
        const long long key = u * n_items + item;
        const long long p = lower_bound_ll(pos_keys, n_pos, key);
        rec_topk[t] = (item >= 0 && item < n_items && p < n_pos && pos_keys[p] == key) ? 1 : 0;
    }
}

// out[j] = (sum over blocks, in block order, of part[b][j]) * scale          j < n
__global__ __launch_bounds__(256) void column_sum_kernel(const double* __restrict__ part, long long blocks, int n,
                                                         double scale, double* __restrict__ out) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double a = 0.0;
    for (long long b = 0; b < blocks; ++b) a += part[b * n + j];
    out[j] = a * scale;
}

static constexpr int GS_GROUP = 16, GS_THREADS = 256, GS_MAXG = 8;

// stats[k][g][0..2] = sum value, count, sum wtrue over the members perm[seg_start[k] .. seg_start[k+1]) with group g
// (a group no member has: 0, 0, 0; a member whose group index is outside [0, G) is counted in no cell)
__global__ __launch_bounds__(GS_THREADS) void group_sums_kernel(const int64_t* __restrict__ perm,
                                                                const int64_t* __restrict__ seg_start, long long K,
                                                                const int32_t* __restrict__ group,
                                                                const float* __restrict__ value,
                                                                const float* __restrict__ wtrue, int G,
                                                                double* __restrict__ stats) {
    const int sub = threadIdx.x & (GS_GROUP - 1);
    const long long k = (long long)blockIdx.x * (GS_THREADS / GS_GROUP) + threadIdx.x / GS_GROUP;
    if (k >= K) return;   // whole 16-lane groups leave together
    double sv[GS_MAXG], sc[GS_MAXG], st[GS_MAXG];
#pragma unroll
    for (int g = 0; g < GS_MAXG; ++g) sv[g] = sc[g] = st[g] = 0.0;
    const long long j0 = seg_start[k], j1 = seg_start[k + 1];
    for (long long j = j0 + sub; j < j1; j += GS_GROUP) {
        const long long b = perm ? perm[j] : j;
        const int g = group[b];
        const double v = (double)value[b], t = wtrue ? (double)wtrue[b] : 0.0;
#pragma unroll
        for (int q = 0; q < GS_MAXG; ++q)
            if (q == g) {
                sv[q] += v;
                sc[q] += 1.0;
                st[q] += t;
            }
    }
#pragma unroll
    for (int q = 0; q < GS_MAXG; ++q) {
        if (q >= G) break;
#pragma unroll
        for (int o = GS_GROUP / 2; o > 0; o >>= 1) {
            sv[q] += __shfl_xor(sv[q], o, 64);
            sc[q] += __shfl_xor(sc[q], o, 64);
            st[q] += __shfl_xor(st[q], o, 64);
        }
        if (sub == 0) {
            double* o3 = stats + ((size_t)k * G + q) * 3;
            o3[0] = sv[q];
            o3[1] = sc[q];
            o3[2] = st[q];
        }
    }
}

// part[block][0..4] = sums over the block's items of: value, absolute, under, over terms (G == 2) and the DF epsilon
__global__ __launch_bounds__(256) void fair_from_stats_kernel(const double* __restrict__ stats, long long K, int G,
                                                              double* __restrict__ part) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    double t[5] = {0, 0, 0, 0, 0};
    if (k < K) {
        const double* s = stats + (size_t)k * G * 3;
        if (G == 2) {
            const double n0 = s[1] + 1e-5, n1 = s[4] + 1e-5;                  // sst_num += 1e-5, metrics.py:962
            const double p0 = s[0] / n0, p1 = s[3] / n1, r0 = s[2] / n0, r1 = s[5] / n1;
            t[0] = fabs((p0 - r0) - (p1 - r1));
            t[1] = fabs(fabs(p0 - r0) - fabs(p1 - r1));
            t[2] = fabs((r0 - p0 > 0 ? r0 - p0 : 0.0) - (r1 - p1 > 0 ? r1 - p1 : 0.0));
            t[3] = fabs((p0 - r0 > 0 ? p0 - r0 : 0.0) - (p1 - r1 > 0 ? p1 - r1 : 0.0));
        }
        // DifferentialFairness: float32 table (score_sum + 1/K) / (count + 1), epsilon = max pairwise |log a - log b|
        // (a NaN difference -- the logarithm of a non-positive entry -- fails `e > eps` and leaves the maximum as it is)
        float eps = 0.f;
        const double alpha = 1.0 / (double)K;
        for (int i = 0; i < G; ++i) {
            const float a = (float)((s[i * 3] + alpha) / (s[i * 3 + 1] + 1.0));
            for (int j = i + 1; j < G; ++j) {
                const float b = (float)((s[j * 3] + alpha) / (s[j * 3 + 1] + 1.0));
                const float e = fabsf(logf(a) - logf(b));
                eps = e > eps ? e : eps;
            }
        }
        t[4] = (double)eps;
    }
    __shared__ double red[5][4];
#pragma unroll
    for (int q = 0; q < 5; ++q) wave_sum_to_lds(t[q], red[q]);
    __syncthreads();
    if (threadIdx.x < 5) part[(size_t)blockIdx.x * 5 + threadIdx.x] = block_sum4(red[threadIdx.x]);
}

// ---- DifferentialFairness for any number of groups: a walk over the sorted (item, group) cells, no items x groups table ----------
// 16 lanes per item (as group_sums_kernel), 16 consecutive members of the item's range per trip.  PRECONDITION: inside an
// item's range the members of one group are contiguous (a run).  A run's sum is a segmented inclusive scan in double over
// the trip's 16 lanes (four __shfl_up steps, each taken only from a lane of the same run) plus the carry of the run left
// open by the trip before; the lane of the run's LAST member finishes the cell: entry, logf, the lane's running maximum and
// minimum of the logarithms, its count of runs.  Order of a cell's additions, for L members: at most four scan additions
// inside a trip, then one per further trip the run reaches into -- at most floor((L + 14) / 16) of them, since a run may
// start anywhere in a trip: every member passes through at most 4 + floor((L + 14) / 16) additions.
// part[block] = sum of the block's 16 epsilons in sub-group order.
// Loads run DF_AHEAD trips ahead of the scan (a popular item is one long chain of trips for its 16 lanes: the chain should
// wait for memory once per DF_AHEAD trips, not once per trip); the order of the additions does not depend on it.
static constexpr int DF_GROUP = 16, DF_THREADS = 256, DF_AHEAD = 4;

struct DfWalk {
    float lmax, lmin;                 // over the logarithms of this lane's finished cells
    long long runs;                   // cells this lane finished
    double carry_s;                   // the run open at the end of the trip before: its sum, its members, its group
    long long carry_c;
    int carry_g;
};

// one trip: member j = base + sub of the range [j0, j1) with group g and value v (anything where j >= j1); g_after: the
// sub-group's lane 0 holds the group of the first member of the NEXT trip
__device__ __forceinline__ void df_trip(DfWalk& w, long long j, long long j0, long long j1, int sub, int lane0, int g, float v,
                                        int g_after, int G, double alpha) {
    const bool have = j < j1;
    const int g_up = __shfl_up(g, 1, DF_GROUP), g_down = __shfl_down(g, 1, DF_GROUP), g_next = __shfl(g_after, 0, DF_GROUP);
    const bool head = have && (j == j0 || (sub == 0 ? w.carry_g : g_up) != g);
    const bool tail = have && (j + 1 >= j1 || (sub == DF_GROUP - 1 ? g_next : g_down) != g);
    const unsigned heads = (unsigned)(__ballot(head) >> lane0) & 0xffffu;
    const unsigned upto = heads & ((2u << sub) - 1u);            // the heads at or before this lane
    const int dist = upto ? sub - (31 - __clz(upto)) : sub;       // members of this lane's run before it in this trip
    double s = have ? (double)v : 0.0;
#pragma unroll
    for (int o = 1; o < DF_GROUP; o <<= 1) {
        const double t = __shfl_up(s, o, DF_GROUP);
        if (dist >= o) s += t;
    }
    long long c = dist + 1;
    if (!upto) {                      // no head up to here: the run came in from the trip before
        s = w.carry_s + s;
        c += w.carry_c;
    }
    if (tail && g >= 0 && g < G) {
        const float l = logf((float)((s + alpha) / ((double)c + 1.0)));
        if (l == l) {                 // a NaN logarithm (a non-positive entry) is left out
            w.lmax = fmaxf(w.lmax, l);
            w.lmin = fminf(w.lmin, l);
        }
        ++w.runs;
    }
    w.carry_s = __shfl(s, DF_GROUP - 1, DF_GROUP);
    w.carry_c = __shfl(c, DF_GROUP - 1, DF_GROUP);
    w.carry_g = __shfl(g, DF_GROUP - 1, DF_GROUP);
}

__global__ __launch_bounds__(DF_THREADS) void df_cells_kernel(const int64_t* __restrict__ perm,
                                                              const int64_t* __restrict__ item_start, long long K,
                                                              const int32_t* __restrict__ group,
                                                              const float* __restrict__ value, int G,
                                                              double* __restrict__ part) {
    const int sub = threadIdx.x & (DF_GROUP - 1), sg = threadIdx.x / DF_GROUP;
    const int lane0 = threadIdx.x & 63 & ~(DF_GROUP - 1);        // the sub-group's first lane in its wave
    const long long k = (long long)blockIdx.x * (DF_THREADS / DF_GROUP) + sg;
    const bool live = k < K;          // (no early exit: every thread reaches the block's fold below)
    const long long j0 = live ? item_start[k] : 0, j1 = live ? item_start[k + 1] : 0;
    const double alpha = 1.0 / (double)K;
    DfWalk w = {-INFINITY, INFINITY, 0, 0.0, 0, 0};
    int g[DF_AHEAD], gn[DF_AHEAD];
    float v[DF_AHEAD], vn[DF_AHEAD];
    // a position past the range reads the range's last member instead (no branch around a load; df_trip ignores it)
    if (j0 < j1) {
#pragma unroll
        for (int q = 0; q < DF_AHEAD; ++q) {
            const long long j = j0 + q * DF_GROUP + sub, jc = j < j1 ? j : j1 - 1, b = perm ? perm[jc] : jc;
            g[q] = group[b];
            v[q] = value[b];
        }
    }
    for (long long base = j0; base < j1; base += DF_AHEAD * DF_GROUP) {   // (the bounds are the sub-group's: its 16 lanes stay together)
#pragma unroll
        for (int q = 0; q < DF_AHEAD; ++q) {          // the next DF_AHEAD trips, in flight during the scans of these
            const long long j = base + (DF_AHEAD + q) * DF_GROUP + sub, jc = j < j1 ? j : j1 - 1, b = perm ? perm[jc] : jc;
            gn[q] = group[b];
            vn[q] = value[b];
        }
#pragma unroll
        for (int q = 0; q < DF_AHEAD; ++q) {
            const long long trip = base + q * DF_GROUP;
            if (trip < j1) df_trip(w, trip + sub, j0, j1, sub, lane0, g[q], v[q], q + 1 < DF_AHEAD ? g[q + 1] : gn[0], G, alpha);
        }
#pragma unroll
        for (int q = 0; q < DF_AHEAD; ++q) {
            g[q] = gn[q];
            v[q] = vn[q];
        }
    }
    float lmax = w.lmax, lmin = w.lmin;
    long long runs = w.runs;
#pragma unroll
    for (int o = DF_GROUP / 2; o > 0; o >>= 1) {
        lmax = fmaxf(lmax, __shfl_xor(lmax, o, 64));
        lmin = fminf(lmin, __shfl_xor(lmin, o, 64));
        runs += __shfl_xor(runs, o, 64);
    }
    if (runs < G) {                   // a group without a run: the entry (0 + 1 / K) / (0 + 1), once
        const float l = logf((float)alpha);
        lmax = fmaxf(lmax, l);
        lmin = fminf(lmin, l);
    }
    const float d = lmax - lmin;      // = the largest |log a - log b| over the pairs: float32 subtraction is monotone
    __shared__ double red[DF_THREADS / DF_GROUP];
    if (sub == 0) red[sg] = live && d > 0.f ? (double)d : 0.0;
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0;
#pragma unroll
        for (int q = 0; q < DF_THREADS / DF_GROUP; ++q) a += red[q];
        part[blockIdx.x] = a;
    }
}

// ---- ranking of the candidates of an evaluation batch (uniN protocol): one wave per user -------------------------------------
// Reference: trainer.py:441-456 scatters every user's candidates (its positives and the negatives sampled for them) into a dense
// [users, n_items] matrix of -inf, collector.py:149 takes torch.topk(matrix, max(topk)) of it.  The evaluation loader emits a
// batch user by user, so a user's candidates are a contiguous SEGMENT of the batch (seg_start), and its list is the K best
// DISTINCT items of that segment (an item drawn twice scores the same twice and occupies one cell of the dense row).  A wave keeps
// the K + 1 best so far in lanes 0..K (sorted, descending) and walks the segment 64 candidates at a time, each time pulling the
// chunk's best through a wave maximum until it no longer beats the (K + 1)-th.  flags[u]: bit 0 = two of the first K + 1 entries
// score EQUAL or a candidate's score is NaN (which of them the reference ranks first is torch.topk's CPU order: the caller
// ranks that row on the host, fr_topk_like_torch_cpu), bit 1 = fewer than K + 1 distinct candidates (the reference's list then continues into -inf cells).
// Replaces three device sorts over the batch's candidates per evaluation batch (1.3 ms -> 0.1 ms at 280 k candidates).
constexpr int TOPK_MAXK = 62;
__global__ __launch_bounds__(256) void eval_topk_segments_kernel(const int64_t* __restrict__ seg_start, long long n_users,
                                                                 const int64_t* __restrict__ items, const float* __restrict__ scores,
                                                                 int k, int64_t* __restrict__ topk_idx, int32_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= n_users) return;
    const long long s = seg_start[u], e = seg_start[u + 1];
    float t_score = -INFINITY;      // lane j < n_in: the j-th best so far
    long long t_item = 0;
    int n_in = 0;
    bool any_nan = false;
    for (long long base = s; base < e; base += 64) {
        const bool have = base + lane < e;
        float c_score = have ? scores[base + lane] : -INFINITY;
        const long long c_item = have ? items[base + lane] : 0;
        // (torch.topk ranks a NaN above every number; a user with one is handed to the host's ranking like a tied one)
        any_nan |= __ballot(have && c_score != c_score) != 0ull;
        unsigned long long valid = __ballot(have && c_score == c_score);
        while (valid) {
            float m = (valid >> lane) & 1ull ? c_score : -INFINITY;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
            const float kth = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, t_score), k));
            if (n_in == k + 1 && !(m > kth)) break;       // nothing left in this chunk enters the first K + 1
            const unsigned long long at = __ballot(((valid >> lane) & 1ull) && c_score == m);
            const int src = __builtin_ctzll(at);
            valid &= ~(1ull << src);
            const long long it = (long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)c_item, src) |
                                 ((long long)__builtin_amdgcn_readlane((int)(c_item >> 32), src) << 32);
            if (__ballot(lane < n_in && t_item == it)) continue;       // the same item again: one cell of the dense row
            // behind every entry that scores >= m (so equal scores keep their order of arrival; which order the reference has
            // is settled on the host when the flag below says it matters)
            const int p = __popcll(__ballot(lane < n_in && t_score >= m));
            const float up_s = __shfl_up(t_score, 1, 64);
            const long long up_i = (long long)(unsigned)__shfl_up((int)(unsigned)t_item, 1, 64) |
                                   ((long long)__shfl_up((int)(t_item >> 32), 1, 64) << 32);
            if (lane > p) { t_score = up_s; t_item = up_i; }
            if (lane == p) { t_score = m; t_item = it; }
            if (n_in < k + 1) ++n_in;
            if (lane >= n_in) t_score = -INFINITY;
        }
    }
    const float prev = __shfl_up(t_score, 1, 64);
    const bool tie = __ballot(lane >= 1 && lane < n_in && lane <= k && t_score == prev) != 0ull;
    if (lane < k) topk_idx[u * k + lane] = lane < n_in ? t_item : 0;       // (short lists are padded with [PAD] item 0)
    if (lane == 0) flags[u] = (tie || any_nan ? 1 : 0) | (n_in < k + 1 ? 2 : 0);
}

// out[q] = the score of candidate item q_items[q] in the segment of user row q_rows[q], -inf if it is not one (a lookup in the
// reference's dense -inf matrix: collector.py:160-175 reads positives' and negatives' scores back out of it)
// (16 lanes per query walk the segment side by side -- every load of the walk in flight at once; one lane per query with a
// break on the match was ~100 dependent loads: 38 us per launch against 13 for the ranking itself.  A candidate drawn twice
// carries the same score twice, so which copy answers does not matter.)
constexpr int LOOKUP_LANES = 16;
__global__ __launch_bounds__(256) void eval_lookup_segments_kernel(const int64_t* __restrict__ seg_start, long long n_users,
                                                                   const int64_t* __restrict__ items, const float* __restrict__ scores,
                                                                   const int64_t* __restrict__ q_rows, const int64_t* __restrict__ q_items,
                                                                   long long n_q, float* __restrict__ out) {
    const long long q = ((long long)blockIdx.x * 256 + threadIdx.x) / LOOKUP_LANES;
    const int sub = threadIdx.x & (LOOKUP_LANES - 1);
    const bool live = q < n_q;
    const long long r = live ? q_rows[q] : -1;
    float v = -INFINITY;
    bool found = false;
    if (r >= 0 && r < n_users) {
        const long long it = q_items[q];
        const long long j1 = seg_start[r + 1];
#pragma unroll 4
        for (long long j = seg_start[r] + sub; j < j1; j += LOOKUP_LANES)
            if (items[j] == it) {
                v = scores[j];
                found = true;
            }
    }
    // the value of the first lane of the group that found it (not a maximum: a score may be NaN and has to come back as NaN)
    const int lane = threadIdx.x & 63, base = lane & ~(LOOKUP_LANES - 1);
    const unsigned bits = (unsigned)(__ballot(found) >> base) & ((1u << LOOKUP_LANES) - 1u);
    const float got = __shfl(v, base + (bits ? __ffs((int)bits) - 1 : 0), 64);
    if (live && sub == 0) out[q] = bits ? got : -INFINITY;
}

// ---- evaluation by value (labeled mode): MAE / RMSE / LogLoss sums and the exact AUC counts ------------------------------------
// Reference: recbole/evaluator/metrics.py AUC / MAE / RMSE / LogLoss over the concatenated (score, label) columns.
constexpr int VM_THREADS = 256, VM_ROWS = 2048, VM_MAXBLOCKS = 2048;

// block b walks rows b*256 + t, + blocks*256, ... in that order (a fixed assignment for a given n): part_d[b][0..2] = sum |e|, sum e^2, LogLoss
// sum of its rows, part_i[b] = its number of rows with label == 1
__global__ __launch_bounds__(VM_THREADS) void value_partials_kernel(const float* __restrict__ score, const float* __restrict__ label,
                                                                    long long n, double* __restrict__ part_d,
                                                                    long long* __restrict__ part_i) {
    double a = 0.0, q = 0.0, l = 0.0;
    long long pos = 0;
    const long long stride = (long long)gridDim.x * VM_THREADS;
    for (long long j0 = (long long)blockIdx.x * VM_THREADS + threadIdx.x; j0 < n; j0 += 4 * stride) {
        float sv[4], yv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {                       // the four loads in flight before the first logarithm
            const long long j = j0 + r * stride;
            sv[r] = j < n ? score[j] : 0.f;
            yv[r] = j < n ? label[j] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (j0 + r * stride >= n) break;
            const double s = (double)sv[r], y = (double)yv[r];
            const double e = s - y;
            a += fabs(e);
            q += e * e;
            const double p = fmin(fmax(s, 1e-15), 1.0 - 1e-15);
            l += -y * log(p) - (1.0 - y) * log(1.0 - p);
            pos += y == 1.0 ? 1 : 0;
        }
    }
    __shared__ double red_d[3][4];
    __shared__ long long red_i[4];
    wave_sum_to_lds(a, red_d[0]);
    wave_sum_to_lds(q, red_d[1]);
    wave_sum_to_lds(l, red_d[2]);
    wave_sum_to_lds(pos, red_i);
    __syncthreads();
    if (threadIdx.x < 3) part_d[(size_t)blockIdx.x * 3 + threadIdx.x] = block_sum4(red_d[threadIdx.x]);
    if (threadIdx.x == 3) part_i[blockIdx.x] = block_sum4(red_i);
}

// one block: thread t folds partials t, t + 256, ... in that order, then the fixed butterfly; counts = n, positives
__global__ __launch_bounds__(VM_THREADS) void value_fold_kernel(const double* __restrict__ part_d, const long long* __restrict__ part_i,
                                                                int blocks, long long n, double* __restrict__ out,
                                                                long long* __restrict__ counts) {
    double v[3] = {0.0, 0.0, 0.0};
    long long pos = 0;
    for (int b = threadIdx.x; b < blocks; b += VM_THREADS) {
        v[0] += part_d[(size_t)b * 3 + 0];
        v[1] += part_d[(size_t)b * 3 + 1];
        v[2] += part_d[(size_t)b * 3 + 2];
        pos += part_i[b];
    }
    __shared__ double red_d[3][4];
    __shared__ long long red_i[4];
#pragma unroll
    for (int c = 0; c < 3; ++c) wave_sum_to_lds(v[c], red_d[c]);
    wave_sum_to_lds(pos, red_i);
    __syncthreads();
    if (threadIdx.x < 3) out[threadIdx.x] = block_sum4(red_d[threadIdx.x]);
    if (threadIdx.x == 3) {
        counts[0] = n;
        counts[1] = block_sum4(red_i);
    }
}

// AUC from the sorted column.  C[j] = number of negatives (label != 1) among rows [0, j), int32 [n + 1] in the workspace: per-tile
// counts (auc_count), their exclusive scan by one block (auc_scan_tiles), the scan inside every tile (auc_prefix).  Then the thread
// of every row that STARTS a run of equal scores [s, e) adds p * (C[s] + C[e]), p = the run's positives = (e - s) - (C[e] - C[s]):
// the sum over the positives of C[s_i] + C[e_i].  e comes from the neighbour for a run of one row, else from a galloping search in
// the sorted column (log of the run length, whether or not the run leaves the tile).
constexpr int AUC_THREADS = 256, AUC_PER = 8, AUC_TILE = AUC_THREADS * AUC_PER;

// exclusive scan of one int per thread over the block; *total = the block's sum
__device__ __forceinline__ int block_excl_scan(int v, int* total, int* lds4) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) lds4[w] = inc;
    __syncthreads();
    int base = 0;
    for (int q = 0; q < w; ++q) base += lds4[q];
    *total = block_sum4(lds4);
    __syncthreads();
    return base + inc - v;
}

__global__ __launch_bounds__(AUC_THREADS) void auc_count_kernel(const float* __restrict__ label, long long n, int32_t* __restrict__ tile_neg) {
    const long long lo = (long long)blockIdx.x * AUC_TILE;
    int c = 0;
#pragma unroll
    for (int i = 0; i < AUC_PER; ++i) {
        const long long j = lo + i * AUC_THREADS + threadIdx.x;
        c += (j < n && label[j] != 1.0f) ? 1 : 0;
    }
    __shared__ int lds4[4];
    int total;
    block_excl_scan(c, &total, lds4);
    if (threadIdx.x == 0) tile_neg[blockIdx.x] = total;
}

// in place: tile_neg[b] <- sum of tile_neg[0 .. b), tile_neg[tiles] <- the total
__global__ __launch_bounds__(AUC_THREADS) void auc_scan_tiles_kernel(int32_t* __restrict__ tile_neg, long long tiles) {
    __shared__ int lds4[4];
    int carry = 0;
    for (long long base = 0; base < tiles; base += AUC_THREADS) {
        const long long b = base + threadIdx.x;
        const int v = b < tiles ? tile_neg[b] : 0;
        int total;
        const int ex = block_excl_scan(v, &total, lds4);
        if (b < tiles) tile_neg[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) tile_neg[tiles] = carry;
}

__global__ __launch_bounds__(AUC_THREADS) void auc_prefix_kernel(const float* __restrict__ label, long long n,
                                                                 const int32_t* __restrict__ tile_off, int32_t* __restrict__ C) {
    const long long lo = (long long)blockIdx.x * AUC_TILE + (long long)threadIdx.x * AUC_PER;       // this thread's 8 rows in a row
    int neg[AUC_PER];
    int c = 0;
#pragma unroll
    for (int i = 0; i < AUC_PER; ++i) {
        neg[i] = (lo + i < n && label[lo + i] != 1.0f) ? 1 : 0;
        c += neg[i];
    }
    __shared__ int lds4[4];
    int total;
    int run = tile_off[blockIdx.x] + block_excl_scan(c, &total, lds4);
    if (blockIdx.x == 0 && threadIdx.x == 0) C[0] = 0;
#pragma unroll
    for (int i = 0; i < AUC_PER; ++i) {
        run += neg[i];
        if (lo + i < n) C[lo + i + 1] = run;
    }
}

__global__ __launch_bounds__(AUC_THREADS) void auc_runs_kernel(const float* __restrict__ score, long long n, const int32_t* __restrict__ C,
                                                               long long* __restrict__ part) {
    const long long lo = (long long)blockIdx.x * AUC_TILE;
    long long acc = 0;
#pragma unroll 2
    for (int i = 0; i < AUC_PER; ++i) {
        const long long j = lo + i * AUC_THREADS + threadIdx.x;
        if (j >= n) continue;
        const float v = score[j];
        if (j > 0 && score[j - 1] == v) continue;          // not the first row of its run
        long long e = j + 1;
        if (e < n && score[e] == v) {
            // gallop: rows [j, j + a] score v; the first row that does not lies in (j + a, min(j + 2a, n)]
            long long a = 1;
            while (j + 2 * a < n && score[j + 2 * a] == v) a *= 2;
            long long l = j + a + 1, h = j + 2 * a < n ? j + 2 * a : n;
            while (l < h) {
                const long long mid = (l + h) >> 1;
                if (score[mid] == v) l = mid + 1;
                else h = mid;
            }
            e = l;
        }
        const long long cs = C[j], ce = C[e];
        acc += ((e - j) - (ce - cs)) * (cs + ce);
    }
    __shared__ long long red[4];
    wave_sum_to_lds(acc, red);
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = block_sum4(red);
}

// out = 2U (the tiles' parts in tile order per thread, then the fixed butterfly), P, Nn
__global__ __launch_bounds__(AUC_THREADS) void auc_fold_kernel(const long long* __restrict__ part, long long tiles, long long n,
                                                               const int32_t* __restrict__ C, long long* __restrict__ out) {
    long long acc = 0;
    for (long long b = threadIdx.x; b < tiles; b += AUC_THREADS) acc += part[b];
    __shared__ long long red[4];
    wave_sum_to_lds(acc, red);
    __syncthreads();
    if (threadIdx.x == 0) {
        const long long nn = C[n];
        out[0] = block_sum4(red);
        out[1] = n - nn;
        out[2] = nn;
    }
}

// ---- GAUC: `rec.meanrank` of an evaluation batch, a wave per user ---------------------------------------------------------------
// Reference: collector.py `rec.meanrank` + metrics.py GAUC on the user's row of the dense [users, n_items] -inf matrix.  The
// user's cells are the DISTINCT items of its segment [seg_start[u], seg_start[u + 1]) (items == NULL: row j of the segment is the
// cell of item j, the dense `full` row); its positives are the items of the keys u * n_items + item in the SORTED pos_keys (what
// fr_eval_hits takes; a key listed twice is one positive, a positive that is no cell of the user is none).
//   out[u] = { 2 * pos_rank_sum, user_len, pos_len },  2 * rank of a positive p = 2 #{cells > p} + #{cells == p} + 1
// Integers, any order.  Phase 1 marks the first copy of every item (first[row], one byte, in the workspace); phase 2 finds each
// positive's score in the segment and walks the cells 64 at a time against it.
__global__ __launch_bounds__(256) void eval_meanrank_segments_kernel(const int64_t* __restrict__ seg_start, long long n_users,
                                                                     const int64_t* __restrict__ items, const float* __restrict__ scores,
                                                                     const int64_t* __restrict__ pos_keys, long long n_pos,
                                                                     long long n_items, uint8_t* __restrict__ first,
                                                                     int64_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool live = u < n_users;
    const long long s = live ? seg_start[u] : 0, e = live ? seg_start[u + 1] : 0;
    if (items) {
        for (long long base = s; base < e; base += 64) {
            const long long j = base + lane;
            const long long it = j < e ? items[j] : -1;
            bool dup = false;
            const long long stop = base + 64 < e ? base + 64 : e;
            for (long long k = s; k < stop; ++k) dup |= (k < j) & (items[k] == it);
            if (j < e) first[j] = dup ? 0 : 1;
        }
        __syncthreads();       // (every thread of the block arrives: no early exit above) the flags are visible to the wave's lanes
    }
    if (!live) return;
    long long user_len = 0, pairs = 0, pos_len = 0;          // pos_len: wave-uniform
    for (long long j = s + lane; j < e; j += 64) user_len += ((!items || first[j]) && scores[j] > -INFINITY) ? 1 : 0;
    const long long p0 = lower_bound_ll(pos_keys, n_pos, u * n_items), p1 = lower_bound_ll(pos_keys, n_pos, (u + 1) * n_items);
    for (long long p = p0; p < p1; ++p) {
        const long long key = pos_keys[p];
        if (p > p0 && pos_keys[p - 1] == key) continue;
        const long long item = key - u * n_items;
        long long at = -1;                                    // the row of the positive's cell
        if (!items) {
            at = item < e - s ? s + item : -1;
        } else {
            for (long long base = s; base < e && at < 0; base += 64) {
                const unsigned long long m = __ballot(base + lane < e && items[base + lane] == item);
                if (m) at = base + __builtin_ctzll(m);
            }
        }
        if (at < 0) continue;
        const float sp = scores[at];
        ++pos_len;
        for (long long j = s + lane; j < e; j += 64) {
            const float sc = scores[j];
            if ((!items || first[j]) && sc > -INFINITY) pairs += (sc > sp ? 2 : 0) + (sc == sp ? 1 : 0);
        }
    }
    user_len = wave_sum(user_len);
    pairs = wave_sum(pairs);
    if (lane == 0) {
        out[u * 3 + 0] = pairs + pos_len;
        out[u * 3 + 1] = user_len;
        out[u * 3 + 2] = pos_len;
    }
}

}  // namespace fr

using namespace fr;

extern "C" size_t fr_topk_metrics_workspace_bytes(int64_t n_users, int32_t k) {
    return n_users < 1 || k < 1 ? 0 : (size_t)((n_users + 63) / 64) * 6 * k * sizeof(double);
}

extern "C" int fr_topk_metrics(const int32_t* rec_topk, int64_t n_users, int32_t k, double* out, void* ws, size_t ws_bytes,
                               void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    FR_CHECK_ARG(rec_topk && out && ws && n_users >= 1 && k >= 1 && ws_bytes >= fr_topk_metrics_workspace_bytes(n_users, k),
                 "fr_topk_metrics: bad argument");
    const long long blocks = (n_users + 63) / 64;
    hipLaunchKernelGGL(topk_metrics_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, rec_topk, (long long)n_users, (int)k,
                       (double*)ws);
    FR_CHECK_LAUNCH();
    hipLaunchKernelGGL(column_sum_kernel, dim3((unsigned)((6 * k + 255) / 256)), dim3(256), 0, stream, (const double*)ws,
                       blocks, 6 * k, 1.0 / (double)n_users, out);
    FR_CHECK_LAUNCH();
    return FR_OK;
}

// The chunk scan and the fold of per-chunk partials, for the grouped entries here and for fr_bootstrap_group_sums
// (bootstrap.hip); declared in kernels.hpp.
int fr::launch_group_chunk_scan(const int64_t* group_start, long long G, long long U, long long chunk_len, long long max_chunks,
                                long long* chunk_start, hipStream_t stream) {
    hipLaunchKernelGGL(group_chunk_scan_kernel, dim3(1), dim3(CS_THREADS), 0, stream, group_start, G, U, chunk_len, max_chunks,
                       chunk_start);
    FR_CHECK_LAUNCH();
    return FR_OK;
}

int fr::launch_group_fold(const double* part, const long long* chunk_start, const int64_t* group_start, long long U, long long G,
                          int n, bool mean, double* out, hipStream_t stream) {
    hipLaunchKernelGGL(group_fold_kernel, dim3((unsigned)((G * n + 255) / 256)), dim3(256), 0, stream, part, chunk_start,
                       group_start, U, G, n, mean, out);
    FR_CHECK_LAUNCH();
    return FR_OK;
}

extern "C" int fr_topk_user_terms(const int32_t* rec_topk, int64_t n_users, int32_t k, const int32_t* metric, const int32_t* cut,
                                  int32_t n_cols, double* out, void* stream_) {
    FR_CHECK_ARG(rec_topk && metric && cut && out, "fr_topk_user_terms: null pointer");
    FR_CHECK_ARG(n_users >= 1 && n_users < (1ll << 31) && k >= 1 && n_cols >= 1 && n_cols <= FR_USER_TERMS_MAX_COLS,
                 "fr_topk_user_terms: 1 <= n_users < 2^31, k >= 1, 1 <= n_cols <= %d (got %lld, %d, %d)", FR_USER_TERMS_MAX_COLS,
                 (long long)n_users, (int)k, (int)n_cols);
    TopkCols cols;
    cols.n = n_cols;
    cols.kmax = 0;
    for (int j = 0; j < FR_USER_TERMS_MAX_COLS; ++j) {
        cols.metric[j] = j < n_cols ? metric[j] : 0;
        cols.cut[j] = j < n_cols ? cut[j] : 0;
        if (j >= n_cols) continue;
        FR_CHECK_ARG(metric[j] >= 0 && metric[j] <= 5 && cut[j] >= 1 && cut[j] <= k,
                     "fr_topk_user_terms: column %d: metric %d not in 0..5 or cut-off %d not in 1..%d", j, (int)metric[j],
                     (int)cut[j], (int)k);
        cols.kmax = cut[j] > cols.kmax ? cut[j] : cols.kmax;
    }
    hipLaunchKernelGGL(topk_user_terms_kernel, dim3((unsigned)((n_users + 255) / 256)), dim3(256), 0, (hipStream_t)stream_,
                       rec_topk, (long long)n_users, (int)k, cols, out);
    FR_CHECK_LAUNCH();
    return FR_OK;
}

extern "C" int fr_gauc_user_terms(const int64_t* meanrank, int64_t n_users, double* out, void* stream_) {
    FR_CHECK_ARG(meanrank && out, "fr_gauc_user_terms: null pointer");
    FR_CHECK_ARG(n_users >= 1 && n_users < (1ll << 31), "fr_gauc_user_terms: 1 <= n_users < 2^31 (got %lld)", (long long)n_users);
    hipLaunchKernelGGL(gauc_user_terms_kernel, dim3((unsigned)((n_users + 255) / 256)), dim3(256), 0, (hipStream_t)stream_,
                       meanrank, (long long)n_users, out);
    FR_CHECK_LAUNCH();
    return FR_OK;
}

// the main grid of the grouped entries: ceil(n_users / 64) + n_groups blocks, an upper bound on the chunks; 0 = out of range
static long long grouped_blocks(int64_t n_users, int64_t n_groups) {
    if (n_users < 1 || n_groups < 1 || n_groups > 0x7fffffffLL) return 0;
    const long long blocks = (n_users + 63) / 64 + n_groups;
    return blocks <= 0x7fffffffLL ? blocks : 0;
}

// workspace: part[blocks][6][k] doubles, then chunk_start[n_groups + 1]
extern "C" size_t fr_topk_metrics_grouped_workspace_bytes(int64_t n_users, int32_t k, int64_t n_groups) {
    const long long blocks = grouped_blocks(n_users, n_groups);
    if (blocks == 0 || k < 1 || blocks > (1ll << 56) / (6ll * k)) return 0;      // (the partials alone would pass 2^59 bytes)
    return ((size_t)blocks * 6 * k + (size_t)n_groups + 1) * 8;
}

extern "C" int fr_topk_metrics_grouped(const int32_t* rec_topk, const int64_t* perm, const int64_t* group_start, int64_t n_users,
                                       int32_t k, int64_t n_groups, double* out, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    FR_CHECK_ARG(rec_topk && group_start && out && ws, "fr_topk_metrics_grouped: null pointer");
    FR_CHECK_ARG(n_users >= 1 && k >= 1 && n_groups >= 1, "fr_topk_metrics_grouped: n_users, k, n_groups >= 1 (got %lld, %d, %lld)",
                 (long long)n_users, (int)k, (long long)n_groups);
    const long long blocks = grouped_blocks(n_users, n_groups);
    FR_CHECK_ARG(blocks > 0 && fr_topk_metrics_grouped_workspace_bytes(n_users, k, n_groups) != 0 &&
                     (long long)n_groups <= 0x7fffffffLL * 256 / (6ll * k),
                 "fr_topk_metrics_grouped: %lld users in %lld groups are more than one launch takes", (long long)n_users,
                 (long long)n_groups);
    FR_CHECK_ARG(ws_bytes >= fr_topk_metrics_grouped_workspace_bytes(n_users, k, n_groups),
                 "fr_topk_metrics_grouped: workspace too small");
    double* part = (double*)ws;
    long long* chunk_start = (long long*)(part + (size_t)blocks * 6 * k);
    if (int rc = launch_group_chunk_scan(group_start, n_groups, n_users, 64, blocks, chunk_start, stream)) return rc;
    hipLaunchKernelGGL(topk_grouped_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, rec_topk, perm, group_start,
                       (long long)n_users, (int)k, (long long)n_groups, (const long long*)chunk_start, part);
    FR_CHECK_LAUNCH();
    return launch_group_fold(part, chunk_start, group_start, n_users, n_groups, 6 * (int)k, true, out, stream);
}

// workspace: part_d[blocks][2] doubles, part_i[blocks][3] int64, then chunk_start[n_groups + 1]
extern "C" size_t fr_gauc_grouped_workspace_bytes(int64_t n_users, int64_t n_groups) {
    const long long blocks = grouped_blocks(n_users, n_groups);
    return blocks == 0 ? 0 : ((size_t)blocks * 5 + (size_t)n_groups + 1) * 8;
}

extern "C" int fr_gauc_grouped(const int64_t* meanrank, const int64_t* perm, const int64_t* group_start, int64_t n_users,
                               int64_t n_groups, double* out, int64_t* kept, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    FR_CHECK_ARG(meanrank && group_start && out && kept && ws, "fr_gauc_grouped: null pointer");
    FR_CHECK_ARG(n_users >= 1 && n_groups >= 1, "fr_gauc_grouped: n_users, n_groups >= 1 (got %lld, %lld)", (long long)n_users,
                 (long long)n_groups);
    const long long blocks = grouped_blocks(n_users, n_groups);
    FR_CHECK_ARG(blocks > 0, "fr_gauc_grouped: %lld users in %lld groups are more than one launch takes", (long long)n_users,
                 (long long)n_groups);
    FR_CHECK_ARG(ws_bytes >= fr_gauc_grouped_workspace_bytes(n_users, n_groups), "fr_gauc_grouped: workspace too small");
    double* part_d = (double*)ws;
    long long* part_i = (long long*)(part_d + (size_t)blocks * 2);
    long long* chunk_start = part_i + (size_t)blocks * 3;
    if (int rc = launch_group_chunk_scan(group_start, n_groups, n_users, 64, blocks, chunk_start, stream)) return rc;
    hipLaunchKernelGGL(gauc_grouped_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, meanrank, perm, group_start,
                       (long long)n_users, (long long)n_groups, (const long long*)chunk_start, part_d, part_i);
    FR_CHECK_LAUNCH();
    if (int rc = launch_group_fold(part_d, chunk_start, group_start, n_users, n_groups, 2, false, out, stream)) return rc;
    hipLaunchKernelGGL(group_fold_counts_kernel, dim3((unsigned)((n_groups * 3 + 255) / 256)), dim3(256), 0, stream,
                       (const long long*)part_i, (const long long*)chunk_start, (long long)n_groups, kept);
    FR_CHECK_LAUNCH();
    return FR_OK;
}

extern "C" int fr_eval_topk_segments(const int64_t* seg_start, int64_t n_users, const int64_t* items, const float* scores,
                                     int32_t k, int64_t* topk_idx, int32_t* flags, void* stream_) {
    FR_CHECK_ARG(seg_start && items && scores && topk_idx && flags && n_users >= 1 && k >= 1 && k <= TOPK_MAXK,
                 "fr_eval_topk_segments: bad argument (1 <= k <= %d)", TOPK_MAXK);
    hipLaunchKernelGGL(eval_topk_segments_kernel, dim3((unsigned)((n_users + 3) / 4)), dim3(256), 0, (hipStream_t)stream_, seg_start,
                       (long long)n_users, items, scores, (int)k, topk_idx, flags);
    FR_CHECK_LAUNCH();
    return FR_OK;
}

extern "C" int fr_eval_lookup_segments(const int64_t* seg_start, int64_t n_users, const int64_t* items, const float* scores,
                                       const int64_t* q_rows, const int64_t* q_items, int64_t n_q, float* out, void* stream_) {
    FR_CHECK_ARG(seg_start && items && scores && (n_q == 0 || (q_rows && q_items && out)) && n_users >= 1 && n_q >= 0,
                 "fr_eval_lookup_segments: bad argument");
    if (n_q == 0) return FR_OK;
    hipLaunchKernelGGL(eval_lookup_segments_kernel, dim3((unsigned)((n_q * LOOKUP_LANES + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, seg_start,
                       (long long)n_users, items, scores, q_rows, q_items, (long long)n_q, out);
    FR_CHECK_LAUNCH();
    return FR_OK;
}

extern "C" int fr_eval_hits(const int64_t* topk_idx, int64_t n_rows, int32_t k, int64_t n_items, const int64_t* pos_keys,
                            int64_t n_pos, int32_t* rec_topk, void* stream_) {
    FR_CHECK_ARG(topk_idx && rec_topk && (pos_keys || n_pos == 0) && n_rows >= 1 && k >= 1 && n_items >= 1 && n_pos >= 0,
                 "fr_eval_hits: bad argument");
    const long long n = (long long)n_rows * (k + 1);
    hipLaunchKernelGGL(eval_hits_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, topk_idx,
                       (long long)n_rows, (int)k, (long long)n_items, pos_keys, (long long)n_pos, rec_topk);
    FR_CHECK_LAUNCH();
    return FR_OK;
}

extern "C" int fr_group_sums(const int64_t* perm, const int64_t* seg_start, int64_t n_segments, const int32_t* group,
                             const float* value, const float* wtrue, int32_t n_groups, double* stats, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    FR_CHECK_ARG(seg_start && group && value && stats && n_segments >= 1 && n_groups >= 1 && n_groups <= GS_MAXG,
                 "fr_group_sums: bad argument (1 <= n_groups <= %d)", GS_MAXG);
    const long long per_block = GS_THREADS / GS_GROUP;
    hipLaunchKernelGGL(group_sums_kernel, dim3((unsigned)((n_segments + per_block - 1) / per_block)), dim3(GS_THREADS), 0,
                       stream, perm, seg_start, (long long)n_segments, group, value, wtrue, (int)n_groups, stats);
    FR_CHECK_LAUNCH();
    return FR_OK;
}

extern "C" size_t fr_fair_metrics_workspace_bytes(int64_t n_segments) {
    return n_segments < 1 ? 0 : (size_t)((n_segments + 255) / 256) * 5 * sizeof(double);
}

extern "C" int fr_fair_metrics_from_stats(const double* stats, int64_t n_segments, int32_t n_groups, double* out, void* ws,
                                          size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    FR_CHECK_ARG(stats && out && ws && n_segments >= 1 && n_groups >= 1 && n_groups <= GS_MAXG &&
                     ws_bytes >= fr_fair_metrics_workspace_bytes(n_segments), "fr_fair_metrics_from_stats: bad argument");
    const long long blocks = (n_segments + 255) / 256;
    hipLaunchKernelGGL(fair_from_stats_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, stats, (long long)n_segments,
                       (int)n_groups, (double*)ws);
    FR_CHECK_LAUNCH();
    hipLaunchKernelGGL(column_sum_kernel, dim3(1), dim3(256), 0, stream, (const double*)ws, blocks, 5,
                       1.0 / (double)n_segments, out);
    FR_CHECK_LAUNCH();
    return FR_OK;
}

// workspace of fr_df_cells: one double per block of 16 items
extern "C" size_t fr_df_cells_workspace_bytes(int64_t n_items) {
    const long long per_block = DF_THREADS / DF_GROUP;
    return n_items < 1 ? 0 : (size_t)((n_items + per_block - 1) / per_block) * sizeof(double);
}

extern "C" int fr_df_cells(const int64_t* perm, const int64_t* item_start, int64_t n_items, const int32_t* group,
                           const float* value, int32_t n_groups, double* out, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    FR_CHECK_ARG(item_start && group && value && out && ws, "fr_df_cells: null pointer");
    FR_CHECK_ARG(n_items >= 1 && n_groups >= 1, "fr_df_cells: n_items >= 1 and n_groups >= 1 (got %lld, %d)",
                 (long long)n_items, (int)n_groups);
    FR_CHECK_ARG(ws_bytes >= fr_df_cells_workspace_bytes(n_items), "fr_df_cells: workspace too small");
    const long long per_block = DF_THREADS / DF_GROUP;
    const long long blocks = (n_items + per_block - 1) / per_block;
    FR_CHECK_ARG(blocks <= 0x7fffffffLL, "fr_df_cells: %lld items are more than one launch takes", (long long)n_items);
    ProfScope prof(K_DF_CELLS, stream);
    FR_LAUNCH(prof, df_cells_kernel, dim3((unsigned)blocks), dim3(DF_THREADS), 0, stream, perm, item_start, (long long)n_items,
              group, value, (int)n_groups, (double*)ws);
    FR_CHECK_LAUNCH();
    hipLaunchKernelGGL(column_sum_kernel, dim3(1), dim3(256), 0, stream, (const double*)ws, blocks, 1, 1.0 / (double)n_items, out);
    FR_CHECK_LAUNCH();
    return FR_OK;
}

static long long value_blocks(int64_t n) {
    const long long b = (n + VM_ROWS - 1) / VM_ROWS;
    return b < VM_MAXBLOCKS ? b : VM_MAXBLOCKS;
}

extern "C" size_t fr_value_metrics_workspace_bytes(int64_t n) {
    return n < 1 || n >= (1ll << 31) ? 0 : (size_t)value_blocks(n) * 4 * sizeof(double);
}

extern "C" int fr_value_metrics(const float* score, const float* label, int64_t n, double* out, int64_t* counts, void* ws,
                                size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    FR_CHECK_ARG(score && label && out && counts && ws, "fr_value_metrics: null pointer");
    FR_CHECK_ARG(n >= 1 && n < (1ll << 31), "fr_value_metrics: 1 <= n < 2^31 (got %lld)", (long long)n);
    FR_CHECK_ARG(ws_bytes >= fr_value_metrics_workspace_bytes(n), "fr_value_metrics: workspace too small");
    const long long blocks = value_blocks(n);
    double* part_d = (double*)ws;
    long long* part_i = (long long*)(part_d + blocks * 3);
    hipLaunchKernelGGL(value_partials_kernel, dim3((unsigned)blocks), dim3(VM_THREADS), 0, stream, score, label, (long long)n,
                       part_d, part_i);
    FR_CHECK_LAUNCH();
    hipLaunchKernelGGL(value_fold_kernel, dim3(1), dim3(VM_THREADS), 0, stream, (const double*)part_d, (const long long*)part_i,
                       (int)blocks, (long long)n, out, (long long*)counts);
    FR_CHECK_LAUNCH();
    return FR_OK;
}

// workspace of fr_auc_sorted: part int64 [tiles] | C int32 [n + 1] | tile_off int32 [tiles + 1]
extern "C" size_t fr_auc_sorted_workspace_bytes(int64_t n) {
    if (n < 1 || n >= (1ll << 31)) return 0;
    const size_t tiles = (size_t)((n + AUC_TILE - 1) / AUC_TILE);
    return tiles * sizeof(long long) + align_up((size_t)(n + 1) * sizeof(int32_t), 8) + (tiles + 1) * sizeof(int32_t);
}

extern "C" int fr_auc_sorted(const float* score_sorted, const float* label_sorted, int64_t n, int64_t* out, void* ws,
                             size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    FR_CHECK_ARG(score_sorted && label_sorted && out && ws, "fr_auc_sorted: null pointer");
    FR_CHECK_ARG(n >= 1 && n < (1ll << 31), "fr_auc_sorted: 1 <= n < 2^31 (got %lld)", (long long)n);
    FR_CHECK_ARG(ws_bytes >= fr_auc_sorted_workspace_bytes(n), "fr_auc_sorted: workspace too small");
    const long long tiles = (n + AUC_TILE - 1) / AUC_TILE;
    long long* part = (long long*)ws;
    int32_t* C = (int32_t*)(part + tiles);
    int32_t* tile_off = (int32_t*)((char*)C + align_up((size_t)(n + 1) * sizeof(int32_t), 8));
    hipLaunchKernelGGL(auc_count_kernel, dim3((unsigned)tiles), dim3(AUC_THREADS), 0, stream, label_sorted, (long long)n, tile_off);
    FR_CHECK_LAUNCH();
    hipLaunchKernelGGL(auc_scan_tiles_kernel, dim3(1), dim3(AUC_THREADS), 0, stream, tile_off, tiles);
    FR_CHECK_LAUNCH();
    hipLaunchKernelGGL(auc_prefix_kernel, dim3((unsigned)tiles), dim3(AUC_THREADS), 0, stream, label_sorted, (long long)n,
                       (const int32_t*)tile_off, C);
    FR_CHECK_LAUNCH();
    hipLaunchKernelGGL(auc_runs_kernel, dim3((unsigned)tiles), dim3(AUC_THREADS), 0, stream, score_sorted, (long long)n,
                       (const int32_t*)C, part);
    FR_CHECK_LAUNCH();
    hipLaunchKernelGGL(auc_fold_kernel, dim3(1), dim3(AUC_THREADS), 0, stream, (const long long*)part, tiles, (long long)n,
                       (const int32_t*)C, (long long*)out);
    FR_CHECK_LAUNCH();
    return FR_OK;
}

extern "C" size_t fr_eval_meanrank_workspace_bytes(int64_t n_rows) { return n_rows < 1 ? 0 : (size_t)n_rows; }

extern "C" int fr_eval_meanrank_segments(const int64_t* seg_start, int64_t n_users, const int64_t* items, const float* scores,
                                         const int64_t* pos_keys, int64_t n_pos, int64_t n_items, int64_t n_rows, int64_t* out,
                                         void* ws, size_t ws_bytes, void* stream_) {
    FR_CHECK_ARG(seg_start && scores && out && (pos_keys || n_pos == 0), "fr_eval_meanrank_segments: null pointer");
    FR_CHECK_ARG(n_users >= 1 && n_rows >= 1 && n_pos >= 0 && n_items >= 1,
                 "fr_eval_meanrank_segments: n_users >= 1, n_rows >= 1, n_pos >= 0 and n_items >= 1");
    FR_CHECK_ARG(!items || (ws && ws_bytes >= fr_eval_meanrank_workspace_bytes(n_rows)),
                 "fr_eval_meanrank_segments: workspace too small (one byte per row when items are given)");
    hipLaunchKernelGGL(eval_meanrank_segments_kernel, dim3((unsigned)((n_users + 3) / 4)), dim3(256), 0, (hipStream_t)stream_,
                       seg_start, (long long)n_users, items, scores, pos_keys, (long long)n_pos, (long long)n_items, (uint8_t*)ws,
                       out);
    FR_CHECK_LAUNCH();
    return FR_OK;
}
