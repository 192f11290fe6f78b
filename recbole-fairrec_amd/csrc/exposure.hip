// Exposure metrics per group of users (GiniIndex, ItemCoverage, ShannonEntropy, PopularityPercentage, TailPercentage,
// AveragePopularity @ k of recbole/evaluator/metrics.py:438-821) for every group and every cut-off in one chain, from the
// list entries sorted by the key (group * n_items + item) * k_cols + rank.  Memory is O(entries): no [groups, items] table.
//
//   exposure_heads_kernel   a thread per EX_PER_THREAD entries (strided by the block: coalesced).  Every entry adds
//                           popular[item], tail[item] and count_items[item] to the sums of its group for each cut-off its
//                           rank lies under (in registers; a wave adds up before its atomics).  The first entry
//                           of a cell (one (group, item) pair) finds the cell's count at every cut-off by a galloping search
//                           for the key cell * k_cols + min(k_j, k_cols) -- the rank is the low part of the key, so a cell is
//                           sorted by rank and no cell is walked -- and adds 1 to the count-of-counts histogram of (group, j)
//                           at that count.  A count above the group's size (a padded list repeats item 0) goes to the short
//                           overflow list of (group, j) instead.
//   exposure_fold_kernel    a workgroup per (group, j): the histogram in ascending count gives the Gini numerator (exact
//                           int64), the distinct items, and the entropy in double in the order fairrec_hip.h states.
//
// Every cross-thread sum is an integer (atomics, order-independent); the entropy is summed in a fixed order without atomics:
// the same input gives the same bits on every call.
#include "eval_common.hpp"

namespace fr {

constexpr int EX_THREADS = 256;
constexpr int EX_PER_THREAD = 32;    // entries per thread: the atomics per (group, cut-off) address fall with it (a wave adds once)
constexpr int EX_MAX_K = 8;
constexpr int EX_SKIP = 8;          // fold: chunks of 256 counts loaded per barrier

struct ExCuts {
    int k[EX_MAX_K];
};

// the first position in [lo, n) whose key is >= target, galloping from lo: O(log(distance)) loads
__device__ __forceinline__ long long ex_lower_bound_from(const int64_t* __restrict__ keys, long long lo, long long n,
                                                         long long target) {
    long long hi = lo, step = 1;
    while (hi < n && keys[hi] < target) {
        lo = hi + 1;
        hi = step < n - hi ? hi + step : n;
        step <<= 1;
    }
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < target) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// one cell of `c` entries under cut-off j of group g (n_g users, segment at seg = group_start[g] + g): the histogram slot c,
// or the overflow list when the count does not fit the segment
__device__ __forceinline__ void ex_count_cell(long long c, long long n_g, long long seg, long long slot, int k_cols,
                                              unsigned* __restrict__ hist_j, int* __restrict__ ovf_cnt,
                                              long long* __restrict__ ovf) {
    if (c <= n_g) {
        atomicAdd(hist_j + seg + c, 1u);
    } else if (__hip_atomic_load(ovf_cnt + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < k_cols) {
        // (fewer than k_cols such cells exist in a well-formed input; a full list takes no more, so the counter stays small)
        const int s = atomicAdd(ovf_cnt + slot, 1);
        if (s >= 0 && s < k_cols) ovf[slot * k_cols + s] = c;
    }
}

__global__ __launch_bounds__(EX_THREADS) void exposure_heads_kernel(
    const int64_t* __restrict__ keys, long long n, long long N, int k_cols, const int64_t* __restrict__ group_start, long long G,
    long long U, ExCuts ks, int n_k, const uint8_t* __restrict__ popular, const uint8_t* __restrict__ tail,
    const int64_t* __restrict__ count_items, unsigned long long* __restrict__ acc, unsigned* __restrict__ hist,
    int* __restrict__ ovf_cnt, long long* __restrict__ ovf) {
    const int lane = threadIdx.x & 63;
    const long long base = (long long)blockIdx.x * (EX_THREADS * EX_PER_THREAD) + threadIdx.x;
    const long long hist_stride = U + G;
    // this thread's sums over its entries of group `cur`: pt = popular | tail << 16, cn = count_items, n1 = cells of count 1
    long long cur = -1, cur_seg = 0, cur_ng = 0;
    int pt[EX_MAX_K], n1[EX_MAX_K];
    long long cn[EX_MAX_K];
#pragma unroll
    for (int j = 0; j < EX_MAX_K; ++j) pt[j] = 0, n1[j] = 0, cn[j] = 0;

    for (int it = 0; it < EX_PER_THREAD; ++it) {
        const long long e = base + (long long)it * EX_THREADS;
        if (e >= n) break;
        long long key = keys[e];
        if (key < 0) key = 0;
        const long long cell = key / k_cols;
        const int r = (int)(key - cell * k_cols);
        long long g = cell / N;
        const long long item = cell - g * N;
        if (g >= G) g = G - 1;
        if (g != cur) {
            if (cur >= 0) {
                // a thread's entries span two groups at a group boundary only: its sums so far go out one by one
#pragma unroll
                for (int j = 0; j < EX_MAX_K; ++j)
                    if (j < n_k) {
                        unsigned long long* a = acc + (cur * n_k + j) * 3;
                        if (pt[j] & 0xffff) atomicAdd(a, (unsigned long long)(pt[j] & 0xffff));
                        if (pt[j] >> 16) atomicAdd(a + 1, (unsigned long long)(pt[j] >> 16));
                        if (cn[j]) atomicAdd(a + 2, (unsigned long long)cn[j]);
                        if (n1[j]) atomicAdd(hist + j * hist_stride + cur_seg + 1, (unsigned)n1[j]);
                        pt[j] = 0, n1[j] = 0, cn[j] = 0;
                    }
            }
            cur = g;
            long long hi;
            group_range(group_start, g, U, cur_seg, hi);
            cur_ng = hi - cur_seg;
            cur_seg += g;
        }
        const int pv = (popular && popular[item] ? 1 : 0) | (tail && tail[item] ? 1 << 16 : 0);
        const long long cv = count_items ? count_items[item] : 0;
#pragma unroll
        for (int j = 0; j < EX_MAX_K; ++j)
            if (j < n_k && r < ks.k[j]) pt[j] += pv, cn[j] += cv;
        const long long first = cell * k_cols;
        bool head = e == 0;
        if (!head) {
            // (unsigned: a malformed key near the ends of the int64 range wraps instead of overflowing)
            head = (unsigned long long)keys[e - 1] - (unsigned long long)first >= (unsigned long long)k_cols;
        }
        if (head) {
            long long pos = e;
#pragma unroll
            for (int j = 0; j < EX_MAX_K; ++j)
                if (j < n_k) {
                    const long long kk = ks.k[j] < k_cols ? ks.k[j] : k_cols;
                    pos = ex_lower_bound_from(keys, pos, n, first <= 0x7fffffffffffffffLL - kk ? first + kk : 0x7fffffffffffffffLL);
                    const long long c = pos - e;
                    if (c == 1 && cur_ng >= 1) ++n1[j];
                    else if (c >= 1) ex_count_cell(c, cur_ng, cur_seg, g * n_k + j, k_cols, hist + j * hist_stride, ovf_cnt, ovf);
                }
        }
    }

    // the lanes of a wave that hold the same group add up before one lane does the atomics (a sorted input: one group, two at
    // a boundary)
    unsigned long long todo = __ballot(cur >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const long long gl = __shfl(cur, leader, 64);
        const bool mine = cur == gl;
#pragma unroll
        for (int j = 0; j < EX_MAX_K; ++j)
            if (j < n_k) {
                const int spt = wave_sum(mine ? pt[j] : 0);       // at most 64 * EX_PER_THREAD < 2^16 per half
                const long long scn = wave_sum(mine ? cn[j] : 0);
                const int sn1 = wave_sum(mine ? n1[j] : 0);
                if (lane == leader) {
                    unsigned long long* a = acc + (gl * n_k + j) * 3;
                    if (spt & 0xffff) atomicAdd(a, (unsigned long long)(spt & 0xffff));
                    if (spt >> 16) atomicAdd(a + 1, (unsigned long long)(spt >> 16));
                    if (scn) atomicAdd(a + 2, (unsigned long long)scn);
                    if (sn1) atomicAdd(hist + j * hist_stride + cur_seg + 1, (unsigned)sn1);
                }
            }
        todo &= ~__ballot(mine);
    }
}

__global__ __launch_bounds__(EX_THREADS) void exposure_fold_kernel(
    const int64_t* __restrict__ group_start, long long G, long long U, long long N, int k_cols, ExCuts ks, int n_k,
    const unsigned long long* __restrict__ acc, const unsigned* __restrict__ hist, const int* __restrict__ ovf_cnt,
    long long* __restrict__ ovf, int64_t* __restrict__ out_i, double* __restrict__ out_entropy) {
    __shared__ long long sh_ll[EX_THREADS / 64];
    __shared__ double sh_d[EX_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long b = blockIdx.x;
    const long long g = b / n_k;
    const int j = (int)(b - g * n_k);
    int kj = 1;
#pragma unroll
    for (int q = 0; q < EX_MAX_K; ++q)
        if (q == j) kj = ks.k[q];
    long long lo, hi;
    group_range(group_start, g, U, lo, hi);
    const long long n_g = hi - lo;
    if (n_g == 0) {                         // an empty group: five zeros, NaN entropy
        if (t < 5) out_i[b * 5 + t] = 0;
        if (t == 5) out_entropy[b] = __longlong_as_double(0x7ff8000000000000LL);
        return;
    }
    const unsigned* seg = hist + j * (U + G) + lo + g;       // slot c = cells of count c, 1 <= c <= n_g
    int n_ovf = ovf_cnt[b];
    n_ovf = n_ovf < 0 ? 0 : (n_ovf < k_cols ? n_ovf : k_cols);
    long long* list = ovf + b * k_cols;

    // m: the distinct items
    long long mine = 0;
    for (long long c = 1 + t; c <= n_g; c += EX_THREADS) mine += seg[c];
    mine = wave_sum(mine);
    if (lane == 0) sh_ll[wave] = mine;
    __syncthreads();
    const long long m = sh_ll[0] + sh_ll[1] + sh_ll[2] + sh_ll[3] + n_ovf;
    __syncthreads();

    // ascending count: p = items placed before the slot (the zero-count items first), S in int64, the entropy chunk by chunk
    const double T = (double)n_g * (double)kj;
    long long p = N - m, S = 0;
    double H = 0.0;
    // (most chunks of a large group hold no cell: EX_SKIP chunks are loaded at once and passed over after one barrier)
    for (long long s0 = 1; s0 <= n_g; s0 += EX_THREADS * EX_SKIP) {
        unsigned held[EX_SKIP];
        unsigned any = 0;
#pragma unroll
        for (int s = 0; s < EX_SKIP; ++s) {
            const long long c = s0 + s * EX_THREADS + t;
            held[s] = c <= n_g ? seg[c] : 0u;
            any |= held[s];
        }
        if (!__syncthreads_or(any != 0)) continue;
#pragma unroll
        for (int s = 0; s < EX_SKIP; ++s) {
            const long long c = s0 + s * EX_THREADS + t;
            const long long h = held[s];
            if (!__syncthreads_or(h != 0)) continue;              // a chunk without a cell adds +0.0 and moves nothing
            long long incl = h;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const long long up = __shfl_up(incl, o, 64);
                if (lane >= o) incl += up;
            }
            double term = 0.0;
            if (h > 0) {
                const double q = (double)c / T;
                term = (double)h * (-(q * log(q)));
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) term += __shfl_xor(term, o, 64);
            if (lane == 63) sh_ll[wave] = incl;
            if (lane == 0) sh_d[wave] = term;
            __syncthreads();
            long long before = 0;
#pragma unroll
            for (int w = 0; w < EX_THREADS / 64; ++w)
                if (w < wave) before += sh_ll[w];
            const long long placed = p + before + incl - h;
            S += (c * h) * (2 * placed + h - N);
            p += sh_ll[0] + sh_ll[1] + sh_ll[2] + sh_ll[3];
            H += ((sh_d[0] + sh_d[1]) + sh_d[2]) + sh_d[3];
        }
    }
    S = wave_sum(S);
    __syncthreads();
    if (lane == 0) sh_ll[wave] = S;
    __syncthreads();
    if (t == 0) {
        S = sh_ll[0] + sh_ll[1] + sh_ll[2] + sh_ll[3];
        // the cells above n_g: sorted ascending (the arrival order of the appends leaves no trace), each placed after everything
        for (int a = 1; a < n_ovf; ++a) {
            const long long v = list[a];
            int q = a - 1;
            for (; q >= 0 && list[q] > v; --q) list[q + 1] = list[q];
            list[q + 1] = v;
        }
        for (int a = 0; a < n_ovf; ++a) {
            const long long c = list[a];
            S += c * (2 * p + 1 - N);
            ++p;
            const double q = (double)c / T;
            H += 1.0 * (-(q * log(q)));
        }
        const unsigned long long* a = acc + b * 3;
        out_i[b * 5 + 0] = m;
        out_i[b * 5 + 1] = S;
        out_i[b * 5 + 2] = (long long)a[0];
        out_i[b * 5 + 3] = (long long)a[1];
        out_i[b * 5 + 4] = (long long)a[2];
        out_entropy[b] = H;
    }
}

// the workspace in 8-byte words: acc[G][n_k][3], ovf[G][n_k][k_cols], hist[n_k][U + G] (uint32), ovf_cnt[G][n_k] (int32)
static bool exposure_layout(int64_t n_users, int32_t k_cols, int64_t n_groups, int32_t n_k, size_t* acc_w, size_t* ovf_w,
                            size_t* hist_w, size_t* cnt_w) {
    if (n_users < 1 || k_cols < 1 || n_groups < 1 || n_k < 1 || n_k > EX_MAX_K) return false;
    if (n_users > (1ll << 40) || n_groups > 0x7fffffffLL / n_k) return false;      // the fold grid: n_groups * n_k blocks
    const unsigned __int128 cells = (unsigned __int128)n_groups * n_k;
    const unsigned __int128 total = cells * 3 + cells * (unsigned)k_cols + ((unsigned __int128)n_k * (n_users + n_groups) + 1) / 2 +
                                    (cells + 1) / 2;
    if (total > ((unsigned __int128)1 << 56)) return false;
    *acc_w = (size_t)cells * 3;
    *ovf_w = (size_t)cells * (size_t)k_cols;
    *hist_w = ((size_t)n_k * (size_t)(n_users + n_groups) + 1) / 2;
    *cnt_w = ((size_t)cells + 1) / 2;
    return true;
}

}  // namespace fr

using namespace fr;

extern "C" size_t fr_exposure_grouped_workspace_bytes(int64_t n_users, int32_t k_cols, int64_t n_groups, int32_t n_k) {
    size_t a, o, h, c;
    return exposure_layout(n_users, k_cols, n_groups, n_k, &a, &o, &h, &c) ? (a + o + h + c) * 8 : 0;
}

extern "C" int fr_exposure_grouped(const int64_t* keys_sorted, int64_t n_entries, int64_t n_items, int32_t k_cols,
                                   const int64_t* group_start, int64_t n_groups, const int32_t* ks, int32_t n_k,
                                   const uint8_t* popular, const uint8_t* tail, const int64_t* count_items, int64_t* out_i,
                                   double* out_entropy, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    FR_CHECK_ARG(keys_sorted && group_start && ks && out_i && out_entropy && ws, "fr_exposure_grouped: null pointer");
    FR_CHECK_ARG(n_entries >= 1 && n_items >= 1 && k_cols >= 1 && n_groups >= 1,
                 "fr_exposure_grouped: n_entries, n_items, k_cols, n_groups >= 1 (got %lld, %lld, %d, %lld)", (long long)n_entries,
                 (long long)n_items, (int)k_cols, (long long)n_groups);
    FR_CHECK_ARG(n_k >= 1 && n_k <= EX_MAX_K, "fr_exposure_grouped: n_k in 1..%d (got %d)", EX_MAX_K, (int)n_k);
    ExCuts cuts;
    for (int j = 0; j < EX_MAX_K; ++j) cuts.k[j] = 0x7fffffff;
    for (int j = 0; j < n_k; ++j) {
        FR_CHECK_ARG(ks[j] >= 1 && (j == 0 || ks[j] > ks[j - 1]),
                     "fr_exposure_grouped: ks must be strictly ascending and >= 1 (ks[%d] = %d)", j, (int)ks[j]);
        cuts.k[j] = ks[j];
    }
    FR_CHECK_ARG(n_entries % k_cols == 0, "fr_exposure_grouped: n_entries %lld is no multiple of k_cols %d", (long long)n_entries,
                 (int)k_cols);
    const int64_t n_users = n_entries / k_cols;
    FR_CHECK_ARG((unsigned __int128)n_groups * (unsigned __int128)n_items * (unsigned)k_cols < ((unsigned __int128)1 << 63),
                 "fr_exposure_grouped: n_groups * n_items * k_cols = %lld * %lld * %d does not fit the int64 key",
                 (long long)n_groups, (long long)n_items, (int)k_cols);
    FR_CHECK_ARG((unsigned __int128)n_items * (unsigned __int128)n_entries < ((unsigned __int128)1 << 62),
                 "fr_exposure_grouped: n_items * n_users * k_cols = %lld * %lld does not fit the int64 Gini numerator",
                 (long long)n_items, (long long)n_entries);
    size_t acc_w, ovf_w, hist_w, cnt_w;
    const long long blocks = (n_entries + EX_THREADS * EX_PER_THREAD - 1) / (EX_THREADS * EX_PER_THREAD);
    FR_CHECK_ARG(exposure_layout(n_users, k_cols, n_groups, n_k, &acc_w, &ovf_w, &hist_w, &cnt_w) && n_entries < (1ll << 32) &&
                     blocks <= 0x7fffffffLL,
                 "fr_exposure_grouped: %lld entries in %lld groups are more than one call takes", (long long)n_entries,
                 (long long)n_groups);
    const size_t need = (acc_w + ovf_w + hist_w + cnt_w) * 8;
    FR_CHECK_ARG(ws_bytes >= need, "fr_exposure_grouped: workspace too small");
    unsigned long long* acc = (unsigned long long*)ws;
    long long* ovf = (long long*)(acc + acc_w);
    unsigned* hist = (unsigned*)(ovf + ovf_w);
    int* ovf_cnt = (int*)((unsigned long long*)hist + hist_w);
    FR_CHECK_HIP(hipMemsetAsync(ws, 0, need, stream));
    hipLaunchKernelGGL(exposure_heads_kernel, dim3((unsigned)blocks), dim3(EX_THREADS), 0, stream, keys_sorted, (long long)n_entries,
                       (long long)n_items, (int)k_cols, group_start, (long long)n_groups, (long long)n_users, cuts, (int)n_k, popular,
                       tail, count_items, acc, hist, ovf_cnt, ovf);
    FR_CHECK_LAUNCH();
    hipLaunchKernelGGL(exposure_fold_kernel, dim3((unsigned)(n_groups * n_k)), dim3(EX_THREADS), 0, stream, group_start,
                       (long long)n_groups, (long long)n_users, (long long)n_items, (int)k_cols, cuts, (int)n_k,
                       (const unsigned long long*)acc, (const unsigned*)hist, (const int*)ovf_cnt, ovf, out_i, out_entropy);
    FR_CHECK_LAUNCH();
    return FR_OK;
}
