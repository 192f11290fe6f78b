// Poisson bootstrap over users of the fairness metrics (fairrec_hip.h: fr_bootstrap_fair_metrics): per replicate b the sums of the
// Value / Absolute / Under / Over terms and of the DifferentialFairness epsilon over the items present in b, the number K_b of
// those items, and NonParity's group totals -- the metric of the multiset in which member j occurs w(unit[j], b) times.  As in
// bootstrap.hip no weight is stored: a lane makes the four weights of its four replicates from ONE Philox call per member, in
// registers; here no per-replicate (item, group) table is stored either: a lane keeps the CURRENT item's cells for its four
// replicates in registers, closes the item after its last member and adds the item's terms to its running sums.
//
//   bf_count_kernel<MAXG, VT>   grid (chunks, replicate tiles of 256), one wave.  K_b, the group totals and (VT, two groups) the
//                               four value-type sums: nothing here needs alpha.
//   bf_df_kernel<MAXG>          the same walk with the cells {S, C} of up to MAXG groups; it starts from alpha = 1 / K_b, which
//                               the fold of the first walk has written.
//   bf_fold_kernel<T>           adds the per-chunk partials [chunk][column][n_rep] in ascending chunk order.
// A chunk is a run of consecutive WHOLE items: item k belongs to chunk floor(item_start[k] / L), found by two binary searches in
// item_start, so the chunks are balanced in members and need no scan.  The wave stages 64 item ends and 64 members at a time in
// LDS (lane = position), then every lane walks the staged members: the LDS reads are broadcasts.  No cross-lane reduction, no
// floating-point atomics.  An item is never split over waves: the longest item bounds the chain of its chunk.
// Work: n_members * n_rep / 4 Philox calls per walk, and per (item, replicate) four divisions (VT) or n_groups logf (DF).
#include "dropout.hpp"
#include "eval_common.hpp"
#include "kernels.hpp"

namespace fr {

static constexpr int BF_LANES = 64, BF_REP_TILE = BF_LANES * 4, BF_MAX_CHUNKS = 1024, BF_MAXG = 8;
static constexpr long long BF_MAX_MEMBERS = 1ll << 28;     // 12 * n_members < 2^32: an item's weight sum fits an unsigned

// the weight of bootstrap.hip: w = #{ j : word >= T[j] }, the inverse CDF of Poisson(1) on 32 bits (the header has the table)
__device__ __forceinline__ int poisson1(unsigned word) {
    return (word >= 0x5e2d58d8u) + (word >= 0xbc5ab1b1u) + (word >= 0xeb715e1du) + (word >= 0xfb239797u) +
           (word >= 0xff1025f5u) + (word >= 0xffd90f3bu) + (word >= 0xfffa8b71u) + (word >= 0xffff540cu) +
           (word >= 0xffffed1fu) + (word >= 0xfffffe21u) + (word >= 0xffffffd4u) + (word >= 0xfffffffcu);
}

struct BfTable {
    const int64_t* __restrict__ perm;
    const int64_t* __restrict__ item_start;
    const int32_t* __restrict__ group;
    const float* __restrict__ value;
    const float* __restrict__ wtrue;
    const int64_t* __restrict__ unit;
    long long K, M, L;
    int G;
};

struct BfTile {                      // what one wave stages: 64 members and the ends of 64 items
    int g[BF_LANES];
    float v[BF_LANES], t[BF_LANES];
    unsigned u[BF_LANES];
    long long end[BF_LANES];
};

// the first item k in [0, K] whose (clamped) start is >= x
__device__ __forceinline__ long long bf_first_item(const BfTable& tb, long long x) {
    long long lo = 0, hi = tb.K;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (clamp_ll(tb.item_start[mid], 0, tb.M) < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Walks chunk blockIdx.x: body.member(group, value, wtrue, unit) for every member in ascending position, body.close() after an
// item's last member (also for an empty item).  Every lane of the wave takes the same path: positions and items are uniform.
template <class Body>
__device__ __forceinline__ void bf_walk(const BfTable& tb, BfTile& s, Body& body) {
    const int lane = threadIdx.x;
    const long long c = blockIdx.x;
    const long long klo = bf_first_item(tb, c * tb.L);
    const long long khi = c + 1 == (long long)gridDim.x ? tb.K : bf_first_item(tb, (c + 1) * tb.L);
    if (klo >= khi) return;
    long long mb = -BF_LANES;                                         // the staged members are positions [mb, mb + 64)
    long long j0 = clamp_ll(tb.item_start[klo], 0, tb.M);
    for (long long k = klo; k < khi; ++k) {
        const int e = (int)((k - klo) & (BF_LANES - 1));
        if (e == 0) {
            __syncthreads();                                          // the ends before are consumed
            const long long kk = k + 1 + lane;
            s.end[lane] = kk <= khi ? clamp_ll(tb.item_start[kk], 0, tb.M) : tb.M;
            __syncthreads();
        }
        const long long j1 = s.end[e];
        for (long long j = j0; j < j1; ++j) {
            if (j < mb || j >= mb + BF_LANES) {
                __syncthreads();                                      // the tile before is consumed
                mb = j;
                const long long p = mb + lane;
                if (p < tb.M) {
                    const long long b = tb.perm ? clamp_ll(tb.perm[p], 0, tb.M - 1) : p;
                    s.g[lane] = tb.group[b];
                    s.v[lane] = tb.value[b];
                    s.t[lane] = tb.wtrue ? tb.wtrue[b] : 0.f;
                    s.u[lane] = (unsigned)tb.unit[b];
                }
                __syncthreads();
            }
            const int i = (int)(j - mb);
            body.member(__builtin_amdgcn_readfirstlane(s.g[i]), s.v[i], s.t[i], s.u[i]);   // (uniform: scalar branches on the group)
        }
        body.close();
        j0 = j1;
    }
}

// the first walk: K_b, the group totals, and with VT (MAXG == 2) the cells {S, C, T} of two groups and the four term sums
template <int MAXG, bool VT>
struct BfCount {
    int G;
    unsigned quad;
    uint2 key;
    double gs[MAXG][4];
    long long gw[MAXG][4];
    double S[VT ? 2 : 1][4], C[VT ? 2 : 1][4], T[VT ? 2 : 1][4], term[4][4];
    unsigned any[4];
    int kb[4];

    __device__ __forceinline__ void init(int G_, unsigned quad_, uint2 key_) {
        G = G_, quad = quad_, key = key_;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int q = 0; q < MAXG; ++q) gs[q][r] = 0.0, gw[q][r] = 0;
#pragma unroll
            for (int q = 0; q < (VT ? 2 : 1); ++q) S[q][r] = C[q][r] = T[q][r] = 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) term[q][r] = 0.0;
            any[r] = 0u, kb[r] = 0;
        }
    }
    __device__ __forceinline__ void member(int g, float v, float t, unsigned u) {
        if ((unsigned)g >= (unsigned)G) return;                       // counted in no cell
        const uint4 x = philox4x32(make_uint4(u, 0u, quad, 0u), key);
        const int w[4] = {poisson1(x.x), poisson1(x.y), poisson1(x.z), poisson1(x.w)};
        const double vd = (double)v, td = (double)t;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double wd = (double)w[r];
            any[r] |= (unsigned)w[r];
#pragma unroll
            for (int q = 0; q < MAXG; ++q)
                if (q == g) {
                    gs[q][r] = fma(wd, vd, gs[q][r]);
                    gw[q][r] += w[r];
                    if constexpr (VT) {
                        S[q][r] = fma(wd, vd, S[q][r]);
                        C[q][r] += wd;
                        T[q][r] = fma(wd, td, T[q][r]);
                    }
                }
        }
    }
    __device__ __forceinline__ void close() {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool present = any[r] != 0u;
            kb[r] += present;
            any[r] = 0u;
            if constexpr (VT) {
                // the terms of fair_from_stats_kernel (metrics.hip); an item that is not present has zero cells and zero terms
                const double n0 = C[0][r] + 1e-5, n1 = C[1][r] + 1e-5;
                const double p0 = S[0][r] / n0, p1 = S[1][r] / n1, r0 = T[0][r] / n0, r1 = T[1][r] / n1;
                term[0][r] += fabs((p0 - r0) - (p1 - r1));
                term[1][r] += fabs(fabs(p0 - r0) - fabs(p1 - r1));
                term[2][r] += fabs((r0 - p0 > 0 ? r0 - p0 : 0.0) - (r1 - p1 > 0 ? r1 - p1 : 0.0));
                term[3][r] += fabs((p0 - r0 > 0 ? p0 - r0 : 0.0) - (p1 - r1 > 0 ? p1 - r1 : 0.0));
#pragma unroll
                for (int q = 0; q < 2; ++q) S[q][r] = C[q][r] = T[q][r] = 0.0;
            }
        }
    }
};

// part_d[chunk][5 + G][n_rep]: columns 0..3 the term sums (zeros without VT), 4 left to bf_df_kernel, 5.. the group sums;
// part_i[chunk][1 + G][n_rep]: K_b, the group weights
template <int MAXG, bool VT>
__global__ __launch_bounds__(BF_LANES) void bf_count_kernel(BfTable tb, int n_rep, uint2 key, double* __restrict__ part_d,
                                                            long long* __restrict__ part_i) {
    __shared__ BfTile s;
    const unsigned quad = blockIdx.y * BF_LANES + threadIdx.x;         // replicates 4 quad .. 4 quad + 3
    BfCount<MAXG, VT> body;
    body.init(tb.G, quad, key);
    bf_walk(tb, s, body);
    double* pd = part_d + (size_t)blockIdx.x * (5 + tb.G) * n_rep;
    long long* pi = part_i + (size_t)blockIdx.x * (1 + tb.G) * n_rep;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long b = (long long)quad * 4 + r;
        if (b >= n_rep) break;
#pragma unroll
        for (int q = 0; q < 4; ++q) pd[(size_t)q * n_rep + b] = body.term[q][r];
        pi[b] = body.kb[r];
#pragma unroll
        for (int q = 0; q < MAXG; ++q)
            if (q < tb.G) {
                pd[(size_t)(5 + q) * n_rep + b] = body.gs[q][r];
                pi[(size_t)(1 + q) * n_rep + b] = body.gw[q][r];
            }
    }
}

// the second walk: the cells {S, C} of up to MAXG groups, alpha = 1 / K_b known
template <int MAXG>
struct BfDf {
    int G;
    unsigned quad;
    uint2 key;
    double S[MAXG][4], alpha[4], total[4];
    unsigned C[MAXG][4];

    __device__ __forceinline__ void member(int g, float v, float, unsigned u) {
        if ((unsigned)g >= (unsigned)G) return;
        const uint4 x = philox4x32(make_uint4(u, 0u, quad, 0u), key);
        const int w[4] = {poisson1(x.x), poisson1(x.y), poisson1(x.z), poisson1(x.w)};
        const double vd = (double)v;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q < MAXG; ++q)
                if (q == g) {
                    S[q][r] = fma((double)w[r], vd, S[q][r]);
                    C[q][r] += (unsigned)w[r];
                }
    }
    __device__ __forceinline__ void close() {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            // fair_from_stats_kernel's epsilon: the largest |logf(a) - logf(b)| over the pairs, a NaN difference left out
            float l[MAXG];
            unsigned any = 0u;
#pragma unroll
            for (int q = 0; q < MAXG; ++q) {
                l[q] = q < G ? logf((float)((S[q][r] + alpha[r]) / ((double)C[q][r] + 1.0))) : 0.f;
                any |= C[q][r];
                S[q][r] = 0.0, C[q][r] = 0u;
            }
            float eps = 0.f;
#pragma unroll
            for (int i = 0; i < MAXG; ++i)
#pragma unroll
                for (int j = i + 1; j < MAXG; ++j)
                    if (j < G) {
                        const float e = fabsf(l[i] - l[j]);
                        eps = e > eps ? e : eps;
                    }
            total[r] += any != 0u ? (double)eps : 0.0;
        }
    }
};

template <int MAXG>
__global__ __launch_bounds__(BF_LANES) void bf_df_kernel(BfTable tb, int n_rep, uint2 key, const int64_t* __restrict__ items,
                                                         double* __restrict__ part_d) {
    __shared__ BfTile s;
    const unsigned quad = blockIdx.y * BF_LANES + threadIdx.x;
    BfDf<MAXG> body;
    body.G = tb.G, body.quad = quad, body.key = key;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long b = (long long)quad * 4 + r;
        body.alpha[r] = 1.0 / (double)(b < n_rep ? items[b] : 1);      // K_b = 0: no item is present, alpha is not used
        body.total[r] = 0.0;
#pragma unroll
        for (int q = 0; q < MAXG; ++q) body.S[q][r] = 0.0, body.C[q][r] = 0u;
    }
    bf_walk(tb, s, body);
    double* pd = part_d + ((size_t)blockIdx.x * (5 + tb.G) + 4) * n_rep;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long b = (long long)quad * 4 + r;
        if (b < n_rep) pd[b] = body.total[r];
    }
}

// out[i] = sum over the chunks, ascending, of part[chunk * stride + i], i < n; the entries from `split` on go to out_b
template <class T>
__global__ __launch_bounds__(256) void bf_fold_kernel(const T* __restrict__ part, size_t stride, int chunks, long long n,
                                                      long long split, T* __restrict__ out_a, T* __restrict__ out_b) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    T a = 0;
    for (int c = 0; c < chunks; ++c) a += part[(size_t)c * stride + i];
    if (i < split) out_a[i] = a;
    else out_b[i - split] = a;
}

}  // namespace fr

using namespace fr;

// the number of chunks; 0 = arguments out of range
static long long bf_chunks(int64_t n_members, int64_t n_items, int32_t n_groups, int32_t n_rep) {
    if (n_members < 1 || n_members > BF_MAX_MEMBERS || n_items < 1 || n_items >= (1ll << 31) || n_groups < 1 ||
        n_groups > BF_MAXG || n_rep < 1 || n_rep > FR_BOOTSTRAP_MAX_REP)
        return 0;
    long long c = BF_MAX_CHUNKS;
    if (c > n_items) c = n_items;
    if (c > (1ll << 20) / n_rep) c = (1ll << 20) / n_rep;
    if (c > (n_members + 63) / 64) c = (n_members + 63) / 64;
    return c < 1 ? 1 : c;
}

// workspace: part_d double [chunks][5 + G][n_rep] | part_i int64 [chunks][1 + G][n_rep]
extern "C" size_t fr_bootstrap_fair_metrics_workspace_bytes(int64_t n_members, int64_t n_items, int32_t n_groups, int32_t n_rep) {
    const long long chunks = bf_chunks(n_members, n_items, n_groups, n_rep);
    return (size_t)chunks * n_rep * (2 * (size_t)(n_groups < 0 ? 0 : n_groups) + 6) * 8;
}

template <int MAXG, bool VT>
static void bf_launch_count(dim3 grid, hipStream_t stream, const BfTable& tb, int n_rep, uint2 key, double* part_d, long long* part_i) {
    hipLaunchKernelGGL((bf_count_kernel<MAXG, VT>), grid, dim3(BF_LANES), 0, stream, tb, n_rep, key, part_d, part_i);
}

extern "C" int fr_bootstrap_fair_metrics(const int64_t* perm, const int64_t* item_start, int64_t n_items, int64_t n_members,
                                         const int32_t* group, const float* value, const float* wtrue, const int64_t* unit,
                                         int32_t n_groups, int32_t n_rep, uint64_t seed, int32_t want, double* out_terms,
                                         int64_t* out_items, double* out_group_sum, int64_t* out_group_weight, void* ws,
                                         size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    FR_CHECK_ARG(item_start && group && value && unit && out_terms && out_items && out_group_sum && out_group_weight && ws,
                 "fr_bootstrap_fair_metrics: null pointer");
    const long long chunks = bf_chunks(n_members, n_items, n_groups, n_rep);
    FR_CHECK_ARG(chunks > 0,
                 "fr_bootstrap_fair_metrics: 1 <= n_members <= 2^28, 1 <= n_items < 2^31, 1 <= n_groups <= %d, 1 <= n_rep <= %d "
                 "(got %lld, %lld, %d, %d)",
                 BF_MAXG, FR_BOOTSTRAP_MAX_REP, (long long)n_members, (long long)n_items, (int)n_groups, (int)n_rep);
    FR_CHECK_ARG((want & ~(FR_FAIR_WANT_VALUE | FR_FAIR_WANT_DF)) == 0, "fr_bootstrap_fair_metrics: want %d has unknown bits", (int)want);
    const bool vt = want & FR_FAIR_WANT_VALUE, df = want & FR_FAIR_WANT_DF;
    FR_CHECK_ARG(!vt || n_groups == 2, "fr_bootstrap_fair_metrics: the value-type terms need n_groups == 2, not %d", (int)n_groups);
    FR_CHECK_ARG(ws_bytes >= fr_bootstrap_fair_metrics_workspace_bytes(n_members, n_items, n_groups, n_rep),
                 "fr_bootstrap_fair_metrics: workspace too small");
    const int G = n_groups;
    const size_t n = (size_t)n_rep;
    double* part_d = (double*)ws;
    long long* part_i = (long long*)(part_d + (size_t)chunks * (5 + G) * n);
    BfTable tb{perm, item_start, group, value, wtrue, unit, (long long)n_items, (long long)n_members,
               (long long)((n_members + chunks - 1) / chunks), G};
    const uint2 key = make_uint2((unsigned)seed, (unsigned)(seed >> 32));
    const dim3 grid((unsigned)chunks, (unsigned)((n_rep + BF_REP_TILE - 1) / BF_REP_TILE));
    if (vt) bf_launch_count<2, true>(grid, stream, tb, n_rep, key, part_d, part_i);
    else if (G <= 2) bf_launch_count<2, false>(grid, stream, tb, n_rep, key, part_d, part_i);
    else bf_launch_count<BF_MAXG, false>(grid, stream, tb, n_rep, key, part_d, part_i);
    FR_CHECK_LAUNCH();
    const long long ni = (long long)(1 + G) * n_rep;
    hipLaunchKernelGGL((bf_fold_kernel<long long>), dim3((unsigned)((ni + 255) / 256)), dim3(256), 0, stream,
                       (const long long*)part_i, (size_t)ni, (int)chunks, ni, (long long)n_rep, (long long*)out_items,
                       (long long*)out_group_weight);
    FR_CHECK_LAUNCH();
    if (df) {
        if (G <= 2)
            hipLaunchKernelGGL((bf_df_kernel<2>), grid, dim3(BF_LANES), 0, stream, tb, (int)n_rep, key, (const int64_t*)out_items, part_d);
        else
            hipLaunchKernelGGL((bf_df_kernel<BF_MAXG>), grid, dim3(BF_LANES), 0, stream, tb, (int)n_rep, key, (const int64_t*)out_items,
                               part_d);
        FR_CHECK_LAUNCH();
    } else {
        FR_CHECK_HIP(hipMemsetAsync(out_terms + 4 * n, 0, n * sizeof(double), stream));
    }
    // columns 0..3 (and 4 with DifferentialFairness) -> out_terms, columns 5.. -> out_group_sum
    const long long nt = (long long)(df ? 5 : 4) * n_rep, ng = (long long)G * n_rep;
    hipLaunchKernelGGL((bf_fold_kernel<double>), dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, stream, (const double*)part_d,
                       (size_t)(5 + G) * n, (int)chunks, nt, nt, out_terms, out_terms);
    FR_CHECK_LAUNCH();
    hipLaunchKernelGGL((bf_fold_kernel<double>), dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, stream,
                       (const double*)(part_d + 5 * n), (size_t)(5 + G) * n, (int)chunks, ng, ng, out_group_sum, out_group_sum);
    FR_CHECK_LAUNCH();
    return FR_OK;
}
