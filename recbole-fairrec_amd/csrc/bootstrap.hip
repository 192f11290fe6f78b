// Poisson bootstrap over rows (fairrec_hip.h: fr_bootstrap_group_sums): per group of rows and per replicate b the weighted column
// sums  sum_r w(r, b) * values[r][c]  and the weight sums  sum_r w(r, b),  w(r, b) ~ Poisson(1) from Philox4x32-10 by the contract
// of the header.  n_rows x n_rep weights are never stored: a lane makes the four weights of its four replicates from ONE Philox
// call per row, in registers -- what fr_recommend_topk does with the score matrix and fr_exposure_grouped with the [groups, items]
// table.
//
//   bootstrap_chunk_kernel   grid (chunks, replicate tiles of 1024, column tiles of 8), 256 threads.  A workgroup stages BS_ROWS
//                            positions of its chunk at a time in LDS (8 columns of the row and the row index), then every lane
//                            walks the staged rows: one Philox call, four weights, 4 x 8 fused multiply-adds into its own
//                            accumulators; the LDS reads are broadcasts (every lane reads the same row).  No cross-lane reduction.
//   group_fold_kernel        (metrics.hip) adds a group's per-chunk partials [chunk][n_rep][n_cols] in ascending chunk order,
//   bootstrap_fold_weight_kernel   the same for the integer weight sums.
// Groups are segments of a permutation cut into chunks as in metrics.hip, with a chunk length that grows with n_rows: at most
// BS_MAX_CHUNKS + n_groups chunks, so the workspace is bounded by that times n_rep * n_cols, never by n_rows * n_rep.
// Work: n_rows * n_rep * n_cols fused multiply-adds and n_rows * n_rep / 4 Philox calls per column tile.
#include "dropout.hpp"
#include "eval_common.hpp"
#include "kernels.hpp"

namespace fr {

static constexpr int BS_THREADS = 256, BS_ROWS = 64, BS_COLS = 8, BS_REP_TILE = BS_THREADS * 4, BS_MAX_CHUNKS = 2048;

// w = #{ j : word >= T[j] },  T[j] = floor(2^32 e^-1 sum_{i <= j} 1 / i!): the inverse CDF of Poisson(1) on 32 bits
__device__ __forceinline__ int poisson1(unsigned word) {
    return (word >= 0x5e2d58d8u) + (word >= 0xbc5ab1b1u) + (word >= 0xeb715e1du) + (word >= 0xfb239797u) +
           (word >= 0xff1025f5u) + (word >= 0xffd90f3bu) + (word >= 0xfffa8b71u) + (word >= 0xffff540cu) +
           (word >= 0xffffed1fu) + (word >= 0xfffffe21u) + (word >= 0xffffffd4u) + (word >= 0xfffffffcu);
}

// part_sums[chunk][n_rep][n_cols], part_w[chunk][n_rep] (written by the workgroups of column tile 0)
__global__ __launch_bounds__(BS_THREADS) void bootstrap_chunk_kernel(const double* __restrict__ values, long long ld, int n_cols,
                                                                     const int64_t* __restrict__ perm,
                                                                     const int64_t* __restrict__ group_start, long long U,
                                                                     long long G, const long long* __restrict__ chunk_start,
                                                                     long long chunk_len, int n_rep, uint2 key,
                                                                     double* __restrict__ part_sums,
                                                                     long long* __restrict__ part_w) {
    __shared__ double sv[BS_ROWS][BS_COLS];
    __shared__ unsigned sr[BS_ROWS];
    long long g, c;
    if (!block_chunk(chunk_start, G, blockIdx.x, g, c)) return;        // (the whole workgroup: before any barrier)
    long long lo, hi;
    group_range(group_start, g, U, lo, hi);
    const long long j0 = lo + c * chunk_len < hi ? lo + c * chunk_len : hi;
    const long long j1 = j0 + chunk_len < hi ? j0 + chunk_len : hi;
    const int col0 = blockIdx.z * BS_COLS;
    const int ncol = n_cols - col0 < BS_COLS ? n_cols - col0 : BS_COLS;
    const unsigned quad = blockIdx.y * BS_THREADS + threadIdx.x;       // replicates 4 quad .. 4 quad + 3
    const bool active = (long long)quad * 4 < n_rep;
    double acc[4][BS_COLS];
    int wsum[4] = {0, 0, 0, 0};                                        // <= 12 * chunk_len < 2^31 (chunk_len <= 2^20)
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int cc = 0; cc < BS_COLS; ++cc) acc[q][cc] = 0.0;
    for (long long base = j0; base < j1; base += BS_ROWS) {
        const int n = (int)(j1 - base < BS_ROWS ? j1 - base : BS_ROWS);
        __syncthreads();                                               // the tile before is consumed
        for (int i = threadIdx.x; i < n * BS_COLS; i += BS_THREADS) {
            const int r = i / BS_COLS, cc = i % BS_COLS;
            const long long row = perm ? clamp_ll(perm[base + r], 0, U - 1) : base + r;
            sv[r][cc] = cc < ncol ? values[row * ld + col0 + cc] : 0.0;
            if (cc == 0) sr[r] = (unsigned)row;
        }
        __syncthreads();
        if (!active) continue;
        for (int r = 0; r < n; ++r) {
            const uint4 x = philox4x32(make_uint4(sr[r], 0u, quad, 0u), key);
            const int w[4] = {poisson1(x.x), poisson1(x.y), poisson1(x.z), poisson1(x.w)};
            double v[BS_COLS];
#pragma unroll
            for (int cc = 0; cc < BS_COLS; ++cc) v[cc] = sv[r][cc];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double wd = (double)w[q];
                wsum[q] += w[q];
#pragma unroll
                for (int cc = 0; cc < BS_COLS; ++cc) acc[q][cc] = fma(wd, v[cc], acc[q][cc]);
            }
        }
    }
    if (!active) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long long b = (long long)quad * 4 + q;
        if (b >= n_rep) break;
        double* o = part_sums + ((size_t)blockIdx.x * n_rep + b) * n_cols + col0;
#pragma unroll
        for (int cc = 0; cc < BS_COLS; ++cc)
            if (cc < ncol) o[cc] = acc[q][cc];
        if (blockIdx.z == 0) part_w[(size_t)blockIdx.x * n_rep + b] = wsum[q];
    }
}

// out_weight[g][b] = sum over group g's chunks of part_w[chunk][b]
__global__ __launch_bounds__(256) void bootstrap_fold_weight_kernel(const long long* __restrict__ part_w,
                                                                    const long long* __restrict__ chunk_start, long long G,
                                                                    int n_rep, int64_t* __restrict__ out_weight) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= G * n_rep) return;
    const long long g = t / n_rep;
    const int b = (int)(t % n_rep);
    long long a = 0;
    for (long long k = chunk_start[g]; k < chunk_start[g + 1]; ++k) a += part_w[k * n_rep + b];
    out_weight[t] = a;
}

}  // namespace fr

using namespace fr;

// chunk length and the grid's first dimension (an upper bound on the chunks); 0 = out of range
static long long bootstrap_blocks(int64_t n_rows, int32_t n_cols, int64_t n_groups, int32_t n_rep, long long* chunk_len) {
    if (n_rows < 1 || n_rows >= (1ll << 31) || n_cols < 1 || n_cols > FR_BOOTSTRAP_MAX_COLS || n_rep < 1 ||
        n_rep > FR_BOOTSTRAP_MAX_REP || n_groups < 1)
        return 0;
    // (the folds: one thread per output cell, 2^31 - 1 blocks of 256 at the most)
    if (n_groups > 0x7fffffffLL * 256 / ((long long)n_rep * n_cols)) return 0;
    const long long len = 64 * ((n_rows + 64ll * BS_MAX_CHUNKS - 1) / (64ll * BS_MAX_CHUNKS));
    const long long blocks = (n_rows + len - 1) / len + n_groups;
    if (blocks > 0x7fffffffLL) return 0;
    if (chunk_len) *chunk_len = len;
    return blocks;
}

// workspace: part_sums double [blocks][n_rep][n_cols] | part_w int64 [blocks][n_rep] | chunk_start int64 [n_groups + 1]
extern "C" size_t fr_bootstrap_group_sums_workspace_bytes(int64_t n_rows, int32_t n_cols, int64_t n_groups, int32_t n_rep) {
    const long long blocks = bootstrap_blocks(n_rows, n_cols, n_groups, n_rep, nullptr);
    if (blocks == 0) return 0;
    return ((size_t)blocks * n_rep * ((size_t)n_cols + 1) + (size_t)n_groups + 1) * 8;
}

extern "C" int fr_bootstrap_group_sums(const double* values, int64_t n_rows, int32_t n_cols, int64_t ld, const int64_t* perm,
                                       const int64_t* group_start, int64_t n_groups, int32_t n_rep, uint64_t seed,
                                       double* out_sums, int64_t* out_weight, void* ws, size_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    FR_CHECK_ARG(values && group_start && out_sums && out_weight && ws, "fr_bootstrap_group_sums: null pointer");
    long long chunk_len = 0;
    const long long blocks = bootstrap_blocks(n_rows, n_cols, n_groups, n_rep, &chunk_len);
    FR_CHECK_ARG(blocks > 0,
                 "fr_bootstrap_group_sums: 1 <= n_rows < 2^31, 1 <= n_cols <= %d, 1 <= n_rep <= %d, n_groups >= 1 and within one "
                 "launch (got %lld, %d, %d, %lld)",
                 FR_BOOTSTRAP_MAX_COLS, FR_BOOTSTRAP_MAX_REP, (long long)n_rows, (int)n_cols, (int)n_rep, (long long)n_groups);
    FR_CHECK_ARG(ld >= n_cols, "fr_bootstrap_group_sums: ld %lld below n_cols %d", (long long)ld, (int)n_cols);
    FR_CHECK_ARG(ws_bytes >= fr_bootstrap_group_sums_workspace_bytes(n_rows, n_cols, n_groups, n_rep),
                 "fr_bootstrap_group_sums: workspace too small");
    double* part_sums = (double*)ws;
    long long* part_w = (long long*)(part_sums + (size_t)blocks * n_rep * n_cols);
    long long* chunk_start = part_w + (size_t)blocks * n_rep;
    if (int rc = launch_group_chunk_scan(group_start, n_groups, n_rows, chunk_len, blocks, chunk_start, stream)) return rc;
    const dim3 grid((unsigned)blocks, (unsigned)((n_rep + BS_REP_TILE - 1) / BS_REP_TILE), (unsigned)((n_cols + BS_COLS - 1) / BS_COLS));
    ProfScope prof(K_BOOTSTRAP, stream);
    FR_LAUNCH(prof, bootstrap_chunk_kernel, grid, dim3(BS_THREADS), 0, stream, values, (long long)ld, (int)n_cols, perm, group_start,
              (long long)n_rows, (long long)n_groups, (const long long*)chunk_start, chunk_len, (int)n_rep,
              make_uint2((unsigned)seed, (unsigned)(seed >> 32)), part_sums, part_w);
    FR_CHECK_LAUNCH();
    if (int rc = launch_group_fold(part_sums, chunk_start, group_start, n_rows, n_groups, n_rep * n_cols, false, out_sums, stream))
        return rc;
    hipLaunchKernelGGL(bootstrap_fold_weight_kernel, dim3((unsigned)((n_groups * n_rep + 255) / 256)), dim3(256), 0, stream,
                       (const long long*)part_w, (const long long*)chunk_start, (long long)n_groups, (int)n_rep, out_weight);
    FR_CHECK_LAUNCH();
    return FR_OK;
}
