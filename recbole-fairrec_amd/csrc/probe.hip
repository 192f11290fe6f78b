// The sensitive-attribute leakage probe (fairrec/evaluator/leakage.py): one optimiser step of up to eight small attackers --
// one per sensitive attribute, a linear probe or an MLP with one hidden layer -- on one batch of user embeddings, in two
// launches whatever the number of heads; the same forward alone for the held-out rows; and the multiclass metric reduction.
//
// probe_step_kernel.  A workgroup of four waves walks `tpw` consecutive tiles of 32 rows (mlp_tile.hpp's tile: [32][odd
// stride] in LDS, 32 output columns per wave on v_mfma_f32_32x32x2_f32).  A tile of X is read ONCE and serves every head:
//     z1 = X W1^T + b1, h = relu(z1)        [32, H]   wave w: hidden units 32w.. of each group of 128
//     z2 = h W2^T + b2                      [32, C]   (H == 0: z2 = X W^T + b)
//     softmax, loss terms, dz2 = (p - onehot) / B      one thread per row, fr_softmax_ce's formulas
//     dW2 = dz2^T h, db2                    products over the 32 ROWS of the tile: 16 MFMA steps per 32 x 32 block
//     dh = dz2 W2, dz1 = dh (h > 0)         written over h
//     dW1 = dz1^T X, db1
// Every chain runs ascending from 0, two inner indices per MFMA step.  The weights are operands from a resident LDS image
// ([n_out][mt_stride(n_in)] per matrix) while all heads' images fit MT_LDS_MAX next to the tile buffers, and from global
// memory (L2) otherwise: the same chains, so the bits do not depend on which.  A 32 x 32 block of a weight gradient leaves
// the MFMA with 16 cells per lane; the lane adds them into ITS cells of the workgroup's own slot of the workspace (first
// tile: a store), so a cell has one owner, there is no atomic and no second writer.  The slot lives in L2 between the
// tiles of a workgroup; LDS goes to the weight images, which every MFMA step reads.
//
// probe_apply_kernel sums the slots in workgroup order, the loss partials likewise, and applies adam_elem -- the function
// fr_adam_dense runs -- to the flat parameter vector.
//
// The grid is probe_grid(B): a function of B alone.  With the fixed chains and the fixed summation orders every output's
// bits depend on the inputs alone.
#include "common.hpp"
#include "kernels.hpp"
#include "mlp_tile.hpp"

namespace fr {

constexpr int PB_ZS = 65;              // LDS row stride of the logit tile (C <= 64)
constexpr int PB_MAX_WG = 256;         // workgroups of a step at the most: a constant (the CUs of an MI355X), never a device query

struct ProbeGrid {
    int tiles, tpw, wgs;
};
// tiles of 32 rows; tiles per workgroup = ceil(tiles / 256); workgroups = ceil(tiles / tiles per workgroup)
__host__ __device__ inline ProbeGrid probe_grid(long long B) {
    ProbeGrid g;
    g.tiles = (int)((B + MT_RT - 1) / MT_RT);
    g.tpw = (g.tiles + PB_MAX_WG - 1) / PB_MAX_WG;
    g.wgs = (g.tiles + g.tpw - 1) / g.tpw;
    return g;
}

struct ProbeK {
    const float* X;
    const long long* rows;
    const long long* labels;
    const float* params;
    float* ws_grad;         // [wgs][P]
    float* ws_loss;         // [wgs][n_heads]
    float* logits;          // forward only: [B][sumC]; null in a step
    uint32_t* err;
    long long U, ldx, ldl;
    int B, D, H, n_heads, tpw, tiles, P, sumC, resident;
    int C[FR_PROBE_MAX_HEADS], p_off[FR_PROBE_MAX_HEADS], c_off[FR_PROBE_MAX_HEADS], img_off[FR_PROBE_MAX_HEADS];
};

// a weight matrix [n_rows][n_cols] with row stride ld, in LDS or in global memory; zero beyond either width
struct ProbeW {
    const float* p;
    int ld, n_rows, n_cols;
    __device__ __forceinline__ float at(int r, int c) const { return (r < n_rows && c < n_cols) ? p[r * ld + c] : 0.f; }
};

// one 32 x 32 block: acc[i][j] = sum_k a(k)[i] b(k)[j], k ascending from 0 in pairs; a(k) is this lane's A[lane & 31][k],
// b(k) its B[k][lane & 31]; both return 0 at k == K when K is odd
template <class FA, class FB>
__device__ __forceinline__ f32x16 pb_chain(const int K, const int h, FA&& a, FB&& b) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    int k = h;
    for (; k + 14 < K + h; k += 16) {      // eight steps' operands fetched ahead of their chain (the order stays ascending)
        float av[8], bv[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            av[q] = a(k + 2 * q);
            bv[q] = b(k + 2 * q);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q], bv[q], acc, 0, 0, 0);
    }
    for (; k < K + h; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a(k), b(k), acc, 0, 0, 0);
    return acc;
}

// dOut[i][j] (+)= sum over the tile's rows of lhs[row][i0 + i] rhs[row][j0 + j] for every 32 x 32 block of the [n_i][n_j]
// gradient `g`; lhs [32][s_l], rhs [32][s_r] in LDS, each with a zero column at index n (the clamp of a block's overhang)
__device__ __forceinline__ void pb_wgrad(const float* lhs, const int s_l, const int n_i, const float* rhs, const int s_r,
                                         const int n_j, float* g, const bool first, const int wave, const int li,
                                         const int h) {
    const int bj = (n_j + 31) >> 5, blocks = ((n_i + 31) >> 5) * bj;
    for (int t = wave; t < blocks; t += 4) {
        const int i0 = (t / bj) * 32, j0 = (t % bj) * 32;
        const int ci = i0 + li < n_i ? i0 + li : n_i, cj = j0 + li < n_j ? j0 + li : n_j;
        const f32x16 acc = pb_chain(MT_RT, h, [&](int k) { return lhs[k * s_l + ci]; },
                                    [&](int k) { return rhs[k * s_r + cj]; });
        const int j = j0 + li;
        if (j < n_j) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = i0 + mt_row(r, h);
                if (i < n_i) {
                    float* cell = g + (size_t)i * n_j + j;
                    *cell = first ? acc[r] : __fadd_rn(*cell, acc[r]);
                }
            }
        }
    }
}

// the bias gradient: column sums of t [32][s] over the rows, ascending
__device__ __forceinline__ void pb_bgrad(const float* t, const int s, const int n, float* g, const bool first, const int tid) {
    for (int c = tid; c < n; c += 256) {
        float a = 0.f;
        for (int r = 0; r < MT_RT; ++r) a = __fadd_rn(a, t[r * s + c]);
        g[c] = first ? a : __fadd_rn(g[c], a);
    }
}

__global__ __launch_bounds__(256) void probe_step_kernel(const ProbeK A) {
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6), li = lane & 31, h = lane >> 5;
    const int D = A.D, H = A.H, sD = mt_stride(D), sH = mt_stride(H);
    const int n_in = H ? H : D, s_in = H ? sH : sD;
    float* xs = lds;                                   // [32][sD]
    float* hs = xs + MT_RT * sD;                       // [32][sH]   (H > 0)
    float* zs = hs + (H ? MT_RT * sH : 0);             // [32][PB_ZS]
    float* lacc = zs + MT_RT * PB_ZS;                  // [heads][32]
    long long* rowid = (long long*)(lacc + FR_PROBE_MAX_HEADS * MT_RT);      // [32]
    float* img = (float*)(rowid + MT_RT);
    const bool fwd_only = A.logits != nullptr;
    lacc[tid] = 0.f;
    if (A.resident) {
        for (int a = 0; a < A.n_heads; ++a) {
            const float* p = A.params + A.p_off[a];
            float* im = img + A.img_off[a];
            if (H) {
                for (int e = tid; e < H * D; e += 256) im[(e / D) * sD + e % D] = p[e];
                im += H * sD;
                p += H * D + H;
            }
            for (int e = tid; e < A.C[a] * n_in; e += 256) im[(e / n_in) * s_in + e % n_in] = p[e];
        }
    }
    float* gslot = A.ws_grad + (size_t)blockIdx.x * A.P;
    const int t_begin = blockIdx.x * A.tpw, t_end = t_begin + A.tpw < A.tiles ? t_begin + A.tpw : A.tiles;
    for (int tile = t_begin; tile < t_end; ++tile) {
        const bool first = tile == t_begin;
        __syncthreads();      // the previous tile is done with every buffer (first tile: lacc and the images are written)
        if (tid < MT_RT) {
            const long long b = (long long)tile * MT_RT + tid;
            long long r = -1;
            if (b < A.B) {
                r = A.rows ? A.rows[b] : b;
                if (r < 0 || r >= A.U) {
                    atomicOr(A.err, FR_DEV_ERR_INDEX_RANGE);
                    r = -1;
                }
            }
            rowid[tid] = r;
        }
        __syncthreads();
        for (int i = 0; i < 8; ++i) {
            const int row = wave * 8 + i;
            const long long r = rowid[row];
            for (int c = lane; c < sD; c += 64) xs[row * sD + c] = (r >= 0 && c < D) ? A.X[r * A.ldx + c] : 0.f;
        }
        for (int a = 0; a < A.n_heads; ++a) {
            const int C = A.C[a];
            const float* p = A.params + A.p_off[a];
            const float* im = img + A.img_off[a];
            ProbeW W1{nullptr, 0, 0, 0};
            const float* b1 = nullptr;
            if (H) {
                W1 = A.resident ? ProbeW{im, sD, H, D} : ProbeW{p, D, H, D};
                b1 = p + H * D;
                p = b1 + H;
                im += H * sD;
            }
            const ProbeW W2 = A.resident ? ProbeW{im, s_in, C, n_in} : ProbeW{p, n_in, C, n_in};
            const float* b2 = p + C * n_in;
            float* g = gslot + A.p_off[a];
            float* gW2 = g + (H ? H * D + H : 0);
            __syncthreads();      // xs is written; the previous head is done with hs and zs
            if (H) {
                for (int cg = wave; cg * 32 < H; cg += 4) {
                    const int u = cg * 32 + li;
                    const f32x16 acc = pb_chain(D, h, [&](int k) { return xs[li * sD + k]; }, [&](int k) { return W1.at(u, k); });
                    if (u < H) {
                        const float bias = b1[u];
#pragma unroll
                        for (int r = 0; r < 16; ++r) hs[mt_row(r, h) * sH + u] = mt_relu(__fadd_rn(acc[r], bias));
                    }
                }
                for (int e = tid; e < MT_RT * (sH - H); e += 256) hs[(e / (sH - H)) * sH + H + e % (sH - H)] = 0.f;
                __syncthreads();
            }
            const float* in = H ? hs : xs;
            for (int cg = wave; cg * 32 < C; cg += 4) {
                const int c = cg * 32 + li;
                const f32x16 acc = pb_chain(n_in, h, [&](int k) { return in[li * s_in + k]; }, [&](int k) { return W2.at(c, k); });
                if (c < C) {
                    const float bias = b2[c];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = mt_row(r, h);
                        const float z = __fadd_rn(acc[r], bias);
                        zs[row * PB_ZS + c] = z;
                        const long long b = (long long)tile * MT_RT + row;
                        if (fwd_only && b < A.B) A.logits[b * A.sumC + A.c_off[a] + c] = z;
                    }
                }
            }
            if (fwd_only) continue;
            __syncthreads();
            if (tid < MT_RT) {      // softmax cross-entropy of one row, as softmax_ce_kernel (pfcn.hip) states it
                float* z = zs + tid * PB_ZS;
                const long long r = rowid[tid];
                long long y = r >= 0 ? A.labels[a * A.ldl + r] : -1;
                if (r >= 0 && (y < 0 || y >= C)) {
                    atomicOr(A.err, FR_DEV_ERR_INDEX_RANGE);
                    y = -1;
                }
                if (y >= 0) {
                    float mx = z[0];
                    for (int c = 1; c < C; ++c) mx = fmaxf(mx, z[c]);
                    float se = 0.f;
                    for (int c = 0; c < C; ++c) se += __expf(z[c] - mx);
                    lacc[a * MT_RT + tid] += __logf(se) - (z[y] - mx);
                    for (int c = 0; c < C; ++c) z[c] = (__expf(z[c] - mx) / se - (c == (int)y ? 1.f : 0.f)) / (float)A.B;
                } else {
                    for (int c = 0; c < C; ++c) z[c] = 0.f;
                }
                for (int c = C; c < PB_ZS; ++c) z[c] = 0.f;
            }
            __syncthreads();
            pb_wgrad(zs, PB_ZS, C, in, s_in, n_in, gW2, first, wave, li, h);
            pb_bgrad(zs, PB_ZS, C, gW2 + C * n_in, first, tid);
            if (H) {
                __syncthreads();      // dW2 has read h; dz1 goes over it, every cell by the lane that owns it
                for (int cg = wave; cg * 32 < H; cg += 4) {
                    const int u = cg * 32 + li;
                    const f32x16 acc = pb_chain(C, h, [&](int k) { return zs[li * PB_ZS + k]; }, [&](int k) { return W2.at(k, u); });
                    if (u < H) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            float* cell = hs + mt_row(r, h) * sH + u;
                            *cell = *cell > 0.f ? acc[r] : 0.f;
                        }
                    }
                }
                __syncthreads();
                pb_wgrad(hs, sH, H, xs, sD, D, g, first, wave, li, h);
                pb_bgrad(hs, sH, H, g + H * D, first, tid);
            }
        }
    }
    if (fwd_only) return;
    __syncthreads();
    if (tid < A.n_heads) {
        float l = 0.f;
        for (int r = 0; r < MT_RT; ++r) l = __fadd_rn(l, lacc[tid * MT_RT + r]);
        A.ws_loss[blockIdx.x * A.n_heads + tid] = l;
    }
}

// gradient = the workgroups' slots added in workgroup order; Adam on every parameter; loss[0] = the heads' mean losses added in
// head order, loss[1 + a] = head a's
__global__ __launch_bounds__(256) void probe_apply_kernel(const float* __restrict__ ws_grad, const float* __restrict__ ws_loss,
                                                          const int wgs, const int P, const int n_heads, const int B,
                                                          float* __restrict__ params, float* __restrict__ m,
                                                          float* __restrict__ v, float* __restrict__ grad_out,
                                                          float* __restrict__ loss, const AdamC c, const int step) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < P) {
        float g = ws_grad[i];
        int w = 1;
        for (; w + 8 <= wgs; w += 8) {      // eight loads in flight, added in workgroup order
            float t[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) t[q] = ws_grad[(size_t)(w + q) * P + i];
#pragma unroll
            for (int q = 0; q < 8; ++q) g = __fadd_rn(g, t[q]);
        }
        for (; w < wgs; ++w) g = __fadd_rn(g, ws_grad[(size_t)w * P + i]);
        if (grad_out) grad_out[i] = g;
        const float2 s = step_scalars(c, step);
        float pp = params[i], mm = m[i], vv = v[i];
        LearnerAdam::elem(pp, mm, vv, g, s.x, s.y, c);
        params[i] = pp;
        m[i] = mm;
        v[i] = vv;
    }
    if (i == 0) {
        float total = 0.f;
        for (int a = 0; a < n_heads; ++a) {
            float l = 0.f;
            for (int w = 0; w < wgs; ++w) l = __fadd_rn(l, ws_loss[w * n_heads + a]);
            l = l * (1.f / (float)B);
            loss[1 + a] = l;
            total = __fadd_rn(total, l);
        }
        loss[0] = total;
    }
}

// ---- metrics of the held-out rows --------------------------------------------------------------------------------------------
// One thread per row, the heads in turn: the argmax (the lowest class among equal maxima), the log-loss term and the
// probabilities in double from the float logits.  A block's counts gather in LDS (integer atomics), its log-loss by a fixed
// butterfly; the partials are added in block order by probe_eval_fold_kernel.
struct ProbeEvalK {
    const float* logits;
    const long long* labels;
    const long long* rows;
    float* probs;
    long long* part_cnt;    // [blocks][n_heads + sumC]
    double* part_ll;        // [blocks][n_heads]
    uint32_t* err;
    long long n, ldl, U;
    int n_heads, sumC;
    int C[FR_PROBE_MAX_HEADS], c_off[FR_PROBE_MAX_HEADS];
};

__global__ __launch_bounds__(256) void probe_eval_kernel(const ProbeEvalK A) {
    __shared__ int cnt[FR_PROBE_MAX_HEADS + FR_PROBE_MAX_HEADS * FR_PROBE_MAX_CLASSES];
    __shared__ double red[FR_PROBE_MAX_HEADS][4];
    const int tid = threadIdx.x, n_cnt = A.n_heads + A.sumC;
    for (int e = tid; e < n_cnt; e += 256) cnt[e] = 0;
    __syncthreads();
    const long long b = (long long)blockIdx.x * 256 + tid;
    long long r = -1;
    if (b < A.n) {
        r = A.rows ? A.rows[b] : b;
        if (r < 0 || r >= A.U) {
            atomicOr(A.err, FR_DEV_ERR_INDEX_RANGE);
            r = -1;
        }
    }
    for (int a = 0; a < A.n_heads; ++a) {
        const int C = A.C[a];
        double ll = 0.0;
        if (b < A.n) {
            const float* z = A.logits + b * A.sumC + A.c_off[a];
            float* pr = A.probs + b * A.sumC + A.c_off[a];
            long long y = r >= 0 ? A.labels[a * A.ldl + r] : -1;
            if (r >= 0 && (y < 0 || y >= C)) {
                atomicOr(A.err, FR_DEV_ERR_INDEX_RANGE);
                y = -1;
            }
            float mx = z[0];
            int am = 0;
            for (int c = 1; c < C; ++c)
                if (z[c] > mx) {
                    mx = z[c];
                    am = c;
                }
            double se = 0.0;
            for (int c = 0; c < C; ++c) se += exp((double)z[c] - (double)mx);
            for (int c = 0; c < C; ++c) pr[c] = (float)(exp((double)z[c] - (double)mx) / se);
            if (y >= 0) {
                ll = log(se) - ((double)z[y] - (double)mx);
                atomicAdd(&cnt[A.n_heads + A.c_off[a] + (int)y], 1);
                if (am == (int)y) atomicAdd(&cnt[a], 1);
            }
        }
        ll = wave_sum(ll);
        if ((tid & 63) == 0) red[a][tid >> 6] = ll;
    }
    __syncthreads();
    if (tid < A.n_heads) A.part_ll[(size_t)blockIdx.x * A.n_heads + tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
    for (int e = tid; e < n_cnt; e += 256) A.part_cnt[(size_t)blockIdx.x * n_cnt + e] = cnt[e];
}

__global__ __launch_bounds__(256) void probe_eval_fold_kernel(const long long* __restrict__ part_cnt, const double* __restrict__ part_ll,
                                                              const int blocks, const int n_heads, const int sumC,
                                                              long long* __restrict__ correct, long long* __restrict__ class_count,
                                                              double* __restrict__ logloss) {
    const int e = blockIdx.x * 256 + threadIdx.x, n_cnt = n_heads + sumC;
    if (e < n_cnt) {
        long long s = 0;
        for (int q = 0; q < blocks; ++q) s += part_cnt[(size_t)q * n_cnt + e];
        if (e < n_heads) correct[e] = s;
        else class_count[e - n_heads] = s;
    } else if (e < n_cnt + n_heads) {
        const int a = e - n_cnt;
        double s = 0.0;
        for (int q = 0; q < blocks; ++q) s += part_ll[(size_t)q * n_heads + a];
        logloss[a] = s;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
static int probe_check_shape(const char* who, int D, int H, int n_heads, const int32_t* classes) {
    FR_CHECK_ARG(classes, "%s: classes is null", who);
    if (D < 1 || D > FR_PROBE_MAX_WIDTH) {
        set_error("%s: D = %d not in 1..%d", who, D, FR_PROBE_MAX_WIDTH);
        return FR_EUNSUPPORTED;
    }
    if (H < 0 || H > FR_PROBE_MAX_WIDTH) {
        set_error("%s: H = %d not in 0..%d", who, H, FR_PROBE_MAX_WIDTH);
        return FR_EUNSUPPORTED;
    }
    if (n_heads < 1 || n_heads > FR_PROBE_MAX_HEADS) {
        set_error("%s: n_heads = %d not in 1..%d", who, n_heads, FR_PROBE_MAX_HEADS);
        return FR_EUNSUPPORTED;
    }
    for (int a = 0; a < n_heads; ++a)
        if (classes[a] < 2 || classes[a] > FR_PROBE_MAX_CLASSES) {
            set_error("%s: classes[%d] = %d not in 2..%d", who, a, classes[a], FR_PROBE_MAX_CLASSES);
            return FR_EUNSUPPORTED;
        }
    return FR_OK;
}

static long long probe_head_params(int D, int H, int C) { return H ? (long long)H * D + H + (long long)C * H + C : (long long)C * D + C; }

static long long probe_params(int D, int H, int n_heads, const int32_t* classes) {
    long long P = 0;
    for (int a = 0; a < n_heads; ++a) P += probe_head_params(D, H, classes[a]);
    return P;
}

// validates the argument block and fills the kernel's; `lds`: the dynamic LDS of the launch
static int probe_plan(const char* who, const fr_probe_args* a, ProbeK& K, size_t& lds) {
    FR_CHECK_ARG(a, "%s: args is null", who);
    int rc = probe_check_shape(who, a->D, a->H, a->n_heads, a->classes);
    if (rc) return rc;
    if (a->B < 1 || a->B > FR_PROBE_MAX_BATCH) {
        set_error("%s: B = %lld not in 1..%d", who, (long long)a->B, FR_PROBE_MAX_BATCH);
        return FR_EUNSUPPORTED;
    }
    FR_CHECK_ARG(a->X, "%s: X is null", who);
    FR_CHECK_ARG(a->U >= 1 && a->U <= 0x7fffffffLL, "%s: U = %lld not in 1..2^31-1", who, (long long)a->U);
    FR_CHECK_ARG(a->ldx >= a->D, "%s: ldx = %lld below D = %d", who, (long long)a->ldx, a->D);
    FR_CHECK_ARG(a->rows || a->B <= a->U, "%s: B = %lld contiguous rows of U = %lld (rows is null)", who, (long long)a->B,
                 (long long)a->U);
    const ProbeGrid g = probe_grid(a->B);
    K.X = a->X;
    K.rows = (const long long*)a->rows;
    K.labels = (const long long*)a->labels;
    K.U = a->U;
    K.ldx = a->ldx;
    K.ldl = a->ldl;
    K.B = (int)a->B;
    K.D = a->D;
    K.H = a->H;
    K.n_heads = a->n_heads;
    K.tpw = g.tpw;
    K.tiles = g.tiles;
    const int sD = mt_stride(a->D), sH = mt_stride(a->H), s_in = a->H ? sH : sD;
    int p = 0, c = 0, im = 0;
    for (int h = 0; h < FR_PROBE_MAX_HEADS; ++h) {
        const int C = h < a->n_heads ? a->classes[h] : 0;
        K.C[h] = C;
        K.p_off[h] = p;
        K.c_off[h] = c;
        K.img_off[h] = im;
        if (!C) continue;
        p += (int)probe_head_params(a->D, a->H, C);
        c += C;
        im += (a->H ? a->H * sD : 0) + C * s_in;
    }
    K.P = p;
    K.sumC = c;
    const size_t fixed = ((size_t)MT_RT * sD + (a->H ? (size_t)MT_RT * sH : 0) + MT_RT * PB_ZS + FR_PROBE_MAX_HEADS * MT_RT) * 4 +
                         MT_RT * sizeof(long long);
    K.resident = mt_resident(fixed, (size_t)im);
    lds = fixed + (K.resident ? (size_t)im * 4 : 0);
    return FR_OK;
}

}  // namespace fr

using namespace fr;

extern "C" int fr_probe_supported(int32_t D, int32_t H, int32_t n_heads, const int32_t* classes) {
    return probe_check_shape("fr_probe_supported", D, H, n_heads, classes);
}

extern "C" int64_t fr_probe_param_count(int32_t D, int32_t H, int32_t n_heads, const int32_t* classes) {
    if (probe_check_shape("fr_probe_param_count", D, H, n_heads, classes)) return 0;
    return probe_params(D, H, n_heads, classes);
}

extern "C" int32_t fr_probe_grid(int64_t B) {
    if (B < 1 || B > FR_PROBE_MAX_BATCH) {
        set_error("fr_probe_grid: B = %lld not in 1..%d", (long long)B, FR_PROBE_MAX_BATCH);
        return 0;
    }
    return probe_grid(B).wgs;
}

extern "C" size_t fr_probe_step_workspace_bytes(int32_t D, int32_t H, int32_t n_heads, const int32_t* classes, int64_t B) {
    if (probe_check_shape("fr_probe_step_workspace_bytes", D, H, n_heads, classes) || fr_probe_grid(B) == 0) return 0;
    return (size_t)probe_grid(B).wgs * (size_t)(probe_params(D, H, n_heads, classes) + n_heads) * sizeof(float);
}

extern "C" int fr_probe_step(const fr_probe_args* a, float* params, float* m, float* v, const fr_adam* adam, int32_t step,
                             float* loss, float* grad_out, void* ws, size_t ws_bytes, uint32_t* err_flag, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    ProbeK K{};
    size_t lds = 0;
    int rc = probe_plan("fr_probe_step", a, K, lds);
    if (rc) return rc;
    if ((rc = check_adam(adam, "fr_probe_step"))) return rc;
    FR_CHECK_ARG(adam->learner == FR_LEARNER_ADAM && adam->weight_decay == 0.0,
                 "fr_probe_step: adam must be learner adam with weight_decay 0 (learner %d, weight_decay %g)", adam->learner,
                 adam->weight_decay);
    FR_CHECK_ARG(step >= 1, "fr_probe_step: step = %d below 1", step);
    FR_CHECK_ARG(a->labels, "fr_probe_step: labels is null");
    FR_CHECK_ARG(a->ldl >= (a->rows ? a->U : a->B), "fr_probe_step: ldl = %lld below the label rows of a head", (long long)a->ldl);
    FR_CHECK_ARG(params && m && v, "fr_probe_step: params, m or v is null");
    FR_CHECK_ARG(loss, "fr_probe_step: loss is null");
    FR_CHECK_ARG(err_flag, "fr_probe_step: err_flag is null");
    const size_t need = fr_probe_step_workspace_bytes(a->D, a->H, a->n_heads, a->classes, a->B);
    FR_CHECK_ARG(ws && ws_bytes >= need, "fr_probe_step: ws is null or ws_bytes = %zu below %zu", ws_bytes, need);
    const ProbeGrid g = probe_grid(a->B);
    K.params = params;
    K.ws_grad = (float*)ws;
    K.ws_loss = K.ws_grad + (size_t)g.wgs * K.P;
    K.logits = nullptr;
    K.err = err_flag;
    FR_CHECK_HIP(mt_allow_lds<probe_step_kernel>(lds));
    {
        ProfScope prof(K_PROBE_STEP, stream);
        prof_work(K_PROBE_STEP, 6.0 * (double)a->B * (double)(K.P - (a->H ? a->n_heads * a->H : 0) - K.sumC));
        FR_LAUNCH(prof, probe_step_kernel, dim3(g.wgs), dim3(256), lds, stream, K);
    }
    FR_CHECK_LAUNCH();
    {
        ProfScope prof(K_PROBE_APPLY, stream);
        FR_LAUNCH(prof, probe_apply_kernel, dim3((K.P + 255) / 256), dim3(256), 0, stream, (const float*)K.ws_grad,
                  (const float*)K.ws_loss, g.wgs, K.P, K.n_heads, K.B, params, m, v, grad_out, loss, make_adamc(adam), (int)step);
    }
    FR_CHECK_LAUNCH();
    return FR_OK;
}

extern "C" int fr_probe_forward(const fr_probe_args* a, const float* params, float* logits, uint32_t* err_flag, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    ProbeK K{};
    size_t lds = 0;
    int rc = probe_plan("fr_probe_forward", a, K, lds);
    if (rc) return rc;
    FR_CHECK_ARG(params, "fr_probe_forward: params is null");
    FR_CHECK_ARG(logits, "fr_probe_forward: logits is null");
    FR_CHECK_ARG(err_flag, "fr_probe_forward: err_flag is null");
    K.params = params;
    K.logits = logits;
    K.err = err_flag;
    FR_CHECK_HIP(mt_allow_lds<probe_step_kernel>(lds));
    {
        ProfScope prof(K_PROBE_STEP, stream);
        FR_LAUNCH(prof, probe_step_kernel, dim3(probe_grid(a->B).wgs), dim3(256), lds, stream, K);
    }
    FR_CHECK_LAUNCH();
    return FR_OK;
}

extern "C" size_t fr_probe_eval_workspace_bytes(int64_t n, int32_t n_heads, const int32_t* classes) {
    if (n < 1 || n_heads < 1 || n_heads > FR_PROBE_MAX_HEADS || !classes) return 0;
    long long sumC = 0;
    for (int a = 0; a < n_heads; ++a) sumC += classes[a];
    return (size_t)((n + 255) / 256) * (size_t)(2 * n_heads + sumC) * 8;
}

extern "C" int fr_probe_eval(const float* logits, const int64_t* labels, int64_t ldl, const int64_t* rows, int64_t U, int64_t n,
                             int32_t n_heads, const int32_t* classes, int64_t* correct, double* logloss, int64_t* class_count,
                             float* probs, void* ws, size_t ws_bytes, uint32_t* err_flag, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = probe_check_shape("fr_probe_eval", 1, 0, n_heads, classes);
    if (rc) return rc;
    FR_CHECK_ARG(n >= 1 && n <= 0x7fffffffLL, "fr_probe_eval: n = %lld not in 1..2^31-1", (long long)n);
    FR_CHECK_ARG(U >= 1, "fr_probe_eval: U = %lld below 1", (long long)U);
    FR_CHECK_ARG(rows || n <= U, "fr_probe_eval: n = %lld contiguous rows of U = %lld (rows is null)", (long long)n, (long long)U);
    FR_CHECK_ARG(logits && labels, "fr_probe_eval: logits or labels is null");
    FR_CHECK_ARG(ldl >= (rows ? U : n), "fr_probe_eval: ldl = %lld below the label rows of a head", (long long)ldl);
    FR_CHECK_ARG(correct && logloss && class_count && probs, "fr_probe_eval: correct, logloss, class_count or probs is null");
    FR_CHECK_ARG(err_flag, "fr_probe_eval: err_flag is null");
    const size_t need = fr_probe_eval_workspace_bytes(n, n_heads, classes);
    FR_CHECK_ARG(ws && ws_bytes >= need, "fr_probe_eval: ws is null or ws_bytes = %zu below %zu", ws_bytes, need);
    ProbeEvalK K{};
    const int blocks = (int)((n + 255) / 256);
    int c = 0;
    for (int a = 0; a < n_heads; ++a) {
        K.C[a] = classes[a];
        K.c_off[a] = c;
        c += classes[a];
    }
    K.logits = logits;
    K.labels = (const long long*)labels;
    K.rows = (const long long*)rows;
    K.probs = probs;
    K.part_cnt = (long long*)ws;
    K.part_ll = (double*)(K.part_cnt + (size_t)blocks * (n_heads + c));
    K.err = err_flag;
    K.n = n;
    K.ldl = ldl;
    K.U = U;
    K.n_heads = n_heads;
    K.sumC = c;
    {
        ProfScope prof(K_PROBE_EVAL, stream);
        FR_LAUNCH(prof, probe_eval_kernel, dim3(blocks), dim3(256), 0, stream, K);
    }
    FR_CHECK_LAUNCH();
    hipLaunchKernelGGL(probe_eval_fold_kernel, dim3((2 * n_heads + c + 255) / 256), dim3(256), 0, stream,
                       (const long long*)K.part_cnt, (const double*)K.part_ll, blocks, (int)n_heads, c, (long long*)correct,
                       (long long*)class_count, logloss);
    FR_CHECK_LAUNCH();
    return FR_OK;
}
