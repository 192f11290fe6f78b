// fr_mlp_infer: a whole MLP (Linear -> [BatchNorm1d on RUNNING statistics] -> activation, per layer) evaluated in one launch,
// for rows that stay in LDS between the layers.  Inference only: nothing is kept for a backward pass, there is no workspace
// and no atomic, and no argument but Y is written (the running statistics are read, never advanced).
//
// A workgroup of four waves owns a tile of 32 rows and runs every layer on the tile machine mlp_tile.hpp describes, the
// weights streamed; the column's bias and BatchNorm constants are per-lane scalars there.  A hidden layer writes its
// activations to the other LDS buffer; the last layer goes to Y.  The layer loop is this kernel's own copy of the streamed
// branch of mt_layer (mlp_tile.hpp): built on the template it computed the same bits from near-identical code, and measured
// 1.2 % slower at a million rows.
//
// Row r's arithmetic (include/fairrec_hip.h states it as the contract) involves row r of the tile and the parameters only
// (mlp_tile.hpp has the argument): rows at or beyond M are zeros in LDS and are never stored.
//
// Several nets: each is evaluated in turn on the resident input tile (reloaded only after a net of three or more layers,
// whose second layer overwrote it); the sum is carried in Y itself -- the thread that wrote a cell for net 0 is the one
// that reads it back, adds and rewrites it for net 1, 2, ... -- and the last net's store divides.
#include "common.hpp"
#include "kernels.hpp"
#include "mlp_tile.hpp"

namespace fr {

constexpr int MI_LAYERS = FR_MLP_INFER_MAX_LAYERS * FR_MLP_INFER_MAX_NETS;

struct MlpLayerK {
    const float *W, *bias, *g, *be, *mu, *var;      // g .. var: all null = no BatchNorm
    float eps;
    unsigned short n_out;
    unsigned char act, pad;
};

struct MlpK {
    const float* X;
    float* Y;
    long long M;
    float out_div;
    int n_nets, k_in;
    int s0, s1;                        // row strides (floats) the two activation buffers are sized for
    unsigned char n_layers[FR_MLP_INFER_MAX_NETS];
    MlpLayerK layer[MI_LAYERS];        // layer l of net n at [n * FR_MLP_INFER_MAX_LAYERS + l]
};

// The activations of this entry (the codes of fr_linear_fwd).  relu and leakyrelu keep a NaN; sigmoid is the IEEE quotient
// over expf, tanh is tanhf (OCML).  The two library calls stay out of line: inlined into the 16 cells of the epilogue they
// cost the kernel a workgroup of occupancy.
__device__ __forceinline__ float mi_act_cheap(float x, int act) {
    if (act == 1) return x < 0.f ? 0.f : x;
    if (act == 2) return x < 0.f ? __fmul_rn(0.01f, x) : x;
    return x;
}

__device__ __noinline__ float mi_act_libm(float x, int act) {
    return act == 3 ? __fdiv_rn(1.f, __fadd_rn(1.f, expf(-x))) : tanhf(x);
}

// (two waves per SIMD: two workgroups on a CU, which is also what the LDS of a [128, 256, 128] filter allows)
__global__ __launch_bounds__(256, 2) void mlp_infer_kernel(MlpK a) {
    extern __shared__ __align__(16) float mi_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
    const int li = lane & 31, h = lane >> 5;
    float* buf0 = mi_smem;                                  // [32][s0]: the input tile; outputs of layers 1, 3, 5
    float* buf1 = buf0 + MT_RT * a.s0;                      // [32][s1]: outputs of layers 0, 2, 4, 6
    float* Ws = buf1 + MT_RT * a.s1;                        // [128][MT_WST]
    const long long row0 = (long long)blockIdx.x * MT_RT;
    const int k_in = a.k_in, sx = mt_stride(k_in);

    for (int net = 0; net < a.n_nets; ++net) {
        const int L = a.n_layers[net];
        if (net == 0 || a.n_layers[net - 1] >= 3) {
            __syncthreads();          // the net before has read its last activations
            for (int e = tid; e < MT_RT * sx; e += 256) {
                const int r = e / sx, c = e - r * sx;
                buf0[e] = (c < k_in && row0 + r < a.M) ? a.X[(size_t)(row0 + r) * k_in + c] : 0.f;
            }
        }
        int n_in = k_in;
        for (int l = 0; l < L; ++l) {
            const MlpLayerK& lay = a.layer[net * FR_MLP_INFER_MAX_LAYERS + l];
            const int n_out = lay.n_out, act = lay.act;
            const bool last = l == L - 1, bn = lay.g != nullptr;
            const float* in = (l & 1) ? buf1 : buf0;
            float* out = (l & 1) ? buf0 : buf1;
            const int s_in = mt_stride(n_in), s_out = mt_stride(n_out);
            const float* W = lay.W;
            float pre[16];
            auto fetch = [&](int col0, int c0) {
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int e = tid + 256 * j, col = col0 + (e >> 5), kc = c0 + (e & 31);
                    pre[j] = (col < n_out && kc < n_in) ? W[(size_t)col * n_in + kc] : 0.f;
                }
            };
            fetch(0, 0);
            for (int col0 = 0; col0 < n_out; col0 += MT_CG) {
                const int col = col0 + wave * 32 + li;
                const bool ok = col < n_out;
                // the column's constants: bias, and BatchNorm as y = fmaf(z - mean, sc, beta), sc = gamma * (1 / sqrtf(var + eps))
                const float bias = ok ? lay.bias[col] : 0.f;
                float mu = 0.f, sc = 1.f, be = 0.f;
                if (bn && ok) {
                    mu = lay.mu[col];
                    be = lay.be[col];
                    sc = __fmul_rn(lay.g[col], __fdiv_rn(1.f, __fsqrt_rn(__fadd_rn(lay.var[col], lay.eps))));
                }
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
                for (int c0 = 0; c0 < n_in; c0 += MT_DK) {
                    __syncthreads();      // the image is free; the layer's input is written
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const int e = tid + 256 * j;
                        Ws[(e >> 5) * MT_WST + (e & 31)] = pre[j];
                    }
                    __syncthreads();
                    if (c0 + MT_DK < n_in) fetch(col0, c0 + MT_DK);
                    else if (col0 + MT_CG < n_out) fetch(col0 + MT_CG, 0);
                    if (wave * 32 < n_out - col0) {      // (a wave whose 32 columns lie beyond the layer only stages)
                        const int left = (n_in - c0 + 1) >> 1, steps = left < MT_DK / 2 ? left : MT_DK / 2;
                        const float* xp = in + li * s_in + c0 + h;
                        const float* wp = Ws + (wave * 32 + li) * MT_WST + h;
                        for (int s = 0; s < steps; ++s)
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xp[2 * s], wp[2 * s], acc, 0, 0, 0);
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = mt_row(r, h);
                    float y = __fadd_rn(acc[r], bias);
                    if (bn) y = fmaf(__fsub_rn(y, mu), sc, be);
                    y = act >= 3 ? mi_act_libm(y, act) : mi_act_cheap(y, act);
                    if (!last) {
                        if (ok) out[row * s_out + col] = y;
                    } else if (ok && row0 + row < a.M) {
                        float* yp = a.Y + (size_t)(row0 + row) * n_out + col;
                        if (net > 0) y = __fadd_rn(*yp, y);
                        if (net == a.n_nets - 1) y = __fdiv_rn(y, a.out_div);
                        *yp = y;
                    }
                }
            }
            if (!last && (n_out & 1) && tid < MT_RT) out[tid * s_out + n_out] = 0.f;
            n_in = n_out;
        }
    }
}

static size_t mi_lds_bytes(int s0, int s1) { return ((size_t)MT_RT * (s0 + s1) + (size_t)MT_CG * MT_WST) * sizeof(float); }

}  // namespace fr

using namespace fr;

extern "C" int fr_mlp_infer(const fr_mlp_net* nets, int32_t n_nets, float out_div, const float* X, int64_t M, float* Y,
                            void* stream_) {
    FR_CHECK_ARG(nets, "fr_mlp_infer: nets is null");
    FR_CHECK_ARG(n_nets >= 1 && n_nets <= FR_MLP_INFER_MAX_NETS, "fr_mlp_infer: n_nets %d not in 1..%d", n_nets,
                 FR_MLP_INFER_MAX_NETS);
    FR_CHECK_ARG(X, "fr_mlp_infer: X is null");
    FR_CHECK_ARG(Y, "fr_mlp_infer: Y is null");
    FR_CHECK_ARG(M >= 0 && (M + MT_RT - 1) / MT_RT <= 0x7fffffffLL, "fr_mlp_infer: M %lld out of range", (long long)M);
    FR_CHECK_ARG(out_div != 0.f, "fr_mlp_infer: out_div is 0");
    MlpK p;
    p.X = X;
    p.Y = Y;
    p.M = M;
    p.out_div = out_div;
    p.n_nets = n_nets;
    p.k_in = nets[0].k_in;
    int w0 = 0, w1 = 0, n_last = 0;      // the widest tile each activation buffer holds
    double flop = 0.0;
    for (int n = 0; n < n_nets; ++n) {
        const fr_mlp_net& net = nets[n];
        FR_CHECK_ARG(net.n_layers >= 1 && net.n_layers <= FR_MLP_INFER_MAX_LAYERS, "fr_mlp_infer: nets[%d].n_layers %d not in 1..%d",
                     n, net.n_layers, FR_MLP_INFER_MAX_LAYERS);
        FR_CHECK_ARG(net.k_in >= 1 && net.k_in <= FR_MLP_INFER_MAX_WIDTH, "fr_mlp_infer: nets[%d].k_in %d not in 1..%d", n, net.k_in,
                     FR_MLP_INFER_MAX_WIDTH);
        FR_CHECK_ARG(net.k_in == nets[0].k_in, "fr_mlp_infer: nets[%d].k_in %d differs from nets[0].k_in %d", n, net.k_in,
                     nets[0].k_in);
        p.n_layers[n] = (unsigned char)net.n_layers;
        w0 = net.k_in > w0 ? net.k_in : w0;
        int n_in = net.k_in;
        for (int l = 0; l < net.n_layers; ++l) {
            const fr_mlp_layer& s = net.layer[l];
            FR_CHECK_ARG(s.W && s.bias, "fr_mlp_infer: nets[%d].layer[%d]: W or bias is null", n, l);
            FR_CHECK_ARG(s.n_out >= 1 && s.n_out <= FR_MLP_INFER_MAX_WIDTH, "fr_mlp_infer: nets[%d].layer[%d].n_out %d not in 1..%d",
                         n, l, s.n_out, FR_MLP_INFER_MAX_WIDTH);
            FR_CHECK_ARG(s.act >= 0 && s.act <= 4, "fr_mlp_infer: nets[%d].layer[%d].act %d not in 0..4", n, l, s.act);
            const int n_bn = (s.bn_weight != nullptr) + (s.bn_bias != nullptr) + (s.bn_mean != nullptr) + (s.bn_var != nullptr);
            FR_CHECK_ARG(n_bn == 0 || n_bn == 4,
                         "fr_mlp_infer: nets[%d].layer[%d]: bn_weight, bn_bias, bn_mean, bn_var must be all set or all null", n, l);
            MlpLayerK& d = p.layer[n * FR_MLP_INFER_MAX_LAYERS + l];
            d.W = s.W;
            d.bias = s.bias;
            d.g = s.bn_weight;
            d.be = s.bn_bias;
            d.mu = s.bn_mean;
            d.var = s.bn_var;
            d.eps = s.bn_eps;
            d.n_out = (unsigned short)s.n_out;
            d.act = (unsigned char)s.act;
            d.pad = 0;
            if (l < net.n_layers - 1) {
                int& w = (l & 1) ? w0 : w1;
                w = s.n_out > w ? s.n_out : w;
            }
            flop += 2.0 * (double)M * n_in * s.n_out;
            n_in = s.n_out;
        }
        if (n == 0) n_last = n_in;
        FR_CHECK_ARG(n_in == n_last, "fr_mlp_infer: nets[%d] ends in %d columns, nets[0] in %d", n, n_in, n_last);
    }
    if (M == 0) return FR_OK;
    p.s0 = mt_stride(w0);
    p.s1 = w1 ? mt_stride(w1) : 0;
    const size_t ldsb = mi_lds_bytes(p.s0, p.s1);
    FR_CHECK_HIP(mt_allow_lds<mlp_infer_kernel>(ldsb));
    hipStream_t stream = (hipStream_t)stream_;
    ProfScope prof(K_MLP_INFER, stream);
    prof_work(K_MLP_INFER, flop);
    FR_LAUNCH(prof, mlp_infer_kernel, dim3((unsigned)((M + MT_RT - 1) / MT_RT)), dim3(256), ldsb, stream, p);
    FR_CHECK_LAUNCH();
    return FR_OK;
}
