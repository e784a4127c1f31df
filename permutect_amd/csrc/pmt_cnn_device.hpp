// Device helpers of the workgroup-per-chunk haplotype-CNN kernels, shared by pmt_cnn.hip (eval-mode stack, BatchNorms folded away) and
// pmt_cnn_bn.hip (the same stack with its BatchNorms on batch statistics): one-hot input, tap tables, the implicit-GEMM convolution
// forward and the vector-ALU layers.  Included behind pmt_device.hpp by a translation unit that has chosen its wave shape
// (PMT_WAVES x PMT_RT).
#pragma once
#include "pmt_device.hpp"

#define CNN_NTIN (PMT_MAX_CNN_TAPS / 16)
#define LEAKY_SLOPE 0.01f

// a / b for 0 <= a < 2^22 without the ~35-instruction integer division sequence (inv_b = 1.0f / b)
DEV int fast_div(int a, int b, float inv_b) {
    int q = (int)((float)a * inv_b);
    if (q * b > a) --q;
    if ((q + 1) * b <= a) ++q;
    return q;
}

DEV float act_fwd(int kind, float x) {
    if (kind == PMT_CNN_LEAKY_RELU) return x > 0.f ? x : LEAKY_SLOPE * x;
    return x > 0.f ? PMT_SELU_SCALE * x : (PMT_SELU_ALPHA * PMT_SELU_SCALE) * expm1f(x);
}
DEV float act_bwd(int kind, float x_in, float y_out) {  // d(out)/d(in)
    if (kind == PMT_CNN_LEAKY_RELU) return x_in > 0.f ? 1.f : LEAKY_SLOPE;
    return x_in > 0.f ? PMT_SELU_SCALE : y_out + PMT_SELU_ALPHA * PMT_SELU_SCALE;
}

// one-hot input of variant v: channel 2*base + (0 ref | 1 alt), position s  (reference data/batch.py:115-130)
DEV void build_one_hot(float* __restrict__ dst, int dst_stride, const long long* __restrict__ hap, int seq_len, int nv,
                       long long hap_stride, int v0) {
    const int per = 10 * seq_len;
    const float inv_len = 1.0f / (float)seq_len;
    for (int v = 0; v < nv; ++v)
        for (int rem = threadIdx.x; rem < per; rem += PMT_THREADS) {
            const int c = fast_div(rem, seq_len, inv_len), s = rem - c * seq_len;
            const long long base = hap[(size_t)(v0 + v) * hap_stride + (c & 1) * seq_len + s];
            dst[v * dst_stride + rem] = (base == (c >> 1)) ? 1.f : 0.f;
        }
}

// per-layer tap table: for im2col feature f = ci * kernel + k :  tap[f] = (ci * in_len) | ((k * dilation - padding + 64) << 16)
DEV void build_taps(int* __restrict__ tap, const PmtCnnLayer& L) {
    const int K = L.in_ch * L.kernel;
    for (int f = threadIdx.x; f < PMT_MAX_CNN_TAPS; f += PMT_THREADS) {
        int v = -1;
        if (f < K) {
            const int ci = f / L.kernel, k = f - ci * L.kernel;
            v = (ci * L.in_len) | ((k * L.dilation - L.padding + 64) << 16);
        }
        tap[f] = v;
    }
}

struct ColMeta {
    int v, so;     // variant within the block, output position
    bool valid;
};
DEV ColMeta col_meta(int tile, int ncol, int out_len) {
    ColMeta m;
    const int col = tile * 16 + (threadIdx.x & 15);
    m.valid = col < ncol;
    m.v = m.valid ? fast_div(col, out_len, 1.0f / (float)out_len) : 0;
    m.so = m.valid ? col - m.v * out_len : 0;
    return m;
}

// im2col columns of this wave's tiles, in the B-operand register layout: x[rt][t][j] = tap feat_of(t, j, g) of column r
DEV void gather_im2col(f4 (&x)[PMT_RT][CNN_NTIN], const float* __restrict__ in, int in_stride, const int* __restrict__ tap,
                       const PmtCnnLayer& L, const ColMeta (&cm)[PMT_RT], int g) {
    const int nkt = (L.in_ch * L.kernel + 15) >> 4;
#pragma unroll
    for (int t = 0; t < CNN_NTIN; ++t) {
        if (t < nkt) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int tp = tap[feat_of(t, j, g)];
                const int base = tp & 0xFFFF, ks = (tp >> 16) - 64;
#pragma unroll
                for (int rt = 0; rt < PMT_RT; ++rt) {
                    const int s = cm[rt].so * L.stride + ks;
                    const bool ok = cm[rt].valid && tp >= 0 && s >= 0 && s < L.in_len;
                    x[rt][t][j] = ok ? in[cm[rt].v * in_stride + base + s] : 0.f;
                }
            }
        } else {
#pragma unroll
            for (int rt = 0; rt < PMT_RT; ++rt) x[rt][t] = f4{0.f, 0.f, 0.f, 0.f};
        }
    }
}

// convolution forward for nv variants (LDS -> LDS) on the matrix cores.
// BIAS_LAST (with `theta`): the products are summed from zero and the bias (theta + L.b_src) is added once, at the end, instead of
// being the accumulator they are summed onto.  The matrix core aligns the products of a step to its largest addend and cuts them
// there: onto a bias far larger than the products every product loses its low bits TOWARDS ZERO, which shrinks the signal
// systematically (bias 100, signal 0.1: the variance of the output 4e-5 short) -- what a BatchNorm behind the convolution divides by.
template <bool BIAS_LAST = false>
DEV void conv_forward(const PmtModel* __restrict__ M, const PmtCnnLayer& L, const float* __restrict__ packed,
                      const float* __restrict__ in, int in_stride, float* __restrict__ out, int out_stride, int nv,
                      const int* __restrict__ tap, const float* __restrict__ theta = nullptr) {
    const int lane = threadIdx.x & 63, g = lane >> 4, wave = uniform((int)(threadIdx.x >> 6));
    const PmtLinear& W = M->lin[uniform(L.lin)];
    const int K = uniform(W.in_dim), OC = uniform(W.out_dim), out_len = uniform(L.out_len);
    const int ncol = nv * out_len, ntiles = (ncol + 15) >> 4;
    for (int tile0 = 0; tile0 < ntiles; tile0 += PMT_WAVES * PMT_RT) {
        ColMeta cm[PMT_RT];
#pragma unroll
        for (int rt = 0; rt < PMT_RT; ++rt) cm[rt] = col_meta(tile0 + wave * PMT_RT + rt, ncol, out_len);
        if (tile0 + wave * PMT_RT < ntiles) {  // wave-uniform
            f4 x[PMT_RT][CNN_NTIN], y[PMT_RT][PMT_NT];
            gather_im2col(x, in, in_stride, tap, L, cm, g);
            init_bias<PMT_NT>(y, BIAS_LAST ? nullptr : packed + uniform(W.b_pvec), OC, g);
            linear_acc<CNN_NTIN, PMT_NT, false>(y, x, packed + uniform(W.w_frag), K, OC);
#pragma unroll
            for (int rt = 0; rt < PMT_RT; ++rt)
                if (cm[rt].valid) {
#pragma unroll
                    for (int t = 0; t < PMT_NT; ++t)
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int co = feat_of(t, j, g);
                            if (co < OC) out[cm[rt].v * out_stride + co * out_len + cm[rt].so] = BIAS_LAST ? y[rt][t][j] + theta[L.b_src + co] : y[rt][t][j];
                        }
                }
        }
    }
}

// the vector-ALU layers (LDS -> LDS)
DEV void small_layer_forward(const PmtCnnLayer& L, const float* __restrict__ theta, const float* __restrict__ in,
                             float* __restrict__ out, int nv, int in_stride, int out_stride) {
    const int kind = L.kind;
    if (kind == PMT_CNN_POOL) {
        const int per = L.out_ch * L.out_len;
        const float inv_len = 1.0f / (float)L.out_len;
        for (int v = 0; v < nv; ++v)
            for (int rem = threadIdx.x; rem < per; rem += PMT_THREADS) {
                const int c = fast_div(rem, L.out_len, inv_len), so = rem - c * L.out_len;
                float m = -INFINITY;
                for (int k = 0; k < L.kernel; ++k) {
                    const int s = so * L.stride + k;
                    if (s < L.in_len) m = fmaxf(m, in[v * in_stride + c * L.in_len + s]);
                }
                out[v * out_stride + rem] = m;
            }
    } else if (kind == PMT_CNN_LEAKY_RELU || kind == PMT_CNN_SELU) {
        const int per = L.out_ch * L.out_len;
        for (int v = 0; v < nv; ++v)
            for (int rem = threadIdx.x; rem < per; rem += PMT_THREADS) out[v * out_stride + rem] = act_fwd(kind, in[v * in_stride + rem]);
    } else if (kind == PMT_CNN_LINEAR) {
        // out[v][o] = b[o] + W[o][:] . in[v][:] : the 16 lanes of a lane-group split the dot product, coalesced weight reads
        const float* W = theta + L.w_src;
        const float* b = theta + L.b_src;
        const int nin = L.in_ch * L.in_len;
        const int sub = threadIdx.x & 15, slot = threadIdx.x >> 4, nslots = PMT_THREADS >> 4;
        const float inv_oc = 1.0f / (float)L.out_ch;
        for (int i = slot; i < nv * L.out_ch; i += nslots) {
            const int v = fast_div(i, L.out_ch, inv_oc), o = i - v * L.out_ch;
            float acc = 0.f;
            for (int k = sub; k < nin; k += 16) acc += W[(size_t)o * nin + k] * in[v * in_stride + k];
            acc += __shfl_xor(acc, 1);
            acc += __shfl_xor(acc, 2);
            acc += __shfl_xor(acc, 4);
            acc += __shfl_xor(acc, 8);
            if (sub == 0) out[v * out_stride + o] = acc + b[o];
        }
    }
}

// host: variants per workgroup (at most 16) whose LDS-resident floats fit beside the kernel's static LDS with blocks_per_cu workgroups per CU
static inline int cnn_pick_vpb(size_t floats_per_variant, size_t static_bytes, int blocks_per_cu) {
    const size_t lds = 156 * 1024 / blocks_per_cu;
    if (lds <= static_bytes) return 0;
    const size_t budget = (lds - static_bytes) / sizeof(float);
    int vpb = (int)(budget / floats_per_variant);
    if (vpb > 16) vpb = 16;
    return vpb;
}
