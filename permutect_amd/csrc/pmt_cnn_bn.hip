// The haplotype CNN with its `batch_norm` tokens on BATCH statistics (reference architecture/dna_sequence_convolution.py:82-83 in train
// mode: torch.nn.BatchNorm1d, eps 1e-5, affine), forward and backward: pmt_cnn_bn_forward / pmt_cnn_bn_backward.
//
// The kernels are the workgroup-per-chunk family of pmt_cnn.hip (same helpers, pmt_cnn_device.hpp; same wave shape) walking a TRAINING
// descriptor, a PmtCnn whose PMT_CNN_BATCHNORM layers are kept.  A BatchNorm needs the mean and variance of its channel over the WHOLE
// batch, and those of BatchNorm k depend on the statistics of every BatchNorm in front of it.  No workgroup can wait for all others
// (no cooperative launch, no grid barrier), so the dependency is carried by the stream: with K BatchNorms at layers b_0 < ... < b_{K-1}
//
//   forward :  for k = 0 .. K-1 :  statistics pass  -- every workgroup walks layers 0 .. b_k - 1 of its variants (BatchNorms in front
//                                  of b_k are per-channel affine maps by now) and stores, per channel, the mean of its values and
//                                  their M2 (sum of squares about THAT mean), two passes over the LDS-resident activation;
//                                  fold             -- one workgroup per channel merges the partials in fp64, every thread a fixed
//                                  set of them and a fixed tree on top:  mean = sum n_i m_i / N,  M2 = sum [M2_i + n_i (m_i - mean)^2];
//                                  stores mean, rstd = 1 / sqrt(M2 / N + eps), unbiased variance M2 / (N - 1)
//              then the full pass, which writes `out`;
//   backward:  for k = K-1 .. 0 :  sums pass        -- recomputes the forward, walks back from d(out) to layer b_k WITHOUT emitting weight
//                                  gradients (BatchNorms behind b_k have their sums already) and stores per-channel partials of
//                                  sum dy and sum dy xhat;  fold -- c1 = sum dy / N, c2 = sum dy xhat / N, and d(bias) += sum dy,
//                                  d(weight) += sum dy xhat
//              then the full pass: a BatchNorm propagates dx = weight rstd (dy - c1 - xhat c2); weight gradients as in pmt_cnn.hip.
//
// 2 K + 1 launches each way (the backward: a fill and a fold's two launches more -- its full pass sums the weight gradients in private rows per workgroup,
// folded in workgroup order), no float atomics anywhere in the statistics nor between workgroups: the same bits on every call.  Every pass recomputes
// what is in front of it; a stash for these kernels is follow-up work.
//
// The STEPPED form (pmt_cnn_bn_forward_moments / _backward_moments, pmt_cnn_bn_merge, pmt_cnn_bn_forward_full / _backward_full) is the same
// computation cut where a caller's collective goes, for statistics over the union of several ranks' batches: the pass and fold of ONE
// BatchNorm stop at this rank's fp64 moments (count, sum, M2 about its own mean | count, sum dy, sum dy xhat), the caller gathers every
// rank's, and pmt_hapbn_merge_kernel finishes them in rank order -- 3 K + 1 launches each way; one rank gives the bits of the one call.
#define PMT_OWN_WAVE_SHAPE
#define PMT_WAVES 4
#define PMT_RT 2
#define PMT_STAGE_PLANES 32  // as pmt_cnn.hip
#include <stdlib.h>
#include <string.h>

#include "pmt_device.hpp"
#include "pmt_bwd_device.hpp"
#include "pmt_cnn_device.hpp"

#define BN_FOLD_THREADS 256

// y = (x - mean) rstd weight + bias per channel (LDS -> LDS; in == out is allowed)
DEV void bn_forward(const PmtCnnLayer& L, const float* __restrict__ theta, const float* __restrict__ st, const float* in, float* out,
                    int nv, int in_stride, int out_stride) {
    const int C = L.in_ch, len = L.in_len, per = C * len;
    const float* w = theta + L.w_src;
    const float* b = theta + L.b_src;
    const float inv_len = 1.0f / (float)len;
    for (int rem = threadIdx.x; rem < per; rem += PMT_THREADS) {
        const int c = fast_div(rem, len, inv_len);
        const float mean = st[c], scale = st[C + c] * w[c], shift = b[c];
        for (int v = 0; v < nv; ++v) out[v * out_stride + rem] = (in[v * in_stride + rem] - mean) * scale + shift;
    }
}

DEV float sum16(float v) {  // over the 16 lanes of a lane group
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    return v;
}

// per channel: (mean of this workgroup's nv * len values, their M2 about that mean) -> part[(c * nblocks + block) * 2 + {0, 1}].
// A lane group of 16 takes a channel; two passes over LDS, so the M2 is as exact as fp32 sums of <= 336 squares are.
DEV void bn_partial_stats(const PmtCnnLayer& L, const float* __restrict__ a, int stride, int nv, float* __restrict__ part, int nblocks) {
    const int C = L.in_ch, len = L.in_len, cnt = nv * len;
    const int sub = threadIdx.x & 15, slot = threadIdx.x >> 4, nslots = PMT_THREADS >> 4;
    const float inv_len = 1.0f / (float)len;
    for (int c = slot; c < C; c += nslots) {
        float s = 0.f;
        for (int i = sub; i < cnt; i += 16) {
            const int v = fast_div(i, len, inv_len), p = i - v * len;
            s += a[v * stride + c * len + p];
        }
        const float mean = sum16(s) / (float)cnt;
        float m2 = 0.f;
        for (int i = sub; i < cnt; i += 16) {
            const int v = fast_div(i, len, inv_len), p = i - v * len;
            const float d = a[v * stride + c * len + p] - mean;
            m2 += d * d;
        }
        m2 = sum16(m2);
        if (sub == 0) {
            float* dst = part + ((size_t)c * nblocks + blockIdx.x) * 2;
            dst[0] = mean;
            dst[1] = m2;
        }
    }
}

// per channel: (sum dy, sum dy xhat) of this workgroup's values, xhat = (x - mean) rstd; same destination layout
DEV void bn_partial_sums(const PmtCnnLayer& L, const float* __restrict__ st, const float* __restrict__ x, int x_stride,
                         const float* __restrict__ dy, int dy_stride, int nv, float* __restrict__ part, int nblocks) {
    const int C = L.in_ch, len = L.in_len, cnt = nv * len;
    const int sub = threadIdx.x & 15, slot = threadIdx.x >> 4, nslots = PMT_THREADS >> 4;
    const float inv_len = 1.0f / (float)len;
    for (int c = slot; c < C; c += nslots) {
        const float mean = st[c], rstd = st[C + c];
        float s1 = 0.f, s2 = 0.f;
        for (int i = sub; i < cnt; i += 16) {
            const int v = fast_div(i, len, inv_len), p = i - v * len;
            const float g = dy[v * dy_stride + c * len + p];
            s1 += g;
            s2 += g * ((x[v * x_stride + c * len + p] - mean) * rstd);
        }
        s1 = sum16(s1);
        s2 = sum16(s2);
        if (sub == 0) {
            float* dst = part + ((size_t)c * nblocks + blockIdx.x) * 2;
            dst[0] = s1;
            dst[1] = s2;
        }
    }
}

DEV double fold_sum(double v, double* sh) {  // a fixed tree over the workgroup; every thread gets the total
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = BN_FOLD_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}

// One workgroup per channel.  Workgroup i of the pass that wrote `part` held min(vpb, n - i * vpb) variants = that many * len values.
// backward == 0: (mean_i, M2_i) -> st[c] = mean, st[C + c] = rstd, st[2 C + c] = unbiased variance
// backward == 1: (sum dy, sum dy xhat) -> st[3 C + c] = c1, st[4 C + c] = c2;  gtheta[b_src + c] += sum dy, gtheta[w_src + c] += sum dy xhat
// (this launch is alone on its stream position and owns channel c: plain adds)
// mom != nullptr (the stepped form): nothing is finished -- the fold's three fp64 numbers of this channel go to mom[k * C + c], k = 0 the
// count N, 1 the sum (forward sum n_i m_i, backward sum dy), 2 forward the M2 about sum / N, backward sum dy xhat: what
// pmt_hapbn_merge_kernel takes from every rank.  st and gtheta are not touched then.
extern "C" __global__ __launch_bounds__(BN_FOLD_THREADS) void pmt_hapbn_fold_kernel(
    const float* __restrict__ part, int nblocks, int vpb, int n, int len, int C, float* __restrict__ st, int backward,
    float* __restrict__ gtheta, int w_src, int b_src, double* __restrict__ mom) {
    __shared__ double sh[BN_FOLD_THREADS];
    const int c = blockIdx.x;
    const float* p = part + (size_t)c * nblocks * 2;
    const double N = (double)n * (double)len;
    if (!backward) {
        double acc = 0.0;
        for (int i = threadIdx.x; i < nblocks; i += BN_FOLD_THREADS)
            acc += (double)(min(vpb, n - i * vpb) * len) * (double)p[2 * i];
        const double sum = fold_sum(acc, sh);
        const double mean = sum / N;
        acc = 0.0;
        for (int i = threadIdx.x; i < nblocks; i += BN_FOLD_THREADS) {
            const double d = (double)p[2 * i] - mean;
            acc += (double)p[2 * i + 1] + (double)(min(vpb, n - i * vpb) * len) * d * d;
        }
        const double m2 = fold_sum(acc, sh);
        if (mom) {
            if (threadIdx.x == 0) {
                mom[c] = N;
                mom[C + c] = sum;
                mom[2 * C + c] = m2;
            }
        } else if (threadIdx.x == 0) {
            st[c] = (float)mean;
            st[C + c] = (float)(1.0 / sqrt(m2 / N + (double)PMT_CNN_BN_EPS));
            st[2 * C + c] = (float)(m2 / (N - 1.0));
        }
    } else {
        double a1 = 0.0, a2 = 0.0;
        for (int i = threadIdx.x; i < nblocks; i += BN_FOLD_THREADS) {
            a1 += (double)p[2 * i];
            a2 += (double)p[2 * i + 1];
        }
        a1 = fold_sum(a1, sh);
        a2 = fold_sum(a2, sh);
        if (mom) {
            if (threadIdx.x == 0) {
                mom[c] = N;
                mom[C + c] = a1;
                mom[2 * C + c] = a2;
            }
        } else if (threadIdx.x == 0) {
            st[3 * C + c] = (float)(a1 / N);
            st[4 * C + c] = (float)(a2 / N);
            gtheta[b_src + c] += (float)a1;
            gtheta[w_src + c] += (float)a2;
        }
    }
}

// The moments of `ranks` ranks (mom[(r * 3 + k) * C + c], written by pmt_hapbn_fold_kernel on each and gathered by the caller) -> the
// statistics of their union.  A thread per channel walks the ranks in order: fp64, no atomics, the same bits wherever it runs.  The sums
// start from rank 0's numbers, not from 0.0, so that one rank gives exactly the one-call fold: mean = sum / N is its expression, and
// sum_0 / cnt_0 - mean is exactly 0.  A rank without values (cnt = 0) has no mean and contributes nothing.
// backward == 1: only rank `self`'s own sums go into gtheta (the gradient all-reduce adds the other ranks' later).
extern "C" __global__ __launch_bounds__(BN_FOLD_THREADS) void pmt_hapbn_merge_kernel(
    const double* __restrict__ mom, int ranks, int self, int C, float* __restrict__ st, int backward, float* __restrict__ gtheta,
    int w_src, int b_src) {
    const int c = blockIdx.x * BN_FOLD_THREADS + threadIdx.x;
    if (c >= C) return;
    double N = mom[c], s1 = mom[C + c], s2 = mom[2 * C + c];
    for (int r = 1; r < ranks; ++r) {
        const double* m = mom + (size_t)r * 3 * C;
        N += m[c];
        s1 += m[C + c];
        if (backward) s2 += m[2 * C + c];
    }
    if (!backward) {
        const double mean = s1 / N;
        double m2 = 0.0;
        bool first = true;
        for (int r = 0; r < ranks; ++r) {
            const double* m = mom + (size_t)r * 3 * C;
            const double cnt = m[c];
            if (cnt > 0.0) {
                const double d = m[C + c] / cnt - mean;
                const double term = m[2 * C + c] + cnt * d * d;
                m2 = first ? term : m2 + term;
                first = false;
            }
        }
        st[c] = (float)mean;
        st[C + c] = (float)(1.0 / sqrt(m2 / N + (double)PMT_CNN_BN_EPS));
        st[2 * C + c] = (float)(m2 / (N - 1.0));
    } else {
        const double* own = mom + (size_t)self * 3 * C;
        st[3 * C + c] = (float)(s1 / N);
        st[4 * C + c] = (float)(s2 / N);
        gtheta[b_src + c] += (float)own[C + c];
        gtheta[w_src + c] += (float)own[2 * C + c];
    }
}

// The private rows of the backward's full pass -> gtheta[lo + i] += their sum, a thread per parameter, in an order that depends on the
// number of rows alone: two launches of this kernel.  First every chunk of BN_WGRAD_CHUNK consecutive rows (blockIdx.y) is summed in row
// order into its first row (dst == nullptr; at vpb = 2 a batch of 65 536 variants has 32 768 rows: one thread walking them all takes
// 10 ms), then the chunks' first rows (row_step = the chunk) are summed in order and added to the gradient.
#define BN_WGRAD_CHUNK 64
extern "C" __global__ __launch_bounds__(BN_FOLD_THREADS) void pmt_hapbn_wgrad_fold_kernel(
    float* __restrict__ priv, int nrows, int row_step, int span, float* __restrict__ dst) {
    const int i = blockIdx.x * BN_FOLD_THREADS + threadIdx.x;
    if (i >= span) return;
    const int r0 = dst ? 0 : blockIdx.y * BN_WGRAD_CHUNK, r1 = dst ? nrows : min(r0 + BN_WGRAD_CHUNK, nrows);
    float acc = 0.f;
    for (int r = r0; r < r1; r += row_step) acc += priv[(size_t)r * span + i];
    if (dst) dst[i] += acc;
    else priv[(size_t)r0 * span + i] = acc;  // (this thread alone reads and writes column i of its chunk)
}

struct BnFwdShared {
    int tap[PMT_MAX_CNN_TAPS];
};

// Layers 0 .. stop - 1 of the training descriptor `C`.  stop == n_layers: the full pass, writes `out`; stop < n_layers: layer `stop` is
// a BatchNorm without statistics yet, and the pass writes this workgroup's partial statistics of its input.
extern "C" __global__ __launch_bounds__(PMT_THREADS, 2) void pmt_hapbn_forward_kernel(
    const PmtModel* __restrict__ M, const PmtCnn* __restrict__ Cp, const float* __restrict__ theta, const float* __restrict__ packed,
    const long long* __restrict__ hap, long long hap_stride, int n, int vpb, int stop, const float* __restrict__ stats,
    float* __restrict__ part, float* __restrict__ out, long long out_stride) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ BnFwdShared sh;
    const PmtCnn& C = *Cp;
    const int v0 = blockIdx.x * vpb;
    const int nv = min(vpb, n - v0);
    const int ma = uniform(C.max_act);
    float* a = lds;
    float* b = lds + (size_t)vpb * ma;
    build_one_hot(a, ma, hap, uniform(C.seq_len), nv, hap_stride, v0);
    __syncthreads();
    const int nl = uniform(C.n_layers);
    for (int l = 0; l < stop; ++l) {
        const PmtCnnLayer& L = C.layers[l];
        const int kind = uniform(L.kind);
        if (kind == PMT_CNN_FLATTEN) continue;
        if (kind == PMT_CNN_CONV) {
            build_taps(sh.tap, L);
            __syncthreads();
            conv_forward<true>(M, L, packed, a, ma, b, ma, nv, sh.tap, theta);  // bias last: a BatchNorm may follow
        } else if (kind == PMT_CNN_LEAKY_RELU || kind == PMT_CNN_SELU) {
            small_layer_forward(L, theta, a, a, nv, ma, ma);
            __syncthreads();
            continue;
        } else if (kind == PMT_CNN_BATCHNORM) {
            bn_forward(L, theta, stats + uniform(L.reserved[0]), a, a, nv, ma, ma);
            __syncthreads();
            continue;
        } else {
            small_layer_forward(L, theta, a, b, nv, ma, ma);
        }
        __syncthreads();
        float* t = a; a = b; b = t;
    }
    if (stop < nl) {
        bn_partial_stats(C.layers[stop], a, ma, nv, part, gridDim.x);
        return;
    }
    const int od = uniform(C.out_dim);
    for (int i = threadIdx.x; i < nv * od; i += PMT_THREADS) {
        const int v = i / od, o = i - v * od;
        out[(size_t)(v0 + v) * out_stride + o] = a[v * ma + o];
    }
}

struct BnBwdShared {
    int tap[PMT_MAX_CNN_TAPS];
    float aux[PMT_WAVES][PMT_AUX_CAP];
    int aux_dst[PMT_AUX_CAP];
    f4 stage[PMT_STAGE_PLANES * 64];
};

// Backward over the training descriptor; LDS as pmt_cnn_backward_kernel (every layer output, stride sum_act, plus two gradient buffers).
// stop < 0: the full pass -- every layer, weight gradients emitted (into `priv`, below), a BatchNorm propagates with its c1 / c2.
// stop >= 0: layer `stop` is a BatchNorm whose sums are wanted: walks back to it without emitting anything and writes the partials.
extern "C" __global__ __launch_bounds__(PMT_THREADS, 2) void pmt_hapbn_backward_kernel(
    const PmtModel* __restrict__ M, const PmtCnn* __restrict__ Cp, const float* __restrict__ theta, const float* __restrict__ packed,
    const long long* __restrict__ hap, long long hap_stride, int n, int vpb, int stop, const float* __restrict__ stats,
    float* __restrict__ part, const float* __restrict__ d_out, long long d_out_stride, float* gtheta, float* __restrict__ priv, int priv_lo,
    int priv_span) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ __attribute__((aligned(16))) BnBwdShared sh;
    // the full pass: this workgroup's weight / bias gradients go to a zeroed row of its own, [priv_lo, priv_lo + priv_span) of the flat
    // buffer, where every address has ONE writer (a wave owns its blocks of a weight gradient, a thread its elements of the linear's) adding
    // in program order; pmt_hapbn_wgrad_fold_kernel sums the rows in workgroup order.  No float atomic meets another: the same bits on every call.
    if (priv) gtheta = priv + (size_t)blockIdx.x * priv_span - priv_lo;
    const PmtCnn& C = *Cp;
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, wave = uniform((int)(tid >> 6));
    const int v0 = blockIdx.x * vpb;
    const int nv = min(vpb, n - v0);
    const int ma = uniform(C.max_act), sa = uniform(C.sum_act), nl = uniform(C.n_layers);
    const bool emit = stop < 0;
    float* acts = lds;
    float* g0 = lds + (size_t)vpb * sa;
    float* g1 = g0 + (size_t)vpb * ma;
    // ---- recompute the forward, keeping everything ----
    build_one_hot(acts, sa, hap, uniform(C.seq_len), nv, hap_stride, v0);
    __syncthreads();
    for (int l = 0; l < nl; ++l) {
        const PmtCnnLayer& L = C.layers[l];
        const int kind = uniform(L.kind);
        if (kind == PMT_CNN_FLATTEN) continue;
        if (kind == PMT_CNN_CONV) {
            build_taps(sh.tap, L);
            __syncthreads();
            conv_forward<true>(M, L, packed, acts + uniform(L.in_off), sa, acts + uniform(L.out_off), sa, nv, sh.tap, theta);
        } else if (kind == PMT_CNN_BATCHNORM) {
            bn_forward(L, theta, stats + uniform(L.reserved[0]), acts + uniform(L.in_off), acts + uniform(L.out_off), nv, sa, sa);
        } else {
            small_layer_forward(L, theta, acts + uniform(L.in_off), acts + uniform(L.out_off), nv, sa, sa);
        }
        __syncthreads();
    }
    // ---- d(out) -> g0 ----
    const int od = uniform(C.out_dim);
    for (int i = tid; i < nv * od; i += PMT_THREADS) {
        const int v = i / od, o = i - v * od;
        g0[v * ma + o] = d_out[(size_t)(v0 + v) * d_out_stride + o];
    }
    __syncthreads();
    BwdCtx c{M, theta, theta, packed, gtheta, gtheta, &sh.stage[0], &sh.aux[0][0], &sh.aux_dst[0], g, 0u,
             wave * PMT_RT, 0, 0, 0, 0, nullptr};
    float* gout = g0;
    float* gin = g1;
    for (int l = nl - 1; l > stop; --l) {
        const PmtCnnLayer& L = C.layers[l];
        const int kind = uniform(L.kind);
        if (kind == PMT_CNN_FLATTEN) continue;
        const float* xin = acts + uniform(L.in_off);
        const float* yout = acts + uniform(L.out_off);
        const int nin = uniform(L.in_ch) * uniform(L.in_len), nout = uniform(L.out_ch) * uniform(L.out_len);
        const bool need_din = uniform(L.in_off) != 0;  // the one-hot input needs no gradient
        if (kind == PMT_CNN_LEAKY_RELU || kind == PMT_CNN_SELU) {
            for (int v = 0; v < nv; ++v)
                for (int rem = tid; rem < nout; rem += PMT_THREADS)
                    gin[v * ma + rem] = gout[v * ma + rem] * act_bwd(kind, xin[v * sa + rem], yout[v * sa + rem]);
        } else if (kind == PMT_CNN_BATCHNORM) {
            // dx = weight rstd (dy - c1 - xhat c2)
            const float* st = stats + uniform(L.reserved[0]);
            const float* w = theta + L.w_src;
            const int nc = uniform(L.in_ch), len = uniform(L.in_len);
            const float inv_len = 1.0f / (float)len;
            for (int rem = tid; rem < nin; rem += PMT_THREADS) {
                const int ch = fast_div(rem, len, inv_len);
                const float mean = st[ch], rstd = st[nc + ch], c1 = st[3 * nc + ch], c2 = st[4 * nc + ch], k = w[ch] * rstd;
                for (int v = 0; v < nv; ++v)
                    gin[v * ma + rem] = k * (gout[v * ma + rem] - c1 - (xin[v * sa + rem] - mean) * rstd * c2);
            }
        } else if (kind == PMT_CNN_POOL) {
            for (int v = 0; v < nv; ++v)
                for (int rem = tid; rem < nin; rem += PMT_THREADS) gin[v * ma + rem] = 0.f;
            __syncthreads();
            const float inv_len = 1.0f / (float)L.out_len;
            for (int i = tid; i < nv * nout; i += PMT_THREADS) {
                const int v = fast_div(i, nout, 1.0f / (float)nout), rem = i - v * nout, ch = fast_div(rem, L.out_len, inv_len), so = rem - ch * L.out_len;
                int arg = so * L.stride;
                float m = -INFINITY;
                for (int k = 0; k < L.kernel; ++k) {  // first maximum wins, like ATen's max_pool backward
                    const int s = so * L.stride + k;
                    if (s < L.in_len) {
                        const float val = xin[v * sa + ch * L.in_len + s];
                        if (val > m) { m = val; arg = s; }
                    }
                }
                float* dst = &gin[v * ma + ch * L.in_len + arg];
                if (L.stride >= L.kernel) *dst = gout[v * ma + rem];  // disjoint windows: one writer per input element
                else atomicAdd(dst, gout[v * ma + rem]);
            }
        } else if (kind == PMT_CNN_LINEAR) {
            const float* W = theta + L.w_src;
            if (emit) {
                for (int o = 0; o < L.out_ch; ++o)  // dW[o][k] += sum_v dout[v][o] x[v][k]
                    for (int k = tid; k < nin; k += PMT_THREADS) {
                        float acc = 0.f;
                        for (int v = 0; v < nv; ++v) acc += gout[v * ma + o] * xin[v * sa + k];
                        atomicAdd(&gtheta[L.w_src + o * nin + k], acc);
                    }
                for (int o = tid; o < L.out_ch; o += PMT_THREADS) {
                    float acc = 0.f;
                    for (int v = 0; v < nv; ++v) acc += gout[v * ma + o];
                    atomicAdd(&gtheta[L.b_src + o], acc);
                }
            }
            if (need_din)
                for (int v = 0; v < nv; ++v)
                    for (int k = tid; k < nin; k += PMT_THREADS) {
                        float acc = 0.f;
                        for (int o = 0; o < L.out_ch; ++o) acc += W[(size_t)o * nin + k] * gout[v * ma + o];
                        gin[v * ma + k] = acc;
                    }
        } else if (kind == PMT_CNN_CONV) {
            const PmtLinear& Wl = M->lin[uniform(L.lin)];
            const int K = uniform(Wl.in_dim), OC = uniform(Wl.out_dim), out_len = uniform(L.out_len);
            const int ncol = nv * out_len, ntiles = (ncol + 15) >> 4;
            build_taps(sh.tap, L);
            if (need_din)
                for (int v = 0; v < nv; ++v)
                    for (int rem = tid; rem < nin; rem += PMT_THREADS) gin[v * ma + rem] = 0.f;
            __syncthreads();
            if (emit || need_din)  // (kernel-uniform)
                for (int tile0 = 0; tile0 < ntiles; tile0 += PMT_WAVES * PMT_RT) {
                    ColMeta cm[PMT_RT];
                    unsigned present = 0;
#pragma unroll
                    for (int rt = 0; rt < PMT_RT; ++rt) {
                        cm[rt] = col_meta(tile0 + wave * PMT_RT + rt, ncol, out_len);
                        if (tile0 + wave * PMT_RT + rt < ntiles) present |= 1u << rt;
                    }
                    f4 dy[PMT_RT][PMT_NT];
#pragma unroll
                    for (int rt = 0; rt < PMT_RT; ++rt)
#pragma unroll
                        for (int t = 0; t < PMT_NT; ++t)
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const int co = feat_of(t, j, g);
                                dy[rt][t][j] = (cm[rt].valid && co < OC) ? gout[cm[rt].v * ma + co * out_len + cm[rt].so] : 0.f;
                            }
                    if (emit) {
                        f4 x[PMT_RT][CNN_NTIN];
                        gather_im2col(x, xin, sa, sh.tap, L, cm, g);
                        c.mask_all = present;
                        c.ntiles = c.tiles_ref = min(PMT_WG_TILES, ntiles - tile0);
                        linear_wgrad<PMT_NT, CNN_NTIN>(c, Wl, dy, x);  // workgroup barriers inside
                    }
                    if (need_din) {
                        f4 dx[PMT_RT][CNN_NTIN];
                        init_bias<CNN_NTIN>(dx, nullptr, K, g);
                        linear_acc<PMT_NT, CNN_NTIN, false>(dx, dy, packed + uniform(Wl.wt_frag), OC, K);
                        const int nkt = (K + 15) >> 4;
#pragma unroll
                        for (int t = 0; t < CNN_NTIN; ++t)
                            if (t < nkt) {
#pragma unroll
                                for (int j = 0; j < 4; ++j) {
                                    const int tp = sh.tap[feat_of(t, j, g)];
                                    const int base = tp & 0xFFFF, ks = (tp >> 16) - 64;
#pragma unroll
                                    for (int rt = 0; rt < PMT_RT; ++rt) {
                                        const int s = cm[rt].so * L.stride + ks;
                                        if (cm[rt].valid && tp >= 0 && s >= 0 && s < L.in_len)
                                            atomicAdd(&gin[cm[rt].v * ma + base + s], dx[rt][t][j]);  // col2im
                                    }
                                }
                            }
                    }
                }
        }
        __syncthreads();
        float* t = gout; gout = gin; gin = t;
    }
    if (stop >= 0) {
        const PmtCnnLayer& L = C.layers[stop];
        bn_partial_sums(L, stats + uniform(L.reserved[0]), acts + uniform(L.in_off), sa, gout, ma, nv, part, gridDim.x);
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
static int bn_check(const PmtModel* m, const PmtCnn* c) {
    if (!m || !c) return PMT_E_INVALID;
    if (c->n_layers < 1 || c->n_layers > PMT_MAX_CNN_LAYERS || c->seq_len < 1 || c->max_act < 10 * c->seq_len || c->sum_act < c->max_act ||
        c->reserved[0] < 0)
        return PMT_E_INVALID;
    int last = 10 * c->seq_len;
    for (int l = 0; l < c->n_layers; ++l) {
        const PmtCnnLayer* L = &c->layers[l];
        if (L->kind < 0 || L->kind > PMT_CNN_BATCHNORM) return PMT_E_UNSUPPORTED;
        if (L->in_ch < 1 || L->in_len < 1 || L->out_ch < 1 || L->out_len < 1) return PMT_E_INVALID;
        const int nin = L->in_ch * L->in_len, nout = L->out_ch * L->out_len;
        // every region inside the per-variant activation record, every activation inside a gradient buffer
        if (nin != last || nin > c->max_act || nout > c->max_act || L->in_off < 0 || L->out_off < 0 || L->in_off + nin > c->sum_act ||
            L->out_off + nout > c->sum_act)
            return PMT_E_INVALID;
        last = nout;
        if (L->kind == PMT_CNN_POOL && (L->padding != 0 || L->dilation != 1 || L->kernel < 1 || L->stride < 1 || L->out_ch != L->in_ch ||
                                        (L->out_len - 1) * L->stride >= L->in_len))
            return PMT_E_UNSUPPORTED;
        if ((L->kind == PMT_CNN_LEAKY_RELU || L->kind == PMT_CNN_SELU || L->kind == PMT_CNN_FLATTEN) && nin != nout) return PMT_E_INVALID;
        if (L->kind == PMT_CNN_LINEAR || L->kind == PMT_CNN_BATCHNORM) {
            const long long nw = L->kind == PMT_CNN_LINEAR ? (long long)nin * nout : L->in_ch, nb = L->kind == PMT_CNN_LINEAR ? nout : L->in_ch;
            if (L->w_src < 0 || L->b_src < 0 || L->w_src + nw > m->theta_size || L->b_src + nb > m->theta_size) return PMT_E_INVALID;
        }
        if (L->kind == PMT_CNN_LINEAR && (L->in_len != 1 || L->out_len != 1)) return PMT_E_INVALID;
        if (L->kind == PMT_CNN_BATCHNORM) {
            if (L->in_ch != L->out_ch || L->in_len != L->out_len || L->out_off == L->in_off) return PMT_E_INVALID;
            if (L->reserved[0] < 0 || L->reserved[0] + PMT_CNN_BN_STATS * L->in_ch > c->reserved[0]) return PMT_E_INVALID;
        }
        if (L->kind == PMT_CNN_CONV) {
            if (L->lin < 0 || L->lin >= m->n_linear) return PMT_E_INVALID;
            const PmtLinear* w = &m->lin[L->lin];
            if (w->in_dim != L->in_ch * L->kernel || w->out_dim != L->out_ch || w->b_pvec < 0) return PMT_E_INVALID;
            if (L->b_src < 0 || L->b_src + L->out_ch > m->theta_size) return PMT_E_INVALID;  // (the forward adds the bias from theta, last)
            // (the backward's private gradient rows span the LAYER's offsets: they must be where the PmtLinear's gradients go)
            if (L->w_src < 0 || L->w_src != w->w_src || L->b_src != w->b_src || (long long)L->w_src + (long long)w->in_dim * w->out_dim > m->theta_size)
                return PMT_E_INVALID;
            if (w->in_dim > PMT_MAX_CNN_TAPS || w->out_dim > PMT_MAX_WIDTH) return PMT_E_UNSUPPORTED;
            if (L->in_ch * L->in_len >= 65536 || L->kernel * L->dilation >= 64 || L->padding >= 64 || L->stride < 1) return PMT_E_UNSUPPORTED;
        }
    }
    if (last != c->out_dim) return PMT_E_INVALID;
    return PMT_OK;
}

static int bn_fwd_vpb(const PmtCnn* c) { return cnn_pick_vpb(2 * (size_t)c->max_act, sizeof(BnFwdShared), 2); }
static int bn_bwd_vpb(const PmtCnn* c) { return cnn_pick_vpb((size_t)c->sum_act + 2 * (size_t)c->max_act, sizeof(BnBwdShared), 2); }

static size_t bn_part_floats(const PmtCnn* c, int n, int vpb) {  // the widest BatchNorm's partials of one pass
    int maxc = 0;
    for (int l = 0; l < c->n_layers; ++l)
        if (c->layers[l].kind == PMT_CNN_BATCHNORM && c->layers[l].in_ch > maxc) maxc = c->layers[l].in_ch;
    return 2 * (size_t)maxc * (size_t)((n + vpb - 1) / vpb);
}

// [lo, hi) of the flat buffer: the weights and biases of the convolutions and the linear, what the backward's full pass adds gradients to
static void bn_wgrad_span(const PmtCnn* c, int* lo, int* hi) {
    *lo = INT32_MAX;
    *hi = 0;
    for (int l = 0; l < c->n_layers; ++l) {
        const PmtCnnLayer* L = &c->layers[l];
        if (L->kind != PMT_CNN_CONV && L->kind != PMT_CNN_LINEAR) continue;
        const int nw = L->kind == PMT_CNN_CONV ? L->in_ch * L->kernel * L->out_ch : L->in_ch * L->in_len * L->out_ch * L->out_len;
        const int nb = L->kind == PMT_CNN_CONV ? L->out_ch : L->out_ch * L->out_len;
        if (L->w_src < *lo) *lo = L->w_src;
        if (L->b_src < *lo) *lo = L->b_src;
        if (L->w_src + nw > *hi) *hi = L->w_src + nw;
        if (L->b_src + nb > *hi) *hi = L->b_src + nb;
    }
    if (*hi <= *lo) *lo = *hi = 0;
}

static size_t bn_priv_floats(const PmtCnn* c, int n, int vpb) {  // a row of the span per workgroup of the backward's full pass
    int lo, hi;
    bn_wgrad_span(c, &lo, &hi);
    return (size_t)(hi - lo) * (size_t)((n + vpb - 1) / vpb);
}

extern "C" size_t pmt_cnn_bn_workspace_floats(const PmtCnn* c, int32_t n) {
    if (!c || n < 1) return 0;
    const int vf = bn_fwd_vpb(c), vb = bn_bwd_vpb(c);
    if (vf < 1 || vb < 1) return 0;
    const size_t a = bn_part_floats(c, n, vf), b = bn_part_floats(c, n, vb), p = bn_priv_floats(c, n, vb);
    return a > b ? (a > p ? a : p) : (b > p ? b : p);
}

static int bn_common_check(const PmtModel* mh, const PmtCnn* c, int32_t n) {
    const int rc = bn_check(mh, c);
    if (rc) return rc;
    if (n < 0) return PMT_E_INVALID;
    for (int l = 0; l < c->n_layers && n > 0; ++l)  // a single value per channel has no variance (torch: ValueError)
        if (c->layers[l].kind == PMT_CNN_BATCHNORM && (long long)n * c->layers[l].in_len < 2) return PMT_E_INVALID;
    return PMT_OK;
}

static int bn_fold(const PmtCnnLayer* L, const float* part, int nblocks, int vpb, int n, float* stats, int backward, float* gtheta,
                   double* moments, hipStream_t s) {
    hipLaunchKernelGGL(pmt_hapbn_fold_kernel, dim3(L->in_ch), dim3(BN_FOLD_THREADS), 0, s, part, nblocks, vpb, (int)n, (int)L->in_len,
                       (int)L->in_ch, stats ? stats + L->reserved[0] : nullptr, backward, gtheta, (int)L->w_src, (int)L->b_src, moments);
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}

// One launch of pmt_hapbn_forward_kernel / pmt_hapbn_backward_kernel: up to layer `stop` (a BatchNorm: partials into `part`) or the full pass
struct BnPass {
    const PmtModel* model_dev;
    const PmtCnn *cnn_host, *cnn_dev;
    const float *theta, *packed;
    const int64_t* hap;
    int64_t hap_stride;
    int n, vpb;
    hipStream_t s;
    int nblocks() const { return (n + vpb - 1) / vpb; }
};

static int bn_forward_pass(const BnPass& p, int stop, const float* stats, float* part, float* out, int64_t out_stride) {
    const size_t lds = (size_t)p.vpb * 2 * p.cnn_host->max_act * sizeof(float);
    hipLaunchKernelGGL(pmt_hapbn_forward_kernel, dim3(p.nblocks()), dim3(PMT_THREADS), lds, p.s, p.model_dev, p.cnn_dev, p.theta, p.packed,
                       (const long long*)p.hap, (long long)p.hap_stride, p.n, p.vpb, stop, stats, part, out, (long long)out_stride);
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}

static int bn_backward_pass(const BnPass& p, int stop, const float* stats, float* part, const float* d_out, int64_t d_out_stride,
                            float* gtheta, float* priv = nullptr, int priv_lo = 0, int priv_span = 0) {
    const size_t lds = (size_t)p.vpb * ((size_t)p.cnn_host->sum_act + 2 * (size_t)p.cnn_host->max_act) * sizeof(float);
    hipLaunchKernelGGL(pmt_hapbn_backward_kernel, dim3(p.nblocks()), dim3(PMT_THREADS), lds, p.s, p.model_dev, p.cnn_dev, p.theta, p.packed,
                       (const long long*)p.hap, (long long)p.hap_stride, p.n, p.vpb, stop, stats, part, d_out, (long long)d_out_stride, gtheta,
                       priv, priv_lo, priv_span);
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}

// The backward's full pass: the workspace (the partials in it are spent by now) becomes a zeroed private gradient row per workgroup,
// folded into grad_theta in workgroup order.  A fill, the pass, the fold's two launches.
static int bn_backward_full_pass(const BnPass& p, const float* stats, const float* d_out, int64_t d_out_stride, float* gtheta, float* workspace,
                                 size_t workspace_floats) {
    int lo, hi;
    bn_wgrad_span(p.cnn_host, &lo, &hi);
    const int span = hi - lo;
    if (span <= 0) return bn_backward_pass(p, -1, stats, nullptr, d_out, d_out_stride, gtheta);  // (no layer with weights: nothing is emitted)
    const size_t need = (size_t)span * (size_t)p.nblocks();
    if (!workspace || workspace_floats < need) return PMT_E_WORKSPACE;
    if (hipMemsetAsync(workspace, 0, need * sizeof(float), p.s) != hipSuccess) return PMT_E_LAUNCH;
    const int rc = bn_backward_pass(p, -1, stats, nullptr, d_out, d_out_stride, gtheta, workspace, lo, span);
    if (rc) return rc;
    const int cols = (span + BN_FOLD_THREADS - 1) / BN_FOLD_THREADS, chunks = (p.nblocks() + BN_WGRAD_CHUNK - 1) / BN_WGRAD_CHUNK;
    hipLaunchKernelGGL(pmt_hapbn_wgrad_fold_kernel, dim3(cols, chunks), dim3(BN_FOLD_THREADS), 0, p.s, workspace, p.nblocks(), 1, span,
                       (float*)nullptr);
    if (hipGetLastError() != hipSuccess) return PMT_E_LAUNCH;
    hipLaunchKernelGGL(pmt_hapbn_wgrad_fold_kernel, dim3(cols), dim3(BN_FOLD_THREADS), 0, p.s, workspace, p.nblocks(), BN_WGRAD_CHUNK, span,
                       gtheta + lo);
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}

// the arguments every entry point shares; `backward` picks the chunk size; with `need_ws` the partials of the widest BatchNorm must fit
static int bn_pass_init(BnPass* p, int backward, const PmtModel* model_dev, const PmtCnn* cnn_host, const PmtCnn* cnn_dev, const float* theta,
                        const float* packed, const int64_t* hap, int64_t hap_stride, int32_t n, bool need_ws, const float* workspace,
                        size_t workspace_floats, void* stream) {
    if (!model_dev || !cnn_dev || !theta || !packed || !hap) return PMT_E_INVALID;
    const int vpb = backward ? bn_bwd_vpb(cnn_host) : bn_fwd_vpb(cnn_host);
    if (vpb < 1) return PMT_E_UNSUPPORTED;
    const size_t need = need_ws ? bn_part_floats(cnn_host, n, vpb) : 0;
    if (need > 0 && (!workspace || workspace_floats < need)) return PMT_E_WORKSPACE;
    *p = BnPass{model_dev, cnn_host, cnn_dev, theta, packed, hap, hap_stride, (int)n, vpb, reinterpret_cast<hipStream_t>(stream)};
    return PMT_OK;
}

extern "C" int pmt_cnn_bn_forward(const PmtModel* model_host, const PmtModel* model_dev, const PmtCnn* cnn_host, const PmtCnn* cnn_dev,
                                  const float* theta, const float* packed, const int64_t* haplotypes, int64_t hap_stride, int32_t n,
                                  float* out, int64_t out_stride, float* stats, float* workspace, size_t workspace_floats, void* stream) {
    int rc = bn_common_check(model_host, cnn_host, n);
    if (rc) return rc;
    if (n == 0) return PMT_OK;
    if (!out || !stats) return PMT_E_INVALID;
    BnPass p;
    if ((rc = bn_pass_init(&p, 0, model_dev, cnn_host, cnn_dev, theta, packed, haplotypes, hap_stride, n, true, workspace, workspace_floats, stream)))
        return rc;
    for (int l = 0; l <= cnn_host->n_layers; ++l) {
        if (l < cnn_host->n_layers && cnn_host->layers[l].kind != PMT_CNN_BATCHNORM) continue;
        if ((rc = bn_forward_pass(p, l, stats, workspace, out, out_stride))) return rc;
        if (l < cnn_host->n_layers && (rc = bn_fold(&cnn_host->layers[l], workspace, p.nblocks(), p.vpb, n, stats, 0, nullptr, nullptr, p.s)))
            return rc;
    }
    return PMT_OK;
}

extern "C" int pmt_cnn_bn_backward(const PmtModel* model_host, const PmtModel* model_dev, const PmtCnn* cnn_host, const PmtCnn* cnn_dev,
                                   const float* theta, const float* packed, const int64_t* haplotypes, int64_t hap_stride, int32_t n,
                                   const float* d_out, int64_t d_out_stride, float* stats, float* grad_theta, float* workspace,
                                   size_t workspace_floats, void* stream) {
    int rc = bn_common_check(model_host, cnn_host, n);
    if (rc) return rc;
    if (n == 0) return PMT_OK;
    if (!d_out || !stats || !grad_theta) return PMT_E_INVALID;
    BnPass p;
    if ((rc = bn_pass_init(&p, 1, model_dev, cnn_host, cnn_dev, theta, packed, haplotypes, hap_stride, n, true, workspace, workspace_floats, stream)))
        return rc;
    if (workspace_floats < bn_priv_floats(cnn_host, n, p.vpb)) return PMT_E_WORKSPACE;
    for (int l = cnn_host->n_layers - 1; l >= 0; --l) {
        if (cnn_host->layers[l].kind != PMT_CNN_BATCHNORM) continue;
        if ((rc = bn_backward_pass(p, l, stats, workspace, d_out, d_out_stride, grad_theta))) return rc;
        if ((rc = bn_fold(&cnn_host->layers[l], workspace, p.nblocks(), p.vpb, n, stats, 1, grad_theta, nullptr, p.s))) return rc;
    }
    return bn_backward_full_pass(p, stats, d_out, d_out_stride, grad_theta, workspace, workspace_floats);
}

// ---- the stepped form: the caller's exchange of moments goes between these calls (include/permutect_amd.h) -------------------------------
static int bn_step_check(const PmtModel* mh, const PmtCnn* c, int32_t n, int32_t layer) {  // layer < 0: a full pass, no layer to name
    const int rc = bn_check(mh, c);
    if (rc) return rc;
    if (n < 1) return PMT_E_INVALID;
    if (layer >= 0 && (layer >= c->n_layers || c->layers[layer].kind != PMT_CNN_BATCHNORM)) return PMT_E_INVALID;
    return PMT_OK;
}

extern "C" int pmt_cnn_bn_forward_moments(const PmtModel* model_host, const PmtModel* model_dev, const PmtCnn* cnn_host, const PmtCnn* cnn_dev,
                                          const float* theta, const float* packed, const int64_t* haplotypes, int64_t hap_stride, int32_t n,
                                          int32_t layer, const float* stats, double* moments, float* workspace, size_t workspace_floats,
                                          void* stream) {
    int rc = layer < 0 ? PMT_E_INVALID : bn_step_check(model_host, cnn_host, n, layer);
    if (rc) return rc;
    if (!stats || !moments) return PMT_E_INVALID;
    BnPass p;
    if ((rc = bn_pass_init(&p, 0, model_dev, cnn_host, cnn_dev, theta, packed, haplotypes, hap_stride, n, true, workspace, workspace_floats, stream)))
        return rc;
    if ((rc = bn_forward_pass(p, layer, stats, workspace, nullptr, 0))) return rc;
    return bn_fold(&cnn_host->layers[layer], workspace, p.nblocks(), p.vpb, n, nullptr, 0, nullptr, moments, p.s);
}

extern "C" int pmt_cnn_bn_backward_moments(const PmtModel* model_host, const PmtModel* model_dev, const PmtCnn* cnn_host, const PmtCnn* cnn_dev,
                                           const float* theta, const float* packed, const int64_t* haplotypes, int64_t hap_stride, int32_t n,
                                           int32_t layer, const float* d_out, int64_t d_out_stride, const float* stats, double* moments,
                                           float* workspace, size_t workspace_floats, void* stream) {
    int rc = layer < 0 ? PMT_E_INVALID : bn_step_check(model_host, cnn_host, n, layer);
    if (rc) return rc;
    if (!d_out || !stats || !moments) return PMT_E_INVALID;
    BnPass p;
    if ((rc = bn_pass_init(&p, 1, model_dev, cnn_host, cnn_dev, theta, packed, haplotypes, hap_stride, n, true, workspace, workspace_floats, stream)))
        return rc;
    if ((rc = bn_backward_pass(p, layer, stats, workspace, d_out, d_out_stride, nullptr))) return rc;  // (a sums pass emits no gradient)
    return bn_fold(&cnn_host->layers[layer], workspace, p.nblocks(), p.vpb, n, nullptr, 1, nullptr, moments, p.s);
}

extern "C" int pmt_cnn_bn_merge(const PmtModel* model_host, const PmtCnn* cnn_host, int32_t layer, int32_t n, const double* moments,
                                int32_t ranks, int32_t rank, int32_t backward, float* stats, float* grad_theta, void* stream) {
    const int rc = layer < 0 ? PMT_E_INVALID : bn_step_check(model_host, cnn_host, n, layer);
    if (rc) return rc;
    const PmtCnnLayer* L = &cnn_host->layers[layer];
    if (ranks < 1 || rank < 0 || rank >= ranks || !moments || !stats || (backward && !grad_theta)) return PMT_E_INVALID;
    if (ranks == 1 && (long long)n * L->in_len < 2) return PMT_E_INVALID;  // a single value per channel has no variance (torch: ValueError)
    hipLaunchKernelGGL(pmt_hapbn_merge_kernel, dim3((L->in_ch + BN_FOLD_THREADS - 1) / BN_FOLD_THREADS), dim3(BN_FOLD_THREADS), 0,
                       reinterpret_cast<hipStream_t>(stream), moments, (int)ranks, (int)rank, (int)L->in_ch, stats + L->reserved[0],
                       backward ? 1 : 0, grad_theta, (int)L->w_src, (int)L->b_src);
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}

extern "C" int pmt_cnn_bn_forward_full(const PmtModel* model_host, const PmtModel* model_dev, const PmtCnn* cnn_host, const PmtCnn* cnn_dev,
                                       const float* theta, const float* packed, const int64_t* haplotypes, int64_t hap_stride, int32_t n,
                                       float* out, int64_t out_stride, const float* stats, void* stream) {
    int rc = bn_step_check(model_host, cnn_host, n, -1);
    if (rc) return rc;
    if (!out || !stats) return PMT_E_INVALID;
    BnPass p;
    if ((rc = bn_pass_init(&p, 0, model_dev, cnn_host, cnn_dev, theta, packed, haplotypes, hap_stride, n, false, nullptr, 0, stream))) return rc;
    return bn_forward_pass(p, cnn_host->n_layers, stats, nullptr, out, out_stride);
}

extern "C" int pmt_cnn_bn_backward_full(const PmtModel* model_host, const PmtModel* model_dev, const PmtCnn* cnn_host, const PmtCnn* cnn_dev,
                                        const float* theta, const float* packed, const int64_t* haplotypes, int64_t hap_stride, int32_t n,
                                        const float* d_out, int64_t d_out_stride, const float* stats, float* grad_theta, float* workspace,
                                        size_t workspace_floats, void* stream) {
    int rc = bn_step_check(model_host, cnn_host, n, -1);
    if (rc) return rc;
    if (!d_out || !stats || !grad_theta) return PMT_E_INVALID;
    BnPass p;
    if ((rc = bn_pass_init(&p, 1, model_dev, cnn_host, cnn_dev, theta, packed, haplotypes, hap_stride, n, false, nullptr, 0, stream))) return rc;
    return bn_backward_full_pass(p, stats, d_out, d_out_stride, grad_theta, workspace, workspace_floats);
}
