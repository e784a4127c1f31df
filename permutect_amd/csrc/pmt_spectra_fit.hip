// The fit of the artifact allele-fraction spectra (reference permutect/architecture/spectra/artifact_spectra.py:58-75, `ArtifactSpectra.fit`;
// this package's torch form: architecture/artifact_spectra.py) as ONE persistent launch (include/permutect_amd.h: pmt_spectra_fit).
//
// A step's loss is minus the mean over its minibatch of log BetaBinomial(k | n, alpha[cell], beta[cell]) with cell = (depth bin, variant
// type) of the row, and Adam is element-wise, so every one of the 3 x 5 cells is its own problem of two unknowns (log alpha, log beta)
// over the same minibatch schedule.  One wavefront (= one workgroup) per cell runs all epochs * ceil(n / batch_size) steps; per step
//
//   lane j takes rows j, j + 64, ... of the batch; rows outside the wave's cell are masked (a chunk without any row of the cell
//   skips the digammas altogether: a wave-uniform branch)
//   A = sum_rows psi(k + alpha) - psi(n + alpha + beta)        B = sum_rows psi(n - k + beta) - psi(n + alpha + beta)       (per lane,
//   c = number of rows of the cell                              then over the wave: four DPP stages inside a row of 16 lanes, the four
//                                                               row sums read back with v_readlane and added in a fixed order)
//   d/d(log alpha) = -(alpha / len) (A + c (psi(alpha + beta) - psi(alpha)))
//   d/d(log beta)  = -(beta  / len) (B + c (psi(alpha + beta) - psi(beta)))                 (the three cell-level digammas: once per step)
//   torch.optim.Adam's update of the two raw parameters, every lane the same numbers.
//
// The lgamma terms of the likelihood are never evaluated: nobody reads the loss.  A cell without rows in a batch has c = 0 and exactly
// zero gradients: Adam's update is 0 / (0 + eps), so a cell without data keeps its starting bits.
//
// The schedule does not depend on the parameters: the rows of the NEXT chunk (of this batch, of the next batch, of the next epoch's
// first batch) are requested before the digammas of the current one, so the loads' latency hides behind the dependent chain.  Each
// input is read once per epoch per cell (15 waves read the same 12 n bytes: L2 hits).  No LDS, no barrier, no atomics, nothing between
// workgroups.  Adam's two bias corrections depend on the step number alone: lane j computes those of step t0 + j + 1 in double
// precision (pow) once every 64 steps and a step reads its pair from its lane (v_readlane), so no running fp32 product.
//
// digamma in fp32: the recurrence psi(x) = psi(x + 1) - 1 / x up to x >= 6 (at most six times), then the asymptotic series
// ln x - 1/(2x) - 1/(12x^2) + 1/(120x^4) - 1/(252x^6) + 1/(240x^8), whose first omitted term is 1/(132 x^10) < 1.3e-10 there.
//
// A launch is a chain of dependent steps of a few hundred instructions: bound by instruction LATENCY of one wave (logf, divisions, the
// cross-lane sums), not by any throughput of the device.  The figure of merit is microseconds per step (DESIGN.md section 4,
// profiles/spectra_fit_device.txt).
#include <hip/hip_runtime.h>
#include <math.h>

#include "permutect_amd.h"

#define SF_D 3  // depth bins: (depth >= 10) + (depth >= 20)
#define SF_V 5  // variant types
#define SF_SHIFT 6.0f

struct SpectraHyper {
    float one_m_beta1;  // Adam: m += (1 - beta1) (g - m)
    float beta2, one_m_beta2, eps;
    double lr, beta1, beta2_d;  // for the bias corrections
};

template <int CTRL>
__device__ __forceinline__ float sf_dpp(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float sf_lane(float x, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), lane)); }
// sum over the 64 lanes, the same bits in every lane and in every run
__device__ __forceinline__ float sf_sum64(float x) {
    x += sf_dpp<0xB1>(x);   // quad_perm [1 0 3 2]
    x += sf_dpp<0x4E>(x);   // quad_perm [2 3 0 1]
    x += sf_dpp<0x141>(x);  // row_half_mirror: the other quad of the eight
    x += sf_dpp<0x140>(x);  // row_mirror: the other eight of the sixteen
    return (sf_lane(x, 0) + sf_lane(x, 16)) + (sf_lane(x, 32) + sf_lane(x, 48));
}

// x > 0 (NaN in, NaN out; the loop is bounded whatever x is)
__device__ __forceinline__ float sf_digamma(float x) {
    float s = 0.f;
    for (int i = 0; i < 6 && x < SF_SHIFT; ++i) {
        s += 1.0f / x;
        x += 1.0f;
    }
    const float r = 1.0f / x, r2 = r * r;
    const float tail = r2 * (8.3333333e-2f - r2 * (8.3333333e-3f - r2 * (3.9682540e-3f - r2 * 4.1666667e-3f)));
    return ((logf(x) - 0.5f * r) - tail) - s;
}

__device__ __forceinline__ void sf_adam(float& p, float& m, float& v, float g, const SpectraHyper& h, float step_size, float bc2_sqrt) {
    m += h.one_m_beta1 * (g - m);
    v = h.beta2 * v + h.one_m_beta2 * g * g;
    p -= step_size * (m / (sqrtf(v) / bc2_sqrt + h.eps));
}

struct SfRow {
    int type, depth, alt;  // type -1: no row
};
__device__ __forceinline__ SfRow sf_load(const int32_t* __restrict__ types, const int32_t* __restrict__ depths, const int32_t* __restrict__ alts,
                                         long long first, long long count, int lane) {
    SfRow r = {-1, 0, 0};
    if (lane < count) {  // first + count <= n
        r.type = types[first + lane];
        r.depth = depths[first + lane];
        r.alt = alts[first + lane];
    }
    return r;
}

__global__ __launch_bounds__(64) void pmt_spectra_fit_kernel(const int32_t* __restrict__ types, const int32_t* __restrict__ depths, const int32_t* __restrict__ alts,
                                                             int n, float* __restrict__ log_alpha, float* __restrict__ log_beta, int batch_size, int epochs,
                                                             SpectraHyper hy) {
    const int cell = blockIdx.x, lane = threadIdx.x;
    const int my_bin = cell / SF_V, my_type = cell % SF_V;
    const long long n_rows = n, bs = batch_size;
    const long long num_batches = (n_rows + bs - 1) / bs;

    float la = log_alpha[cell], lb = log_beta[cell];
    float m_a = 0.f, m_b = 0.f, v_a = 0.f, v_b = 0.f;
    float step_size = 0.f, bc2_sqrt = 1.f;  // of step (t & ~63) + lane + 1
    long long t = 0;

    SfRow next = sf_load(types, depths, alts, 0, bs < n_rows ? bs : n_rows, lane);
    for (int epoch = 0; epoch < epochs; ++epoch) {
        for (long long b = 0; b < num_batches; ++b, ++t) {
            const long long start = b * bs;
            const long long len = n_rows - start < bs ? n_rows - start : bs;
            const float alpha = expf(la), beta = expf(lb), ab = alpha + beta;

            float sum_a = 0.f, sum_b = 0.f, cnt = 0.f;
            for (long long off = 0; off < len; off += 64) {
                const SfRow row = next;
                // the next chunk: of this batch, else of the next batch, else of the next epoch's first batch (after the last step: loaded, unused)
                long long nfirst, ncount;
                if (off + 64 < len) {
                    nfirst = start + off + 64;
                    ncount = len - off - 64;
                } else {
                    nfirst = b + 1 < num_batches ? start + bs : 0;
                    ncount = n_rows - nfirst < bs ? n_rows - nfirst : bs;
                }
                next = sf_load(types, depths, alts, nfirst, ncount, lane);

                const int bin = (row.depth >= 10) + (row.depth >= 20);
                if (row.type == my_type && bin == my_bin) {
                    const float k = (float)row.alt, nn = (float)row.depth;
                    const float dn = sf_digamma(nn + ab);
                    sum_a += sf_digamma(k + alpha) - dn;
                    sum_b += sf_digamma(nn - k + beta) - dn;
                    cnt += 1.0f;
                }
            }
            const float c = sf_sum64(cnt);
            float g_a = 0.f, g_b = 0.f;  // a batch without a row of this cell: zero gradients, as autograd gives
            if (c > 0.f) {
                const float dab = sf_digamma(ab);
                const float inv_len = 1.0f / (float)len;
                g_a = -(alpha * inv_len) * (sf_sum64(sum_a) + c * (dab - sf_digamma(alpha)));
                g_b = -(beta * inv_len) * (sf_sum64(sum_b) + c * (dab - sf_digamma(beta)));
            }

            if ((t & 63) == 0) {
                const double step = (double)(t + lane + 1);
                step_size = (float)(hy.lr / (1.0 - pow(hy.beta1, step)));
                bc2_sqrt = (float)sqrt(1.0 - pow(hy.beta2_d, step));
            }
            const float ss = sf_lane(step_size, (int)(t & 63));
            const float bq = sf_lane(bc2_sqrt, (int)(t & 63));
            sf_adam(la, m_a, v_a, g_a, hy, ss, bq);
            sf_adam(lb, m_b, v_b, g_b, hy, ss, bq);
        }
    }
    if (lane == 0) {
        log_alpha[cell] = la;
        log_beta[cell] = lb;
    }
}

extern "C" int pmt_spectra_fit(const int32_t* variant_types, const int32_t* depths, const int32_t* alt_counts, int32_t n, float* log_alpha_dv,
                               float* log_beta_dv, int32_t batch_size, int32_t epochs, double lr, double beta1, double beta2, double eps,
                               void* stream) {
    if (!variant_types || !depths || !alt_counts || !log_alpha_dv || !log_beta_dv) return PMT_E_INVALID;
    if (n < 0 || batch_size < 1 || epochs < 0) return PMT_E_INVALID;
    if (n == 0 || epochs == 0) return PMT_OK;  // the reference makes no step then
    SpectraHyper hy;
    hy.one_m_beta1 = (float)(1.0 - beta1);
    hy.beta2 = (float)beta2;
    hy.one_m_beta2 = (float)(1.0 - beta2);
    hy.eps = (float)eps;
    hy.lr = lr;
    hy.beta1 = beta1;
    hy.beta2_d = beta2;
    hipLaunchKernelGGL(pmt_spectra_fit_kernel, dim3(SF_D * SF_V), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), variant_types, depths,
                       alt_counts, (int)n, log_alpha_dv, log_beta_dv, (int)batch_size, (int)epochs, hy);
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}
