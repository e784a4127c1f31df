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
// workgroups.  The fp32 digamma, the sum over the wave, Adam's update and its per-lane table of bias corrections are
// pmt_stats_device.hpp's (fit_digamma, fit_sum64, fit_adam, FitSchedule).
//
// A launch is a chain of dependent steps of a few hundred instructions: bound by instruction LATENCY of one wave (logf, divisions, the
// cross-lane sums), not by any throughput of the device.  The figure of merit is microseconds per step (DESIGN.md section 4,
// profiles/spectra_fit_device.txt).
#include <hip/hip_runtime.h>
#include <math.h>

#include "permutect_amd.h"
#include "pmt_stats_device.hpp"

#define SF_D 3  // depth bins: (depth >= 10) + (depth >= 20)
#define SF_V 5  // variant types

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
                                                             FitAdam hy) {
    const int cell = blockIdx.x, lane = threadIdx.x;
    const int my_bin = cell / SF_V, my_type = cell % SF_V;
    const long long n_rows = n, bs = batch_size;
    const long long num_batches = (n_rows + bs - 1) / bs;

    float la = log_alpha[cell], lb = log_beta[cell];
    float m_a = 0.f, m_b = 0.f, v_a = 0.f, v_b = 0.f;
    FitSchedule schedule;
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
                    const float dn = fit_digamma(nn + ab);
                    sum_a += fit_digamma(k + alpha) - dn;
                    sum_b += fit_digamma(nn - k + beta) - dn;
                    cnt += 1.0f;
                }
            }
            const float c = fit_sum64(cnt);
            float g_a = 0.f, g_b = 0.f;  // a batch without a row of this cell: zero gradients, as autograd gives
            if (c > 0.f) {
                const float dab = fit_digamma(ab);
                const float inv_len = 1.0f / (float)len;
                g_a = -(alpha * inv_len) * (fit_sum64(sum_a) + c * (dab - fit_digamma(alpha)));
                g_b = -(beta * inv_len) * (fit_sum64(sum_b) + c * (dab - fit_digamma(beta)));
            }

            float ss, bq;
            schedule.at(hy, t & 63, (double)(t + lane + 1), ss, bq);
            fit_adam(la, m_a, v_a, g_a, hy, ss, bq);
            fit_adam(lb, m_b, v_b, g_b, hy, ss, bq);
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
    hipLaunchKernelGGL(pmt_spectra_fit_kernel, dim3(SF_D * SF_V), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), variant_types, depths,
                       alt_counts, (int)n, log_alpha_dv, log_beta_dv, (int)batch_size, (int)epochs, fit_adam_hyper(lr, beta1, beta2, eps));
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}
