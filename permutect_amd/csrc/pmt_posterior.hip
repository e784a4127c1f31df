// The posterior model's per-candidate evaluation and the minibatch fit of its spectra (include/permutect_amd.h: pmt_posterior_forward,
// pmt_posterior_step, pmt_posterior_step_context, pmt_posterior_update; the torch form this was written from: permutect_amd/architecture/posterior_model.py,
// posterior_spectra.py, posterior_priors.py; reference architecture/posterior_model.py:69-157).
//
// A lane per candidate, workgroups of one wavefront.  Per candidate (48 bytes in):
//   * the somatic spectrum: 5 components x 100 binomial mixture points p_i = cf (maf' + (1 - 2 maf') t_i), each point
//     k log p + (n - k) log(1 - p) folded into a running-max logsumexp -- 1000 logf and 500 expf, fp32, nothing leaves registers.  With
//     GRAD the same pass carries sum_i w_i (k / p_i - (n - k) / (1 - p_i)) dp_i / dcf under the same running maximum (one reciprocal more
//     per point);
//   * the log binomial coefficients and the beta-binomials (tumor artifact, normal artifact's tumor and normal parts, germline hom
//     alt and, with het_beta, het) in DOUBLE: ~30 lgamma of arguments up to the depth, whose differences lose 2e-3 in fp32 at depth 4000.
//     The background cluster BetaBinomial(k | n, 1, 1) is -log(n + 1) exactly;
//   * the two three-way germline mixtures, the log_softmax of the priors and the softmax over the five calls in double (a few dozen
//     operations);
//   * with GRAD 18 fp32 digammas (pmt_stats_device.hpp, as are the beta-binomial and Adam's update) for the three learned beta-binomials.
// The transformed parameters (sigmoid, exp, log_softmax of the 80 raw values) and the 100 mixture points are computed once per workgroup
// into LDS.
//
// pmt_posterior_step leaves ONE row of 128 floats per workgroup.  A lane's gradient contributions belong to the parameters of its own
// (depth bin, variant type) cells; they are scattered deterministically: every lane puts its 22 values and three cell keys into LDS,
// then output thread o adds, in lane order 0 .. 63, the values of the lanes whose key is o's cell into a register it keeps across the
// grid-stride loop.  No atomics, no workgroup waits for another; the second launch (pmt_posterior_update, one workgroup) adds the rows
// in row order and applies Adam.
//
// pmt_posterior_step_context is the same kernel body with one addition for the context-dependent SNV priors' E step: every SNV row
// adds llrintf(p_somatic 2^30) into its context's 64-bit bin with an integer atomic.  Integer adds commute, so the 625 bins are the same
// bits from run to run and for any grid -- this file's rule kept without a second pass; `partials` do not change by a bit.
#include "pmt_posterior_device.hpp"

__global__ __launch_bounds__(PO_WAVE) void pmt_posterior_forward_kernel(PmtPosteriorRows rows, long long first, long long count, PmtPosteriorParams P,
                                                                       float* __restrict__ priors, float* __restrict__ spectra,
                                                                       float* __restrict__ normals, float* __restrict__ posteriors) {
    __shared__ PoShared sh;
    po_prepare(sh, P.raw);
    const long long i = (long long)blockIdx.x * PO_WAVE + threadIdx.x;
    if (i >= count) return;
    const PoRow w = po_load(rows, first + i);
    PoOut o;
    po_row<false>(w, sh, P, o, nullptr, nullptr);
    for (int c = 0; c < PO_CALLS; ++c) {
        if (priors) priors[i * PO_CALLS + c] = (float)o.prior[c];
        if (spectra) spectra[i * PO_CALLS + c] = (float)o.spec[c];
        if (normals) normals[i * PO_CALLS + c] = (float)o.norm[c];
        if (posteriors) posteriors[i * PO_CALLS + c] = (float)o.post[c];
    }
}

// which per-lane value and which key output o adds: key index -1 = every lane, -2 = nothing
__device__ __forceinline__ void po_output_map(int o, int& value, int& key, int& cell) {
    if (o < 10) { value = o; key = -1; cell = 0; }
    else if (o < 25) { value = 10; key = 0; cell = o - 10; }
    else if (o < 40) { value = 11; key = 0; cell = o - 25; }
    else if (o < 55) { value = 12; key = 1; cell = o - 40; }
    else if (o < 70) { value = 13; key = 1; cell = o - 55; }
    else if (o < 75) { value = 14; key = 2; cell = o - 70; }
    else if (o < 80) { value = 15; key = 2; cell = o - 75; }
    else if (o < 105) { value = 16 + (o - 80) % PO_CALLS; key = 2; cell = (o - 80) / PO_CALLS; }
    else if (o == 105) { value = 21; key = -1; cell = 0; }
    else { value = 0; key = -2; cell = 0; }
}

// CONTEXT: every SNV row also adds its somatic posterior, in 2^-30 fixed point, into its context's bin (pmt_posterior_step_context).
// Integer adds commute, so the bins do not depend on the order the workgroups arrive in; everything else is the same code.
template <bool CONTEXT>
__device__ __forceinline__ void po_step(PoShared& sh, const PmtPosteriorRows& rows, long long first, long long count, const PmtPosteriorParams& P,
                                        float* __restrict__ partials, unsigned long long* __restrict__ somatic_snv_fixed_rrra) {
    po_prepare(sh, P.raw);
    const int lane = threadIdx.x;
    float acc[2] = {0.f, 0.f};
    int value[2], key[2], cell[2];
    po_output_map(lane, value[0], key[0], cell[0]);
    po_output_map(lane + PO_WAVE, value[1], key[1], cell[1]);
    const long long stride = (long long)gridDim.x * PO_WAVE;
    for (long long base = (long long)blockIdx.x * PO_WAVE; base < count; base += stride) {  // (uniform over the workgroup)
        float v[PO_VALUES];
        int keys[3] = {-1, -1, -1};
        for (int j = 0; j < PO_VALUES; ++j) v[j] = 0.f;
        if (base + lane < count) {
            const PoRow w = po_load(rows, first + base + lane);
            PoOut o;
            po_row<true>(w, sh, P, o, v, keys);
            if (CONTEXT && w.type == 0) {  // (w.ctx is clamped into 0 .. 624: po_load)
                const long long q = llrintf(v[16 + PO_SOMATIC] * (float)PMT_CONTEXT_FIXED_ONE);
                if (q > 0) atomicAdd(somatic_snv_fixed_rrra + w.ctx, (unsigned long long)q);
            }
        }
        for (int j = 0; j < PO_VALUES; ++j) sh.values[lane][j] = v[j];
        for (int j = 0; j < 3; ++j) sh.keys[lane][j] = keys[j];
        __syncthreads();
        for (int h = 0; h < 2; ++h) {
            if (key[h] == -2) continue;
            float a = acc[h];
            for (int l = 0; l < PO_WAVE; ++l) {  // lane order: the same sum in every run
                const bool mine = key[h] == -1 ? sh.keys[l][2] >= 0 : sh.keys[l][key[h]] == cell[h];
                if (mine) a += sh.values[l][value[h]];
            }
            acc[h] = a;
        }
        __syncthreads();
    }
    const float scale = -1.0f / (float)count;  // the loss is minus the MEAN log evidence
    float* out = partials + (size_t)blockIdx.x * PMT_POSTERIOR_PARTIAL;
    out[lane] = acc[0] * scale;
    out[lane + PO_WAVE] = lane + PO_WAVE < PMT_POSTERIOR_RAW ? acc[1] * scale : acc[1];
}

__global__ __launch_bounds__(PO_WAVE) void pmt_posterior_step_kernel(PmtPosteriorRows rows, long long first, long long count, PmtPosteriorParams P,
                                                                    float* __restrict__ partials) {
    __shared__ PoShared sh;
    po_step<false>(sh, rows, first, count, P, partials, nullptr);
}

__global__ __launch_bounds__(PO_WAVE) void pmt_posterior_step_context_kernel(PmtPosteriorRows rows, long long first, long long count,
                                                                            PmtPosteriorParams P, float* __restrict__ partials,
                                                                            unsigned long long* __restrict__ somatic_snv_fixed_rrra) {
    __shared__ PoShared sh;
    po_step<true>(sh, rows, first, count, P, partials, somatic_snv_fixed_rrra);
}

__global__ __launch_bounds__(PMT_POSTERIOR_PARTIAL) void pmt_posterior_update_kernel(const float* __restrict__ partials, int num_partial_rows,
                                                                                    float* __restrict__ raw, float* __restrict__ adam_m,
                                                                                    float* __restrict__ adam_v, FitAdam h, float step_size, float bc2_sqrt,
                                                                                    float* __restrict__ totals_tc, double* __restrict__ loss_sum) {
    const int j = threadIdx.x;
    float s = 0.f;
    for (int r = 0; r < num_partial_rows; ++r) s += partials[(size_t)r * PMT_POSTERIOR_PARTIAL + j];  // row order: the same sum in every run
    if (j < PMT_POSTERIOR_RAW) {  // torch.optim.Adam
        float p = raw[j], m = adam_m[j], v = adam_v[j];
        fit_adam(p, m, v, s, h, step_size, bc2_sqrt);
        raw[j] = p;
        adam_m[j] = m;
        adam_v[j] = v;
    } else if (j < PMT_POSTERIOR_RAW + PO_TYPES * PO_CALLS) {
        totals_tc[j - PMT_POSTERIOR_RAW] += s;
    } else if (j == PMT_POSTERIOR_RAW + PO_TYPES * PO_CALLS) {
        *loss_sum += (double)s;
    }
}

extern "C" int pmt_posterior_forward(const PmtPosteriorRows* rows, int64_t first, int64_t count, const PmtPosteriorParams* params,
                                     float* log_priors_bc, float* spectra_log_lks_bc, float* normal_log_lks_bc, float* log_posteriors_bc,
                                     void* stream) {
    const int rc = po_check(rows, first, count, params);
    if (rc != PMT_OK) return rc;
    if (count == 0) return PMT_OK;
    const int64_t blocks = (count + PO_WAVE - 1) / PO_WAVE;
    if (blocks > 0x7fffffffLL) return PMT_E_INVALID;
    hipLaunchKernelGGL(pmt_posterior_forward_kernel, dim3((unsigned)blocks), dim3(PO_WAVE), 0, reinterpret_cast<hipStream_t>(stream), *rows,
                       (long long)first, (long long)count, *params, log_priors_bc, spectra_log_lks_bc, normal_log_lks_bc, log_posteriors_bc);
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}

extern "C" int pmt_posterior_step(const PmtPosteriorRows* rows, int64_t first, int64_t count, const PmtPosteriorParams* params, float* partials,
                                  int32_t num_partial_rows, void* stream) {
    const int rc = po_check(rows, first, count, params);
    if (rc != PMT_OK) return rc;
    if (!partials || num_partial_rows < 1) return PMT_E_INVALID;
    if (count == 0) return PMT_OK;
    hipLaunchKernelGGL(pmt_posterior_step_kernel, dim3((unsigned)num_partial_rows), dim3(PO_WAVE), 0, reinterpret_cast<hipStream_t>(stream), *rows,
                       (long long)first, (long long)count, *params, partials);
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}

extern "C" int pmt_posterior_step_context(const PmtPosteriorRows* rows, int64_t first, int64_t count, const PmtPosteriorParams* params,
                                          float* partials, int32_t num_partial_rows, unsigned long long* somatic_snv_fixed_rrra, void* stream) {
    const int rc = po_check(rows, first, count, params);
    if (rc != PMT_OK) return rc;
    if (!partials || num_partial_rows < 1 || !somatic_snv_fixed_rrra) return PMT_E_INVALID;
    if (count == 0) return PMT_OK;
    hipLaunchKernelGGL(pmt_posterior_step_context_kernel, dim3((unsigned)num_partial_rows), dim3(PO_WAVE), 0, reinterpret_cast<hipStream_t>(stream),
                       *rows, (long long)first, (long long)count, *params, partials, somatic_snv_fixed_rrra);
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}

extern "C" int pmt_posterior_update(const float* partials, int32_t num_partial_rows, int64_t count, float* raw, float* adam_m, float* adam_v,
                                    int64_t step, double lr, double beta1, double beta2, double eps, float* totals_tc, double* loss_sum,
                                    void* stream) {
    if (!partials || !raw || !adam_m || !adam_v || !totals_tc || !loss_sum) return PMT_E_INVALID;
    if (num_partial_rows < 1 || count < 0 || step < 1) return PMT_E_INVALID;
    if (count == 0) return PMT_OK;
    const FitAdam h = fit_adam_hyper(lr, beta1, beta2, eps);
    float step_size, bc2_sqrt;
    fit_bias_corrections(h, (double)step, step_size, bc2_sqrt);  // on the host
    hipLaunchKernelGGL(pmt_posterior_update_kernel, dim3(1), dim3(PMT_POSTERIOR_PARTIAL), 0, reinterpret_cast<hipStream_t>(stream), partials,
                       (int)num_partial_rows, raw, adam_m, adam_v, h, step_size, bc2_sqrt, totals_tc, loss_sum);
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}
