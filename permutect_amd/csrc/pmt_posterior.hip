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
#include <hip/hip_runtime.h>
#include <math.h>

#include "permutect_amd.h"
#include "pmt_stats_device.hpp"

#define PO_WAVE 64
#define PO_K 5        // somatic components
#define PO_POINTS 100 // len(torch.arange(0.001, 0.999, 0.01))
#define PO_CALLS 5
#define PO_TYPES 5
#define PO_CELLS 15
#define PO_VALUES 22  // per lane: 5 d/d cf, 5 d/d weight logit, 2 tumor artifact, 2 normal spectrum, 2 normal artifact, 5 posteriors, log evidence
#define PO_MINUS_INF_CALL (-9999.0)
enum { PO_SOMATIC = 0, PO_ARTIFACT = 1, PO_SEQ_ERROR = 2, PO_GERMLINE = 3, PO_NORMAL_ARTIFACT = 4 };
// offsets into raw / the transformed parameters
enum { PO_CF = 0, PO_LW = 5, PO_TA = 10, PO_TB = 25, PO_NA = 40, PO_NB = 55, PO_MM = 70, PO_CONC = 75 };

struct PoShared {
    double prm[PMT_POSTERIOR_RAW];  // cf, log weights, alphas, betas, mean multipliers, concentrations: transformed
    float points[PO_POINTS];
    float values[PO_WAVE][PO_VALUES + 1];
    int keys[PO_WAVE][3];  // tumor artifact cell, normal spectrum cell, variant type; -1: none
};

__device__ __forceinline__ void po_prepare(PoShared& sh, const float* __restrict__ raw) {
    for (int j = threadIdx.x; j < PMT_POSTERIOR_RAW; j += blockDim.x) {
        const double x = (double)raw[j];
        double y;
        if (j < PO_LW || (j >= PO_MM && j < PO_CONC)) {
            y = 1.0 / (1.0 + exp(-x));  // BoundedNumber(0, 1)
        } else if (j < PO_TA) {         // LogWeights: log_softmax of the five logits
            double m = (double)raw[PO_LW];
            for (int i = 1; i < PO_K; ++i) m = fmax(m, (double)raw[PO_LW + i]);
            double s = 0.0;
            for (int i = 0; i < PO_K; ++i) s += exp((double)raw[PO_LW + i] - m);
            y = x - m - log(s);
        } else {
            y = exp(x);  // PositiveNumber
        }
        sh.prm[j] = y;
    }
    for (int i = threadIdx.x; i < PO_POINTS; i += blockDim.x) sh.points[i] = (float)(0.001 + 0.01 * (double)i);
    __syncthreads();
}

__device__ __forceinline__ double po_lse3(double a, double b, double c) {
    const double m = fmax(a, fmax(b, c));
    return m + log(exp(a - m) + exp(b - m) + exp(c - m));
}

// reference posterior_model_spectra.py:18-54
__device__ __forceinline__ double po_germline(double af, double maf, double k, double n, double comb, bool has_het_beta, double het_beta) {
    const double het = 2.0 * af * (1.0 - af), hom = af * af;
    const double het_prop = het / (het + hom), hom_prop = 1.0 - het_prop;
    const double log_half_het = log(het_prop / 2.0);
    double minor, major;
    if (has_het_beta) {
        minor = major = pm_beta_binomial(comb, n, k, het_beta, het_beta);
    } else {
        const double lm = log(maf), l1m = log(1.0 - maf), r = n - k;
        minor = comb + k * lm + r * l1m;
        major = comb + r * lm + k * l1m;
    }
    return po_lse3(log_half_het + minor, log_half_het + major, log(hom_prop) + pm_beta_binomial(comb, n, k, 98.0, 2.0));
}

struct PoRow {
    int type, depth, alt, ndepth, nalt, ctx;
    float se, nse, af, maf, nmaf, logit;
};

__device__ __forceinline__ PoRow po_load(const PmtPosteriorRows& r, long long i) {
    PoRow w;
    w.type = min(max(r.variant_types[i], 0), PO_TYPES - 1);
    w.depth = r.depths[i];
    w.alt = r.alt_counts[i];
    w.ndepth = r.normal_depths[i];
    w.nalt = r.normal_alt_counts[i];
    w.ctx = min(max(r.contexts[i], 0), 624);
    w.se = r.seq_error_log_lks[i];
    w.nse = r.normal_seq_error_log_lks[i];
    w.af = r.allele_frequencies[i];
    w.maf = r.mafs[i];
    w.nmaf = r.normal_mafs[i];
    w.logit = r.artifact_logits[i];
    return w;
}

struct PoOut {
    double prior[PO_CALLS], spec[PO_CALLS], norm[PO_CALLS], post[PO_CALLS];
};

// One candidate.  GRAD: v[0 .. 21] and keys as described above (v is d(log evidence) / d(raw), unscaled).
template <bool GRAD>
__device__ __forceinline__ void po_row(const PoRow& w, const PoShared& sh, const PmtPosteriorParams& P, PoOut& o, float* v, int* keys) {
    const int t = w.type;
    const double n = (double)w.depth, k = (double)w.alt, nn = (double)w.ndepth, nk = (double)w.nalt;
    const int tcell = ((w.depth >= 10) + (w.depth >= 20)) * PO_TYPES + t;
    const int ncell = ((w.ndepth >= 10) + (w.ndepth >= 20)) * PO_TYPES + t;

    // ---- priors (reference posterior_model_priors.py:129-145)
    {
        double x[PO_CALLS];
        for (int c = 0; c < PO_CALLS; ++c) x[c] = (double)P.log_priors_vc[t * PO_CALLS + c];
        x[PO_SEQ_ERROR] = 0.0;
        const double hom_ref = 1.0 - (double)w.af;
        x[PO_GERMLINE] = P.no_germline ? PO_MINUS_INF_CALL : log(1.0 - hom_ref * hom_ref);
        if (P.use_context) {
            const double is_snv = t == 0 ? 1.0 : 0.0;
            x[PO_SOMATIC] = is_snv * (double)P.snv_log_priors_rrra[w.ctx] + (1.0 - is_snv) * x[PO_SOMATIC];
        }
        double m = x[0];
        for (int c = 1; c < PO_CALLS; ++c) m = fmax(m, x[c]);
        double s = 0.0;
        for (int c = 0; c < PO_CALLS; ++c) s += exp(x[c] - m);
        const double lse = m + log(s);
        for (int c = 0; c < PO_CALLS; ++c) o.prior[c] = x[c] - lse;
    }

    const double comb = pm_log_choose(n, k), ncomb = pm_log_choose(nn, nk);

    // ---- somatic spectrum (reference somatic_spectrum.py:72-96, utils/stats_utils.py:160-175)
    float ub[PO_K], dub[PO_K];  // log uniform-binomial without the coefficient; its derivative by cf
    {
        const float kf = (float)w.alt, rf = (float)(w.depth - w.alt);
        const float mafc = fminf(w.maf, 0.49f);
        const float span = 1.0f - mafc;
        for (int j = 0; j < PO_K; ++j) {
            const float cf = (float)sh.prm[PO_CF + j];
            const float x1 = mafc * cf, x2 = span * cf;
            float M = -INFINITY, S = 0.f, G = 0.f;
#pragma unroll 4
            for (int i = 0; i < PO_POINTS; ++i) {
                const float ti = sh.points[i];
                const float p = x2 * ti + x1 * (1.0f - ti);
                const float q = 1.0f - p;
                const float ll = kf * logf(p) + rf * logf(q);
                const float d = ll - M;
                const float e = expf(-fabsf(d));
                float g = 0.f;
                if (GRAD) g = kf - rf * p / q;  // (k / p - (n - k) / (1 - p)) p, to be divided by cf
                if (d > 0.f) {
                    S = S * e + 1.0f;
                    if (GRAD) G = G * e + g;
                    M = ll;
                } else {
                    S += e;
                    if (GRAD) G += e * g;
                }
            }
            ub[j] = M + logf(S) - 4.605170185988092f;  // log 100
            dub[j] = GRAD ? G / (S * cf) : 0.f;
        }
    }
    double resp[PO_K], nb;  // responsibilities of the components
    {
        double y[PO_K], m = -INFINITY;
        for (int j = 0; j < PO_K; ++j) {
            y[j] = sh.prm[PO_LW + j] + (double)ub[j];
            m = fmax(m, y[j]);
        }
        double s = 0.0;
        for (int j = 0; j < PO_K; ++j) s += exp(y[j] - m);
        nb = m + log(s);
        for (int j = 0; j < PO_K; ++j) resp[j] = exp(y[j] - nb);
        nb += comb;
    }
    const double log_bg = -9.210340371976182, log_non_bg = -1.0000500033334732e-4;  // log 1e-4, log(1 - 1e-4)
    const double A = log_non_bg + nb, B = log_bg - log(n + 1.0);                    // BetaBinomial(k | n, 1, 1) = 1 / (n + 1)
    const double mab = fmax(A, B);
    o.spec[PO_SOMATIC] = mab + log(exp(A - mab) + exp(B - mab));

    // ---- the beta-binomials
    const double ta = sh.prm[PO_TA + tcell], tb = sh.prm[PO_TB + tcell];
    o.spec[PO_ARTIFACT] = pm_beta_binomial(comb, n, k, ta, tb);
    const double mm = sh.prm[PO_MM + t], conc = sh.prm[PO_CONC + t];
    const double f = nk / (nn + 0.001);
    const double na_a = 0.001 + f * mm * conc;
    const bool clamped = conc - na_a < 0.001;
    const double na_b = clamped ? 0.001 : conc - na_a;
    o.spec[PO_NORMAL_ARTIFACT] = pm_beta_binomial(comb, n, k, na_a, na_b);
    o.spec[PO_SEQ_ERROR] = (double)w.se;
    o.spec[PO_GERMLINE] = po_germline((double)w.af, (double)w.maf, k, n, comb, P.has_het_beta != 0, (double)P.het_beta);

    const double nalpha = sh.prm[PO_NA + ncell], nbeta = sh.prm[PO_NB + ncell];
    const bool no_normal_alt = w.nalt < 1;
    o.norm[PO_SOMATIC] = o.norm[PO_ARTIFACT] = o.norm[PO_SEQ_ERROR] = (double)w.nse;
    o.norm[PO_NORMAL_ARTIFACT] = no_normal_alt ? PO_MINUS_INF_CALL : pm_beta_binomial(ncomb, nn, nk, nalpha, nbeta);
    o.norm[PO_GERMLINE] = po_germline((double)w.af, (double)w.nmaf, nk, nn, ncomb, P.has_het_beta != 0, (double)P.het_beta);

    // ---- posteriors (reference posterior_model.py:82-95)
    for (int c = 0; c < PO_CALLS; ++c) o.post[c] = o.prior[c] + o.spec[c] + o.norm[c];
    o.post[PO_ARTIFACT] += (double)w.logit;
    o.post[PO_NORMAL_ARTIFACT] += (double)w.logit;
    const bool artifact_off = w.logit < 0.f;
    if (artifact_off) o.post[PO_ARTIFACT] = PO_MINUS_INF_CALL;

    if (GRAD) {
        double m = o.post[0];
        for (int c = 1; c < PO_CALLS; ++c) m = fmax(m, o.post[c]);
        double e[PO_CALLS], s = 0.0;
        for (int c = 0; c < PO_CALLS; ++c) {
            e[c] = exp(o.post[c] - m);
            s += e[c];
        }
        const double evidence = m + log(s);
        float pr[PO_CALLS];
        for (int c = 0; c < PO_CALLS; ++c) pr[c] = (float)(e[c] / s);
        for (int c = 0; c < PO_CALLS; ++c) v[16 + c] = pr[c];
        v[21] = (float)evidence;
        keys[0] = tcell;
        keys[1] = ncell;
        keys[2] = t;

        // somatic: posterior x share of the non-background clusters x responsibilities
        const float ws = pr[PO_SOMATIC] * (float)exp(A - o.spec[PO_SOMATIC]);
        for (int j = 0; j < PO_K; ++j) {
            const float cf = (float)sh.prm[PO_CF + j];
            v[j] = ws * (float)resp[j] * dub[j] * (cf * (1.0f - cf));
            v[5 + j] = ws * ((float)resp[j] - (float)exp(sh.prm[PO_LW + j]));
        }
        // tumor artifact spectrum: nothing through the -9999 of a negative artifact logit
        v[10] = v[11] = 0.f;
        if (!artifact_off) {
            float da, db;
            pm_beta_binomial_grad((float)w.depth, (float)w.alt, (float)ta, (float)tb, da, db);
            v[10] = pr[PO_ARTIFACT] * da * (float)ta;
            v[11] = pr[PO_ARTIFACT] * db * (float)tb;
        }
        // normal artifact: the normal's own spectrum (nothing through the -9999 of a normal without alt reads) ...
        v[12] = v[13] = 0.f;
        const float wna = pr[PO_NORMAL_ARTIFACT];
        if (!no_normal_alt) {
            float da, db;
            pm_beta_binomial_grad((float)w.ndepth, (float)w.nalt, (float)nalpha, (float)nbeta, da, db);
            v[12] = wna * da * (float)nalpha;
            v[13] = wna * db * (float)nbeta;
        }
        // ... and the tumor's beta-binomial around the normal's allele fraction: alpha = 0.001 + f mm conc, beta = max(conc - alpha, 0.001)
        {
            float da, db;
            pm_beta_binomial_grad((float)w.depth, (float)w.alt, (float)na_a, (float)na_b, da, db);
            if (clamped) db = 0.f;  // a binding clamp passes nothing
            const float ff = (float)f, mmf = (float)mm, cc = (float)conc;
            const float d_mm = (da - db) * ff * cc;
            const float d_conc = da * ff * mmf + db * (1.0f - ff * mmf);
            v[14] = wna * d_mm * (mmf * (1.0f - mmf));
            v[15] = wna * d_conc * cc;
        }
    }
}

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

static int po_check(const PmtPosteriorRows* r, int64_t first, int64_t count, const PmtPosteriorParams* p) {
    if (!r || !p) return PMT_E_INVALID;
    if (!r->variant_types || !r->depths || !r->alt_counts || !r->normal_depths || !r->normal_alt_counts || !r->contexts ||
        !r->seq_error_log_lks || !r->normal_seq_error_log_lks || !r->allele_frequencies || !r->mafs || !r->normal_mafs || !r->artifact_logits)
        return PMT_E_INVALID;
    if (!p->log_priors_vc || !p->snv_log_priors_rrra || !p->raw) return PMT_E_INVALID;
    if (r->n < 0 || first < 0 || count < 0 || first > r->n || count > r->n - first) return PMT_E_INVALID;
    return PMT_OK;
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
