// The posterior model's per-candidate device code, shared by pmt_posterior.hip (evaluation and the fit of the spectra) and
// pmt_posterior_eval.hip (the scoring of a filtering run against truth labels): the transformed parameters in LDS (PoShared,
// po_prepare), a candidate's 48 bytes (po_load) and its priors, likelihoods and log posteriors (po_row; po_germline).  What each part
// computes and in which precision: the comment at the top of pmt_posterior.hip.
#pragma once
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

// the argument check every entry point over the rows starts with (host)
static int po_check(const PmtPosteriorRows* r, int64_t first, int64_t count, const PmtPosteriorParams* p) {
    if (!r || !p) return PMT_E_INVALID;
    if (!r->variant_types || !r->depths || !r->alt_counts || !r->normal_depths || !r->normal_alt_counts || !r->contexts ||
        !r->seq_error_log_lks || !r->normal_seq_error_log_lks || !r->allele_frequencies || !r->mafs || !r->normal_mafs || !r->artifact_logits)
        return PMT_E_INVALID;
    if (!p->log_priors_vc || !p->snv_log_priors_rrra || !p->raw) return PMT_E_INVALID;
    if (r->n < 0 || first < 0 || count < 0 || first > r->n || count > r->n - first) return PMT_E_INVALID;
    return PMT_OK;
}
