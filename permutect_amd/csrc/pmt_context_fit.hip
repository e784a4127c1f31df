// The M step of the context-dependent somatic SNV priors (reference permutect/architecture/posterior_model_priors.py:158-222; this package's
// torch form: architecture/posterior_priors.py, `fit_context_rates`) as ONE persistent launch (include/permutect_amd.h:
// pmt_context_priors_fit, where the estimator is stated in full).
//
// The reference fits its model of the 12 x 16 mutation rates -- Beta(1, 1e6) overall rate R, Gamma(4, 5) concentrations kappa_s and
// kappa_c, theta_s ~ Dirichlet(kappa_s 1_12), theta_s. ~ Dirichlet(kappa_c 1_16), k_sc ~ Binomial(n_sc, R 12 theta_s 16 theta_sc) -- by
// pymc's mean-field ADVI and averages 1000 draws: stochastic and unseeded.  This is NOT that fit and claims none of its numbers: it is
// the maximiser of the same model's log joint F with every prior density taken in its unconstrained coordinate (u = logit R, a = log
// kappa_s, b = log kappa_c, theta = softmax), where the mode of each conjugate piece is its posterior mean, found by Adam with a
// learning rate that decays linearly to zero.
//
// One wavefront, 207 unknowns.  Lane j holds the flanks c = j & 15 of the three substitutions s = (j >> 4) + 4 i, i = 0 .. 2: three
// y[s][c] with their Adam moments; u, a, b and x[12] are replicated, every lane makes the same update of them from the same bits.  Per
// step
//
//   log theta_s  = log_softmax(x)                      (replicated)       log theta_sc = log_softmax over the row of 16 lanes (fit_max16, fit_sum16)
//   log p        = min(log R + log 192 + log theta_s + log theta_sc, log(1 - 1e-6))
//   w            = k - (n - k) p / (1 - p), 0 where the cap binds         W_s = sum_c w (fit_sum16)       W = sum_sc w (fit_sum64 of the lane's three)
//   dF/du        = (1 - R)(W + 1) - 1e6 R
//   dF/dx_s      = W_s + kappa_s - theta_s (W + 12 kappa_s)               (the twelve W_s: v_readlane from the four rows)
//   dF/dy_sc     = w + kappa_c - theta_sc (W_s + 16 kappa_c)
//   dF/da        = 4 - 5 kappa_s + kappa_s (12 psi(12 kappa_s) - 12 psi(kappa_s) + sum_s log theta_s)
//   dF/db        = 4 - 5 kappa_c + kappa_c (12 (16 psi(16 kappa_c) - 16 psi(kappa_c)) + sum_sc log theta_sc)
//   torch.optim.Adam on -F / max(sum k, 1), step size times (1 - t / T).
//
// F itself is never evaluated.  The launch also does what surrounds the fit: sum(totals_tc), the rrra -> sc gather, the two roundings
// and the write-back of log p into the table's 192 SNV entries; nothing is read back.  No LDS, no barrier, no atomics: a chain of
// dependent steps bound by the instruction LATENCY of one wave (profiles/context_priors_device.txt).  The fp32 digamma, the sums and
// maxima over the wave, Adam's update and its table of bias corrections are pmt_stats_device.hpp's.
#include <hip/hip_runtime.h>
#include <math.h>

#include "permutect_amd.h"
#include "pmt_stats_device.hpp"

#define CF_S 12
#define CF_MINE 3                        // substitutions per lane
#define CF_LOG_192 5.257495372027781f    // log(12 * 16)
#define CF_LOG_CAP (-1.0000005000003e-6f)  // log(1 - 1e-6)
#define CF_BETA_B 1.0e6f

struct CfForward {
    float lts[CF_S], ts[CF_S], sum_lts;  // replicated
    float ltsc[CF_MINE], tsc[CF_MINE], logp[CF_MINE];
    float log_r, r;
    bool capped[CF_MINE];
};

// the value of a replicated array of twelve at s = q + 4 i (q = lane >> 4): constant indices, nothing indexed by a register
__device__ __forceinline__ float cf_pick(const float* v, int q, int i) {
    const float a = v[4 * i], b = v[4 * i + 1], c = v[4 * i + 2], d = v[4 * i + 3];
    return q == 0 ? a : q == 1 ? b : q == 2 ? c : d;
}

__device__ __forceinline__ void cf_forward(CfForward& f, float u, const float* x, const float* y, int q) {
    float xm = x[0];
#pragma unroll
    for (int s = 1; s < CF_S; ++s) xm = fmaxf(xm, x[s]);
    float e[CF_S], xs = 0.f;
#pragma unroll
    for (int s = 0; s < CF_S; ++s) {
        e[s] = expf(x[s] - xm);
        xs += e[s];
    }
    const float lxs = logf(xs), inv_xs = 1.0f / xs;
    f.sum_lts = 0.f;
#pragma unroll
    for (int s = 0; s < CF_S; ++s) {
        f.lts[s] = (x[s] - xm) - lxs;
        f.ts[s] = e[s] * inv_xs;
        f.sum_lts += f.lts[s];
    }
    // log sigmoid(u) without overflow on either side
    f.log_r = u <= 0.f ? u - log1pf(expf(u)) : -log1pf(expf(-u));
    f.r = expf(f.log_r);
#pragma unroll
    for (int i = 0; i < CF_MINE; ++i) {
        const float ym = fit_max16(y[i]);
        const float ey = expf(y[i] - ym);
        const float se = fit_sum16(ey);
        f.ltsc[i] = (y[i] - ym) - logf(se);
        f.tsc[i] = ey / se;
        const float lp = ((f.log_r + CF_LOG_192) + cf_pick(f.lts, q, i)) + f.ltsc[i];
        f.capped[i] = lp >= CF_LOG_CAP;
        f.logp[i] = f.capped[i] ? CF_LOG_CAP : lp;
    }
}

__global__ __launch_bounds__(64) void pmt_context_priors_fit_kernel(const unsigned long long* __restrict__ fixed_rrra, const long long* __restrict__ counts_rrra,
                                                                    const float* __restrict__ totals_tc, double ratio, float* __restrict__ table_rrra,
                                                                    int steps, FitAdam hy, float* __restrict__ diagnostics) {
    const int lane = threadIdx.x, c = lane & 15, q = lane >> 4;

    // ---- the data: reference :158-171.  sum(totals_tc) in double and rounded to float once (a float32 torch.sum, whatever its order,
    // is within an ulp of it); the ignored sites per context as the float the reference's float32 addition takes
    double total = 0.0;
    for (int i = 0; i < 25; ++i) total += (double)totals_tc[i];
    const float ignored_per_context = (float)(ratio * (double)(float)total / 64.0);
    int idx[CF_MINE];
    float n[CF_MINE], k[CF_MINE];
    double lane_n = 0.0, lane_k = 0.0;
#pragma unroll
    for (int i = 0; i < CF_MINE; ++i) {
        const int s = q + 4 * i;
        const int ref = s / 3, r = s % 3, alt = r + (r >= ref ? 1 : 0);  // s = ref * 4 + alt without the ref == alt entries
        idx[i] = (((c >> 2) * 5 + ref) * 5 + (c & 3)) * 5 + alt;        // [left][ref][right][alt] of 5 x 5 x 5 x 5: always < 625
        n[i] = fmaxf(rintf((float)counts_rrra[idx[i]] + ignored_per_context), 0.f);
        k[i] = fminf(rintf((float)((double)fixed_rrra[idx[i]] * (1.0 / (double)PMT_CONTEXT_FIXED_ONE))), n[i]);
        lane_n += (double)n[i];
        lane_k += (double)k[i];
    }
    const double sum_n = fit_sum64(lane_n), sum_k = fit_sum64(lane_k);
    const float inv_scale = (float)(1.0 / fmax(sum_k, 1.0));

    // ---- the start
    float u, a, b, x[CF_S], y[CF_MINE];
    {
        const double r0 = (sum_k + 1.0) / (sum_n + 1.0e6 + 1.0);
        u = (float)(log(r0) - log1p(-r0));
        a = b = -0.2231435513142098f;  // log 0.8
    }
    float m_u = 0.f, v_u = 0.f, m_a = 0.f, v_a = 0.f, m_b = 0.f, v_b = 0.f, m_x[CF_S], v_x[CF_S], m_y[CF_MINE], v_y[CF_MINE];
#pragma unroll
    for (int s = 0; s < CF_S; ++s) x[s] = m_x[s] = v_x[s] = 0.f;
#pragma unroll
    for (int i = 0; i < CF_MINE; ++i) y[i] = m_y[i] = v_y[i] = 0.f;

    FitSchedule schedule;
    CfForward f;
    float last_max = 0.f;
    for (int t = 0; t < steps; ++t) {
        cf_forward(f, u, x, y, q);
        const float ks = expf(a), kc = expf(b);

        float w[CF_MINE], ws_mine[CF_MINE];
#pragma unroll
        for (int i = 0; i < CF_MINE; ++i) {
            const float p = expf(f.logp[i]);
            w[i] = f.capped[i] ? 0.f : k[i] - (n[i] - k[i]) * p / (1.0f - p);
            ws_mine[i] = fit_sum16(w[i]);
        }
        const float W = fit_sum64((w[0] + w[1]) + w[2]);
        const float sum_ltsc = fit_sum64((f.ltsc[0] + f.ltsc[1]) + f.ltsc[2]);

        // minus the gradient of F, to be scaled by 1 / max(sum k, 1)
        const float d_u = (1.0f - f.r) * (W + 1.0f) - CF_BETA_B * f.r;
        const float d_a = 4.0f - 5.0f * ks + ks * ((12.0f * fit_digamma(12.0f * ks) - 12.0f * fit_digamma(ks)) + f.sum_lts);
        const float d_b = 4.0f - 5.0f * kc + kc * (12.0f * (16.0f * fit_digamma(16.0f * kc) - 16.0f * fit_digamma(kc)) + sum_ltsc);
        float d_x[CF_S], d_y[CF_MINE];
#pragma unroll
        for (int i = 0; i < CF_MINE; ++i) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int s = r + 4 * i;
                d_x[s] = fit_lane(ws_mine[i], 16 * r) + ks - f.ts[s] * (W + 12.0f * ks);
            }
            d_y[i] = w[i] + kc - f.tsc[i] * (ws_mine[i] + 16.0f * kc);
        }

        if (t == steps - 1) {  // (uniform) what the caller logs: the largest gradient entry the last step saw
            float mx = fmaxf(fabsf(d_u), fmaxf(fabsf(d_a), fabsf(d_b)));
#pragma unroll
            for (int s = 0; s < CF_S; ++s) mx = fmaxf(mx, fabsf(d_x[s]));
#pragma unroll
            for (int i = 0; i < CF_MINE; ++i) mx = fmaxf(mx, fabsf(d_y[i]));
            last_max = fit_max64(mx) * inv_scale;
        }

        float ss, bq;
        schedule.at(hy, t & 63, (double)(t + lane + 1), ss, bq);
        ss *= 1.0f - (float)t / (float)steps;  // the learning rate lr0 (1 - t / T)
        fit_adam(u, m_u, v_u, -d_u * inv_scale, hy, ss, bq);
        fit_adam(a, m_a, v_a, -d_a * inv_scale, hy, ss, bq);
        fit_adam(b, m_b, v_b, -d_b * inv_scale, hy, ss, bq);
#pragma unroll
        for (int s = 0; s < CF_S; ++s) fit_adam(x[s], m_x[s], v_x[s], -d_x[s] * inv_scale, hy, ss, bq);
#pragma unroll
        for (int i = 0; i < CF_MINE; ++i) fit_adam(y[i], m_y[i], v_y[i], -d_y[i] * inv_scale, hy, ss, bq);
    }

    // ---- the write-back (reference :212-222): log p of the last iterate into the 192 SNV entries, every lane its three
    cf_forward(f, u, x, y, q);
#pragma unroll
    for (int i = 0; i < CF_MINE; ++i) table_rrra[idx[i]] = f.logp[i];
    if (diagnostics) {
        if (lane == 0) {
            diagnostics[0] = last_max;
            diagnostics[1] = (float)sum_k;
            diagnostics[2] = expf(a);
            diagnostics[3] = expf(b);
        }
#pragma unroll
        for (int i = 0; i < CF_MINE; ++i) {
            const int cell = (q + 4 * i) * 16 + c;  // < 192
            diagnostics[4 + cell] = n[i];
            diagnostics[4 + 192 + cell] = k[i];
        }
    }
}

extern "C" int pmt_context_priors_fit(const unsigned long long* somatic_snv_fixed_rrra, const int64_t* snv_context_totals_rrra, const float* totals_tc,
                                      double ratio, float* snv_log_priors_rrra, int32_t steps, double lr0, double beta1, double beta2, double eps,
                                      float* diagnostics, void* stream) {
    if (!somatic_snv_fixed_rrra || !snv_context_totals_rrra || !totals_tc || !snv_log_priors_rrra) return PMT_E_INVALID;
    if (steps < 1 || steps > PMT_FIT_MAX_STEPS) return PMT_E_INVALID;
    if (!(lr0 > 0.0) || !isfinite(lr0) || !(ratio >= 0.0) || !isfinite(ratio)) return PMT_E_INVALID;
    hipLaunchKernelGGL(pmt_context_priors_fit_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), somatic_snv_fixed_rrra,
                       reinterpret_cast<const long long*>(snv_context_totals_rrra), totals_tc, ratio, snv_log_priors_rrra, (int)steps,
                       fit_adam_hyper(lr0, beta1, beta2, eps), diagnostics);
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}
