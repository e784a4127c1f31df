// Special functions of the posterior kernels (pmt_posterior.hip is the only unit that includes this).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// digamma in fp32, x > 0: the recurrence psi(x) = psi(x + 1) - 1 / x up to x >= 6 (at most six times), then the asymptotic series
// ln x - 1/(2x) - 1/(12x^2) + 1/(120x^4) - 1/(252x^6) + 1/(240x^8) (first omitted term 1/(132 x^10) < 1.3e-10 there): the series of
// pmt_spectra_fit.hip (sf_digamma), the same constants.  NaN in, NaN out; the loop is bounded whatever x is.
__device__ __forceinline__ float pm_digamma(float x) {
    float s = 0.f;
    for (int i = 0; i < 6 && x < 6.0f; ++i) {
        s += 1.0f / x;
        x += 1.0f;
    }
    const float r = 1.0f / x, r2 = r * r;
    const float tail = r2 * (8.3333333e-2f - r2 * (8.3333333e-3f - r2 * (3.9682540e-3f - r2 * 4.1666667e-3f)));
    return ((logf(x) - 0.5f * r) - tail) - s;
}

// log of the binomial coefficient, in double: at depths in the thousands the three lgammas are ~3e4 and their difference a few
// hundred, which costs fp32 2e-3 absolute
__device__ __forceinline__ double pm_log_choose(double n, double k) { return lgamma(n + 1.0) - lgamma(n - k + 1.0) - lgamma(k + 1.0); }

// log BetaBinomial(k | n, alpha, beta) given the log binomial coefficient (reference utils/stats_utils.py:28-40)
__device__ __forceinline__ double pm_beta_binomial(double comb, double n, double k, double alpha, double beta) {
    return comb + lgamma(k + alpha) + lgamma(n - k + beta) + lgamma(alpha + beta) - lgamma(n + alpha + beta) - lgamma(alpha) - lgamma(beta);
}

// d/d alpha and d/d beta of log BetaBinomial(k | n, alpha, beta)
__device__ __forceinline__ void pm_beta_binomial_grad(float n, float k, float alpha, float beta, float& d_alpha, float& d_beta) {
    const float common = pm_digamma(alpha + beta) - pm_digamma(n + alpha + beta);
    d_alpha = (pm_digamma(k + alpha) - pm_digamma(alpha)) + common;
    d_beta = (pm_digamma(n - k + beta) - pm_digamma(beta)) + common;
}
