// What the statistical kernels share (pmt_downsample_fit.hip, pmt_spectra_fit.hip, pmt_posterior.hip, pmt_context_fit.hip, pmt_prune.hip): torch.optim.Adam's
// update and
// its bias corrections, the sums over a wavefront, the fp32 digamma and the beta-binomial.  One definition each: the fits are pinned
// by trajectory against float64 references, so a change here reaches all of them or none.  Every expression keeps its written order
// of operations (plain fp32 / double, IEEE division and square root).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// ---- Adam ------------------------------------------------------------------------------------------------------------------------
struct FitAdam {
    float one_m_beta1;  // m += (1 - beta1) (g - m)
    float beta2, one_m_beta2, eps;
    double lr, beta1, beta2_d;  // for the bias corrections
};

inline FitAdam fit_adam_hyper(double lr, double beta1, double beta2, double eps) {
    FitAdam h;
    h.one_m_beta1 = (float)(1.0 - beta1);
    h.beta2 = (float)beta2;
    h.one_m_beta2 = (float)(1.0 - beta2);
    h.eps = (float)eps;
    h.lr = lr;
    h.beta1 = beta1;
    h.beta2_d = beta2;
    return h;
}

// The two bias corrections of step `step` (1, 2, ...) depend on the step number alone: in double precision (pow), so no running fp32
// product.  The persistent fits evaluate this on the device, pmt_posterior_update on the host (the two pows need not agree in the
// last bit).
__host__ __device__ __forceinline__ void fit_bias_corrections(const FitAdam& h, double step, float& step_size, float& bc2_sqrt) {
    step_size = (float)(h.lr / (1.0 - pow(h.beta1, step)));
    bc2_sqrt = (float)sqrt(1.0 - pow(h.beta2_d, step));
}

// torch.optim.Adam's update of one parameter (no weight decay: AdamW's `p *= 1 - lr * weight_decay` is its caller's, before this)
__device__ __forceinline__ void fit_adam(float& p, float& m, float& v, float g, const FitAdam& h, float step_size, float bc2_sqrt) {
    m += h.one_m_beta1 * (g - m);
    v = h.beta2 * v + h.one_m_beta2 * g * g;
    p -= step_size * (m / (sqrtf(v) / bc2_sqrt + h.eps));
}

// ---- across the wavefront --------------------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ float fit_dpp(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float fit_lane(float x, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), lane)); }
// sum over each row of 16 lanes; every lane of a row ends with the same bits
__device__ __forceinline__ float fit_sum16(float x) {
    x += fit_dpp<0xB1>(x);   // quad_perm [1 0 3 2]
    x += fit_dpp<0x4E>(x);   // quad_perm [2 3 0 1]
    x += fit_dpp<0x141>(x);  // row_half_mirror: the other quad of the eight
    x += fit_dpp<0x140>(x);  // row_mirror: the other eight of the sixteen
    return x;
}
// sum over lanes 0 .. 31 (lanes 32 .. 63 get the sum of their own half); every lane of a half ends with the same bits
__device__ __forceinline__ float fit_sum32(float x) {
    x = fit_sum16(x);
    x += __shfl_xor(x, 16);
    return x;
}
// sum over the 64 lanes, the same bits in every lane and in every run
__device__ __forceinline__ float fit_sum64(float x) {
    x = fit_sum16(x);
    return (fit_lane(x, 0) + fit_lane(x, 16)) + (fit_lane(x, 32) + fit_lane(x, 48));
}

// the largest value of each row of 16 lanes / of the 64 lanes (pmt_context_fit.hip: the softmax over a row, the largest gradient)
__device__ __forceinline__ float fit_max16(float x) {
    x = fmaxf(x, fit_dpp<0xB1>(x));
    x = fmaxf(x, fit_dpp<0x4E>(x));
    x = fmaxf(x, fit_dpp<0x141>(x));
    x = fmaxf(x, fit_dpp<0x140>(x));
    return x;
}
__device__ __forceinline__ float fit_max64(float x) {
    x = fit_max16(x);
    return fmaxf(fmaxf(fit_lane(x, 0), fit_lane(x, 16)), fmaxf(fit_lane(x, 32), fit_lane(x, 48)));
}

// the same in double (pmt_prune.hip): an xor butterfly, whose two addends at every level are the same pair in both lanes
__device__ __forceinline__ double fit_sum64(double x) {
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
    return x;
}

// The bias corrections of a persistent fit: lane j holds those of step (t & ~63) + j + 1, computed once every 64 steps, and step t
// (0, 1, ...: uniform over the wave) reads its pair from lane t & 63 (v_readlane).  `at(h, t & 63, (double)(t + lane + 1), ...)`: the
// caller's integer type for the step number (int or long long) is the type of both, and the conversion is made in the refresh alone.
// `slot` MUST be t & 63 and `lane_step` t + lane + 1 of the SAME t: nothing here ties them (a helper that takes t and converts inside
// costs the downsampler's kernel a double conversion and two spilled SGPRs, profiles/stats_header_refactor.txt).
struct FitSchedule {
    float step_size = 0.f, bc2_sqrt = 1.f;
    template <typename T>
    __device__ __forceinline__ void at(const FitAdam& h, T slot, double lane_step, float& ss, float& bs) {
        if (slot == 0) fit_bias_corrections(h, lane_step, step_size, bc2_sqrt);
        ss = fit_lane(step_size, (int)slot);
        bs = fit_lane(bc2_sqrt, (int)slot);
    }
};

// ---- special functions -----------------------------------------------------------------------------------------------------------
// digamma in fp32, x > 0: the recurrence psi(x) = psi(x + 1) - 1 / x up to x >= 6 (at most six times), then the asymptotic series
// ln x - 1/(2x) - 1/(12x^2) + 1/(120x^4) - 1/(252x^6) + 1/(240x^8), whose first omitted term is 1/(132 x^10) < 1.3e-10 there.
// NaN in, NaN out; the loop is bounded whatever x is.
__device__ __forceinline__ float fit_digamma(float x) {
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
    const float common = fit_digamma(alpha + beta) - fit_digamma(n + alpha + beta);
    d_alpha = (fit_digamma(k + alpha) - fit_digamma(alpha)) + common;
    d_beta = (fit_digamma(n - k + beta) - fit_digamma(beta)) + common;
}
