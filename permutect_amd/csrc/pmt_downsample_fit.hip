// The fit of the downsampler's mixture weights (reference permutect/training/downsampler.py:125-158, `optimize_downsampling_balance`;
// this package's torch form: training/downsampler.py) as ONE persistent launch (include/permutect_amd.h: pmt_downsample_fit).
//
// The loss is a sum over (source, label, variant type) cells and AdamW is element-wise, so every cell is its own problem of
// 2 * R * A * K = 160 unknowns.  One wavefront (= one workgroup) per cell runs all `steps` iterations: lane l < 20 owns the
// (r, a) = (l / 5, l % 5) entry of the cell -- its count, its 4 + 4 logits, their 16 AdamW moments, and the rows Tr[:, r, :] and
// Ta[:, a, :] of the two transition tables -- in registers from the first step to the last.  Per step and cell
//
//   pr = softmax(theta_r), pa = softmax(theta_a)                       (per lane)
//   u[y] = sum_k pr[k] Tr[k,r,y]      w[z] = sum_h pa[h] Ta[h,a,z]     (per lane)
//   E[y,z] = sum_lanes c u[y] w[z]                                     (20 sums over the wave: four DPP stages inside a row of 16
//                                                                       lanes, one shuffle between the two rows that hold data)
//   T = sum E, N = E / T, loss = sum N^2, G = 2 (N - loss) / T         (every lane, the same numbers)
//   d pr[k] = c sum_y Tr[k,r,y] sum_z G[y,z] w[z]      d pa[h] = c sum_z Ta[h,a,z] sum_y G[y,z] u[y]
//   d theta = p (d p - sum_j p[j] d p[j])                              (softmax backward), then torch.optim.AdamW's update.
//
// (`- loss` in G: T depends on the logits only through the fp32 rounding of the tables' row sums, 2e-6, but the torch fit
// differentiates through it, so this does too.)  A cell without data (T = 0) and an entry with a zero count have exactly zero
// gradients: AdamW's update is 0 / (0 + eps) there and only the weight decay acts, as in torch.  Lanes 20 .. 63 carry a zero count and
// zero logits and take part in the sums with zeros; nothing is stored from them.
//
// No LDS, no barrier, no atomics, nothing between workgroups; the loop count is the launch argument.  Plain fp32 with expf and IEEE
// division / square root.  The sums over the wave, AdamW's moment update and its per-lane table of bias corrections are
// pmt_stats_device.hpp's (fit_sum32, fit_adam, FitSchedule); the weight decay `theta *= 1 - lr * weight_decay` comes first, here.
//
// A launch is a chain of `steps` dependent iterations of ~1 480 instructions on 20 lanes: it is bound by instruction LATENCY -- the
// issue time of one wave's dependent stream (expf, division, the cross-lane sums) --, not by any throughput of the device.  The figure of
// merit is microseconds per step: 2.82 measured on an MI355X (profiles/downsampler_fit_device.txt).
#include <hip/hip_runtime.h>
#include <math.h>

#include "permutect_amd.h"
#include "pmt_stats_device.hpp"

#define FIT_L 3
#define FIT_V 5
#define FIT_R 4
#define FIT_A 5
#define FIT_K 4
#define FIT_ENTRIES (FIT_R * FIT_A)  // 20 (r, a) entries per cell, one lane each

__device__ __forceinline__ void fit_softmax4(const float (&t)[FIT_K], float (&p)[FIT_K]) {
    const float mx = fmaxf(fmaxf(t[0], t[1]), fmaxf(t[2], t[3]));
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < FIT_K; ++k) {
        p[k] = expf(t[k] - mx);
        s += p[k];
    }
#pragma unroll
    for (int k = 0; k < FIT_K; ++k) p[k] = p[k] / s;
}

// pr, pa -> u, w, N (the normalised expected counts, the same in every lane of the lower half), the divisor and the loss
__device__ __forceinline__ float fit_forward(float c, const float (&tr)[FIT_K][FIT_R], const float (&ta)[FIT_K][FIT_A], const float (&pr)[FIT_K],
                                             const float (&pa)[FIT_K], float (&u)[FIT_R], float (&w)[FIT_A], float (&n)[FIT_R][FIT_A], float& tsafe) {
#pragma unroll
    for (int y = 0; y < FIT_R; ++y) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < FIT_K; ++k) s += pr[k] * tr[k][y];
        u[y] = s;
    }
#pragma unroll
    for (int z = 0; z < FIT_A; ++z) {
        float s = 0.f;
#pragma unroll
        for (int h = 0; h < FIT_K; ++h) s += pa[h] * ta[h][z];
        w[z] = s;
    }
    float total = 0.f;
#pragma unroll
    for (int y = 0; y < FIT_R; ++y)
#pragma unroll
        for (int z = 0; z < FIT_A; ++z) {
            n[y][z] = fit_sum32(c * u[y] * w[z]);
            total += n[y][z];
        }
    tsafe = total > 0.f ? total : 1.0f;  // a cell without data: 0 / 1 (training/downsampler.py)
    float loss = 0.f;
#pragma unroll
    for (int y = 0; y < FIT_R; ++y)
#pragma unroll
        for (int z = 0; z < FIT_A; ++z) {
            n[y][z] = n[y][z] / tsafe;
            loss += n[y][z] * n[y][z];
        }
    return loss;
}

// torch.optim.AdamW: the decay (1 - lr * weight_decay), then Adam
__device__ __forceinline__ void fit_adamw(float& p, float& m, float& v, float g, float decay, const FitAdam& h, float step_size, float bc2_sqrt) {
    p *= decay;
    fit_adam(p, m, v, g, h, step_size, bc2_sqrt);
}

__global__ __launch_bounds__(64) void pmt_downsample_fit_kernel(const float* __restrict__ counts, const float* __restrict__ ref_trans, const float* __restrict__ alt_trans,
                                                                float* __restrict__ ref_logits, float* __restrict__ alt_logits, int steps, FitAdam hy, float decay, float* __restrict__ losses) {
    const int cell = blockIdx.x, lane = threadIdx.x;
    const bool owner = lane < FIT_ENTRIES;
    const int e = owner ? lane : 0, r = e / FIT_A, a = e % FIT_A;
    const size_t entry = (size_t)cell * FIT_ENTRIES + e;

    float tr[FIT_K][FIT_R], ta[FIT_K][FIT_A];
#pragma unroll
    for (int k = 0; k < FIT_K; ++k) {
#pragma unroll
        for (int y = 0; y < FIT_R; ++y) tr[k][y] = ref_trans[(k * FIT_R + r) * FIT_R + y];
#pragma unroll
        for (int z = 0; z < FIT_A; ++z) ta[k][z] = alt_trans[(k * FIT_A + a) * FIT_A + z];
    }
    const float c = owner ? counts[entry] : 0.f;
    float th_r[FIT_K], th_a[FIT_K], m_r[FIT_K], m_a[FIT_K], v_r[FIT_K], v_a[FIT_K];
#pragma unroll
    for (int k = 0; k < FIT_K; ++k) {
        th_r[k] = owner ? ref_logits[entry * FIT_K + k] : 0.f;
        th_a[k] = owner ? alt_logits[entry * FIT_K + k] : 0.f;
        m_r[k] = m_a[k] = v_r[k] = v_a[k] = 0.f;
    }

    FitSchedule schedule;
    for (int t = 0;; ++t) {
        float pr[FIT_K], pa[FIT_K], u[FIT_R], w[FIT_A], n[FIT_R][FIT_A], tsafe;
        fit_softmax4(th_r, pr);
        fit_softmax4(th_a, pa);
        const float loss = fit_forward(c, tr, ta, pr, pa, u, w, n, tsafe);
        if (t == 0 && losses != nullptr && lane == 0) losses[2 * cell] = loss;
        if (t == steps) {
            if (losses != nullptr && lane == 0) losses[2 * cell + 1] = loss;
            break;
        }
        float ss, bs;
        schedule.at(hy, t & 63, (double)(t + lane + 1), ss, bs);

        // G = dloss / dE, folded at once into  gw[y] = sum_z G[y,z] w[z]  and  gu[z] = sum_y G[y,z] u[y]
        float gw[FIT_R], gu[FIT_A];
#pragma unroll
        for (int z = 0; z < FIT_A; ++z) gu[z] = 0.f;
#pragma unroll
        for (int y = 0; y < FIT_R; ++y) {
            gw[y] = 0.f;
#pragma unroll
            for (int z = 0; z < FIT_A; ++z) {
                const float g = 2.0f * (n[y][z] - loss) / tsafe;
                gw[y] += g * w[z];
                gu[z] += g * u[y];
            }
        }
        float dpr[FIT_K], dpa[FIT_K], dot_r = 0.f, dot_a = 0.f;
#pragma unroll
        for (int k = 0; k < FIT_K; ++k) {
            float sr = 0.f, sa = 0.f;
#pragma unroll
            for (int y = 0; y < FIT_R; ++y) sr += tr[k][y] * gw[y];
#pragma unroll
            for (int z = 0; z < FIT_A; ++z) sa += ta[k][z] * gu[z];
            dpr[k] = c * sr;
            dpa[k] = c * sa;
            dot_r += pr[k] * dpr[k];
            dot_a += pa[k] * dpa[k];
        }
#pragma unroll
        for (int k = 0; k < FIT_K; ++k) {
            fit_adamw(th_r[k], m_r[k], v_r[k], pr[k] * (dpr[k] - dot_r), decay, hy, ss, bs);
            fit_adamw(th_a[k], m_a[k], v_a[k], pa[k] * (dpa[k] - dot_a), decay, hy, ss, bs);
        }
    }
    if (owner && steps > 0) {
#pragma unroll
        for (int k = 0; k < FIT_K; ++k) {
            ref_logits[entry * FIT_K + k] = th_r[k];
            alt_logits[entry * FIT_K + k] = th_a[k];
        }
    }
}

extern "C" int pmt_downsample_fit(const float* counts_slvra, int32_t num_sources, const float* ref_trans_kry, const float* alt_trans_haz,
                                  float* ref_logits_slvrak, float* alt_logits_slvrah, int32_t steps, double lr, double beta1, double beta2,
                                  double eps, double weight_decay, float* loss_before_after, void* stream) {
    if (!counts_slvra || !ref_trans_kry || !alt_trans_haz || !ref_logits_slvrak || !alt_logits_slvrah) return PMT_E_INVALID;
    if (num_sources < 1 || steps < 0 || steps > PMT_FIT_MAX_STEPS) return PMT_E_INVALID;
    if (steps == 0 && loss_before_after == nullptr) return PMT_OK;
    const float decay = (float)(1.0 - lr * weight_decay);
    hipLaunchKernelGGL(pmt_downsample_fit_kernel, dim3((unsigned)num_sources * (FIT_L * FIT_V)), dim3(64), 0, reinterpret_cast<hipStream_t>(stream),
                       counts_slvra, ref_trans_kry, alt_trans_haz, ref_logits_slvrak, alt_logits_slvrah, (int)steps, fit_adam_hyper(lr, beta1, beta2, eps), decay, loss_before_after);
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}
