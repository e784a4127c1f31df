// Rank pruning of mislabeled data (reference tools/prune_dataset.py:30-164) from the artifact probabilities of one forward sweep:
// pmt_prune_thresholds replaces `calculate_pruning_thresholds` (two sweeps, a Python loop over every datum after each, a Python list
// of every agreement probability handed to torch.quantile), pmt_prune_select the keep / drop rule of `generated_pruned_data_for_fold`
// (a third sweep and loop).  Everything is a short chain of ordinary launches on the caller's stream; a stage reads what the one before
// left in device memory, and no workgroup ever waits for another.
//
// Classes: 1 = labeled artifact (Label 0), 0 = labeled non-artifact (Label 1), as the reference's confusion matrix numbers its rows.
// The agreement probability of a row is p under class 1 and 1 - p (fp32, as torch computes it) under class 0.
#include <hip/hip_runtime.h>
#include <math.h>

#include "permutect_amd.h"
#include "pmt_stats_device.hpp"

// ATen's rank, weight and interpolation are reproduced operation by operation: nothing here may be contracted into a fused multiply-add
// that the source does not spell fmaf (HIP's __fmul_rn / __fsub_rn are plain operators and do not prevent it)
#pragma clang fp contract(off)

#define PRUNE_THREADS 256
#define PRUNE_WAVES (PRUNE_THREADS / 64)
#define PRUNE_ITEMS 8
#define PRUNE_SPAN (PRUNE_THREADS * PRUNE_ITEMS)  // rows of one workgroup in one turn
#define PRUNE_MAX_GRID 1024                       // workgroups of the statistics' sweeps (grid-stride beyond)
#define PRUNE_PASSES 4
#define PRUNE_SCAN_THREADS 1024

// The fixed part of the scratch buffer; the selection's per-workgroup counts follow it.
struct PruneTarget {
    unsigned long long k;  // rank of the order statistic among the keys that still share `prefix`
    unsigned int prefix;   // the key's bits decided so far (the top 8 * pass bits)
    unsigned int active;
};
struct PruneScratch {
    double partial[PRUNE_MAX_GRID][2];
    unsigned long long hist[PRUNE_PASSES][2][2][256];  // [pass][class][0 floor(rank), 1 ceil(rank)][digit]
    PruneTarget target[PRUNE_PASSES + 1][2][2];        // [before pass][class][neighbour]
    double weight[2];                                   // rank - floor(rank)
    int wide[2];                                        // 1: the class has more than 2^24 rows (double arithmetic)
    int pad[2];
};

__device__ __forceinline__ long long prune_label(const PmtIntColumn& c, long long i) {
    return c.elem_bytes == 8 ? reinterpret_cast<const long long*>(c.ptr)[i * c.stride]
                             : (long long)reinterpret_cast<const int*>(c.ptr)[i * c.stride];
}
// -1 unlabeled, 0 non-artifact, 1 artifact
__device__ __forceinline__ int prune_class(long long label) { return label == 0 ? 1 : (label == 1 ? 0 : -1); }
// (+ 0.0f: 1 - 1 is +0 already, and a -0 that came in would order above every positive key)
__device__ __forceinline__ float prune_agreement(float p, int cls) { return (cls == 1 ? p : 1.0f - p) + 0.0f; }

static inline int prune_grid(long long n) {
    const long long g = (n + PRUNE_SPAN - 1) / PRUNE_SPAN;
    return (int)(g < 1 ? 1 : (g > PRUNE_MAX_GRID ? PRUNE_MAX_GRID : g));
}

// ---- stage 1: the confidence sums (double, one partial per workgroup) and the class counts -------------------------------------------
__global__ __launch_bounds__(PRUNE_THREADS) void prune_sums_kernel(PmtPruneArgs a, PmtPruneStats* __restrict__ stats,
                                                                   PruneScratch* __restrict__ sc) {
    __shared__ double sh_sum[PRUNE_WAVES][2];
    __shared__ unsigned int sh_count[2];
    if (threadIdx.x < 2) sh_count[threadIdx.x] = 0;
    __syncthreads();
    double sum[2] = {0.0, 0.0};
    unsigned int cnt[2] = {0, 0};
    for (long long i = (long long)blockIdx.x * PRUNE_THREADS + threadIdx.x; i < a.n; i += (long long)gridDim.x * PRUNE_THREADS) {
        const int cls = prune_class(prune_label(a.labels, i));
        if (cls < 0) continue;
        const double v = (double)prune_agreement(a.art_probs[i], cls);
        if (cls == 1) { sum[1] += v; cnt[1]++; } else { sum[0] += v; cnt[0]++; }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int c = 0; c < 2; ++c) {
        const double s = fit_sum64(sum[c]);
        if (lane == 0) sh_sum[wave][c] = s;
        if (cnt[c]) atomicAdd(&sh_count[c], cnt[c]);
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        double s = 0.0;
        for (int w = 0; w < PRUNE_WAVES; ++w) s += sh_sum[w][threadIdx.x];
        sc->partial[blockIdx.x][threadIdx.x] = s;
        if (sh_count[threadIdx.x])
            atomicAdd(reinterpret_cast<unsigned long long*>(&stats->count[threadIdx.x]), (unsigned long long)sh_count[threadIdx.x]);
    }
}

// ---- stage 2: fold the partials in workgroup order; StreamingAverage.get -------------------------------------------------------------
__global__ void prune_confidence_kernel(PmtPruneStats* __restrict__ stats, const PruneScratch* __restrict__ sc, int grid) {
    const int c = threadIdx.x;
    if (c >= 2) return;
    double s = 0.0;
    for (int b = 0; b < grid; ++b) s += sc->partial[b][c];
    stats->confidence_sum[c] = s;
    stats->confidence[c] = s / ((double)stats->count[c] + 1e-4);
}

// ---- stage 3: the confusion counts against the two confidences (fp32 comparisons) ----------------------------------------------------
__global__ __launch_bounds__(PRUNE_THREADS) void prune_confusion_kernel(PmtPruneArgs a, PmtPruneStats* __restrict__ stats) {
    __shared__ unsigned int sh[4];
    if (threadIdx.x < 4) sh[threadIdx.x] = 0;
    __syncthreads();
    const float art_conf = (float)stats->confidence[1], nonart_conf = (float)stats->confidence[0];
    unsigned int cnt[4] = {0, 0, 0, 0};
    for (long long i = (long long)blockIdx.x * PRUNE_THREADS + threadIdx.x; i < a.n; i += (long long)gridDim.x * PRUNE_THREADS) {
        const int cls = prune_class(prune_label(a.labels, i));
        if (cls < 0) continue;
        const float p = a.art_probs[i];
        if (p >= art_conf) cnt[cls * 2 + 1]++;
        if (1.0f - p >= nonart_conf) cnt[cls * 2 + 0]++;
    }
    for (int j = 0; j < 4; ++j)
        if (cnt[j]) atomicAdd(&sh[j], cnt[j]);
    __syncthreads();
    if (threadIdx.x < 4 && sh[threadIdx.x])
        atomicAdd(reinterpret_cast<unsigned long long*>(&stats->confusion[0][0]) + threadIdx.x, (unsigned long long)sh[threadIdx.x]);
}

// ---- stage 4: error rates, quantile levels, and the two ranks of each class ----------------------------------------------------------
__global__ void prune_rates_kernel(PmtPruneArgs a, PmtPruneStats* __restrict__ stats, PruneScratch* __restrict__ sc) {
    if (threadIdx.x != 0) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const long long n0 = stats->count[0], n1 = stats->count[1];
    const double f_art = a.label_art_frac, f_non = 1.0 - a.label_art_frac;
    int status = 0;
    if (n1 == 0 || (!a.levels_given && f_art == 0.0)) status |= PMT_PRUNE_NO_ARTIFACT;
    if (n0 == 0 || (!a.levels_given && f_non == 0.0)) status |= PMT_PRUNE_NO_NONARTIFACT;
    const long long c00 = stats->confusion[0][0], c01 = stats->confusion[0][1], c10 = stats->confusion[1][0], c11 = stats->confusion[1][1];
    double e_art = nan, e_non = nan, level[2] = {nan, nan};
    const bool columns = c01 + c11 > 0 && c00 + c10 > 0;
    if (columns) {
        e_art = (double)c01 / (double)(c01 + c11);
        e_non = (double)c10 / (double)(c00 + c10);
    } else if (!a.levels_given) {
        status |= PMT_PRUNE_CONFUSION_COLUMN;
    }
    if (a.levels_given) {
        level[0] = a.levels[0];
        level[1] = a.levels[1];
    } else if (status == 0) {
        const double denom = 1.0 - e_art - e_non;
        if (denom == 0.0) {
            status |= PMT_PRUNE_RATES_SUM_TO_ONE;
        } else {
            level[1] = (e_non / f_art) * (f_non - e_art) / denom;  // inv_art_error_rate
            level[0] = (e_art / f_non) * (f_art - e_non) / denom;  // inv_nonart_error_rate
        }
    }
    if (status == 0 && !(level[0] >= 0.0 && level[0] <= 1.0 && level[1] >= 0.0 && level[1] <= 1.0)) status |= PMT_PRUNE_LEVEL_RANGE;
    stats->error_rate[1] = e_art;
    stats->error_rate[0] = e_non;
    stats->inv_error_rate[0] = level[0];
    stats->inv_error_rate[1] = level[1];
    stats->status = status;
    for (int c = 0; c < 2; ++c) {
        const long long nc = c ? n1 : n0;
        long long lo = 0, hi = 0;
        double w = 0.0;
        int wide = 0;
        if (status == 0) {
            if (nc <= (1LL << 24)) {  // ATen: the level as a tensor of the input's dtype, times the last index, in fp32
                const float rank = (float)level[c] * (float)(nc - 1);
                const float below = floorf(rank);
                w = (double)(rank - below);
                lo = (long long)below;
                hi = (long long)ceilf(rank);
            } else {
                wide = 1;
                const double rank = level[c] * (double)(nc - 1);
                const double below = floor(rank);
                w = rank - below;
                lo = (long long)below;
                hi = (long long)ceil(rank);
            }
            lo = lo < 0 ? 0 : (lo > nc - 1 ? nc - 1 : lo);
            hi = hi < 0 ? 0 : (hi > nc - 1 ? nc - 1 : hi);
        }
        sc->weight[c] = w;
        sc->wide[c] = wide;
        sc->target[0][c][0] = PruneTarget{(unsigned long long)lo, 0u, status == 0 ? 1u : 0u};
        sc->target[0][c][1] = PruneTarget{(unsigned long long)hi, 0u, status == 0 ? 1u : 0u};
    }
}

// The four targets before pass `pass` from those before the pass in front of it and its histograms: the digit whose bin holds rank k.
// Every workgroup computes the same; the caller's workgroup 0 stores them.  Called by all PRUNE_THREADS threads; sh_hist is scratch.
__device__ __forceinline__ void prune_advance(const PruneScratch* __restrict__ sc, int pass, unsigned long long (*sh_hist)[256],
                                              PruneTarget* sh_target) {
    if (pass == 0) {
        if (threadIdx.x < 4) sh_target[threadIdx.x] = sc->target[0][threadIdx.x >> 1][threadIdx.x & 1];
        __syncthreads();
        return;
    }
    for (int j = threadIdx.x; j < 4 * 256; j += PRUNE_THREADS) sh_hist[j >> 8][j & 255] = (&sc->hist[pass - 1][0][0][0])[j];
    __syncthreads();
    if (threadIdx.x < 4) {
        PruneTarget t = sc->target[pass - 1][threadIdx.x >> 1][threadIdx.x & 1];
        if (t.active) {
            unsigned long long before = 0;
            int d = 0;
            for (; d < 255; ++d) {  // (the last bin takes whatever is left: d stays inside the histogram whatever the counts say)
                const unsigned long long h = sh_hist[threadIdx.x][d];
                if (t.k < before + h) break;
                before += h;
            }
            t.k -= before;
            t.prefix = (t.prefix << 8) | (unsigned int)d;
        }
        sh_target[threadIdx.x] = t;
    }
    __syncthreads();
}

// ---- stages 5 - 8: one radix pass: histogram of the next 8 bits over the keys that share a target's prefix ----------------------------
__global__ __launch_bounds__(PRUNE_THREADS) void prune_histogram_kernel(PmtPruneArgs a, PruneScratch* __restrict__ sc, int pass) {
    __shared__ unsigned long long sh_hist[4][256];
    __shared__ PruneTarget sh_target[4];
    __shared__ unsigned int sh_bins[4][256];
    prune_advance(sc, pass, sh_hist, sh_target);
    if (blockIdx.x == 0 && threadIdx.x < 4) sc->target[pass][threadIdx.x >> 1][threadIdx.x & 1] = sh_target[threadIdx.x];
    if (!sh_target[0].active) return;  // (a degenerate input: uniform over the grid)
    for (int j = threadIdx.x; j < 4 * 256; j += PRUNE_THREADS) sh_bins[j >> 8][j & 255] = 0;
    __syncthreads();
    const int shift = 24 - 8 * pass;  // this pass's digit; the bits above it are the prefix
    for (long long i = (long long)blockIdx.x * PRUNE_THREADS + threadIdx.x; i < a.n; i += (long long)gridDim.x * PRUNE_THREADS) {
        const int cls = prune_class(prune_label(a.labels, i));
        if (cls < 0) continue;
        const unsigned int key = __float_as_uint(prune_agreement(a.art_probs[i], cls));
        const unsigned int above = pass == 0 ? 0u : key >> (shift + 8);
        const unsigned int digit = (key >> shift) & 255u;
        if (above == sh_target[cls * 2].prefix) atomicAdd(&sh_bins[cls * 2][digit], 1u);
        if (above == sh_target[cls * 2 + 1].prefix) atomicAdd(&sh_bins[cls * 2 + 1][digit], 1u);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < 4 * 256; j += PRUNE_THREADS) {
        const unsigned int v = sh_bins[j >> 8][j & 255];
        if (v) atomicAdd(&sc->hist[pass][0][0][0] + j, (unsigned long long)v);
    }
}

// ---- stage 9: the selected keys are the order statistics; ATen's interpolation between them ------------------------------------------
__global__ __launch_bounds__(PRUNE_THREADS) void prune_thresholds_kernel(PmtPruneStats* __restrict__ stats, PruneScratch* __restrict__ sc) {
    __shared__ unsigned long long sh_hist[4][256];
    __shared__ PruneTarget sh_target[4];
    prune_advance(sc, PRUNE_PASSES, sh_hist, sh_target);
    if (threadIdx.x < 4) sc->target[PRUNE_PASSES][threadIdx.x >> 1][threadIdx.x & 1] = sh_target[threadIdx.x];
    if (threadIdx.x >= 2) return;
    const int c = threadIdx.x;
    float result = __uint_as_float(0x7fc00000u);
    if (sh_target[2 * c].active) {
        const float lo = __uint_as_float(sh_target[2 * c].prefix), hi = __uint_as_float(sh_target[2 * c + 1].prefix);
        if (!sc->wide[c]) {  // ATen's lerp (Lerp.h) as the CPU build contracts it
            const float w = (float)sc->weight[c], diff = hi - lo;
            result = fabsf(w) < 0.5f ? fmaf(w, diff, lo) : fmaf(-diff, 1.0f - w, hi);
        } else {
            const double w = sc->weight[c], diff = (double)hi - (double)lo;
            result = (float)((double)lo + w * diff);
        }
    }
    stats->threshold[c] = result;
}

extern "C" size_t pmt_prune_scratch_bytes(int64_t n) {
    const long long groups = n > 0 ? (n + PRUNE_SPAN - 1) / PRUNE_SPAN : 0;
    return sizeof(PruneScratch) + (size_t)(groups + 1) * sizeof(long long);
}

static int prune_args_check(const PmtPruneArgs* a) {
    if (!a || a->n < 0) return PMT_E_INVALID;
    if (a->n > 0 && (!a->art_probs || !a->labels.ptr || (a->labels.elem_bytes != 4 && a->labels.elem_bytes != 8))) return PMT_E_INVALID;
    return PMT_OK;
}

extern "C" int pmt_prune_thresholds(const PmtPruneArgs* args, PmtPruneStats* stats, void* scratch, void* stream) {
    if (prune_args_check(args) != PMT_OK || !stats || !scratch) return PMT_E_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PruneScratch* sc = reinterpret_cast<PruneScratch*>(scratch);
    const int grid = prune_grid(args->n);
    if (hipMemsetAsync(stats, 0, sizeof(PmtPruneStats), s) != hipSuccess) return PMT_E_LAUNCH;
    if (hipMemsetAsync(sc, 0, sizeof(PruneScratch), s) != hipSuccess) return PMT_E_LAUNCH;
    hipLaunchKernelGGL(prune_sums_kernel, dim3(grid), dim3(PRUNE_THREADS), 0, s, *args, stats, sc);
    hipLaunchKernelGGL(prune_confidence_kernel, dim3(1), dim3(64), 0, s, stats, sc, grid);
    hipLaunchKernelGGL(prune_confusion_kernel, dim3(grid), dim3(PRUNE_THREADS), 0, s, *args, stats);
    hipLaunchKernelGGL(prune_rates_kernel, dim3(1), dim3(64), 0, s, *args, stats, sc);
    for (int pass = 0; pass < PRUNE_PASSES; ++pass)
        hipLaunchKernelGGL(prune_histogram_kernel, dim3(grid), dim3(PRUNE_THREADS), 0, s, *args, sc, pass);
    hipLaunchKernelGGL(prune_thresholds_kernel, dim3(1), dim3(PRUNE_THREADS), 0, s, stats, sc);
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}

// ---- the selection: an ordered stream compaction ----------------------------------------------------------------------------------------
// Workgroup g owns rows [g * PRUNE_SPAN, (g + 1) * PRUNE_SPAN): turn t of wave w covers the 64 rows from (t * PRUNE_WAVES + w) * 64 of it,
// so (turn, wave, lane) ascends with the row.
__device__ __forceinline__ bool prune_keeps(const PmtPruneArgs& a, long long i, float art_threshold, float nonart_threshold) {
    const int cls = prune_class(prune_label(a.labels, i));
    if (cls < 0) return true;
    const float p = a.art_probs[i];
    return cls == 1 ? !(p < art_threshold) : !(1.0f - p < nonart_threshold);
}

__global__ __launch_bounds__(PRUNE_THREADS) void prune_count_kernel(PmtPruneArgs a, float art_threshold, float nonart_threshold,
                                                                    long long* __restrict__ group_count) {
    __shared__ unsigned int sh;
    if (threadIdx.x == 0) sh = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * PRUNE_SPAN;
    unsigned int cnt = 0;
    for (int t = 0; t < PRUNE_ITEMS; ++t) {
        const long long i = base + t * PRUNE_THREADS + threadIdx.x;
        if (i < a.n && prune_keeps(a, i, art_threshold, nonart_threshold)) cnt++;
    }
    if (cnt) atomicAdd(&sh, cnt);
    __syncthreads();
    if (threadIdx.x == 0) group_count[blockIdx.x] = sh;
}

// one workgroup: counts -> exclusive offsets in place, the total into *kept_count
__global__ __launch_bounds__(PRUNE_SCAN_THREADS) void prune_scan_kernel(long long* __restrict__ group_count, long long groups,
                                                                        long long* __restrict__ kept_count) {
    __shared__ long long sh_wave[PRUNE_SCAN_THREADS / 64];
    __shared__ long long sh_carry;
    if (threadIdx.x == 0) sh_carry = 0;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (long long start = 0; start < groups; start += PRUNE_SCAN_THREADS) {
        const long long g = start + threadIdx.x;
        const long long own = g < groups ? group_count[g] : 0;
        long long incl = own;
        for (int m = 1; m < 64; m <<= 1) {
            const long long up = __shfl_up(incl, m);
            if (lane >= m) incl += up;
        }
        if (lane == 63) sh_wave[wave] = incl;
        __syncthreads();
        long long before = sh_carry;
        for (int w = 0; w < wave; ++w) before += sh_wave[w];
        if (g < groups) group_count[g] = before + incl - own;
        __syncthreads();
        if (threadIdx.x == PRUNE_SCAN_THREADS - 1) sh_carry = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) *kept_count = sh_carry;
}

__global__ __launch_bounds__(PRUNE_THREADS) void prune_scatter_kernel(PmtPruneArgs a, float art_threshold, float nonart_threshold,
                                                                      const long long* __restrict__ group_offset,
                                                                      long long* __restrict__ kept_ids) {
    __shared__ unsigned int sh_cell[PRUNE_ITEMS * PRUNE_WAVES];  // kept rows of (turn, wave), then their exclusive scan
    const long long base = (long long)blockIdx.x * PRUNE_SPAN;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned long long ballots[PRUNE_ITEMS];
#pragma unroll
    for (int t = 0; t < PRUNE_ITEMS; ++t) {
        const long long i = base + t * PRUNE_THREADS + threadIdx.x;
        ballots[t] = __ballot(i < a.n && prune_keeps(a, i, art_threshold, nonart_threshold));
        if (lane == 0) sh_cell[t * PRUNE_WAVES + wave] = (unsigned int)__popcll(ballots[t]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int run = 0;
        for (int j = 0; j < PRUNE_ITEMS * PRUNE_WAVES; ++j) {
            const unsigned int c = sh_cell[j];
            sh_cell[j] = run;
            run += c;
        }
    }
    __syncthreads();
    const long long out = group_offset[blockIdx.x];
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
    for (int t = 0; t < PRUNE_ITEMS; ++t) {
        if ((ballots[t] >> lane) & 1ull) {
            // (a kept row's index in the output is at most the row itself: inside kept_ids [n])
            kept_ids[out + sh_cell[t * PRUNE_WAVES + wave] + __popcll(ballots[t] & below)] = base + t * PRUNE_THREADS + threadIdx.x;
        }
    }
}

extern "C" int pmt_prune_select(const PmtPruneArgs* args, float art_threshold, float nonart_threshold, int64_t* kept_ids, int64_t* kept_count,
                                void* scratch, void* stream) {
    if (prune_args_check(args) != PMT_OK || !kept_count || !scratch || (args->n > 0 && !kept_ids)) return PMT_E_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (args->n == 0) return hipMemsetAsync(kept_count, 0, sizeof(int64_t), s) == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
    const long long groups = (args->n + PRUNE_SPAN - 1) / PRUNE_SPAN;
    if (groups > 0x7fffffffLL) return PMT_E_UNSUPPORTED;
    long long* group_count = reinterpret_cast<long long*>(reinterpret_cast<char*>(scratch) + sizeof(PruneScratch));
    hipLaunchKernelGGL(prune_count_kernel, dim3((unsigned)groups), dim3(PRUNE_THREADS), 0, s, *args, art_threshold, nonart_threshold, group_count);
    hipLaunchKernelGGL(prune_scan_kernel, dim3(1), dim3(PRUNE_SCAN_THREADS), 0, s, group_count, groups, reinterpret_cast<long long*>(kept_count));
    hipLaunchKernelGGL(prune_scatter_kernel, dim3((unsigned)groups), dim3(PRUNE_THREADS), 0, s, *args, art_threshold, nonart_threshold,
                       group_count, reinterpret_cast<long long*>(kept_ids));
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}
