// A filtering run scored against truth labels (include/permutect_amd.h: pmt_posterior_evaluate; the torch form:
// permutect_amd/architecture/posterior_evaluation.py; reference tools/filter_variants.py:381-411, :534-588).
//
// A lane per candidate, persistent workgroups of four wavefronts walking the rows grid-stride.  The posterior is po_row<false>
// (pmt_posterior_device.hpp) behind a call (pe_posterior below), its five log posteriors are kept in double; softmax, error probability, error logit, calls, the
// correctness code and the bin indices are a few dozen operations behind it.  What is tallied is integers only:
//   * truth_hist (6300 cells), confusion (30), mistakes (25) and invalid (1) are COUNTS: a private 32-bit copy in LDS (25 KB) takes an
//     LDS atomic per row and is added to the caller's 64-bit words once per workgroup, cell by non-zero cell;
//   * call_hist (31500 cells of 2^-30 fixed point, 252 KB: no room in LDS) goes to memory, but a wavefront first sums the values of
//     lanes with EQUAL keys: the leader of every distinct key issues one 64-bit vector atomic.  Real data piles into few cells, so the
//     common case is one or two atomics per 64 rows instead of 64 on one word.
// Integer sums commute: the tables are the same bits for any grid, any slicing and from run to run.
#include "pmt_posterior_device.hpp"

#define PE_THREADS 256
#define PE_COUNTS (PMT_EVAL_CELLS + 5 * PMT_EVAL_LABELS * 2 + 5 * 5 + 1)  // truth_hist, then confusion, mistakes, invalid as in `tables`
static_assert(PMT_EVAL_MISTAKES == PMT_EVAL_CONFUSION + 30 && PMT_EVAL_INVALID == PMT_EVAL_MISTAKES + 25, "the small tables are contiguous");

// 21 bins of width 1 over [-10, 10], the ends clamped (reference data/count_binning.py:39-44).  (x is never NaN here.)
__device__ __forceinline__ int pe_logit_bin(float x) {
    return (int)floorf(fminf(fmaxf(x, -10.0f), 10.0f) + 10.0f);
}

// table[key] += val for every lane with key >= 0; lanes of one wavefront with equal keys add once.  Called by whole wavefronts.
__device__ __forceinline__ void pe_wave_add(unsigned long long* __restrict__ table, int key, unsigned long long val) {
    const int lane = threadIdx.x & (PO_WAVE - 1);
    unsigned long long todo = __ballot(key >= 0);
    while (todo) {  // (uniform over the wavefront)
        const int leader = __ffsll((long long)todo) - 1;
        const int k = __shfl(key, leader);
        const bool mine = key == k;
        const unsigned long long peers = __ballot(mine);
        unsigned long long v = mine ? val : 0ull;
        if (__popcll(peers) > 1) {
            for (int o = PO_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
        }
        if (lane == leader && v) atomicAdd(table + k, v);
        todo &= ~peers;
    }
}

// One candidate's log posteriors, behind a CALL.  Inlined into the persistent loop below, po_row's 198 registers became 390 (one
// wavefront per SIMD) and the pass took 1.78 x pmt_posterior_forward's time; as a call the kernel needs 248 (two per SIMD; the row and its
// five doubles cross on the stack, nothing spills) and takes 1.18 x (profiles/posterior_evaluation_device.txt).
__device__ __noinline__ void pe_posterior(const PmtPosteriorRows& rows, long long index, const PoShared& sh, const PmtPosteriorParams& P, PoRow& w,
                                          double* post) {
    w = po_load(rows, index);
    PoOut o;
    po_row<false>(w, sh, P, o, nullptr, nullptr);
    for (int c = 0; c < PO_CALLS; ++c) post[c] = o.post[c];
}

__global__ __launch_bounds__(PE_THREADS) void pmt_posterior_evaluate_kernel(PmtPosteriorRows rows, long long first, long long count,
                                                                           PmtPosteriorParams P, PmtPosteriorEvalArgs a) {
    __shared__ PoShared sh;
    __shared__ unsigned int counts[PE_COUNTS];
    for (int j = threadIdx.x; j < PE_COUNTS; j += PE_THREADS) counts[j] = 0u;
    po_prepare(sh, P.raw);  // (ends with a barrier)
    const int pass = a.passing_call;
    const long long stride = (long long)gridDim.x * PE_THREADS;
    for (long long base = (long long)blockIdx.x * PE_THREADS; base < count; base += stride) {  // (uniform over the workgroup)
        const long long i = base + threadIdx.x;
        int key = -1;
        unsigned long long val = 0ull;
        if (i < count) {
            PoRow w;
            PoOut o;
            pe_posterior(rows, first + i, sh, P, w, o.post);
            const int label = a.labels[first + i];
            bool valid = label >= 0 && label < PMT_EVAL_LABELS && w.logit == w.logit;
            double m = o.post[0];
            for (int c = 1; c < PO_CALLS; ++c) m = fmax(m, o.post[c]);
            double p[PO_CALLS], s = 0.0;
            for (int c = 0; c < PO_CALLS; ++c) {
                valid = valid && o.post[c] == o.post[c];
                p[c] = exp(o.post[c] - m);
                s += p[c];
            }
            for (int c = 0; c < PO_CALLS; ++c) {
                p[c] /= s;
                valid = valid && p[c] == p[c];
            }
            float ep = NAN, el = NAN, mp = NAN;
            int mc = -1, ec = -1, correctness = -1;
            bool filtered = false;
            if (valid) {
                mc = 0;
                for (int c = 1; c < PO_CALLS; ++c) mc = p[c] > p[mc] ? c : mc;
                mp = (float)p[mc];
                const double epd = 1.0 - p[pass];
                ep = (float)epd;
                const double clipped = 0.5 + 0.9999999 * (epd - 0.5);
                el = (float)log(clipped / (1.0 - clipped));
                const int t = w.type;
                filtered = a.filtered_in ? a.filtered_in[first + i] != 0 : ep > a.thresholds_v[t];
                if (filtered) {
                    for (int c = 0; c < PO_CALLS; ++c)
                        if (c != pass && (ec < 0 || p[c] > p[ec])) ec = c;
                }
                const bool ec_artifact = ec == PO_ARTIFACT || ec == PO_NORMAL_ARTIFACT;
                correctness = 0;
                if (label != 2) {
                    const bool correct = filtered ? label == 0 : label == 1;
                    if (correct) {
                        correctness = label == 1 ? 1 : (ec_artifact ? 2 : 0);
                    } else {
                        correctness = filtered ? (ec_artifact ? 3 : 0) : 4;
                        atomicAdd(&counts[PMT_EVAL_CELLS + 30 + (filtered ? ec : pass) * PO_TYPES + t], 1u);
                    }
                }
                const int ref_bin = min(max(w.depth - w.alt, 0), 10) / 3, alt_bin = (min(max(w.alt, 1), 15) - 1) / 3;
                const int cell = (((label * PO_TYPES + t) * PMT_EVAL_REF_BINS + ref_bin) * PMT_EVAL_ALT_BINS + alt_bin) * PMT_EVAL_LOGIT_BINS;
                if (label != 2) atomicAdd(&counts[cell + pe_logit_bin(el)], 1u);
                atomicAdd(&counts[PMT_EVAL_CELLS + (t * PMT_EVAL_LABELS + label) * 2 + (filtered ? 1 : 0)], 1u);
                key = mc * PMT_EVAL_CELLS + cell + pe_logit_bin(w.logit);
                val = (unsigned long long)llrintf(mp * (float)PMT_CONTEXT_FIXED_ONE);
            } else {
                atomicAdd(&counts[PE_COUNTS - 1], 1u);
            }
            if (a.error_probs_b) a.error_probs_b[i] = ep;
            if (a.error_logits_b) a.error_logits_b[i] = el;
            if (a.most_confident_call_b) a.most_confident_call_b[i] = mc;
            if (a.most_confident_prob_b) a.most_confident_prob_b[i] = mp;
            if (a.filtered_out_b) a.filtered_out_b[i] = filtered ? 1 : 0;
            if (a.error_call_b) a.error_call_b[i] = ec;
            if (a.correctness_b) a.correctness_b[i] = correctness;
        }
        pe_wave_add(a.tables + PMT_EVAL_CALL_HIST, key, val);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < PE_COUNTS; j += PE_THREADS) {
        const unsigned int c = counts[j];
        if (c) atomicAdd(a.tables + (j < PMT_EVAL_CELLS ? PMT_EVAL_TRUTH_HIST + j : PMT_EVAL_CONFUSION + (j - PMT_EVAL_CELLS)), (unsigned long long)c);
    }
}

extern "C" int pmt_posterior_evaluate(const PmtPosteriorRows* rows, int64_t first, int64_t count, const PmtPosteriorParams* params,
                                      const PmtPosteriorEvalArgs* args, void* stream) {
    const int rc = po_check(rows, first, count, params);
    if (rc != PMT_OK) return rc;
    if (!args || !args->labels || !args->thresholds_v || !args->tables) return PMT_E_INVALID;
    if ((args->passing_call != PO_SOMATIC && args->passing_call != PO_GERMLINE) || args->num_workgroups < 0) return PMT_E_INVALID;
    if (count == 0) return PMT_OK;
    const int64_t needed = (count + PE_THREADS - 1) / PE_THREADS;
    int64_t blocks = args->num_workgroups;
    if (blocks == 0) {  // two workgroups per compute unit: eight wavefronts, 2 x 32 KB of LDS
        static int cus = 0;
        if (cus == 0) {
            int dev = 0, n = 0;
            if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
            cus = n > 0 ? n : 256;
        }
        blocks = 2 * (int64_t)cus;
    }
    if (blocks > needed) blocks = needed;
    if ((needed + blocks - 1) / blocks > 0xffffffffLL / PE_THREADS) return PMT_E_INVALID;  // a workgroup's 32-bit counts
    hipLaunchKernelGGL(pmt_posterior_evaluate_kernel, dim3((unsigned)blocks), dim3(PE_THREADS), 0, reinterpret_cast<hipStream_t>(stream), *rows,
                       (long long)first, (long long)count, *params, *args);
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}
