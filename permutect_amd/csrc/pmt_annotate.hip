// The site annotation of filter_variants (reference data/memory_mapped_data.py:131-175, tools/filter_variants.py:167-182, misc_utils.py
// `encode`): a lane per candidate rebuilds the reference's string key as a 32-bit number, looks it up in the sorted site table and looks
// the locus up in the two sorted segment tables (include/permutect_amd.h: PmtAnnotateArgs).  ONE launch.
//
// Every search runs a FIXED number of steps, ceil(log2(n + 1)), computed on the host, and a step is a clamped load and a select: no lane
// leaves a loop before another, so a wavefront never diverges over the lookups (the digit loops have fixed trip counts too).  The tables
// are read through the caches only: a 2^22-row site table is 71 MB, its top levels are shared by every lane.  Counts: ballots per
// wavefront, LDS integer atomics per workgroup, one 64-bit integer atomic per non-zero counter per workgroup.
#include <hip/hip_runtime.h>

#include "permutect_amd.h"
#include "pmt_annotate_device.hpp"

#define ANNOTATE_MAX_THREADS 1024
#define ANNOTATE_COUNTERS 6      // kept, excluded, unmatched, unknown contig (the host's), maf hits, normal-maf hits

// how many rows of the sorted site table lie before (locus, alt): `steps` = ceil(log2(n + 1)) probes, each a clamped load and a select
__device__ __forceinline__ long long annotate_site_lower_bound(const uint64_t* __restrict__ table_locus,
                                                               const unsigned int* __restrict__ table_alt, long long n, int steps,
                                                               unsigned long long locus, unsigned int alt) {
    long long base = 0;
    for (int s = steps - 1; s >= 0; --s) {
        const long long probe = base + (1LL << s);  // rows [0, probe) are all before the key iff row probe - 1 is
        const long long at = (probe <= n ? probe : n) - 1;
        const unsigned long long l = table_locus[at];
        const unsigned int a = table_alt[at];
        const bool before = l < locus || (l == locus && a < alt);
        base = (probe <= n && before) ? probe : base;
    }
    return base;
}
// how many rows of a sorted key column are at or before `key`
__device__ __forceinline__ long long annotate_upper_bound(const uint64_t* __restrict__ keys, long long n, int steps,
                                                          unsigned long long key) {
    long long base = 0;
    for (int s = steps - 1; s >= 0; --s) {
        const long long probe = base + (1LL << s);
        const long long at = (probe <= n ? probe : n) - 1;
        const bool at_or_before = keys[at] <= key;
        base = (probe <= n && at_or_before) ? probe : base;
    }
    return base;
}
// the maf of the segment that covers (contig, position), 0.5 when none does
__device__ __forceinline__ float annotate_segment(const uint64_t* __restrict__ start, const uint64_t* __restrict__ stop,
                                                  const float* __restrict__ maf, long long n, int steps, unsigned long long locus, bool& hit) {
    const long long after = annotate_upper_bound(start, n, steps, locus);
    hit = false;
    float answer = 0.5f;
    if (after > 0) {
        const long long p = after - 1;
        hit = (start[p] >> 32) == (locus >> 32) && (locus & 0xFFFFFFFFull) < stop[p];
        if (hit) answer = maf[p];
    }
    return answer;
}

__global__ __launch_bounds__(ANNOTATE_MAX_THREADS) void annotate_kernel(PmtAnnotateArgs a, int site_steps, int seg_steps, int normal_steps) {
    __shared__ unsigned int sh_count[ANNOTATE_COUNTERS];
    if (threadIdx.x < ANNOTATE_COUNTERS) sh_count[threadIdx.x] = 0u;
    __syncthreads();
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < a.num_candidates;
    bool kept = false, excluded = false, unmatched = false, maf_hit = false, normal_hit = false;
    if (valid) {
        const long long row = i * a.int_row_stride + a.first_column;  // CONTIG; POSITION +1/+2, REF_ALLELE_AS_BASE_5 +3/+4, ALT_ALLELE_AS_BASE_5 +5/+6
        long long c[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) c[j] = annotate_int(a.int_rows, row + j, a.int_elem_bytes);
        const unsigned int position = annotate_pair(c[1], c[2]);
        const unsigned long long locus = ((unsigned long long)(unsigned int)(int)c[0] << 32) | position;
        const unsigned int alt = annotate_allele_key(annotate_pair(c[3], c[4]), annotate_pair(c[5], c[6]));

        const long long at = annotate_site_lower_bound(a.site_locus, a.site_alt, a.n_sites, site_steps, locus, alt);
        bool found = false;
        float af = 0.0f;
        if (at < a.n_sites) {
            found = a.site_locus[at] == locus && a.site_alt[at] == alt;
            if (found) {
                excluded = a.site_excluded[at] != 0;
                af = a.site_af[at];
            }
        }
        kept = found && !excluded;
        unmatched = !found;
        a.allele_frequencies[i] = af;
        a.keep[i] = kept ? 1 : 0;
        a.mafs[i] = annotate_segment(a.seg_start, a.seg_stop, a.seg_maf, a.n_segments, seg_steps, locus, maf_hit);
        a.normal_mafs[i] = annotate_segment(a.normal_seg_start, a.normal_seg_stop, a.normal_seg_maf, a.n_normal_segments, normal_steps, locus, normal_hit);
    }
    // the counts: a ballot per wavefront, its first lane adds to the workgroup's, the workgroup adds what is not zero
    const bool flags[ANNOTATE_COUNTERS] = {kept, excluded, unmatched, false, maf_hit, normal_hit};
#pragma unroll
    for (int k = 0; k < ANNOTATE_COUNTERS; ++k) {
        const unsigned int in_wave = (unsigned int)__popcll(__ballot(flags[k]));
        if ((threadIdx.x & 63) == 0 && in_wave) atomicAdd(&sh_count[k], in_wave);
    }
    __syncthreads();
    if (threadIdx.x < ANNOTATE_COUNTERS && sh_count[threadIdx.x])
        atomicAdd(reinterpret_cast<unsigned long long*>(a.counters) + threadIdx.x, (unsigned long long)sh_count[threadIdx.x]);
}

static int annotate_steps(int64_t n) {  // ceil(log2(n + 1)): the smallest s with 2^s > n
    int s = 0;
    while ((1LL << s) <= n) ++s;
    return s;
}

extern "C" int pmt_annotate_sites(const PmtAnnotateArgs* args, void* stream) {
    const int64_t limit = 0x7fffffffLL;
    if (!args || args->num_candidates < 0 || args->num_candidates > limit) return PMT_E_INVALID;
    if (args->n_sites < 0 || args->n_sites > limit || args->n_segments < 0 || args->n_segments > limit || args->n_normal_segments < 0 ||
        args->n_normal_segments > limit)
        return PMT_E_INVALID;
    if (args->int_elem_bytes != 2 && args->int_elem_bytes != 4 && args->int_elem_bytes != 8) return PMT_E_INVALID;
    const int threads = args->threads_hint == 0 ? 256 : args->threads_hint;
    if (threads != 64 && threads != 128 && threads != 256 && threads != 512 && threads != 1024) return PMT_E_INVALID;
    if (args->n_sites > 0 && (!args->site_locus || !args->site_alt || !args->site_af || !args->site_excluded)) return PMT_E_INVALID;
    if (args->n_segments > 0 && (!args->seg_start || !args->seg_stop || !args->seg_maf)) return PMT_E_INVALID;
    if (args->n_normal_segments > 0 && (!args->normal_seg_start || !args->normal_seg_stop || !args->normal_seg_maf)) return PMT_E_INVALID;
    if (args->num_candidates == 0) return PMT_OK;  // (empty outputs may well be NULL)
    if (!args->allele_frequencies || !args->mafs || !args->normal_mafs || !args->keep || !args->counters) return PMT_E_INVALID;
    if (!args->int_rows || args->first_column < 0 || args->int_row_stride < (int64_t)args->first_column + 7) return PMT_E_INVALID;
    const unsigned int blocks = (unsigned int)((args->num_candidates + threads - 1) / threads);
    hipLaunchKernelGGL(annotate_kernel, dim3(blocks), dim3((unsigned)threads), 0, reinterpret_cast<hipStream_t>(stream), *args,
                       annotate_steps(args->n_sites), annotate_steps(args->n_segments), annotate_steps(args->n_normal_segments));
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}
