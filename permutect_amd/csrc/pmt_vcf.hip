// The filtered VCF of filter_variants (reference tools/filter_variants.py:369-617 `apply_filtering_to_vcf`; the rule is stated once in
// include/permutect_amd.h: PmtVcfArgs).  The reference builds a Datum and a PosteriorResult per candidate, a dict keyed by the string
// `contig:pos:alt`, and per cyvcf2 record does a lookup, 21 "{:.3f}".format calls, a torch.topk and a set of filter names.  Here:
//   pmt_site_keys   a lane per candidate: the identity columns as (locus, allele key) -- the key of pmt_annotate_sites, one definition
//                   (pmt_annotate_device.hpp);
//   pmt_vcf_match   a lane per record: a FIXED number of probes of the candidates' keys sorted by (locus, key, row) finds the last of
//                   equal keys;
//   pmt_vcf_plan    a lane per record: the filter mask, the error call and the exact byte length of the output line (the 21 roundings
//                   with their carries), and the counters;
//   pmt_vcf_write   a wavefront per record: lanes 0 .. 20 format a value each into LDS at the place a shuffle prefix sum gives them,
//                   lane 21 spells the FILTER text, then the 64 lanes copy the line's five pieces with consecutive lanes on consecutive
//                   bytes (global loads and stores of a wavefront then fall into one or two 64-byte lines).
// Integer arithmetic only (the one float operation is the comparison of two probabilities), so every output byte is the same for any workgroup size, any
// slab and from run to run.  Plain C++; counts as in pmt_annotate.hip (ballots, LDS atomics, one 64-bit atomic per non-zero counter per
// workgroup).
#include <hip/hip_runtime.h>

#include "permutect_amd.h"
#include "pmt_annotate_device.hpp"

#define VCF_MAX_THREADS 1024
#define VCF_APPEND_MAX 512  // 53 literal bytes + 21 numbers of a sign, 19 digits (q < 1000 * 2^53 < 10^19) and a point at most = 494
#define VCF_FILTER_MAX 64   // contamination;slippage;normal_artifact = 38
#define VCF_NUM_CALLS 5
#define VCF_FINITE 0
#define VCF_NAN 1
#define VCF_INF 2
#define VCF_UNFORMATTABLE 3

__constant__ char VCF_NAMES[7][16] = {"contamination", "slippage", "somatic", "artifact", "seq_error", "germline", "normal_artifact"};
__constant__ int VCF_NAME_LENGTH[7] = {13, 8, 7, 8, 9, 8, 15};
__constant__ char VCF_INFO_KEYS[5][9] = {";POST=", ";PRIOR=", ";SPECLL=", ";ARTLOD=", ";NORMLL="};
__constant__ int VCF_INFO_KEY_LENGTH[5] = {6, 7, 8, 8, 8};

struct VcfNumber {
    unsigned long long q;  // round_half_even(|x| * 1000)
    int kind, negative, digits, length;
};

// "{:.3f}".format(float(x)) of a float32 in integers (include/permutect_amd.h)
__device__ __forceinline__ VcfNumber vcf_number(unsigned int bits) {
    VcfNumber n;
    n.negative = (int)(bits >> 31);
    n.q = 0;
    n.digits = 0;
    const int exponent = (int)((bits >> 23) & 255u);
    const unsigned int fraction = bits & 0x7FFFFFu;
    if (exponent == 255) {
        n.kind = fraction ? VCF_NAN : VCF_INF;
        n.length = fraction ? 3 : 3 + n.negative;
        return n;
    }
    if (exponent >= 127 + 53) {  // |x| >= 2^53
        n.kind = VCF_UNFORMATTABLE;
        n.length = 0;
        return n;
    }
    n.kind = VCF_FINITE;
    const unsigned long long m = (unsigned long long)(exponent ? (fraction | 0x800000u) : fraction) * 1000ull;  // below 2^34
    const int e = exponent ? exponent - 150 : -149;
    if (e >= 0) {
        n.q = m << e;  // e <= 29: below 2^63
    } else if (e > -64) {
        const int s = -e;
        const unsigned long long remainder = m & ((1ull << s) - 1ull), half = 1ull << (s - 1);
        n.q = m >> s;
        n.q += (remainder > half || (remainder == half && (n.q & 1ull))) ? 1ull : 0ull;
    }
    n.digits = 4;
    for (unsigned long long p = 10000ull; n.q >= p; p *= 10ull) ++n.digits;  // (q < 10^19 < 2^64: p never wraps before the loop ends)
    n.length = n.negative + n.digits + 1;
    return n;
}

// the text of a number, written backwards from its last byte at `end`
__device__ __forceinline__ void vcf_spell(const VcfNumber& n, unsigned char* end) {
    if (n.kind == VCF_NAN) {
        end[-2] = 'n', end[-1] = 'a', end[0] = 'n';
    } else if (n.kind == VCF_INF) {
        end[-2] = 'i', end[-1] = 'n', end[0] = 'f';
        if (n.negative) end[-3] = '-';
    } else if (n.kind == VCF_FINITE) {
        unsigned long long q = n.q;
        for (int k = 0; k < n.digits; ++k) {
            if (k == 3) *end-- = '.';
            *end-- = (unsigned char)('0' + (int)(q % 10ull));
            q /= 10ull;
        }
        if (n.negative) *end = '-';
    }
}

// value j of the 21 stands behind this literal: the key of its field, or a comma
__device__ __forceinline__ int vcf_literal(int j, int& key) {
    key = j < 5 ? 0 : (j < 10 ? 1 : (j < 15 ? 2 : (j == 15 ? 3 : 4)));
    const bool first = j == 0 || j == 5 || j == 10 || j == 15 || j == 16;
    if (!first) key = -1;
    return first ? VCF_INFO_KEY_LENGTH[key] : 1;
}

__device__ __forceinline__ int vcf_filter_length(unsigned int mask) {
    if (mask == 0u) return 4;  // PASS
    int length = -1;
#pragma unroll
    for (int k = 0; k < 7; ++k) length += ((mask >> k) & 1u) ? VCF_NAME_LENGTH[k] + 1 : 0;
    return length;
}

// how many entries of the candidates' sorted keys are at or before (locus, key): `steps` probes, each a clamped load and a select
__device__ __forceinline__ long long vcf_upper_bound(const uint64_t* __restrict__ cand_locus, const unsigned int* __restrict__ cand_key, long long n,
                                                     int steps, unsigned long long locus, unsigned int key) {
    long long base = 0;
    for (int s = steps - 1; s >= 0; --s) {
        const long long probe = base + (1LL << s);
        const long long at = (probe <= n ? probe : n) - 1;
        const unsigned long long l = cand_locus[at];
        const unsigned int k = cand_key[at];
        const bool at_or_before = l < locus || (l == locus && k <= key);
        base = (probe <= n && at_or_before) ? probe : base;
    }
    return base;
}

__global__ __launch_bounds__(VCF_MAX_THREADS) void vcf_site_keys_kernel(PmtSiteKeysArgs a) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.num_candidates) return;
    const long long row = i * a.int_row_stride + a.first_column;
    long long c[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) c[j] = annotate_int(a.int_rows, row + j, a.int_elem_bytes);
    a.locus[i] = ((unsigned long long)(unsigned int)(int)c[0] << 32) | annotate_pair(c[1], c[2]);
    a.allele_key[i] = annotate_allele_key(annotate_pair(c[3], c[4]), annotate_pair(c[5], c[6]));
}

__global__ __launch_bounds__(VCF_MAX_THREADS) void vcf_match_kernel(PmtVcfArgs a, int steps) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.num_records) return;
    int row = -1;
    const unsigned int flags = a.rec_flags[i];
    if ((flags & PMT_VCF_HAS_KEY) && !(flags & PMT_VCF_VERBATIM) && a.num_candidates > 0) {
        const unsigned long long locus = a.rec_locus[i];
        const unsigned int key = a.rec_key[i];
        const long long after = vcf_upper_bound(a.cand_locus, a.cand_key, a.num_candidates, steps, locus, key);
        if (after > 0 && a.cand_locus[after - 1] == locus && a.cand_key[after - 1] == key) row = (int)a.cand_row[after - 1];
    }
    a.matched[i] = row;
}

__global__ __launch_bounds__(VCF_MAX_THREADS) void vcf_plan_kernel(PmtVcfArgs a) {
    __shared__ unsigned int sh_count[PMT_VCF_COUNTERS];
    if (threadIdx.x < PMT_VCF_COUNTERS) sh_count[threadIdx.x] = 0u;
    __syncthreads();
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned int counts[PMT_VCF_COUNTERS];
#pragma unroll
    for (int k = 0; k < PMT_VCF_COUNTERS; ++k) counts[k] = 0u;
    if (i < a.num_records) {
        const unsigned int flags = a.rec_flags[i];
        const long long line_length = a.line_start[i + 1] - a.line_start[i];
        unsigned int mask = 0u;
        int error_call = -1;
        long long length = line_length;
        if (!(flags & PMT_VCF_VERBATIM)) {
            const int row = a.matched[i];
            mask = flags & (PMT_VCF_CONTAMINATION | PMT_VCF_SLIPPAGE);
            if (row >= 0 && row < a.num_candidates) {
                const float* values = a.values + (long long)row * PMT_VCF_VALUES;
                int append = 0;
                for (int j = 0; j < PMT_VCF_VALUES; ++j) {
                    int key;
                    const VcfNumber n = vcf_number(__float_as_uint(values[j]));
                    append += vcf_literal(j, key) + n.length;
                    counts[11] += n.kind == VCF_UNFORMATTABLE;
                }
                length += append - ((flags & PMT_VCF_INFO_DOT) ? 2 : 0);
                if (a.filtered[row]) {
                    float best = 0.0f;
                    for (int c = 0; c < VCF_NUM_CALLS; ++c) {  // first_argmax over the calls that are not the passing one
                        const float p = values[c];
                        if (c != a.passing_call && (error_call < 0 || p > best)) error_call = c, best = p;
                    }
                    mask |= 4u << error_call;
                }
                counts[0] = 1u;
                counts[10] = a.rec_variation[i] != a.variant_types[row];
            } else {
                counts[1] = 1u;
                if (flags & PMT_VCF_ZERO_ALT_DEPTH) mask |= 4u << 2, counts[2] = 1u;  // Call.SEQ_ERROR
            }
            length += vcf_filter_length(mask) - (long long)(a.filter_end[i] - a.filter_begin[i]);
            counts[3] = mask == 0u;
#pragma unroll
            for (int c = 0; c < VCF_NUM_CALLS; ++c) counts[4 + c] = (mask >> (2 + c)) & 1u;
            counts[9] = (mask & 3u) != 0u;
        }
        a.mask[i] = (uint8_t)mask;
        a.error_call[i] = (int8_t)error_call;
        a.out_length[i] = length;
    }
#pragma unroll
    for (int k = 0; k < PMT_VCF_COUNTERS; ++k) {
        unsigned int in_wave = counts[k];  // (unformattable values: up to 21 per lane, so a sum, not a ballot)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) in_wave += __shfl_xor(in_wave, d, 64);
        if ((threadIdx.x & 63) == 0 && in_wave) atomicAdd(&sh_count[k], in_wave);
    }
    __syncthreads();
    if (threadIdx.x < PMT_VCF_COUNTERS && sh_count[threadIdx.x])
        atomicAdd(reinterpret_cast<unsigned long long*>(a.counters) + threadIdx.x, (unsigned long long)sh_count[threadIdx.x]);
}

__global__ __launch_bounds__(VCF_MAX_THREADS) void vcf_write_kernel(PmtVcfArgs a) {
    __shared__ unsigned char sh_append[VCF_MAX_THREADS / 64][VCF_APPEND_MAX];
    __shared__ unsigned char sh_filter[VCF_MAX_THREADS / 64][VCF_FILTER_MAX];
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const long long slot = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
    const bool valid = slot < a.count;
    const long long i = a.first_record + (valid ? slot : 0);
    const unsigned int flags = valid ? a.rec_flags[i] : (unsigned int)PMT_VCF_VERBATIM;
    const bool verbatim = (flags & PMT_VCF_VERBATIM) != 0u;
    const int row = verbatim ? -1 : a.matched[i];
    const bool matched = row >= 0 && row < a.num_candidates;
    const unsigned int mask = verbatim ? 0u : a.mask[i];

    // lanes 0 .. 20: a value each, behind its literal; an inclusive prefix sum over the wavefront places them
    VcfNumber number;
    number.kind = VCF_UNFORMATTABLE, number.length = 0, number.negative = 0, number.digits = 0, number.q = 0;
    int key = -1, literal = 0;
    if (matched && lane < PMT_VCF_VALUES) {
        number = vcf_number(__float_as_uint(a.values[(long long)row * PMT_VCF_VALUES + lane]));
        literal = vcf_literal(lane, key);
    }
    const int mine = literal + number.length;
    int upto = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int below = __shfl_up(upto, d, 64);
        upto += lane >= d ? below : 0;
    }
    const int append_length = __shfl(upto, 63, 64);
    if (mine > 0) {
        unsigned char* at = &sh_append[wave][upto - mine];
        if (key >= 0) {
            for (int k = 0; k < literal; ++k) at[k] = (unsigned char)VCF_INFO_KEYS[key][k];
        } else {
            at[0] = ',';
        }
        if (number.length > 0) vcf_spell(number, at + mine - 1);
    }
    const int filter_length = verbatim ? 0 : vcf_filter_length(mask);
    if (lane == PMT_VCF_VALUES && !verbatim) {
        unsigned char* at = sh_filter[wave];
        if (mask == 0u) {
            at[0] = 'P', at[1] = 'A', at[2] = 'S', at[3] = 'S';
        } else {
            bool first = true;
            for (int k = 0; k < 7; ++k) {
                if (!((mask >> k) & 1u)) continue;
                if (!first) *at++ = ';';
                first = false;
                for (int c = 0; c < VCF_NAME_LENGTH[k]; ++c) *at++ = (unsigned char)VCF_NAMES[k][c];
            }
        }
    }
    __syncthreads();  // (every wavefront of the workgroup arrives: nothing above returns)
    if (!valid) return;

    // the output line: [line begin, FILTER) | the FILTER text | [the tab behind FILTER, INFO's end) | the appended text | the rest
    const long long line = a.line_start[i], line_length = a.line_start[i + 1] - line;
    const long long filter_begin = verbatim ? line_length : a.filter_begin[i], filter_end = verbatim ? line_length : a.filter_end[i];
    const long long info_end = verbatim ? line_length : a.info_end[i];
    const bool dot = matched && (flags & PMT_VCF_INFO_DOT);            // `\t.` becomes `\t`, the text loses its leading `;`
    const long long middle = (dot ? filter_end + 1 : info_end) - filter_end;
    const long long skip = dot ? 1 : 0, appended = matched ? append_length - skip : 0;
    const long long p1 = filter_begin, p2 = p1 + filter_length, p3 = p2 + middle, p4 = p3 + appended;
    const long long total = p4 + (line_length - info_end);
    const long long source = line - a.text_base, target = a.out_start[i] - a.out_base;
    const long long room = a.out_start[i + 1] - a.out_start[i];
    for (long long p = lane; p < total && p < room; p += 64) {
        long long from = -1;
        unsigned char byte = 0;
        if (p < p1) from = source + p;
        else if (p < p2) byte = sh_filter[wave][p - p1];
        else if (p < p3) from = source + filter_end + (p - p2);
        else if (p < p4) byte = sh_append[wave][skip + (p - p3)];
        else from = source + info_end + (p - p4);
        const bool from_text = p < p1 || (p >= p2 && p < p3) || p >= p4;
        if (from_text) {
            if (from < 0 || from >= a.text_bytes) continue;
            byte = a.text[from];
        }
        const long long to = target + p;
        if (to >= 0 && to < a.out_bytes) a.out[to] = byte;
    }
}

static int vcf_steps(int64_t n) {  // ceil(log2(n + 1)): the smallest s with 2^s > n
    int s = 0;
    while ((1LL << s) <= n) ++s;
    return s;
}
static bool vcf_threads(int hint, int* threads) {
    *threads = hint == 0 ? 256 : hint;
    return *threads == 64 || *threads == 128 || *threads == 256 || *threads == 512 || *threads == 1024;
}
static const int64_t VCF_LIMIT = 0x7fffffffLL;

extern "C" int pmt_site_keys(const PmtSiteKeysArgs* args, void* stream) {
    int threads;
    if (!args || args->num_candidates < 0 || args->num_candidates > VCF_LIMIT || !vcf_threads(args->threads_hint, &threads)) return PMT_E_INVALID;
    if (args->int_elem_bytes != 2 && args->int_elem_bytes != 4 && args->int_elem_bytes != 8) return PMT_E_INVALID;
    if (args->num_candidates == 0) return PMT_OK;
    if (!args->int_rows || !args->locus || !args->allele_key || args->first_column < 0 || args->int_row_stride < (int64_t)args->first_column + 7)
        return PMT_E_INVALID;
    const unsigned int blocks = (unsigned int)((args->num_candidates + threads - 1) / threads);
    hipLaunchKernelGGL(vcf_site_keys_kernel, dim3(blocks), dim3((unsigned)threads), 0, reinterpret_cast<hipStream_t>(stream), *args);
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}

// what match, plan and write share: sizes, the workgroup size, the record table
static int vcf_check(const PmtVcfArgs* a, int* threads) {
    if (!a || a->num_records < 0 || a->num_records > VCF_LIMIT || a->num_candidates < 0 || a->num_candidates > VCF_LIMIT) return PMT_E_INVALID;
    if (!vcf_threads(a->threads_hint, threads) || a->passing_call < 0 || a->passing_call >= VCF_NUM_CALLS) return PMT_E_INVALID;
    return PMT_OK;
}

extern "C" int pmt_vcf_match(const PmtVcfArgs* args, void* stream) {
    int threads;
    if (vcf_check(args, &threads) != PMT_OK) return PMT_E_INVALID;
    if (args->num_records == 0) return PMT_OK;
    if (!args->rec_locus || !args->rec_key || !args->rec_flags || !args->matched) return PMT_E_INVALID;
    if (args->num_candidates > 0 && (!args->cand_locus || !args->cand_key || !args->cand_row)) return PMT_E_INVALID;
    const unsigned int blocks = (unsigned int)((args->num_records + threads - 1) / threads);
    hipLaunchKernelGGL(vcf_match_kernel, dim3(blocks), dim3((unsigned)threads), 0, reinterpret_cast<hipStream_t>(stream), *args,
                       vcf_steps(args->num_candidates));
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}

extern "C" int pmt_vcf_plan(const PmtVcfArgs* args, void* stream) {
    int threads;
    if (vcf_check(args, &threads) != PMT_OK) return PMT_E_INVALID;
    if (args->num_records == 0) return PMT_OK;
    if (!args->line_start || !args->filter_begin || !args->filter_end || !args->rec_flags || !args->rec_variation || !args->matched) return PMT_E_INVALID;
    if (!args->mask || !args->error_call || !args->out_length || !args->counters) return PMT_E_INVALID;
    if (args->num_candidates > 0 && (!args->values || !args->filtered || !args->variant_types)) return PMT_E_INVALID;
    const unsigned int blocks = (unsigned int)((args->num_records + threads - 1) / threads);
    hipLaunchKernelGGL(vcf_plan_kernel, dim3(blocks), dim3((unsigned)threads), 0, reinterpret_cast<hipStream_t>(stream), *args);
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}

extern "C" int pmt_vcf_write(const PmtVcfArgs* args, void* stream) {
    int threads;
    if (vcf_check(args, &threads) != PMT_OK) return PMT_E_INVALID;
    if (args->first_record < 0 || args->count < 0 || args->first_record > args->num_records || args->count > args->num_records - args->first_record)
        return PMT_E_INVALID;
    if (args->text_bytes < 0 || args->out_bytes < 0) return PMT_E_INVALID;
    if (args->count == 0) return PMT_OK;
    if (!args->line_start || !args->filter_begin || !args->filter_end || !args->info_end || !args->rec_flags || !args->matched || !args->mask ||
        !args->out_start)
        return PMT_E_INVALID;
    if ((args->text_bytes > 0 && !args->text) || (args->out_bytes > 0 && !args->out)) return PMT_E_INVALID;
    if (args->num_candidates > 0 && !args->values) return PMT_E_INVALID;
    const int64_t per_block = threads / 64;
    const unsigned int blocks = (unsigned int)((args->count + per_block - 1) / per_block);
    hipLaunchKernelGGL(vcf_write_kernel, dim3(blocks), dim3((unsigned)threads), 0, reinterpret_cast<hipStream_t>(stream), *args);
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}
