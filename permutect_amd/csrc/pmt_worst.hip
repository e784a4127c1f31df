// The worst offenders of an evaluation pass (reference training/model_training.py:232-268): per (true label, alt-count bin) the
// queue_size labeled variants the model contradicts most confidently, kept as a table in device memory in CANONICAL FORM (every key's
// slots sorted, unused slots zero: include/permutect_amd.h), so that the table's bytes are a function of the multiset of recorded rows.
//
// pmt_worst_record is two ordinary launches on the caller's stream.  worst_filter_kernel (a grid over the rows) rejects a row with one
// compare against its key's cut and leaves the survivors of each workgroup in that workgroup's OWN segment of the scratch, with their
// number -- every segment's count is stored by its workgroup on every call, so the scratch needs no initialisation and no counter is
// shared.  worst_sort_kernel (a workgroup per key) gathers its key's survivors from all segments and sorts them with the kept slots in
// LDS.  Which workgroup ran first decides nothing: the order inside a segment and inside the LDS buffer is arbitrary (LDS integer
// atomics hand out the places) and the sort, a TOTAL order in which equal records are equal in every word, removes it.
#include <hip/hip_runtime.h>

#include "permutect_amd.h"

#define WORST_THREADS 256
#define WORST_ITEMS 4
#define WORST_SPAN (WORST_THREADS * WORST_ITEMS)  // rows of one workgroup of the filter = records of one scratch segment
#define WORST_CAP 2048                            // records of one LDS pass: 5 words each, 40 KB
#define WORST_WORDS 5                             // confidence bits, contig, position, ref code, alt code
#define WORST_FIRST_COLUMN 9                      // CONTIG; POSITION 10/11, REF_ALLELE_AS_BASE_5 12/13, ALT_ALLELE_AS_BASE_5 14/15

static_assert(PMT_WORST_MAX_QUEUE + WORST_THREADS <= WORST_CAP, "a pass must take a full queue and one sweep of the workgroup");
static_assert(2 * PMT_WORST_MAX_QUEUE <= WORST_CAP, "a merge sorts two full queues in one pass");

struct WorstRecord {
    unsigned int w[WORST_WORDS];
};

// the table's regions (32-bit words)
__host__ __device__ static inline size_t worst_fill_at(int key) { return (size_t)PMT_WORST_HEADER_WORDS + (size_t)key; }
__host__ __device__ static inline size_t worst_slot_at(int num_keys, int queue_size, int key, int slot) {
    return (size_t)PMT_WORST_HEADER_WORDS + (size_t)num_keys + ((size_t)key * queue_size + slot) * WORST_WORDS;
}
// the scratch's regions for `segments` segments: counts [segments], keys [segments * SPAN], then the five record words, each [segments * SPAN]
static inline size_t worst_scratch_words(long long segments) { return (size_t)segments * (1 + (size_t)WORST_SPAN * (1 + WORST_WORDS)); }
static inline long long worst_segments(long long n) { return (n + WORST_SPAN - 1) / WORST_SPAN; }

__device__ __forceinline__ long long worst_column(const PmtIntColumn& c, long long i) {
    return c.elem_bytes == 8 ? reinterpret_cast<const long long*>(c.ptr)[i * c.stride]
                             : (long long)reinterpret_cast<const int*>(c.ptr)[i * c.stride];
}
__device__ __forceinline__ long long worst_int(const void* rows, long long at, int elem_bytes) {
    return elem_bytes == 8 ? reinterpret_cast<const long long*>(rows)[at]
                           : (elem_bytes == 4 ? (long long)reinterpret_cast<const int*>(rows)[at] : (long long)reinterpret_cast<const short*>(rows)[at]);
}
// reference data/datum.py:46-48 (BIGGEST_UINT16 = 65535 is the multiplier), in 32 bits
__device__ __forceinline__ unsigned int worst_pair(long long hi, long long lo) {
    return 65535u * (unsigned int)(hi + 32768) + (unsigned int)(lo + 32768);
}

// a in front of b: confidence descending, then contig (signed), position, ref code, alt code ascending
__device__ __forceinline__ bool worst_before(const WorstRecord& a, const WorstRecord& b) {
    if (a.w[0] != b.w[0]) return a.w[0] > b.w[0];
    if (a.w[1] != b.w[1]) return (int)a.w[1] < (int)b.w[1];
    if (a.w[2] != b.w[2]) return a.w[2] < b.w[2];
    if (a.w[3] != b.w[3]) return a.w[3] < b.w[3];
    return a.w[4] < b.w[4];
}

// ---- launch 1: predicate, key, the compare against the cut, the survivors into this workgroup's segment --------------------------------
__global__ __launch_bounds__(WORST_THREADS) void worst_filter_kernel(PmtWorstArgs a, unsigned int* __restrict__ table,
                                                                     unsigned int* __restrict__ scratch, long long segments) {
    __shared__ unsigned int sh_kept, sh_beyond, sh_wrong[2];
    __shared__ int sh_max_alt;
    if (threadIdx.x == 0) {
        sh_kept = sh_beyond = sh_wrong[0] = sh_wrong[1] = 0;
        sh_max_alt = 0;
    }
    __syncthreads();
    const int num_keys = 2 * a.num_alt_keys;
    const size_t cap = (size_t)segments * WORST_SPAN;
    unsigned int* seg_keys = scratch + segments + (size_t)blockIdx.x * WORST_SPAN;
    unsigned int* seg_words = scratch + segments + cap + (size_t)blockIdx.x * WORST_SPAN;  // word f of record j at seg_words[f * cap + j]
    const long long base = (long long)blockIdx.x * WORST_SPAN;
    int max_alt = 0;
#pragma unroll
    for (int t = 0; t < WORST_ITEMS; ++t) {
        const long long i = base + t * WORST_THREADS + threadIdx.x;
        if (i >= a.num_variants) continue;
        const long long label = worst_column(a.labels, i);
        const long long alt_ll = worst_column(a.alt_counts, i);
        const int alt = alt_ll > 0x7fffffffLL ? 0x7fffffff : (alt_ll < 0 ? 0 : (int)alt_ll);
        max_alt = alt > max_alt ? alt : max_alt;
        const float logit = a.logits_b[i];
        const bool wrong = (label == 0 && logit < 0.0f) || (label == 1 && logit > 0.0f);  // (false for a NaN and for either zero)
        if (!wrong) continue;
        atomicAdd(&sh_wrong[label], 1u);
        const long long bin = alt_ll >= 1 ? (alt_ll - 1) / 3 : -1;
        if (bin < 0 || bin >= a.num_alt_keys) {
            atomicAdd(&sh_beyond, 1u);
            continue;
        }
        const int key = (int)label * a.num_alt_keys + (int)bin;
        const unsigned int conf = __float_as_uint(fabsf(logit));
        // the ONE compare of a late batch: the key is full and the row is below its last slot
        if (table[worst_fill_at(key)] == (unsigned int)a.queue_size &&
            conf < table[worst_slot_at(num_keys, a.queue_size, key, a.queue_size - 1)]) continue;
        const long long row = i * a.int_row_stride + WORST_FIRST_COLUMN;
        long long c[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) c[j] = worst_int(a.int_rows, row + j, a.int_elem_bytes);
        const unsigned int j = atomicAdd(&sh_kept, 1u);  // (< WORST_SPAN: one place per row of this workgroup at most)
        seg_keys[j] = (unsigned int)key;
        seg_words[0 * cap + j] = conf;
        seg_words[1 * cap + j] = (unsigned int)(int)c[0];
        seg_words[2 * cap + j] = worst_pair(c[1], c[2]);
        seg_words[3 * cap + j] = worst_pair(c[3], c[4]);
        seg_words[4 * cap + j] = worst_pair(c[5], c[6]);
    }
    if (max_alt > 0) atomicMax(&sh_max_alt, max_alt);
    __syncthreads();
    if (threadIdx.x == 0) {
        scratch[blockIdx.x] = sh_kept;
        unsigned long long* h64 = reinterpret_cast<unsigned long long*>(table);
        if (sh_beyond) atomicAdd(&h64[0], (unsigned long long)sh_beyond);
        if (sh_max_alt > 0) atomicMax(reinterpret_cast<int*>(table) + 2, sh_max_alt);
        if (sh_wrong[0]) atomicAdd(&h64[2], (unsigned long long)sh_wrong[0]);
        if (sh_wrong[1]) atomicAdd(&h64[3], (unsigned long long)sh_wrong[1]);
    }
}

// ---- the sort of one key's records in LDS ------------------------------------------------------------------------------------------------
struct WorstLds {
    unsigned int w[WORST_WORDS][WORST_CAP];
    unsigned int count;
};

__device__ __forceinline__ WorstRecord worst_load(const WorstLds& s, int i) {
    WorstRecord r;
#pragma unroll
    for (int f = 0; f < WORST_WORDS; ++f) r.w[f] = s.w[f][i];
    return r;
}
__device__ __forceinline__ void worst_store(WorstLds& s, int i, const WorstRecord& r) {
#pragma unroll
    for (int f = 0; f < WORST_WORDS; ++f) s.w[f][i] = r.w[f];
}

// Sorts records [0, n) into the order of worst_before and leaves min(n, keep) of them counted (what lies behind them is rubbish that
// the next append overwrites or the next sort clears).  Bitonic over the next power of two, padded with the all-zero record, which every
// real record precedes (a wrong row's confidence is never zero).  All WORST_THREADS threads call it with the same arguments; it begins
// and ends with a barrier.
__device__ void worst_sort(WorstLds& s, int n, int keep) {
    int m = 1;
    while (m < n) m <<= 1;
    for (int i = n + threadIdx.x; i < m; i += WORST_THREADS) {
#pragma unroll
        for (int f = 0; f < WORST_WORDS; ++f) s.w[f][i] = 0u;
    }
    __syncthreads();
    for (int k = 2; k <= m; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (m >> 1); t += WORST_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));  // the lower index of compare-exchange t at distance j
                const int l = i | j;
                const WorstRecord x = worst_load(s, i), y = worst_load(s, l);
                const bool ascending = (i & k) == 0;  // "ascending": in the order of worst_before
                if (ascending ? worst_before(y, x) : worst_before(x, y)) {
                    worst_store(s, i, y);
                    worst_store(s, l, x);
                }
            }
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) s.count = (unsigned int)(n < keep ? n : keep);
    __syncthreads();
}

// the first `fill` records of the LDS buffer into the key's slots, and its fill count (slots behind them are zero already: a key's
// fill never shrinks)
__device__ __forceinline__ void worst_write_key(const WorstLds& s, unsigned int* __restrict__ table, int num_keys, int queue_size, int key,
                                                int fill) {
    unsigned int* slots = table + worst_slot_at(num_keys, queue_size, key, 0);
    for (int j = threadIdx.x; j < fill * WORST_WORDS; j += WORST_THREADS) slots[j] = s.w[j % WORST_WORDS][j / WORST_WORDS];
    if (threadIdx.x == 0) table[worst_fill_at(key)] = (unsigned int)fill;
}

// ---- launch 2: a workgroup per key --------------------------------------------------------------------------------------------------------
// The survivors lie scattered over the segments.  A workgroup takes the segments' counts WORST_THREADS at a time (one coalesced load),
// scans them into offsets, and then walks the chunk's survivors by a FLAT index, thread i taking survivor i, i + 256, ...: the loads of
// a sweep are independent of one another, and a late batch, whose segments are nearly all empty, costs a workgroup one load and one scan.
// (Walking the segments one after the other, a dependent load each, was measured at 48 us a call with 64 segments and 78 us with 256:
// the whole cost of a late batch.)
struct WorstSegments {
    unsigned int start[WORST_THREADS + 1];  // exclusive offsets of the chunk's segments; [WORST_THREADS]: the chunk's survivors
    unsigned int wave_total[WORST_THREADS / 64];
};
// Stages segments [base, base + WORST_THREADS) and returns their survivors (the same in every thread); begins and ends with a barrier.
__device__ unsigned int worst_stage(const unsigned int* __restrict__ scratch, long long segments, long long base, WorstSegments& g) {
    const long long b = base + threadIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned int own = b < segments ? min(scratch[b], (unsigned int)WORST_SPAN) : 0u;  // (the clamp: whatever the scratch holds stays inside it)
    unsigned int incl = own;
    for (int m = 1; m < 64; m <<= 1) {
        const unsigned int up = __shfl_up(incl, m);
        if (lane >= m) incl += up;
    }
    __syncthreads();  // (the chunk before is done with `g`)
    if (lane == 63) g.wave_total[wave] = incl;
    __syncthreads();
    unsigned int before = 0;
    for (int w = 0; w < wave; ++w) before += g.wave_total[w];
    g.start[threadIdx.x] = before + incl - own;
    if (threadIdx.x == WORST_THREADS - 1) g.start[WORST_THREADS] = before + incl;
    __syncthreads();
    return g.start[WORST_THREADS];
}
// where survivor i (< the chunk's survivors) of the staged chunk lies in the scratch's key / word arrays: in the last segment that starts
// at or before i (empty segments share their start with the next one)
__device__ __forceinline__ size_t worst_survivor_at(const WorstSegments& g, long long base, unsigned int i) {
    int lo = 0, hi = WORST_THREADS;  // start[lo] <= i < start[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (g.start[mid] <= i) lo = mid; else hi = mid;
    }
    return (size_t)(base + lo) * WORST_SPAN + (i - g.start[lo]);
}

__global__ __launch_bounds__(WORST_THREADS) void worst_sort_kernel(int queue_size, int num_alt_keys, unsigned int* __restrict__ table,
                                                                   const unsigned int* __restrict__ scratch, long long segments) {
    __shared__ WorstLds s;
    __shared__ WorstSegments g;
    const int key = blockIdx.x, num_keys = 2 * num_alt_keys;
    const size_t cap = (size_t)segments * WORST_SPAN;
    const unsigned int* keys = scratch + segments;
    const unsigned int* words = scratch + segments + cap;
    // has this key a survivor at all?
    int mine = 0;
    for (long long base = 0; base < segments; base += WORST_THREADS) {
        const unsigned int total = worst_stage(scratch, segments, base, g);
        for (unsigned int i = threadIdx.x; i < total; i += WORST_THREADS) mine |= keys[worst_survivor_at(g, base, i)] == (unsigned int)key;
    }
    if (!__syncthreads_or(mine)) return;
    const int fill = min((int)table[worst_fill_at(key)], queue_size);  // (the clamp: a table that is not one must not overrun the LDS)
    const unsigned int* slots = table + worst_slot_at(num_keys, queue_size, key, 0);
    for (int j = threadIdx.x; j < fill * WORST_WORDS; j += WORST_THREADS) s.w[j % WORST_WORDS][j / WORST_WORDS] = slots[j];
    if (threadIdx.x == 0) s.count = (unsigned int)fill;
    for (long long base = 0; base < segments; base += WORST_THREADS) {
        const unsigned int total = worst_stage(scratch, segments, base, g);
        for (unsigned int at = 0; at < total; at += WORST_THREADS) {  // (uniform: every thread takes every turn)
            __syncthreads();  // (the appends of the turn before are counted)
            const int have = (int)s.count;
            __syncthreads();  // (and nobody appends before everybody has read the count: the branch below is uniform)
            if (have + WORST_THREADS > WORST_CAP) worst_sort(s, have, queue_size);  // make room: the best queue_size so far stay
            const unsigned int i = at + threadIdx.x;
            if (i < total) {
                const size_t from = worst_survivor_at(g, base, i);
                if (keys[from] == (unsigned int)key) {
                    const unsigned int place = atomicAdd(&s.count, 1u);  // (< WORST_CAP: at most WORST_THREADS appends since the check)
#pragma unroll
                    for (int f = 0; f < WORST_WORDS; ++f) s.w[f][place] = words[f * cap + from];
                }
            }
        }
    }
    __syncthreads();
    worst_sort(s, (int)s.count, queue_size);
    worst_write_key(s, table, num_keys, queue_size, key, (int)s.count);
}

// ---- the merge: a workgroup per key, both tables' slots of the key sorted together ------------------------------------------------------
__global__ __launch_bounds__(WORST_THREADS) void worst_merge_kernel(int queue_size, int num_alt_keys, unsigned int* __restrict__ table,
                                                                    const unsigned int* __restrict__ other) {
    __shared__ WorstLds s;
    const int key = blockIdx.x, num_keys = 2 * num_alt_keys;
    if (key == 0 && threadIdx.x == 0) {  // the header: this workgroup alone touches it
        unsigned long long* mine = reinterpret_cast<unsigned long long*>(table);
        const unsigned long long* theirs = reinterpret_cast<const unsigned long long*>(other);
        mine[0] += theirs[0];
        mine[2] += theirs[2];
        mine[3] += theirs[3];
        const int a = (int)table[2], b = (int)other[2];
        table[2] = (unsigned int)(a > b ? a : b);
    }
    const int fill = min((int)table[worst_fill_at(key)], queue_size), more = min((int)other[worst_fill_at(key)], queue_size);
    if (more == 0) return;  // (uniform)
    const unsigned int* slots = table + worst_slot_at(num_keys, queue_size, key, 0);
    const unsigned int* other_slots = other + worst_slot_at(num_keys, queue_size, key, 0);
    for (int j = threadIdx.x; j < fill * WORST_WORDS; j += WORST_THREADS) s.w[j % WORST_WORDS][j / WORST_WORDS] = slots[j];
    for (int j = threadIdx.x; j < more * WORST_WORDS; j += WORST_THREADS) s.w[j % WORST_WORDS][fill + j / WORST_WORDS] = other_slots[j];
    __syncthreads();
    worst_sort(s, fill + more, queue_size);
    worst_write_key(s, table, num_keys, queue_size, key, (int)s.count);
}

// ---- the entry points ---------------------------------------------------------------------------------------------------------------------
static bool worst_shape_ok(int32_t queue_size, int32_t num_alt_keys) {
    return queue_size >= 1 && queue_size <= PMT_WORST_MAX_QUEUE && num_alt_keys >= 1 && num_alt_keys <= (1 << 24);
}

extern "C" size_t pmt_worst_table_bytes(int32_t queue_size, int32_t num_alt_keys) {
    if (!worst_shape_ok(queue_size, num_alt_keys)) return 0;
    return worst_slot_at(2 * num_alt_keys, queue_size, 2 * num_alt_keys, 0) * sizeof(unsigned int);
}

extern "C" size_t pmt_worst_scratch_bytes(int64_t max_variants, int32_t queue_size, int32_t num_alt_keys) {
    if (!worst_shape_ok(queue_size, num_alt_keys) || max_variants < 0 || max_variants > 0x7fffffffLL) return 0;
    return worst_scratch_words(worst_segments(max_variants)) * sizeof(unsigned int);
}

extern "C" int pmt_worst_record(const PmtWorstArgs* args, void* table, void* scratch, void* stream) {
    if (!args || !table || args->num_variants < 0 || args->num_alt_keys < 1) return PMT_E_INVALID;
    if (args->queue_size < 1 || args->queue_size > PMT_WORST_MAX_QUEUE) return PMT_E_UNSUPPORTED;
    if (!worst_shape_ok(args->queue_size, args->num_alt_keys)) return PMT_E_INVALID;
    if (args->num_variants == 0) return PMT_OK;
    if (!scratch || !args->labels.ptr || !args->alt_counts.ptr || !args->int_rows || !args->logits_b) return PMT_E_INVALID;
    if ((args->labels.elem_bytes != 4 && args->labels.elem_bytes != 8) || (args->alt_counts.elem_bytes != 4 && args->alt_counts.elem_bytes != 8))
        return PMT_E_INVALID;
    if (args->int_elem_bytes != 2 && args->int_elem_bytes != 4 && args->int_elem_bytes != 8) return PMT_E_INVALID;
    const long long segments = worst_segments(args->num_variants);
    if (args->scratch_bytes < 0 || (size_t)args->scratch_bytes < worst_scratch_words(segments) * sizeof(unsigned int)) return PMT_E_WORKSPACE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    unsigned int* t = reinterpret_cast<unsigned int*>(table);
    unsigned int* sc = reinterpret_cast<unsigned int*>(scratch);
    hipLaunchKernelGGL(worst_filter_kernel, dim3((unsigned)segments), dim3(WORST_THREADS), 0, s, *args, t, sc, segments);
    hipLaunchKernelGGL(worst_sort_kernel, dim3((unsigned)(2 * args->num_alt_keys)), dim3(WORST_THREADS), 0, s, args->queue_size,
                       args->num_alt_keys, t, sc, segments);
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}

extern "C" int pmt_worst_merge(void* table, const void* other, int32_t queue_size, int32_t num_alt_keys, void* scratch, void* stream) {
    (void)scratch;
    if (!table || !other || table == other || num_alt_keys < 1) return PMT_E_INVALID;
    if (queue_size < 1 || queue_size > PMT_WORST_MAX_QUEUE) return PMT_E_UNSUPPORTED;
    if (!worst_shape_ok(queue_size, num_alt_keys)) return PMT_E_INVALID;
    hipLaunchKernelGGL(worst_merge_kernel, dim3((unsigned)(2 * num_alt_keys)), dim3(WORST_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       queue_size, num_alt_keys, reinterpret_cast<unsigned int*>(table), reinterpret_cast<const unsigned int*>(other));
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}
