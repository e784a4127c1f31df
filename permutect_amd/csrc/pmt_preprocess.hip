// The normalisation of preprocess_dataset (reference data/plain_text_data.py:205-479; include/permutect_amd.h: PmtPreprocessArgs).
//
// pmt_preprocess_fit: the fitted column is float16, so a chunk's order statistics are exact from a table of counts keyed by the 16-bit
// pattern.  A lane per read adds its ref read to its chunk's table with a 32-bit integer atomic (the table is 256 KB per chunk: more than
// the 160 KB of LDS, so it lives in memory and the adds meet in L2); then a workgroup per chunk scans its table and interpolates the 100
// quantiles as np.nanpercentile does.  Integer counts: the same bits for any grid and from run to run.
// pmt_preprocess_normalize: a lane per read writes the read's 12 bytes; a lane per datum writes its float16 row, going once more over
// the datum's alt reads (15 at most) for the medians and boolean means.
//
// Everything the reference rounds is rounded here at the same point: float16 ufuncs are a float operation rounded once to float16,
// float32 stays float32, np.interp / _lerp / the uniform value are double.  The unit is compiled with -ffp-contract=off (csrc/Makefile)
// and says so again below: a fused multiply-add would change the last bit of a slope or a lerp.
#include <hip/hip_runtime.h>

#include "permutect_amd.h"

#pragma clang fp contract(off)

#define PRE_FIT_THREADS 256
#define PRE_KEYS_PER_THREAD (PMT_PREPROCESS_KEYS / PRE_FIT_THREADS)
#define PRE_Q PMT_PREPROCESS_QUANTILES
#define PRE_MAX_ALT PMT_PREPROCESS_MAX_ALT
#define PRE_SCALARS 6      // scalars in front of the info of a float row
#define PRE_RAW_INFO 11
#define PRE_INFO_OUT 38
#define PRE_READ_SCALARS 9
#define PRE_MAX_BITS 55    // 10 + 3 * 15

// ---- float16 as the reference's numpy handles it ------------------------------------------------------------------------------------
__device__ __forceinline__ float pre_h2f(uint16_t bits) { return (float)__builtin_bit_cast(_Float16, bits); }
__device__ __forceinline__ uint16_t pre_f2h(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }  // round to nearest even, once
__device__ __forceinline__ bool pre_is_nan16(uint16_t bits) { return (bits & 0x7fffu) > 0x7c00u; }
// double -> float16 in ONE rounding to nearest even, as numpy's npy_double_to_half (a detour over float would round twice)
__device__ __forceinline__ uint16_t pre_d2h(double d) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(d);
    const uint16_t sign = (uint16_t)((b >> 48) & 0x8000ull);
    const int e = (int)((b >> 52) & 0x7ffull);
    const unsigned long long m = b & 0xFFFFFFFFFFFFFull;
    if (e == 0x7ff) return sign | (m ? 0x7e00u : 0x7c00u);
    const int ue = e - 1023;
    if (ue > 15) return sign | 0x7c00u;
    if (e == 0 || ue < -26) return sign;  // below half of the smallest float16 subnormal
    const bool normal = ue >= -14;
    const int shift = normal ? 42 : 42 + (-14 - ue);
    const unsigned long long full = normal ? m : (m | (1ull << 52));
    const unsigned long long kept = full >> shift, rem = full & ((1ull << shift) - 1ull), half = 1ull << (shift - 1);
    unsigned int h = (normal ? (unsigned int)(ue + 15) << 10 : 0u) + (unsigned int)kept;
    if (rem > half || (rem == half && (h & 1u))) ++h;  // a carry runs into the exponent, and into infinity at the top
    return sign | (uint16_t)h;
}
// the count table's key: the 16-bit pattern made order-preserving; -0 counts as +0
__device__ __forceinline__ unsigned int pre_key(uint16_t bits) {
    if (bits == 0x8000u) bits = 0;
    return (bits & 0x8000u) ? 0xFFFFu - bits : bits + 0x8000u;
}
__device__ __forceinline__ uint16_t pre_key_bits(unsigned int key) { return (uint16_t)(key >= 0x8000u ? key - 0x8000u : 0xFFFFu - key); }

// float16 patterns as integers in their total order (-0 before +0), and back
__device__ __forceinline__ int pre_order(uint16_t bits) { return (bits & 0x8000u) ? -(int)(bits & 0x7fffu) - 1 : (int)bits; }
__device__ __forceinline__ uint16_t pre_order_bits(int key) { return key < 0 ? (uint16_t)((unsigned int)(-key - 1) | 0x8000u) : (uint16_t)key; }

// the datum of read r: the last d < n with read_start[d] <= r, in a fixed number of steps (each a clamped load and a select)
__device__ __forceinline__ long long pre_datum_of(const int64_t* __restrict__ read_start, long long n, int steps, long long r) {
    long long base = 0;  // how many of read_start[0 .. n) are <= r
    for (int s = steps - 1; s >= 0; --s) {
        const long long probe = base + (1LL << s);
        const long long at = (probe <= n ? probe : n) - 1;
        base = (probe <= n && read_start[at] <= r) ? probe : base;
    }
    return base - 1;
}

// ---- the fit ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void preprocess_count_kernel(PmtPreprocessArgs a, int steps) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.num_reads) return;
    const long long d = pre_datum_of(a.read_start, a.num_data, steps, r);
    if (d < 0 || r >= a.read_start[d + 1]) return;  // (rows behind the last datum's)
    const long long ref_count = a.int_rows[d * a.int_row_stride];
    const int chunk = a.chunk_of[d];
    if (r - a.read_start[d] >= ref_count || chunk < 0 || chunk >= a.num_chunks) return;
    const uint16_t bits = a.reads[r * (PRE_READ_SCALARS + a.num_error_columns) + 6];
    if (pre_is_nan16(bits)) return;  // np.nanpercentile leaves it out
    atomicAdd(a.counts + (size_t)chunk * PMT_PREPROCESS_KEYS + pre_key(bits), 1u);
}

__device__ __forceinline__ double pre_reference(int i, int nq) {  // np.linspace(0, 1, nq)[i]
    return (nq > 1 && i == nq - 1) ? 1.0 : (double)i * (1.0 / (double)(nq - 1 > 0 ? nq - 1 : 1));
}

__global__ __launch_bounds__(PRE_FIT_THREADS) void preprocess_quantile_kernel(PmtPreprocessArgs a) {
    __shared__ long long sh_base[PRE_FIT_THREADS + 1];
    __shared__ long long sh_rank[2][PRE_Q];     // the ranks of the two order statistics around every virtual index
    __shared__ unsigned int sh_keys[2][PRE_Q];  // ... and their keys
    __shared__ double sh_gamma[PRE_Q], sh_value[PRE_Q];
    const int chunk = blockIdx.x, t = threadIdx.x;
    const unsigned int* __restrict__ table = a.counts + (size_t)chunk * PMT_PREPROCESS_KEYS + (size_t)t * PRE_KEYS_PER_THREAD;
    long long mine = 0;
    for (int j = 0; j < PRE_KEYS_PER_THREAD; j += 4) {
        const uint4 c = *reinterpret_cast<const uint4*>(table + j);
        mine += (long long)c.x + c.y + c.z + c.w;
    }
    sh_base[t + 1] = mine;
    __syncthreads();
    if (t == 0) {
        sh_base[0] = 0;
        for (int j = 1; j <= PRE_FIT_THREADS; ++j) sh_base[j] += sh_base[j - 1];
    }
    __syncthreads();
    const long long n = sh_base[PRE_FIT_THREADS];
    const int nq = n < PRE_Q ? (int)n : PRE_Q;
    double* __restrict__ out = a.quantiles + (size_t)chunk * PRE_Q;
    if (t == 0) a.ref_reads[chunk] = n;
    if (n == 0) {
        if (t < PRE_Q) out[t] = __longlong_as_double(0x7ff8000000000000LL);
        return;
    }
    if (t < nq) {  // numpy's percentile: q = (reference * 100) / 100; "linear": the virtual index (n - 1) * q, its floor and the next
        const double q = (pre_reference(t, nq) * 100.0) / 100.0;
        const double last = (double)(n - 1), at = last * q;
        const bool above = at >= last;
        const double below = floor(at);
        sh_rank[0][t] = above ? n - 1 : (long long)below;
        sh_rank[1][t] = above ? n - 1 : (long long)below + 1;
        sh_gamma[t] = at - (above ? -1.0 : below);  // (numpy takes the difference after it has set the index to -1: the two neighbours are equal there)
    }
    __syncthreads();
    if (mine > 0) {  // this thread's keys hold ranks [sh_base[t], sh_base[t + 1])
        long long first = sh_base[t];
        for (int j = 0; j < PRE_KEYS_PER_THREAD; ++j) {
            const long long count = table[j];
            if (count == 0) continue;
            for (int i = 0; i < nq; ++i) {
#pragma unroll
                for (int side = 0; side < 2; ++side) {
                    const long long rank = sh_rank[side][i];
                    if (rank >= first && rank < first + count) sh_keys[side][i] = (unsigned int)(t * PRE_KEYS_PER_THREAD + j);
                }
            }
            first += count;
        }
    }
    __syncthreads();
    if (t < nq) {  // numpy's _lerp: the difference of the two float16 neighbours is a float16; the rest is double
        const uint16_t lo = pre_key_bits(sh_keys[0][t]), hi = pre_key_bits(sh_keys[1][t]);
        const double va = (double)pre_h2f(lo), vb = (double)pre_h2f(hi), g = sh_gamma[t];
        const double diff = (double)pre_h2f(pre_f2h(pre_h2f(hi) - pre_h2f(lo)));
        double v = va + diff * g;
        if (g >= 0.5) v = vb - diff * (1.0 - g);
        sh_value[t] = v;
    }
    __syncthreads();
    if (t == 0) {  // np.maximum.accumulate
        double running = sh_value[0];
        for (int i = 0; i < PRE_Q; ++i) {
            if (i < nq) running = sh_value[i] > running ? sh_value[i] : running;
            out[i] = i < nq ? running : __longlong_as_double(0x7ff8000000000000LL);
        }
    }
}

// ---- a read -------------------------------------------------------------------------------------------------------------------------
// np.interp(x, xp, fp) over nq >= 1 points; forward: xp = q, fp = r; backward: xp = -q[::-1], fp = -r[::-1]
template <bool BACKWARD>
__device__ __forceinline__ double pre_interp(double x, const double* __restrict__ q, int nq) {
    auto xp = [&](int j) { return BACKWARD ? -q[nq - 1 - j] : q[j]; };
    auto fp = [&](int j) { return BACKWARD ? -pre_reference(nq - 1 - j, nq) : pre_reference(j, nq); };
    if (nq == 1) return fp(0);
    int count = 0;  // how many xp are <= x: 7 steps cover 100 points
#pragma unroll
    for (int s = 6; s >= 0; --s) {
        const int probe = count + (1 << s);
        const int at = (probe <= nq ? probe : nq) - 1;
        count = (probe <= nq && xp(at) <= x) ? probe : count;
    }
    const int j = count - 1;
    if (j < 0) return fp(0);
    if (j >= nq - 1) return fp(nq - 1);
    const double x0 = xp(j), y0 = fp(j);
    if (x0 == x) return y0;
    const double x1 = xp(j + 1), y1 = fp(j + 1);
    const double slope = (y1 - y0) / (x1 - x0);
    double v = slope * (x - x0) + y0;
    if (isnan(v)) {
        v = slope * (x - x1) + y1;
        if (isnan(v) && y0 == y1) v = y0;
    }
    return v;
}

// sklearn's _transform_col on one float16 value: the clipped normal quantile as float16 bits
__device__ __forceinline__ uint16_t pre_quantile_transform(uint16_t x_bits, const double* __restrict__ q, int nq,
                                                           const uint16_t* __restrict__ ppf) {
    if (pre_is_nan16(x_bits) || nq < 1) return 0x7e00u;
    const float xf = pre_h2f(x_bits), eps = pre_h2f(0x0002u);  // float16(1e-7)
    const bool below = (double)pre_h2f(pre_f2h(xf - eps)) < q[0];
    const bool above = (double)pre_h2f(pre_f2h(xf + eps)) > q[nq - 1];
    const double x = (double)xf;
    const double uniform = 0.5 * (pre_interp<false>(x, q, nq) - pre_interp<true>(-x, q, nq));
    uint16_t u = pre_d2h(uniform);
    if (above) u = 0x3c00u;
    if (below) u = 0;
    if (u == 0x8000u) u = 0;
    return u < PMT_PREPROCESS_PPF ? ppf[u] : (uint16_t)0x7e00u;
}

__device__ __forceinline__ uint16_t pre_tanh20(uint16_t x_bits) {  // np.tanh(x / 20) of a float16
    const float quotient = pre_h2f(pre_f2h(__fdiv_rn(pre_h2f(x_bits), 20.0f)));
    return pre_d2h(tanh((double)quotient));
}
__device__ __forceinline__ unsigned int pre_byte(uint16_t v_bits) {  // clip(v * 32 + 128, 0, 255) truncated
    if (pre_is_nan16(v_bits)) return 0u;
    const float scaled = pre_h2f(pre_f2h(pre_h2f(v_bits) * 32.0f));
    float shifted = pre_h2f(pre_f2h(scaled + 128.0f));
    shifted = shifted < 0.0f ? 0.0f : (shifted > 255.0f ? 255.0f : shifted);
    return (unsigned int)shifted;
}

struct PreRead {
    unsigned long long bits;  // the 10 + 3k booleans, the first highest, in the low 10 + 3k bits
    uint16_t values[5];       // the float columns: tanh of raw columns 4, 5, 7, 8, the transformed column 6
};

__device__ __forceinline__ PreRead pre_read(const uint16_t* __restrict__ row, int k, const double* __restrict__ q, int nq,
                                            const uint16_t* __restrict__ ppf) {
    PreRead out;
    const float mq = pre_h2f(row[0]), bq = pre_h2f(row[1]);
    unsigned long long bits = 0;
    auto push = [&](bool b) { bits = (bits << 1) | (b ? 1ull : 0ull); };
    push(mq > 59.0f); push(mq <= 59.0f && mq >= 40.0f); push(mq < 40.0f && mq >= 20.0f); push(mq < 20.0f);
    push(bq >= 30.0f); push(bq < 30.0f && bq >= 20.0f); push(bq < 20.0f && bq >= 10.0f); push(bq < 10.0f);
    push(pre_h2f(row[2]) < 0.5f); push(pre_h2f(row[3]) < 0.5f);
    for (int j = 0; j < k; ++j) push(pre_h2f(row[PRE_READ_SCALARS + j]) < 0.5f);
    for (int j = 0; j < k; ++j) { const float e = pre_h2f(row[PRE_READ_SCALARS + j]); push(e > 0.5f && e < 1.5f); }
    for (int j = 0; j < k; ++j) push(pre_h2f(row[PRE_READ_SCALARS + j]) > 1.5f);
    out.bits = bits;
    out.values[0] = pre_tanh20(row[4]);
    out.values[1] = pre_tanh20(row[5]);
    out.values[2] = pre_tanh20(row[7]);
    out.values[3] = pre_tanh20(row[8]);
    out.values[4] = pre_quantile_transform(row[6], q, nq, ppf);
    return out;
}

__global__ __launch_bounds__(512) void preprocess_reads_kernel(PmtPreprocessArgs a, int steps) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.num_reads) return;
    const long long d = pre_datum_of(a.read_start, a.num_data, steps, r);
    unsigned int w0 = 0, w1 = 0, w2 = 0;
    if (d >= 0 && r < a.read_start[d + 1]) {
        const int chunk = a.chunk_of[d];
        if (chunk >= 0 && chunk < a.num_chunks) {
            const int k = a.num_error_columns;
            const long long n = a.ref_reads[chunk];
            const PreRead x = pre_read(a.reads + r * (PRE_READ_SCALARS + k), k, a.quantiles + (size_t)chunk * PRE_Q, n < PRE_Q ? (int)n : PRE_Q,
                                       a.ppf_table);
            const unsigned long long packed = x.bits << (56 - (10 + 3 * k));  // np.packbits: the first boolean is bit 7 of byte 0
            unsigned int b[PMT_PREPROCESS_READ_BYTES];
#pragma unroll
            for (int j = 0; j < 7; ++j) b[j] = (unsigned int)((packed >> (8 * (6 - j))) & 0xffull);
#pragma unroll
            for (int j = 0; j < 5; ++j) b[7 + j] = pre_byte(x.values[j]);
            w0 = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
            w1 = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
            w2 = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
        }
    }
    unsigned int* __restrict__ out = reinterpret_cast<unsigned int*>(a.out_reads + r * PMT_PREPROCESS_READ_BYTES);  // 12-byte rows: 4-byte aligned
    out[0] = w0;
    out[1] = w1;
    out[2] = w2;
}

// ---- a datum ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint16_t pre_flag(bool b) { return b ? 0x3c00u : 0u; }  // float16 1 / 0

// (256 lanes at most: five sorted columns and 55 counters per lane want more than the 256 registers that eight wavefronts would leave)
__global__ __launch_bounds__(256) void preprocess_data_kernel(PmtPreprocessArgs a) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.num_data) return;
    const int k = a.num_error_columns, nbits = 10 + 3 * k;
    const int16_t* __restrict__ ints = a.int_rows + i * a.int_row_stride;
    const long long ref = ints[0], alt = ints[1], start = a.read_start[i], stop = a.read_start[i + 1];
    const int chunk = a.chunk_of[i];
    if (ref < 0 || alt < 1 || alt > PRE_MAX_ALT || start < 0 || start + ref + alt != stop || stop > a.num_reads || chunk < 0 || chunk >= a.num_chunks) {
        atomicMax(a.fault, (int)(i + 1));
        return;
    }
    const uint16_t* __restrict__ in = a.float_rows + i * (PRE_SCALARS + PRE_RAW_INFO);
    uint16_t* __restrict__ out = a.out_floats + i * (PRE_SCALARS + PRE_INFO_OUT + 5 + nbits);
    for (int j = 0; j < PRE_SCALARS; ++j) out[j] = in[j];
    float info[PRE_RAW_INFO];
#pragma unroll
    for (int j = 0; j < PRE_RAW_INFO; ++j) info[j] = pre_h2f(in[PRE_SCALARS + j]);
    // a Python number compared with a float16 array is a float16 first
    const float c01 = pre_h2f(pre_f2h(0.1f)), c025 = 0.25f, c09 = pre_h2f(pre_f2h(0.9f)), c07 = pre_h2f(pre_f2h(0.7f));
    uint16_t* o = out + PRE_SCALARS;
    *o++ = pre_flag(info[0] < c01); *o++ = pre_flag(info[1] < c01);
    *o++ = pre_flag(info[0] >= c01 && info[0] < c025); *o++ = pre_flag(info[1] >= c01 && info[1] < c025);
    *o++ = pre_flag(info[0] >= c025); *o++ = pre_flag(info[1] >= c025);
    *o++ = pre_flag(info[2] == 0.0f); *o++ = pre_flag(info[2] == 1.0f); *o++ = pre_flag(info[2] == 2.0f); *o++ = pre_flag(info[2] >= 3.0f);
    *o++ = pre_flag(info[3] > c09); *o++ = pre_flag(info[3] <= c09 && info[3] > c07);
    *o++ = pre_f2h(__fdiv_rn(info[5], 10.0f)); *o++ = pre_f2h(__fdiv_rn(info[6], 10.0f));
    *o++ = pre_flag(info[7] == 1.0f); *o++ = pre_flag(info[7] == 2.0f); *o++ = pre_flag(info[7] == 3.0f); *o++ = pre_flag(info[7] == 4.0f);
    *o++ = pre_flag(info[7] >= 5.0f);
#pragma unroll
    for (int other = 8; other <= 10; ++other) {  // the repeat's total length, its length before and after the variant: a float16 product
        const float length = pre_h2f(pre_f2h(info[7] * info[other]));
        *o++ = pre_flag(length == 1.0f); *o++ = pre_flag(length > 1.0f && length < 4.0f); *o++ = pre_flag(length > 3.0f && length < 6.0f);
        *o++ = pre_flag(length > 5.0f && length < 9.0f); *o++ = pre_flag(length > 8.0f && length < 13.0f); *o++ = pre_flag(length > 12.0f);
    }
    {   // the quality feature (:367-377): a float16 product, then float32 with the int16 counts (whose sums wrap as int16) and lgamma's float32
        const int16_t depth = ints[5], alt_original = ints[6];
        const float la = a.lgamma_table[(int)(int16_t)(depth + 1) + 32768], lb = a.lgamma_table[(int)(int16_t)(alt_original + 1) + 32768],
                    lc = a.lgamma_table[(int)(int16_t)((int16_t)(depth - alt_original) + 1) + 32768];
        const float log_tlod = pre_h2f(pre_f2h(pre_h2f(pre_f2h(2.30258509299f)) * info[4])) * (float)alt_original;
        const float correction = (la - lb) - lc;
        const uint16_t quality = pre_f2h(__fdiv_rn(__fdiv_rn(log_tlod + correction, (float)alt_original), 10.0f));
        *o++ = pre_is_nan16(quality) ? (uint16_t)0x7e00u : quality;  // (one NaN pattern, as the mirror's)
    }

    // the alt reads: every float column sorted by insertion into registers, every boolean column counted
    const long long n_chunk = a.ref_reads[chunk];
    const int nq = n_chunk < PRE_Q ? (int)n_chunk : PRE_Q;
    const double* __restrict__ q = a.quantiles + (size_t)chunk * PRE_Q;
    int sorted[5][PRE_MAX_ALT];  // as integers in float16's total order (pre_order): -0 sorts before +0, here and in the mirror
    int ones[PRE_MAX_BITS];
#pragma unroll
    for (int c = 0; c < 5; ++c)
#pragma unroll
        for (int s = 0; s < PRE_MAX_ALT; ++s) sorted[c][s] = 0x7fffffff;
#pragma unroll
    for (int b = 0; b < PRE_MAX_BITS; ++b) ones[b] = 0;
    for (long long r = start + ref; r < stop; ++r) {
        const PreRead x = pre_read(a.reads + r * (PRE_READ_SCALARS + k), k, q, nq, a.ppf_table);
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            int v = pre_order(x.values[c]);
#pragma unroll
            for (int s = 0; s < PRE_MAX_ALT; ++s) {
                const int held = sorted[c][s];
                const bool before = v < held;
                sorted[c][s] = before ? v : held;
                v = before ? held : v;
            }
        }
        const unsigned long long aligned = x.bits << (PRE_MAX_BITS - nbits);  // boolean b at bit PRE_MAX_BITS - 1 - b
#pragma unroll
        for (int b = 0; b < PRE_MAX_BITS; ++b) ones[b] += (int)((aligned >> (PRE_MAX_BITS - 1 - b)) & 1ull);
    }
    const int lo = (int)((alt - 1) / 2), hi = (int)(alt / 2);
#pragma unroll
    for (int c = 0; c < 5; ++c) {  // np.median: np.mean of the middle one or two -- a float32 sum halved, rounded once to float16
        int low = 0, high = 0;
#pragma unroll
        for (int s = 0; s < PRE_MAX_ALT; ++s) {
            low = s == lo ? sorted[c][s] : low;
            high = s == hi ? sorted[c][s] : high;
        }
        const uint16_t median = pre_f2h((pre_h2f(pre_order_bits(low)) + pre_h2f(pre_order_bits(high))) / 2.0f);
        *o++ = pre_is_nan16(median) ? (uint16_t)0x7e00u : median;
    }
#pragma unroll
    for (int b = 0; b < PRE_MAX_BITS; ++b)
        if (b < nbits) o[b] = pre_d2h((double)ones[b] / (double)alt);  // np.mean of booleans: a double
}

// ---- the entries --------------------------------------------------------------------------------------------------------------------
static int preprocess_steps(int64_t n) {  // ceil(log2(n + 1))
    int s = 0;
    while ((1LL << s) <= n) ++s;
    return s;
}

static int preprocess_check(const PmtPreprocessArgs* a, bool fit, int* threads) {
    const int64_t limit = 0x7fffffffLL;
    if (!a || a->num_data < 0 || a->num_data > limit || a->num_reads < 0 || a->num_reads > limit) return PMT_E_INVALID;
    if (a->num_chunks < 1 || a->num_error_columns < 13 || a->num_error_columns > 15 || a->int_row_stride < 7) return PMT_E_INVALID;
    *threads = a->threads_hint == 0 ? 256 : a->threads_hint;
    if (*threads != 64 && *threads != 128 && *threads != 256 && *threads != 512) return PMT_E_INVALID;
    if (a->num_data == 0) return PMT_OK;
    if (!a->int_rows || !a->read_start || !a->chunk_of || !a->quantiles || !a->ref_reads || (a->num_reads > 0 && !a->reads)) return PMT_E_INVALID;
    if (fit) return a->counts ? PMT_OK : PMT_E_INVALID;
    if (!a->float_rows || !a->lgamma_table || !a->ppf_table || !a->out_floats || !a->fault || (a->num_reads > 0 && !a->out_reads)) return PMT_E_INVALID;
    return PMT_OK;
}

extern "C" int pmt_preprocess_fit(const PmtPreprocessArgs* args, void* stream_) {
    int threads = 0;
    const int rc = preprocess_check(args, true, &threads);
    if (rc != PMT_OK || args->num_data == 0) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (hipMemsetAsync(args->counts, 0, (size_t)args->num_chunks * PMT_PREPROCESS_KEYS * sizeof(uint32_t), stream) != hipSuccess) return PMT_E_LAUNCH;
    if (args->num_reads > 0)
        hipLaunchKernelGGL(preprocess_count_kernel, dim3((unsigned)((args->num_reads + threads - 1) / threads)), dim3((unsigned)threads), 0, stream,
                           *args, preprocess_steps(args->num_data));
    hipLaunchKernelGGL(preprocess_quantile_kernel, dim3((unsigned)args->num_chunks), dim3(PRE_FIT_THREADS), 0, stream, *args);
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}

extern "C" int pmt_preprocess_normalize(const PmtPreprocessArgs* args, void* stream_) {
    int threads = 0;
    const int rc = preprocess_check(args, false, &threads);
    if (rc != PMT_OK || args->num_data == 0) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (hipMemsetAsync(args->fault, 0, sizeof(int32_t), stream) != hipSuccess) return PMT_E_LAUNCH;
    if (args->num_reads > 0)
        hipLaunchKernelGGL(preprocess_reads_kernel, dim3((unsigned)((args->num_reads + threads - 1) / threads)), dim3((unsigned)threads), 0, stream,
                           *args, preprocess_steps(args->num_data));
    const int data_threads = threads < 256 ? threads : 256;
    hipLaunchKernelGGL(preprocess_data_kernel, dim3((unsigned)((args->num_data + data_threads - 1) / data_threads)), dim3((unsigned)data_threads), 0,
                       stream, *args);
    if (hipGetLastError() != hipSuccess) return PMT_E_LAUNCH;
    int32_t fault = 0;
    if (hipMemcpyAsync(&fault, args->fault, sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess) return PMT_E_LAUNCH;
    if (hipStreamSynchronize(stream) != hipSuccess) return PMT_E_LAUNCH;
    return fault ? PMT_E_CAPACITY : PMT_OK;
}
