// The candidate key of the site annotation and of the filtered VCF (csrc/pmt_annotate.hip, csrc/pmt_vcf.hip): the reference's string key
// `contig:position:truncate(trim(ref, alt).alt)` (misc_utils.py `encode`) of a candidate's identity columns as a 64-bit locus and a
// 32-bit allele key.  ONE definition: both files include it.
#pragma once
#include <hip/hip_runtime.h>

#define ANNOTATE_MAX_DIGITS 14   // base-5 digits of a 32-bit code: 5^13 < 2^32 < 5^14
#define ANNOTATE_KEY_DIGITS 13   // MAX_NUM_BASES_FOR_ENCODING

__device__ __forceinline__ long long annotate_int(const void* rows, long long at, int elem_bytes) {
    return elem_bytes == 8 ? reinterpret_cast<const long long*>(rows)[at]
                           : (elem_bytes == 4 ? (long long)reinterpret_cast<const int*>(rows)[at] : (long long)reinterpret_cast<const short*>(rows)[at]);
}
// reference data/datum.py:46-48 (BIGGEST_UINT16 = 65535 is the multiplier), in 32 bits
__device__ __forceinline__ unsigned int annotate_pair(long long hi, long long lo) {
    return 65535u * (unsigned int)(hi + 32768) + (unsigned int)(lo + 32768);
}

// bases5_as_base_string: the digits of `code`, least significant first, three bits each (0 reads as 4, "T"), and their number
__device__ __forceinline__ unsigned long long annotate_digits(unsigned int code, int& length) {
    unsigned long long packed = 0;
    int n = 0;
#pragma unroll
    for (int k = 0; k < ANNOTATE_MAX_DIGITS; ++k) {
        const unsigned int digit = code % 5u;
        const unsigned long long d = (digit == 0u || code == 0u) ? (code == 0u ? 0ull : 4ull) : (unsigned long long)digit;
        packed |= d << (3 * k);
        n += code != 0u;
        code /= 5u;
    }
    length = n;
    return packed;
}

// truncate(trim(ref, alt).alt) of the two decoded strings, re-encoded: 0 for an empty alt
__device__ __forceinline__ unsigned int annotate_allele_key(unsigned int ref_code, unsigned int alt_code) {
    int ref_len, alt_len;
    const unsigned long long ref = annotate_digits(ref_code, ref_len), alt = annotate_digits(alt_code, alt_len);
    bool go = true;
#pragma unroll
    for (int k = 0; k < ANNOTATE_MAX_DIGITS - 1; ++k) {  // (a trim leaves one digit at least)
        const int r = ref_len > 0 ? ref_len - 1 : 0, a = alt_len > 0 ? alt_len - 1 : 0;
        go = go && ref_len > 1 && alt_len > 1 && ((ref >> (3 * r)) & 7ull) == ((alt >> (3 * a)) & 7ull);
        ref_len -= go;
        alt_len -= go;
    }
    unsigned int key = 0, power = 1;
#pragma unroll
    for (int k = 0; k < ANNOTATE_KEY_DIGITS; ++k) {
        const unsigned int d = (unsigned int)((alt >> (3 * k)) & 7ull);
        key += k < alt_len ? d * power : 0u;
        power *= 5u;
    }
    return key;
}
