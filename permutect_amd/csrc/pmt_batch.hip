// Batch composition on the device: the exclusive scans of the per-variant read counts (pmt_scan_counts), the gather index of a batch's
// reads (pmt_build_read_index) and a batch drawn from a dataset chunk resident in HBM (pmt_compose_batch, pmt_compose_batch_planned).
#include <hip/hip_runtime.h>

#include "permutect_amd.h"

// exclusive scans of ref / alt counts.  The counts sit in a strided column of the batch's integer table: every element in
// its own cache line (and, at 464 bytes per row, a new page every 9 rows), so the scan is bound by how many of those loads
// are in flight, and every element should be read exactly once.  Three small launches, no scratch memory:
//   1. every 1024-thread workgroup scans its own segment (local exclusive prefixes) and leaves the segment's TOTAL in the
//      first slot of the next segment (whose own local prefix is known to be 0); the last total goes to o[n];
//   2. one wave turns the totals in those slots into segment offsets (and completes o[n]);
//   3. every workgroup adds its offset to the rest of its segment.
#define PMT_SCAN_SEG 4096
template <typename T>
__global__ __launch_bounds__(1024) void pmt_scan_local_kernel(const T* __restrict__ c0, const T* __restrict__ c1,
                                                              long long stride, int n, int* __restrict__ o0, int* __restrict__ o1) {
    const T* c = blockIdx.y == 0 ? c0 : c1;
    int* o = blockIdx.y == 0 ? o0 : o1;
    __shared__ int wave_tot[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int begin = blockIdx.x * PMT_SCAN_SEG, end = min(n, begin + PMT_SCAN_SEG);
    int v[4], local = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = begin + tid * 4 + k;
        v[k] = i < end ? (int)c[(size_t)i * stride] : 0;
        local += v[k];
    }
    int incl = local;  // inclusive scan of `local` across the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int wave_prefix = 0, total = 0;
    for (int w = 0; w < 16; ++w) {
        if (w < wave) wave_prefix += wave_tot[w];
        total += wave_tot[w];
    }
    int run = wave_prefix + incl - local;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = begin + tid * 4 + k;
        if (i < end && i != begin) o[i] = run;  // (slot `begin` belongs to the previous segment's total until step 2)
        run += v[k];
    }
    if (tid == 0) {
        if (begin == 0) o[0] = 0;
        o[end == n ? n : begin + PMT_SCAN_SEG] = total;  // n > 0 here, so end == n only in the last segment
    }
}
__global__ __launch_bounds__(64) void pmt_scan_offsets_kernel(int n, int* __restrict__ o0, int* __restrict__ o1) {
    int* o = blockIdx.x == 0 ? o0 : o1;
    if (threadIdx.x != 0) return;  // at most n / 4096 totals: a serial walk of a few hundred L2 hits at the very most
    int run = 0;
    for (int s = PMT_SCAN_SEG; s < n; s += PMT_SCAN_SEG) {
        run += o[s];
        o[s] = run;
    }
    o[n] += run;  // (step 1 left the last segment's total there)
}
__global__ __launch_bounds__(1024) void pmt_scan_add_kernel(int n, int* __restrict__ o0, int* __restrict__ o1) {
    int* o = blockIdx.y == 0 ? o0 : o1;
    const int begin = (blockIdx.x + 1) * PMT_SCAN_SEG, end = min(n, begin + PMT_SCAN_SEG);
    const int off = o[begin];
    for (int i = begin + 1 + threadIdx.x; i < end; i += 1024) o[i] += off;
}

extern "C" int pmt_scan_counts(const void* ref_counts, const void* alt_counts, int32_t count_elem_bytes,
                               int64_t count_stride, int32_t num_variants, int32_t* ref_offsets, int32_t* alt_offsets,
                               void* stream) {
    if (!ref_counts || !alt_counts || !ref_offsets || !alt_offsets || num_variants < 0 || count_stride < 1) return PMT_E_INVALID;
    if (count_elem_bytes != 4 && count_elem_bytes != 8) return PMT_E_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (num_variants == 0) {
        if (hipMemsetAsync(ref_offsets, 0, sizeof(int32_t), s) != hipSuccess || hipMemsetAsync(alt_offsets, 0, sizeof(int32_t), s) != hipSuccess)
            return PMT_E_LAUNCH;
        return PMT_OK;
    }
    const int blocks = (num_variants + PMT_SCAN_SEG - 1) / PMT_SCAN_SEG;
    if (count_elem_bytes == 4)
        hipLaunchKernelGGL(pmt_scan_local_kernel<int32_t>, dim3(blocks, 2), dim3(1024), 0, s, (const int32_t*)ref_counts,
                           (const int32_t*)alt_counts, (long long)count_stride, num_variants, ref_offsets, alt_offsets);
    else
        hipLaunchKernelGGL(pmt_scan_local_kernel<int64_t>, dim3(blocks, 2), dim3(1024), 0, s, (const int64_t*)ref_counts,
                           (const int64_t*)alt_counts, (long long)count_stride, num_variants, ref_offsets, alt_offsets);
    if (blocks > 1) {
        hipLaunchKernelGGL(pmt_scan_offsets_kernel, dim3(2), dim3(64), 0, s, num_variants, ref_offsets, alt_offsets);
        hipLaunchKernelGGL(pmt_scan_add_kernel, dim3(blocks - 1, 2), dim3(1024), 0, s, num_variants, ref_offsets, alt_offsets);
    }
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}

// batch composition on the device: gather index of a batch drawn from a dataset chunk that is resident in HBM
// On disk (reference data/memory_mapped_data.py:39-40) a datum's rows are its ref reads then its alt reads; a batch wants
// all ref rows of all its variants, then all alt rows (reference data/batch.py:45-47).  One workgroup per variant.
__global__ __launch_bounds__(64) void pmt_read_index_kernel(const long long* __restrict__ row_start, const int* __restrict__ ref_off,
                                                            const int* __restrict__ alt_off, int nb, long long* __restrict__ index) {
    const int b = blockIdx.x;
    const int r0 = ref_off[b], nr = ref_off[b + 1] - r0, a0 = alt_off[b], na = alt_off[b + 1] - a0;
    const long long total_ref = ref_off[nb], start = row_start[b];
    for (int i = threadIdx.x; i < nr; i += 64) index[r0 + i] = start + i;
    for (int i = threadIdx.x; i < na; i += 64) index[total_ref + a0 + i] = start + nr + i;
}

extern "C" int pmt_build_read_index(const int64_t* row_start, const int32_t* ref_offsets, const int32_t* alt_offsets,
                                    int32_t num_variants, int64_t* read_index, void* stream) {
    if (!row_start || !ref_offsets || !alt_offsets || !read_index || num_variants < 0) return PMT_E_INVALID;
    if (num_variants == 0) return PMT_OK;
    hipLaunchKernelGGL(pmt_read_index_kernel, dim3(num_variants), dim3(64), 0, reinterpret_cast<hipStream_t>(stream),
                       (const long long*)row_start, ref_offsets, alt_offsets, num_variants, (long long*)read_index);
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}

// One batch composed from a chunk of the dataset that is resident in HBM as it lies on disk (reference data/batch.py:41-62 does
// this collate on the host, Datum by Datum): the batch's variants are rows `ids` of the chunk.  ONE call = the per-variant
// tables in the Batch's dtypes (int16 -> int64, float16 -> float32: reference data/batch.py:47-49), the rows' read offsets, the
// exclusive scans of the counts and the gather index of the reads (ref rows of all variants, then alt rows).
__global__ __launch_bounds__(256) void pmt_gather_rows_kernel(const short* __restrict__ ints, int int_cols, const _Float16* __restrict__ floats,
                                                              int float_cols, const long long* __restrict__ row_start,
                                                              const long long* __restrict__ ids, int n, long long* __restrict__ ints_out,
                                                              float* __restrict__ floats_out, long long* __restrict__ row_start_out) {
    // a 64-lane slice per variant row: coalesced along the columns
    const int rows_per_block = 256 / 64, lane = threadIdx.x & 63;
    const int b = blockIdx.x * rows_per_block + (threadIdx.x >> 6);
    if (b >= n) return;
    const long long src = ids[b];
    const short* ip = ints + (size_t)src * int_cols;
    for (int c = lane; c < int_cols; c += 64) ints_out[(size_t)b * int_cols + c] = (long long)ip[c];
    const _Float16* fp = floats + (size_t)src * float_cols;
    for (int c = lane; c < float_cols; c += 64) floats_out[(size_t)b * float_cols + c] = (float)fp[c];
    if (lane == 0) row_start_out[b] = row_start[src];
}

// The same with the exclusive scans of the counts already known (pmt_prepare_chunk computes them on the host, beside the group
// plan): ONE launch per batch -- a 64-lane slice per variant gathers its two table rows AND writes its entries of the read index --
// where pmt_compose_batch needs five (gather, three for the scans, one workgroup per variant for the index).  Composition runs
// beside the consumer's read-set kernels, which leave it only the slots their retiring workgroups free: every launch less counts.
__global__ __launch_bounds__(256) void pmt_compose_planned_kernel(const short* __restrict__ ints, int int_cols, const _Float16* __restrict__ floats,
                                                                  int float_cols, const long long* __restrict__ row_start,
                                                                  const long long* __restrict__ ids, int n, const int* __restrict__ ref_off,
                                                                  const int* __restrict__ alt_off, long long* __restrict__ ints_out,
                                                                  float* __restrict__ floats_out, long long* __restrict__ row_start_out,
                                                                  long long* __restrict__ index) {
    const int rows_per_block = 256 / 64, lane = threadIdx.x & 63;
    const int b = blockIdx.x * rows_per_block + (threadIdx.x >> 6);
    if (b >= n) return;
    const long long src = ids[b];
    const long long start = row_start[src];
    const int r0 = ref_off[b], nr = ref_off[b + 1] - r0, a0 = alt_off[b], na = alt_off[b + 1] - a0;
    const long long total_ref = ref_off[n];
    const short* ip = ints + (size_t)src * int_cols;
    for (int c = lane; c < int_cols; c += 64) ints_out[(size_t)b * int_cols + c] = (long long)ip[c];
    const _Float16* fp = floats + (size_t)src * float_cols;
    for (int c = lane; c < float_cols; c += 64) floats_out[(size_t)b * float_cols + c] = (float)fp[c];
    for (int i = lane; i < nr; i += 64) index[r0 + i] = start + i;
    for (int i = lane; i < na; i += 64) index[total_ref + a0 + i] = start + nr + i;
    if (lane == 0) row_start_out[b] = start;
}

extern "C" int pmt_compose_batch_planned(const int16_t* chunk_ints, int32_t int_cols, const void* chunk_floats_f16, int32_t float_cols,
                                         const int64_t* chunk_row_start, const int64_t* ids, int32_t num_variants,
                                         const int32_t* ref_offsets, const int32_t* alt_offsets, int64_t* int_tensor, float* float_tensor,
                                         int64_t* row_start, int64_t* read_index, void* stream) {
    if (!chunk_ints || !chunk_floats_f16 || !chunk_row_start || !ids || !int_tensor || !float_tensor || !row_start || !ref_offsets ||
        !alt_offsets || !read_index || num_variants < 0 || int_cols < 2 || float_cols < 1)
        return PMT_E_INVALID;
    if (num_variants == 0) return PMT_OK;
    hipLaunchKernelGGL(pmt_compose_planned_kernel, dim3((num_variants + 3) / 4), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       (const short*)chunk_ints, int_cols, (const _Float16*)chunk_floats_f16, float_cols, (const long long*)chunk_row_start,
                       (const long long*)ids, num_variants, ref_offsets, alt_offsets, (long long*)int_tensor, float_tensor, (long long*)row_start,
                       (long long*)read_index);
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}

extern "C" int pmt_compose_batch(const int16_t* chunk_ints, int32_t int_cols, const void* chunk_floats_f16, int32_t float_cols,
                                 const int64_t* chunk_row_start, const int64_t* ids, int32_t num_variants, int32_t ref_col, int32_t alt_col,
                                 int64_t* int_tensor, float* float_tensor, int64_t* row_start, int32_t* ref_offsets, int32_t* alt_offsets,
                                 int64_t* read_index, void* stream) {
    if (!chunk_ints || !chunk_floats_f16 || !chunk_row_start || !ids || !int_tensor || !float_tensor || !row_start || !ref_offsets ||
        !alt_offsets || !read_index || num_variants < 0 || int_cols < 2 || float_cols < 1 || ref_col < 0 || alt_col < 0 || ref_col >= int_cols ||
        alt_col >= int_cols)
        return PMT_E_INVALID;
    if (num_variants == 0) return pmt_scan_counts(int_tensor, int_tensor, 8, int_cols, 0, ref_offsets, alt_offsets, stream);
    hipLaunchKernelGGL(pmt_gather_rows_kernel, dim3((num_variants + 3) / 4), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       (const short*)chunk_ints, int_cols, (const _Float16*)chunk_floats_f16, float_cols, (const long long*)chunk_row_start,
                       (const long long*)ids, num_variants, (long long*)int_tensor, float_tensor, (long long*)row_start);
    if (hipGetLastError() != hipSuccess) return PMT_E_LAUNCH;
    int rc = pmt_scan_counts(int_tensor + ref_col, int_tensor + alt_col, 8, int_cols, num_variants, ref_offsets, alt_offsets, stream);
    if (rc != PMT_OK) return rc;
    return pmt_build_read_index(row_start, ref_offsets, alt_offsets, num_variants, read_index, stream);
}
