// The parameter re-pack: theta / phi in their natural layouts -> MFMA fragment order, 16-bit pieces, tile-position vectors and the
// weight-gradient emit tables of `packed` (pmt_pack_params, one launch per optimizer step).
#include <hip/hip_runtime.h>

#include "pmt_device.hpp"

// parameter re-pack: natural layouts (theta / phi) -> MFMA A-fragment order and tile-position vectors
// virtual row -> source row for a linear whose output rows are split into two 16-row tiles (out_split = h)
DEV int split_row(int v, int h) {
    if (h <= 0) return v;
    if (v < PMT_SPLIT0) return v < h ? v : -1;
    return (v - PMT_SPLIT0) < h ? h + (v - PMT_SPLIT0) : -1;
}

// one job per workgroup: (lin, 0) forward frags, (lin, 1) transposed frags, (lin, 2) bias, (lin, 3 / 4) the same two matrices
// as bf16 pieces, (lin, 5) the weight-gradient emit table, (lin, 6) the forward matrix as two f16 pieces, then per-block vectors
#define PMT_PACK_KINDS 7
// bias_cols: the model runs the exact-width instances of the read-set backward (PMT_SHAPE_EXACT / _EXACT_BF16), whose weight-gradient exchange sums
// a bias gradient in the padding column in_dim of dW (pmt_bwd_device.hpp: PMT_BC_OF)
__global__ void pmt_pack_kernel(const PmtModel* __restrict__ M, const float* __restrict__ theta,
                                const float* __restrict__ phi, float* __restrict__ packed, int bias_cols) {
    const int job = blockIdx.x;
    const int n_lin_jobs = M->n_linear * PMT_PACK_KINDS;
    if (job < n_lin_jobs) {
        const PmtLinear& L = M->lin[job / PMT_PACK_KINDS];
        const int kind = job % PMT_PACK_KINDS;
        const int h = L.out_split;
        const int out_v = h > 0 ? PMT_SPLIT0 + h : L.out_dim;  // virtual output rows
        if (kind == 5) {
            // PmtLinear.emit_tab: destination of every element of every 16 x 16 block of dW as the matrix core leaves it
            // (C layout: lane (g, c) register j = row position 4 g + j, column position c; position p of a tile = feature
            // 4 (p & 3) + (p >> 2), pmt_device.hpp), then the bias gradient's destinations per out tile in position order
            if (L.emit_tab < 0) return;
            int* tab = reinterpret_cast<int*>(packed + L.emit_tab);
            const int nmt = (out_v + 15) >> 4, nkt = (L.in_dim + 15) >> 4;
            const int w_off = L.w_src >= 0 ? L.w_src : -(L.w_src + 2);
            // A width that leaves padding in its last input tile, in a model of the exact-width instances: column in_dim of row o is the
            // bias gradient of row o (the kernel stages 1.0 at that position of x) and the bias tail stays empty.  The column lands in
            // the buffer of the weights, so a bias that lives elsewhere has no destination (as in the tail).
            const bool bias_col = bias_cols != 0 && (L.in_dim & 15) != 0;
            const bool bias_same = L.w_src >= 0 && L.b_src >= 0;
            for (int i = threadIdx.x; i < nmt * nkt * 256; i += blockDim.x) {
                const int j = i & 3, lane = (i >> 2) & 63, blk = i >> 8;
                const int ot = blk / nkt, it = blk - ot * nkt;
                const int pf = 16 * ot + 4 * j + (lane >> 4), o = pf < out_v ? split_row(pf, h) : -1;
                const int cp = lane & 15, col = 16 * it + 4 * (cp & 3) + (cp >> 2);
                tab[i] = (o >= 0 && o < L.out_dim && col < L.in_dim) ? w_off + o * L.in_dim + col
                         : (bias_col && bias_same && o >= 0 && o < L.out_dim && col == L.in_dim) ? L.b_src + o : -1;
            }
            int* btab = tab + nmt * nkt * 256;
            for (int i = threadIdx.x; i < nmt * 16; i += blockDim.x) {
                const int p = i & 15, pf = 16 * (i >> 4) + 4 * (p & 3) + (p >> 2), o = pf < out_v ? split_row(pf, h) : -1;
                btab[i] = (!bias_col && L.b_src >= 0 && o >= 0 && o < L.out_dim) ? L.b_src + o : -1;
            }
            return;
        }
        if (kind == 6) {
            // PmtLinear.wh_frag: two f16 pieces per weight, (out tile, k block) order, the element order of the bf16 pieces
            // below.  hi = f16(w), lo = f16(2^12 (w - hi)): w - hi is exact in fp32 and at most 2^-11 |w|, so the scaled low
            // piece is a NORMAL f16 with all 11 bits wherever hi is normal (unscaled it would be a denormal for |w| < 1/4 --
            // every weight of a 60-wide layer); linear_acc_f16 keeps the products of the low pieces in an accumulator of
            // their own and scales it back.  |w| beyond the f16 range saturates at 65504 (no trained weight is near it).
            if (L.wh_frag < 0) return;
            const float* W = src_ptr(L.w_src, theta, phi);
            const int nmt = (out_v + 15) >> 4, nkt = (L.in_dim + 15) >> 4, nkb = (nkt + 1) >> 1;
            _Float16* dst = reinterpret_cast<_Float16*>(packed + L.wh_frag);
            const int total = nkb * nmt * 512;
            for (int i = threadIdx.x; i < total; i += blockDim.x) {
                const int e = i & 7, lane = (i >> 3) & 63, blk = i >> 9;
                const int kb = blk % nkb, mt = blk / nkb;
                const int m = lane & 15, kg = lane >> 4;
                const int mv = 16 * mt + 4 * (m & 3) + (m >> 2);
                const int kv = 16 * (2 * kb + (e >> 2)) + 4 * (e & 3) + kg;
                float val = 0.f;
                if (mv < out_v && kv < L.in_dim && (2 * kb + (e >> 2)) < nkt) {
                    const int orow = split_row(mv, h);
                    if (orow >= 0 && orow < L.out_dim) val = W[(size_t)orow * L.in_dim + kv];
                }
                val = fminf(fmaxf(val, -65504.f), 65504.f);
                const _Float16 hi = (_Float16)val;
                const _Float16 lo = (_Float16)((val - (float)hi) * 4096.f);
                const size_t base = (size_t)blk * 2 * 512 + lane * 8 + e;
                dst[base] = hi;
                dst[base + 512] = lo;
            }
            return;
        }
        if (kind >= 3) {
            // k block kb of 32 = activation tiles 2 kb and 2 kb + 1; lane (m, kg) element e: tile 2 kb + (e >> 2), register
            // e & 3 of lane group kg, i.e. the SAME feature order as the fp32 activation registers, so a layer's C-layout
            // output still feeds the next layer without any shuffle
            const int off = kind == 3 ? L.wb_frag : L.wtb_frag;
            if (off < 0) return;
            const float* W = src_ptr(L.w_src, theta, phi);
            const int Mv = kind == 3 ? out_v : L.in_dim, Kv = kind == 3 ? L.in_dim : out_v;
            const int nmt = (Mv + 15) >> 4, nkt = (Kv + 15) >> 4, nkb = (nkt + 1) >> 1;
            __bf16* dst = reinterpret_cast<__bf16*>(packed + off);
            const int total = nkb * nmt * 512;
            for (int i = threadIdx.x; i < total; i += blockDim.x) {
                const int e = i & 7, lane = (i >> 3) & 63, blk = i >> 9;
                const int mt = blk % nmt, kb = blk / nmt;
                const int m = lane & 15, kg = lane >> 4;
                const int mv = 16 * mt + 4 * (m & 3) + (m >> 2);
                const int kv = 16 * (2 * kb + (e >> 2)) + 4 * (e & 3) + kg;
                float val = 0.f;
                if (mv < Mv && kv < Kv && (2 * kb + (e >> 2)) < nkt) {
                    const int orow = kind == 3 ? split_row(mv, h) : split_row(kv, h);
                    const int icol = kind == 3 ? kv : mv;
                    if (orow >= 0 && orow < L.out_dim && icol < L.in_dim) val = W[(size_t)orow * L.in_dim + icol];
                }
                __bf16 hi, mid, lo;
                split_bf16x3(val, hi, mid, lo);
                const size_t base = (size_t)blk * 3 * 512 + lane * 8 + e;
                dst[base] = hi;
                dst[base + 512] = mid;
                dst[base + 1024] = lo;
            }
            return;
        }
        if (kind == 2) {
            if (L.b_pvec < 0) return;
            const float* b = src_ptr(L.b_src, theta, phi);
            const int n = ((out_v + 15) >> 4) * 16;
            for (int i = threadIdx.x; i < n; i += blockDim.x) {
                const int t = i >> 4, g = (i >> 2) & 3, j = i & 3;
                const int v = 16 * t + 4 * j + g;
                const int r = v < out_v ? split_row(v, h) : -1;
                packed[L.b_pvec + i] = (r >= 0 && r < L.out_dim) ? b[r] : 0.f;
            }
            return;
        }
        const float* W = src_ptr(L.w_src, theta, phi);
        // forward: A_v[m][k] = W[row(m)][k], Mv = out_v, Kv = in_dim; transposed: A_v[m][k] = W[row(k)][m]
        const int Mv = kind == 0 ? out_v : L.in_dim, Kv = kind == 0 ? L.in_dim : out_v;
        const int nmt = (Mv + 15) >> 4, nkt = (Kv + 15) >> 4;
        float* dst = packed + (kind == 0 ? L.w_frag : L.wt_frag);
        const int total = nmt * nkt * 256;
        for (int i = threadIdx.x; i < total; i += blockDim.x) {
            const int j = i & 3, lane = (i >> 2) & 63, tile = i >> 8;
            const int mt = tile % nmt, kt = tile / nmt;  // kt-major: the order linear_acc walks the fragments
            const int m = lane & 15, g = lane >> 4;
            const int mv = 16 * mt + 4 * (m & 3) + (m >> 2);
            const int kv = 16 * kt + 4 * j + g;
            float val = 0.f;
            if (mv < Mv && kv < Kv) {
                const int orow = kind == 0 ? split_row(mv, h) : split_row(kv, h);
                const int icol = kind == 0 ? kv : mv;
                if (orow >= 0 && orow < L.out_dim && icol < L.in_dim) val = W[(size_t)orow * L.in_dim + icol];
            }
            dst[i] = val;
        }
        return;
    }
    int v = job - n_lin_jobs;  // vector jobs
    int src = -1, dst = -1, n = 0;
    if (v < M->num_blocks * 5) {
        const PmtBlock& B = M->blocks[v / 5];
        const int hh = M->d_ffn / 2;
        switch (v % 5) {
            case 0: src = B.norm_w_src; dst = B.norm_w_pvec; n = M->d_model; break;
            case 1: src = B.norm_b_src; dst = B.norm_b_pvec; n = M->d_model; break;
            case 2: src = B.sgu_norm_w_src; dst = B.sgu_norm_w_pvec; n = hh; break;
            case 3: src = B.sgu_norm_b_src; dst = B.sgu_norm_b_pvec; n = hh; break;
            default: src = B.ref_reg_src; dst = B.ref_reg_pvec; n = hh; break;
        }
    } else {
        src = M->translation_src; dst = M->translation_pvec; n = M->feature_dim;
    }
    const int padded = ((n + 15) >> 4) * 16;
    const float* s = src_ptr(src, theta, phi);
    for (int i = threadIdx.x; i < padded; i += blockDim.x) {
        const int t = i >> 4, g = (i >> 2) & 3, j = i & 3;
        const int f = 16 * t + 4 * j + g;
        packed[dst + i] = f < n ? s[f] : 0.f;
    }
}

extern "C" int pmt_pack_params(const PmtModel* model_host, const PmtModel* model_dev, const float* theta,
                               const float* phi, float* packed, void* stream) {
    if (!model_host || !model_dev || !theta || !packed) return PMT_E_INVALID;
    const int rc = pmt_model_check(model_host);
    if (rc) return rc;
    const int jobs = model_host->n_linear * PMT_PACK_KINDS + model_host->num_blocks * 5 + 1;
    const int shape = pmt_shape_id(model_host);
    hipLaunchKernelGGL(pmt_pack_kernel, dim3(jobs), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), model_dev, theta,
                       phi, packed, (shape == PMT_SHAPE_EXACT || shape == PMT_SHAPE_EXACT_BF16) ? 1 : 0);
    return hipGetLastError() == hipSuccess ? PMT_OK : PMT_E_LAUNCH;
}
