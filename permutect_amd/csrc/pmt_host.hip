// The host-only part of the C ABI, no kernel: what this build is (ABI version, build id, struct sizes, shape, limits), which instance a
// model runs in it and whether it can run at all (pmt_shape_id, pmt_model_shape, pmt_model_check), the stash size, the staging copies
// and the dropout-mask mirror.  The one object that depends on every source of the tree: it embeds their hash (PMT_BUILD_ID).
#include <hip/hip_runtime.h>
#include <string.h>

#include "pmt_device.hpp"
#include "pmt_jobs.hpp"

extern "C" int pmt_abi_version(void) { return PMT_ABI_VERSION; }
#ifndef PMT_BUILD_ID
#define PMT_BUILD_ID "0000000000000000"  // (csrc/Makefile passes the hash of the sources)
#endif
extern "C" int pmt_build_id(char* out, int32_t capacity) {
    static const char tagged[] = "PMT_BUILD_ID=" PMT_BUILD_ID;  // (the tag: engine/instances.py reads the id out of the FILE of a library it has not mapped)
    const char* id = tagged + 13;
    const int n = (int)sizeof(tagged) - 13;
    if (!out || capacity < n) return PMT_E_INVALID;
    memcpy(out, id, n);
    return n - 1;
}

extern "C" int pmt_struct_bytes(int which) {
    switch (which) {
        case 0: return (int)sizeof(PmtModel);
        case 1: return (int)sizeof(PmtBatch);
        case 2: return (int)sizeof(PmtOutputs);
        case 3: return (int)sizeof(PmtOutputGrads);
        case 4: return (int)sizeof(PmtAdamW);
        case 5: return (int)sizeof(PmtLinear);
        case 6: return (int)sizeof(PmtOp);
        case 7: return (int)sizeof(PmtMlp);
        case 8: return (int)sizeof(PmtBlock);
        case 9: return (int)sizeof(PmtHead);
        case 10: return (int)sizeof(PmtPhiProgram);
        case 11: return (int)sizeof(PmtLossArgs);
        case 12: return (int)sizeof(PmtDownsample);
        case 13: return (int)sizeof(PmtRecordArgs);
        case 14: return (int)sizeof(PmtBalanceArgs);
        case 15: return (int)sizeof(PmtEvalArgs);
        case 16: return (int)sizeof(PmtPosteriorRows);
        case 17: return (int)sizeof(PmtPosteriorParams);
        case 18: return (int)sizeof(PmtPruneArgs);
        case 19: return (int)sizeof(PmtPruneStats);
        case 20: return (int)sizeof(PmtWorstArgs);
        case 21: return (int)sizeof(PmtPosteriorEvalArgs);
        case 22: return (int)sizeof(PmtAnnotateArgs);
        case 23: return (int)sizeof(PmtPreprocessArgs);
        case 24: return (int)sizeof(PmtSiteKeysArgs);
        case 25: return (int)sizeof(PmtVcfArgs);
        default: return PMT_E_INVALID;
    }
}

extern "C" int pmt_stash_slots(const PmtModel* m) { return (m->read_mlp.n_ops - 1) + (m->num_blocks + 1) + (m->reducer.n_ops - 1) + m->num_blocks; }
extern "C" size_t pmt_stash_bytes(const PmtModel* m, int64_t total_tiles, int32_t num_variants) {
    if (!m) return 0;
    const size_t tile_part = (size_t)total_tiles * (size_t)pmt_stash_slots(m) * PMT_SLOT_FLOATS;
    const size_t nb = (size_t)(m->num_blocks > 0 ? m->num_blocks : 1);
    const size_t zsum_part = (size_t)num_variants * nb * PMT_ZW;   // per-set z2 sums of every block
    const size_t rstd_part = (size_t)total_tiles * nb * 16;    // LayerNorm(D) rstd of every read of every block
    return (tile_part + zsum_part + rstd_part) * sizeof(float);
}

// Which register-array shape the read-set kernels run with (pmt_device.hpp: Shape; the tile counts and widths of the exact
// instances are the BUILD's shape, PMT_SH_*: the production hyperparameters by default).  The ids: permutect_amd.h, PMT_SHAPE_*.
//   ANY = ShapeAny: any supported model;
//   TILES_F32 = ShapeP0: every layer fills the shape's tile arrays exactly -- read features and the first read linear NTF -> NTR tiles,
//       the rest of the read MLP NTR wide, d_model and the reducer NTD wide up to a last LINEAR NTD -> NTE, feature_dim NTE -- fp32
//       MFMAs, widths at run time (PMT_FORCE_TILES_F32 only);
//   TILES = ShapeP0T / ShapeP0TH: the same tile-exact models on the 16-bit matrix pipes, widths at run time;
//   EXACT = ShapeP0X / ShapeP0XH: additionally every width equals the build's (compiled in); EXACT_BF16 = the same with plain bf16 products.
// PMT_FORCE_ANY / PMT_FORCE_TILES_F32 force the generic / the fp32 tile-exact instance (the parity tests cover all).
extern "C" int pmt_shape_info(int32_t* nine) {  // the build's shape: tile counts NTF, NTR, NTD, NTE, then widths F, R, D, H, E
    const int32_t v[9] = {PMT_SH_NTF, PMT_SH_NTR, PMT_SH_NTD, PMT_SH_NTE, PMT_SH_F, PMT_SH_R, PMT_SH_D, PMT_SH_H, PMT_SH_E};
    if (nine) memcpy(nine, v, sizeof(v));
    return PMT_OK;
}
static int tiles_of(int dim) { return (dim + 15) / 16; }
// ops [first, last) of an MLP keep `nt` tiles; *same_width is cleared when some layer of them is not exactly `width` wide
static bool mlp_ops_fill(const PmtModel* m, const PmtMlp* mlp, int first, int last, int nt, int width, bool* same_width) {
    for (int i = first; i < last; ++i) {
        const PmtOp* o = &mlp->ops[i];
        const int nl = o->kind == PMT_OP_SKIP ? o->n_layers : 1;
        if (nl > 2) return false;  // (skip blocks of three and four layers: the generic instances' interpreter only)
        for (int k = 0; k < nl; ++k) {
            const PmtLinear* L = &m->lin[o->lin[k]];
            if (tiles_of(L->in_dim) != nt || tiles_of(L->out_dim) != nt) return false;
            if (L->in_dim != width || L->out_dim != width) *same_width = false;
        }
    }
    return true;
}
// The tile-exact shape a model fills, if any (permutect_amd.h: pmt_model_shape): the read features and the first read linear NTF -> NTR
// tiles, the rest of the read MLP NTR wide, d_model and the reducer NTD wide up to a last LINEAR NTD -> NTE, feature_dim NTE.
// *same_width: additionally every layer has exactly the width of its place (F, R, D, H, E), what compiled-in widths need.
static int model_shape(const PmtModel* m, int32_t* nine, bool* same_width) {
    const PmtMlp* rm = &m->read_mlp;
    const PmtMlp* red = &m->reducer;
    if (rm->n_ops < 1 || red->n_ops < 1) return PMT_E_UNSUPPORTED;
    const PmtOp* first = &rm->ops[0];
    const PmtOp* last = &red->ops[red->n_ops - 1];
    if (first->kind != PMT_OP_LINEAR || last->kind != PMT_OP_LINEAR) return PMT_E_UNSUPPORTED;
    const PmtLinear* Lf = &m->lin[first->lin[0]];
    const PmtLinear* Ll = &m->lin[last->lin[0]];
    const int F = m->num_read_features, R = Lf->out_dim, D = m->d_model, H = m->d_ffn / 2, E = m->feature_dim;
    const int32_t v[9] = {tiles_of(F), tiles_of(R), tiles_of(D), tiles_of(E), F, R, D, H, E};
    *same_width = Lf->in_dim == F && m->read_embed_dim == R && m->d_ffn == 2 * H && Ll->in_dim == D && Ll->out_dim == E;
    const bool ok = tiles_of(Lf->in_dim) == v[0] && mlp_ops_fill(m, rm, 1, rm->n_ops, v[1], R, same_width) && tiles_of(m->read_embed_dim) == v[1] &&
                    m->d_ffn >= 2 && mlp_ops_fill(m, red, 0, red->n_ops - 1, v[2], D, same_width) && tiles_of(Ll->in_dim) == v[2] &&
                    tiles_of(Ll->out_dim) == v[3];
    if (!ok || v[0] > 8 || v[1] > 8 || v[2] > 8 || v[3] > 8) return PMT_E_UNSUPPORTED;  // (more than four tiles: the wide build's 8-tile register arrays, csrc/Makefile)
    if (nine) memcpy(nine, v, sizeof(v));
    return PMT_OK;
}
extern "C" int pmt_model_shape(const PmtModel* m, int32_t* nine) { bool w; return m ? model_shape(m, nine, &w) : PMT_E_INVALID; }
extern "C" int pmt_limits(int32_t* four) {  // the build's compile-time limits: widest activation, d_ffn / 2, floats of a stash slot, waves per group
    const int32_t v[4] = {PMT_MAX_WIDTH, PMT_MAX_HALF_FFN, PMT_MAX_WIDTH * 16, PMT_GROUP_WAVES};
    if (four) memcpy(four, v, sizeof(v));
    return PMT_OK;
}
extern "C" int pmt_shape_id(const PmtModel* m) {
    if (m->force_shape == PMT_FORCE_ANY || PMT_GENERIC_ONLY) return PMT_SHAPE_ANY;  // (PMT_FORCE_FWD_BF16X3 = auto for every kernel but the forward, whose launchers read it themselves)
    int32_t model[9], build[9];
    bool same_width;
    pmt_shape_info(build);
    if (m->num_blocks < 0 || model_shape(m, model, &same_width) != PMT_OK || memcmp(model, build, 4 * sizeof(int32_t)) != 0) return PMT_SHAPE_ANY;
    if (m->force_shape == PMT_FORCE_TILES_F32) return PMT_SHAPE_TILES_F32;
    const bool exact = same_width && memcmp(model + 4, build + 4, 5 * sizeof(int32_t)) == 0;
    if (!exact) return PMT_SHAPE_TILES;  // the shape's tiles, other widths: the 16-bit pipes with the widths read at run time
    return m->force_shape == PMT_FORCE_EXACT_BF16 ? PMT_SHAPE_EXACT_BF16 : PMT_SHAPE_EXACT;  // (plain bf16 products: asked for explicitly only)
}

// ---------------------------------------------------------------------------------------------------------------------
// descriptor validation
// ---------------------------------------------------------------------------------------------------------------------
static int check_linear(const PmtModel* m, int id, int in_dim, int out_dim, int max_in = PMT_MAX_WIDTH) {
    if (id < 0 || id >= m->n_linear) return PMT_E_INVALID;
    const PmtLinear* l = &m->lin[id];
    if (l->in_dim != in_dim || l->out_dim != out_dim) return PMT_E_INVALID;
    if (in_dim < 1 || out_dim < 1 || in_dim > max_in || out_dim > PMT_MAX_WIDTH) return PMT_E_UNSUPPORTED;
    if (l->w_frag < 0 || l->wt_frag < 0 || (l->w_frag & 3) || (l->wt_frag & 3)) return PMT_E_INVALID;
    if (l->b_pvec >= 0 && (l->b_pvec & 3)) return PMT_E_INVALID;
    return PMT_OK;
}

static int check_mlp(const PmtModel* m, const PmtMlp* mlp, int max_in = PMT_MAX_WIDTH) {
    if (mlp->n_ops < 1 || mlp->n_ops > PMT_MAX_OPS) return PMT_E_UNSUPPORTED;
    int width = mlp->in_dim;
    if (width > PMT_MAX_WIDTH && mlp->ops[0].kind != PMT_OP_LINEAR) return PMT_E_UNSUPPORTED;
    for (int i = 0; i < mlp->n_ops; ++i) {
        const PmtOp* o = &mlp->ops[i];
        if (o->kind == PMT_OP_LINEAR) {
            if (o->lin[0] < 0 || o->lin[0] >= m->n_linear) return PMT_E_INVALID;
            const int out = m->lin[o->lin[0]].out_dim;
            const int rc = check_linear(m, o->lin[0], width, out, i == 0 ? max_in : PMT_MAX_WIDTH);
            if (rc) return rc;
            width = out;
        } else if (o->kind == PMT_OP_SKIP) {
            if (o->n_layers < 1 || o->n_layers > PMT_MAX_SKIP_LAYERS) return PMT_E_UNSUPPORTED;  /* (three and four: the generic instances, pmt_shape_id) */
            if (o->alpha_src < 0) return PMT_E_INVALID;
            for (int k = 0; k < o->n_layers; ++k) {
                const int rc = check_linear(m, o->lin[k], width, width);
                if (rc) return rc;
                if (m->lin[o->lin[k]].b_pvec < 0) return PMT_E_INVALID;
            }
        } else {
            return PMT_E_INVALID;
        }
    }
    return width == mlp->out_dim ? PMT_OK : PMT_E_INVALID;
}

extern "C" int pmt_model_check(const PmtModel* m) {
    if (!m || m->abi_version != PMT_ABI_VERSION) return PMT_E_INVALID;
    if (m->n_linear < 1 || m->n_linear > PMT_MAX_LINEAR) return PMT_E_UNSUPPORTED;
    if (m->num_read_features < 1 || m->num_read_features > PMT_MAX_WIDTH) return PMT_E_UNSUPPORTED;
    if (m->d_model != m->read_embed_dim + m->variant_embed_dim || m->d_model > PMT_MAX_WIDTH) return PMT_E_UNSUPPORTED;
    if (m->d_ffn < 2 || (m->d_ffn & 1) || m->d_ffn / 2 > PMT_MAX_HALF_FFN) return PMT_E_UNSUPPORTED;
    if (m->num_blocks > 0 && (m->d_ffn / 2 + 15) / 16 != PMT_HT) return PMT_E_UNSUPPORTED;  // (the two-tile layout of a PMT_MAX_HALF_FFN = 32 build is not the one-tile model's)
    if (m->num_blocks < 0 || m->num_blocks > PMT_MAX_BLOCKS) return PMT_E_UNSUPPORTED;
    if (m->feature_dim < 2 || m->feature_dim > PMT_MAX_WIDTH) return PMT_E_UNSUPPORTED;
    if (m->num_clusters < 1 || m->num_clusters > PMT_MAX_CLUSTERS) return PMT_E_UNSUPPORTED;
    if (!(m->dropout_p >= 0.f && m->dropout_p < 1.f)) return PMT_E_INVALID;
    if (m->read_mlp.in_dim != m->num_read_features || m->read_mlp.out_dim != m->read_embed_dim) return PMT_E_INVALID;
    if (m->reducer.in_dim != m->d_model || m->reducer.out_dim != m->feature_dim) return PMT_E_INVALID;
    int rc = check_mlp(m, &m->read_mlp);
    if (rc) return rc;
    rc = check_mlp(m, &m->reducer);
    if (rc) return rc;
    for (int k = 0; k < 3; ++k) {
        if (m->row_mlp[k].n_ops == 0 && k == PMT_ROWS_SOURCE) continue;
        if ((rc = check_mlp(m, &m->row_mlp[k], PMT_MAX_ROW_INPUT))) return rc;
    }
    const int h = m->d_ffn / 2;
    for (int l = 0; l < m->num_blocks; ++l) {
        const PmtBlock* b = &m->blocks[l];
        for (int s = 0; s < 2; ++s) {
            if ((rc = check_linear(m, b->proj1[s], m->d_model, m->d_ffn))) return rc;
            if (m->lin[b->proj1[s]].out_split != h || m->lin[b->proj1[s]].b_pvec < 0) return PMT_E_INVALID;
            if ((rc = check_linear(m, b->proj2[s], h, m->d_model))) return rc;
            if (m->lin[b->proj2[s]].b_pvec < 0) return PMT_E_INVALID;
        }
    }
    if ((rc = check_linear(m, m->rotation_lin, m->feature_dim, m->feature_dim))) return rc;
    return PMT_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// host staging copy (dataset chunk -> pinned buffer), multi-threaded and GIL-free
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int pmt_host_copy(void* dst, const void* src, size_t bytes, int32_t threads) {
    if ((!dst || !src) && bytes > 0) return PMT_E_INVALID;
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    const size_t min_part = (size_t)1 << 20;
    size_t parts = bytes / min_part;
    if (parts > (size_t)threads) parts = (size_t)threads;
    if (parts <= 1) {
        memcpy(dst, src, bytes);
        return PMT_OK;
    }
    const size_t per = ((bytes / parts) + 4095) & ~(size_t)4095;
    const int jobs = (int)((bytes + per - 1) / per);  // (<= parts: rounding `per` up to pages can leave the last parts empty)
    for_each_job(jobs, jobs, [=](int i) {
        const size_t lo = (size_t)i * per, hi = i + 1 == jobs ? bytes : lo + per;
        memcpy((char*)dst + lo, (const char*)src + lo, hi - lo);
    });
    return PMT_OK;
}

// The dropout masks as the kernels generate them (pmt_dropout.hpp), for the parity tests.
extern "C" int pmt_dropout_mask(uint64_t seed, float p, int32_t lin, int64_t row0, int64_t rows, int32_t width, float* out) {
    if (!out || rows < 0 || width < 0 || !(p >= 0.f && p < 1.f) || lin < 0) return PMT_E_INVALID;
    const unsigned thresh = pmt_drop_threshold(p);
    const float scale = 1.0f / (1.0f - p);
    for (int64_t r = 0; r < rows; ++r) {
        const unsigned key = pmt_drop_row_key((unsigned)seed, (unsigned)(seed >> 32), lin, (int)(row0 + r));
        for (int f = 0; f < width; ++f) out[r * width + f] = (seed == 0 || pmt_drop_keep(key, f, thresh)) ? (seed == 0 ? 1.0f : scale) : 0.f;
    }
    return PMT_OK;
}

// The same for a table of fixed-size rows, with one byte range of every row cleared on the way (the posterior hand-off's integer
// rows are the dataset's own with the two read counts zeroed, reference tools/filter_variants.py:305-308): one pass over the
// memory instead of a copy and a strided clearing pass.
extern "C" int pmt_host_copy_rows(void* dst, const void* src, int64_t rows, int64_t row_bytes, int64_t zero_offset, int64_t zero_bytes,
                                  int32_t threads) {
    if (rows < 0 || row_bytes < 1 || zero_offset < 0 || zero_bytes < 0 || zero_offset + zero_bytes > row_bytes) return PMT_E_INVALID;
    if ((!dst || !src) && rows > 0) return PMT_E_INVALID;
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    int64_t parts = rows * row_bytes / ((int64_t)1 << 20);
    if (parts > threads) parts = threads;
    if (parts < 1) parts = 1;
    auto work = [=](int64_t lo, int64_t hi) {
        char* d = (char*)dst + lo * row_bytes;
        memcpy(d, (const char*)src + lo * row_bytes, (size_t)((hi - lo) * row_bytes));
        if (zero_bytes > 0)
            for (int64_t r = 0; r < hi - lo; ++r) memset(d + r * row_bytes + zero_offset, 0, (size_t)zero_bytes);
    };
    // (blocks of 4096 rows: the clearing pass then finds the rows it just copied in the cache)
    for_each_job((int)parts, (int)parts, [=](int i) {
        const int64_t lo = rows * i / parts, hi = rows * (i + 1) / parts;
        for (int64_t b = lo; b < hi; b += 4096) work(b, b + 4096 < hi ? b + 4096 : hi);
    });
    return PMT_OK;
}
