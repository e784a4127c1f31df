/*
 * permutect_amd.h -- C ABI of the MI355X (gfx950) engine for the Permutect artifact-model hot path.
 *
 * The reference (broadinstitute/permutect) is pure Python on PyTorch and has no FFI or operator registry; the seam
 * this library plugs into is the Python object boundary of `ArtifactModel`
 * (reference permutect/architecture/artifact_model.py:239-325) plus `backpropagate`
 * (reference permutect/misc_utils.py:125-129).  Each entry point below names the reference code it replaces.
 * INTEGRATION.md shows the ctypes binding a maintainer would add on the reference side.
 *
 * Conventions
 *   - plain C: pointers + sizes only.  Device pointers are raw HBM addresses; `stream` is a hipStream_t passed as
 *     void* (NULL = default stream).  The caller owns every buffer; the library allocates nothing on the device
 *     and keeps no global state, so it is thread-safe per stream and graph-capturable.
 *   - every function returns 0 on success or a negative PMT_E_* code; it never throws and never falls back to a
 *     CPU path.
 *   - offsets inside descriptors are in units of floats into the buffer named in the field comment.
 */
#ifndef PERMUTECT_AMD_H
#define PERMUTECT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMT_ABI_VERSION 12

/* bits of the fault word (PmtBatch.join_fault) */
#define PMT_FAULT_JOIN 1
#define PMT_FAULT_F16_RANGE 2
#define PMT_FAULT_PLAN 4        /* pmt_plan_groups_device: more groups than the capacity given, or a read set beyond one workgroup */

/* error codes */
#define PMT_OK 0
#define PMT_E_INVALID (-1)      /* bad argument / descriptor out of supported range */
#define PMT_E_UNSUPPORTED (-2)  /* configuration the gfx950 kernels do not cover (stated in DESIGN.md) */
#define PMT_E_CAPACITY (-3)     /* a read set does not fit the register-resident group capacity */
#define PMT_E_LAUNCH (-4)       /* HIP launch failure (hipGetLastError is left set) */
#define PMT_E_WORKSPACE (-5)    /* workspace too small */

/* compile-time limits of the kernels */
#ifndef PMT_MAX_WIDTH
#define PMT_MAX_WIDTH 64        /* widest activation (features) kept register-resident: 4 tiles of 16.  The WIDE build of the
                                   library (csrc/Makefile: `make wide`, -DPMT_MAX_WIDTH=128) keeps 8: pmt_limits() reports it */
#endif
#ifndef PMT_MAX_HALF_FFN
#define PMT_MAX_HALF_FFN 16     /* d_ffn / 2: one 16-feature tile per half of a gated block's hidden layer.  A build with 32 (csrc/Makefile:
                                   `make wide32`) gives every half TWO tiles -- it runs models with d_ffn / 2 in 17 .. 32 only */
#endif
#define PMT_MAX_CLUSTERS 16
#define PMT_MAX_OPS 8           /* top-level ops per MLP program */
#define PMT_MAX_ROW_INPUT 128    /* widest input of a per-variant row MLP (info vector) */
#define PMT_MAX_CNN_TAPS 192     /* widest im2col column of a haplotype-CNN convolution: in_channels * kernel_size (64 x 3; 32 x 5) */
#define PMT_ROWS_INFO 0
#define PMT_ROWS_ALT_COUNT 1
#define PMT_ROWS_SOURCE 2
#define PMT_MAX_SKIP_LAYERS 4
#define PMT_MAX_BLOCKS 16
#define PMT_MAX_LINEAR 96
#ifndef PMT_GROUP_WAVES
#define PMT_GROUP_WAVES 8       /* waves per workgroup */
#endif
#define PMT_GROUP_TILES (2 * PMT_GROUP_WAVES)      /* 16-read tiles per group (two per wave) */
#define PMT_GROUP_MAX_SETS (8 * PMT_GROUP_WAVES)   /* read sets (variants) per group */
#define PMT_TILE 16

/* read-row formats accepted at the boundary (reference data/batch.py:41-62, data/datum.py:35) */
#define PMT_READS_PACKED_U8 0   /* [R][7 + nf] uint8: 7 MSB-first bit-packed bytes, then nf quantile bytes */
#define PMT_READS_F16 1         /* [R][F] float16 (Batch.reads_re as the reference collates it) */
#define PMT_READS_F32 2         /* [R][F] float32 (Batch.copy_to(device, float32)); any values: float16 / float32 rows run the wide-range, guarded instances (pmt_forward.hip) */

/* One nn.Linear.  Weights are consumed in MFMA fragment order from the packed buffer. */
typedef struct PmtLinear {
    int32_t in_dim, out_dim;
    int32_t w_frag;      /* packed: A fragments of W   [out][in]  (forward, y = W x + b)            */
    int32_t wt_frag;     /* packed: A fragments of W^T [in][out]  (backward, dx = W^T dy)           */
    int32_t b_pvec;      /* packed: bias in tile-position order, -1 = no bias                       */
    int32_t w_src;       /* natural-layout source of W: offset into theta (>=0) or phi (<= -2: -(off+2)) */
    int32_t b_src;       /* same for the bias, -1 = none                                            */
    int32_t out_split;   /* 0, or h: the 2h output rows are laid out as two 16-row tiles (rows 0..h-1 -> tile 0,
                            rows h..2h-1 -> tile 1) so that z1 / z2 of the gating unit are tile aligned       */
    int32_t wb_frag;     /* packed: W as THREE bf16 pieces (hi + mid + lo = the fp32 value) in the operand order of
                            v_mfma_f32_16x16x32_bf16: [k block of 32][out tile][piece][lane][8 bf16]; -1 = none */
    int32_t wtb_frag;    /* the same for W^T                                                                   */
    int32_t wh_frag;     /* packed: W as TWO f16 pieces in the operand order of v_mfma_f32_16x16x32_f16:
                            [out tile][k block of 32][piece][lane][8 f16], piece 0 = f16(w), piece 1 = f16(2^12 (w - piece 0)):
                            the low piece is stored scaled so that it keeps its 11 bits whatever the weight's size
                            (pmt_device.hpp: linear_acc_f16); -1 = none                                        */
    int32_t emit_tab;    /* packed (read as int32): where the weight-gradient blocks of this linear go.  For every 16 x 16
                            block (out tile ot, in tile it) of dW in the matrix core's C layout, [(ot * nkt + it)][lane][4]
                            element offsets into the buffer w_src names (theta, or phi when w_src <= -2), -1 = padding;
                            then per out tile 16 offsets of the bias gradient in position order (theta), -1 = none.
                            Written by pmt_pack_params; lets pmt_backward add a block with four atomics and no index
                            arithmetic.  -1 = none                                                                */
} PmtLinear;

#define PMT_OP_LINEAR 0         /* y = W x + b, optional SELU after   (reference mlp.py:55-61)          */
#define PMT_OP_SKIP 1           /* y = x + alpha * f(x), f = (SELU, Linear) x n   (reference mlp.py:15-22) */
typedef struct PmtOp {
    int32_t kind;
    int32_t n_layers;                       /* SKIP: number of (SELU, Linear) pairs; LINEAR: 1 */
    int32_t selu_after;                     /* LINEAR only */
    int32_t alpha_src;                      /* SKIP: theta offset of the scalar alpha */
    int32_t lin[PMT_MAX_SKIP_LAYERS];       /* indices into PmtModel.lin */
} PmtOp;

typedef struct PmtMlp {
    int32_t n_ops, in_dim, out_dim;
    int32_t dropout;            /* 1: the reference built this MLP with dropout_p (an nn.Dropout behind every Linear) */
    PmtOp ops[PMT_MAX_OPS];
} PmtMlp;

/* One GatedRefAltMLPBlock (reference gated_mlp.py:148-251). */
typedef struct PmtBlock {
    int32_t norm_w_pvec, norm_b_pvec;       /* packed LayerNorm(D) weight / bias */
    int32_t norm_w_src, norm_b_src;         /* theta offsets */
    int32_t proj1[2], proj2[2];             /* linear ids, [0] = ref, [1] = alt; proj1 rows are permuted so
                                               that z1 and z2 each start on a 16-row tile */
    int32_t sgu_norm_w_pvec, sgu_norm_b_pvec;
    int32_t sgu_norm_w_src, sgu_norm_b_src;
    int32_t alpha_src[2], beta_src[2];      /* theta offsets of alpha_ref/alt, beta_ref/alt */
    int32_t gamma_src;
    int32_t ref_reg_pvec, ref_reg_src;      /* ref_regularizer [h] */
    int32_t reg_weight_phi;                 /* phi offset of exp(reg_weight.original) (the +0.25 is applied in-kernel) */
} PmtBlock;

/* FeatureClustering + EMG head (reference feature_clustering.py:82-135, exponentially_modified_gaussian.py:30-89).
 * All entries are offsets into phi (materialised values) except mu (theta). */
typedef struct PmtHead {
    int32_t stdev_e_phi;        /* [E] nonartifact stdev                                   */
    int32_t dirs_ke_phi;        /* [K][E] unit direction vectors (already normalised)      */
    int32_t art_stdev_k_phi;    /* [K]                                                     */
    int32_t log_w_k_phi;        /* [K] log_softmax cluster weights                         */
    int32_t mu_k_src;           /* [K] theta offset                                        */
    int32_t sigma_k_phi;        /* [K]                                                     */
    int32_t lambda_k_phi;       /* [K]                                                     */
    int32_t reserved;
} PmtHead;

/* Haplotype CNN (reference architecture/dna_sequence_convolution.py:31-111): a short list of 1-D layers applied to the
 * [10][S] one-hot of the ref/alt haplotypes; evaluated per variant entirely in LDS by pmt_cnn_forward / _backward. */
#define PMT_MAX_CNN_LAYERS 12
#define PMT_CNN_CONV 0
#define PMT_CNN_POOL 1
#define PMT_CNN_LEAKY_RELU 2
#define PMT_CNN_SELU 3
#define PMT_CNN_FLATTEN 4
#define PMT_CNN_LINEAR 5
#define PMT_CNN_BATCHNORM 6     /* BatchNorm1d on BATCH statistics: only in the training descriptor handed to pmt_cnn_bn_forward / _backward
                                   (PmtModel.cnn never holds one: there the BatchNorms are folded into their neighbours, eval mode).
                                   in_ch / in_len = out_ch / out_len (behind a flatten: in_ch = C * L, in_len = 1, every flattened feature
                                   its own channel); w_src / b_src = theta offsets of weight / bias; a region of its own
                                   (out_off != in_off); reserved[0] = offset of its PMT_CNN_BN_STATS * in_ch floats in the statistics buffer */
#define PMT_CNN_BN_STATS 5      /* per BatchNorm channel c of C, at reserved[0] + k * C + c: k = 0 batch mean, 1 rstd = 1 / sqrt(biased variance + eps),
                                   2 unbiased variance (forward); 3 mean of dy, 4 mean of dy * xhat (backward) */
#define PMT_CNN_BN_EPS 1e-5f    /* torch.nn.BatchNorm1d's default */
typedef struct PmtCnnLayer {
    int32_t kind;
    int32_t in_ch, in_len, out_ch, out_len;     /* LINEAR (after FLATTEN): in_ch = features, in_len = out_len = 1 */
    int32_t kernel, stride, padding, dilation;  /* CONV / POOL */
    int32_t w_src, b_src;                       /* theta offsets of weight ([out][in][k] or [out][in]) and bias */
    int32_t in_off, out_off;                    /* per-variant offsets of this layer's input / output in the backward's
                                                   activation region (the one-hot input sits at offset 0)         */
    int32_t lin;                                /* CONV: PmtLinear id of the weight viewed as [out_ch][in_ch * kernel]
                                                   (packed fragments for the implicit-GEMM kernels), else -1      */
    int32_t reserved[2];
} PmtCnnLayer;
typedef struct PmtCnn {
    int32_t n_layers;
    int32_t seq_len;    /* S = haplotypes_length / 2 */
    int32_t out_dim;    /* width of the haplotype embedding */
    int32_t max_act;    /* max floats of any single activation (including the 10*S input) */
    int32_t sum_act;    /* floats of input + every layer output (backward keeps them all in LDS) */
    int32_t reserved[3];  /* training descriptor: [0] = floats of the statistics buffer */
    PmtCnnLayer layers[PMT_MAX_CNN_LAYERS];
} PmtCnn;

typedef struct PmtModel {
    int32_t abi_version;
    int32_t num_read_features;  /* F */
    int32_t read_embed_dim;     /* E_r */
    int32_t variant_embed_dim;  /* E_v = info embedding + haplotype embedding widths */
    int32_t d_model;            /* D = E_r + E_v */
    int32_t d_ffn;              /* 2 h */
    int32_t num_blocks;         /* L */
    int32_t feature_dim;        /* E */
    int32_t num_clusters;       /* K */
    int32_t n_linear;
    int32_t theta_size, phi_size, packed_size; /* floats */
    int32_t translation_src;    /* theta offset of pre_clustering_transform.translation_e [E] */
    int32_t translation_pvec;
    int32_t rotation_lin;       /* linear id, weight source = phi (materialised Q), no bias */
    PmtMlp read_mlp;            /* read_embedding  */
    PmtMlp reducer;             /* reducer         */
    PmtMlp row_mlp[3];          /* per-variant row MLPs (pmt_rows_*): [0] info_embedding, [1] alt_count_predictor,
                                   [2] source_predictor (n_ops = 0 when there is a single source).  Their first
                                   linear may read up to PMT_MAX_ROW_INPUT features                               */
    PmtBlock blocks[PMT_MAX_BLOCKS];
    PmtHead head;
    PmtCnn cnn;                 /* haplotypes_cnn */
    PmtLinear lin[PMT_MAX_LINEAR];
    /* Kernel-instance selection, part of the descriptor (the library reads no environment variables and keeps no state).
     * 0 everywhere = the library's own choice; the other values exist so that the parity tests can run every instance. */
    int32_t force_shape;        /* read-set kernels: 0 auto, 1 at most the tile-exact instance, 2 the generic instance,
                                   3 plain bf16 products where the exact-width instance applies (NOT a parity mode:
                                   one bf16 MFMA per product instead of the fp32-equivalent ones; bench.py --dtype bf16),
                                   5 the exact-width FORWARD with its products as six bf16 MFMAs on three-piece splits (the
                                   round-3 form; auto = three f16 MFMAs on two-piece splits, pmt_device.hpp: linear_acc_f16) */
    int32_t force_cnn;          /* haplotype CNN: 0 auto, 1 general (workgroup-per-chunk) kernels, 2 wave-per-variant
                                   kernels (pmt_cnn2), 3 batched-column kernels (pmt_cnn3)                               */
    int32_t cnn_debug;          /* development switches of pmt_cnn2_backward (0 in production)                           */
    int32_t emit_base;          /* packed: the linears' emit tables lie back to back in [emit_base, emit_base + emit_len) */
    int32_t emit_len;           /*   (floats); a row of pmt_backward's `grad_partials` mirrors exactly this region        */
    float dropout_p;            /* reference parameters.py:26 / mlp.py:57-58: nn.Dropout(p) behind every Linear of the MLPs flagged
                                   PmtMlp.dropout.  Applied only to a batch that brings a dropout_seed (train mode); such a batch
                                   runs the generic kernel instances */
} PmtModel;

/* Inputs of one forward / backward pass.  Reads are ordered as the reference's Batch orders them: all ref reads
 * of all variants, then all alt reads (reference data/batch.py:45-47). */
typedef struct PmtBatch {
    int32_t num_variants;           /* B */
    int32_t num_groups;             /* G */
    int32_t read_format;            /* PMT_READS_* */
    int32_t read_row_bytes;         /* stride of one read row */
    const void* reads;              /* device */
    const int64_t* read_index;      /* device, optional gather (DownsampledBatch.read_indices), NULL = identity */
    const int32_t* ref_offsets;     /* device [B+1] exclusive scan of ref counts; [B] = total ref reads */
    const int32_t* alt_offsets;     /* device [B+1] exclusive scan of alt counts */
    const float* variant_embed;     /* device [B][E_v]: info embedding | haplotype embedding */
    const int32_t* group_start;     /* device [G+1] first variant of each group (pmt_plan_groups) */
    const int32_t* group_tile_base; /* device [G+1] first stash tile of each group (pmt_plan_groups) */
    int64_t total_tiles;            /* host value of group_tile_base[G] (sizes the stash)             */
    int32_t* debug_flags;           /* device, optional [64 + 4096]: [0] unused, [1] development
                                       switches of the backward kernel (0 in production), [8:56] 24 x u64 cycle counters */
    const int32_t* group_span;      /* device [G][6] or NULL.  With it a group may cover only PART of a read set (read sets
                                       beyond one workgroup, pmt_plan_groups_split): v0, v1 (variants [v0, v1)), ref_begin,
                                       ref_end, alt_begin, alt_end (rows of the batch's ref / alt regions); group_start is
                                       then ignored.  Only pmt_forward_layered / pmt_backward_layered accept it. */
    const int32_t* num_groups_dev;  /* device, optional [1]: the number of groups of THIS batch when num_groups is only the
                                       capacity the launch is sized for: workgroups beyond it return at once.  Lets one
                                       captured HIP graph (fixed grids) serve batches with different group plans;
                                       pmt_forward / pmt_backward only */
    const int32_t* set_groups;      /* device, optional [B] (with group_span): how many groups cover each variant, i.e. the
                                       number of g with span[g].v0 <= b < span[g].v1.  With it pmt_forward_layered /
                                       pmt_backward_layered run ONE launch each way in which the groups of a split read set
                                       join their per-set sums through HBM (arrival counters) while the activations stay in
                                       registers; NULL = num_blocks + 1 launches with the activations parked in between */
    uint64_t dropout_seed;          /* 0 = no dropout (eval mode, or dropout_p = 0).  Otherwise the seed of THIS step's masks
                                       (pmt_dropout_mask): the forward and the backward of one step get the same value */
    int32_t* join_fault;            /* device, optional [1], caller-owned and never cleared by the library: the launches' fault
                                       word.  Bit 0 (PMT_FAULT_JOIN): a joined launch (set_groups) whose bounded wait for another
                                       workgroup gave up -- its numbers are wrong.  Bit 1 (PMT_FAULT_F16_RANGE): a forward whose
                                       residual stream or reducer output left the range of its f16 operand pieces (+-65504: they
                                       saturate) -- the logits of that launch are wrong.  One persistent word serves every launch
                                       of a run; the host reads it where it synchronises anyway (end of an epoch / of a filtering
                                       pass) and raises.  NULL = join faults go to the launch's own scratch, range faults nowhere */
} PmtBatch;

typedef struct PmtOutputs {
    float* logits_b;                /* [B]            capped artifact logit                    */
    float* logits_bk;               /* [B][K+2]       nonartifact, outlier, K clusters         */
    float* features_be;             /* [B][E]         alt-set mean embedding                   */
    float* ref_features_be;         /* [B][E]         ref-set mean embedding                   */
} PmtOutputs;

/* dL/d(outputs), same shapes as PmtOutputs; any pointer may be NULL (= zero). */
typedef struct PmtOutputGrads {
    const float* d_logits_b;
    const float* d_logits_bk;
    const float* d_features_be;
    const float* d_ref_features_be;
} PmtOutputGrads;

typedef struct PmtAdamW {
    float lr, beta1, beta2, eps, weight_decay, max_grad_norm;
    int32_t step;                   /* 1-based step number of this update, or PMT_STEP_ON_DEVICE: the step count lives in
                                       `scratch` (int32 at float index PMT_STEP_SLOT, zero before the first step) and the
                                       launch increments it itself, so that a captured graph can be replayed */
    int32_t reserved;
} PmtAdamW;
#define PMT_STEP_ON_DEVICE (-1)
#define PMT_STEP_SLOT 1000

/* ---- host-side helpers (no GPU needed) ------------------------------------------------------------------- */

int pmt_abi_version(void);

/* The shape the exact-width kernel instances of THIS build of the library are compiled for: tile counts (16 features each) of the
 * read features, the read-MLP widths, d_model / the reducer's widths, feature_dim, then the widths themselves: read features,
 * read-MLP width, d_model, d_ffn / 2, feature_dim.  The default build carries the production hyperparameters
 * (4, 2, 4, 1; 61, 30, 60, 10, 10); `make -C permutect_amd/csrc instance SHAPE="..."` builds the library around another shape,
 * and permutect_amd/engine/instances.py picks (or builds) the library whose TILE counts a model fills.  pmt_shape_id: which
 * instance a model runs in this build -- 0 generic (fp32 MFMAs, any supported model), 1 the build's tiles with fp32 MFMAs (asked for
 * through force_shape only), 6 the build's tiles on the 16-bit matrix pipes with the widths read at run time, 2 the build's widths
 * compiled in, 3 the same with plain bf16 products.  Replaces nothing in the reference: its ATen kernels take any width
 * (architecture/mlp.py:32-67, parameters.py:70-156). */
#define PMT_SHAPE_ANY 0            /* generic: any supported model, fp32 MFMAs, every tile guarded                                    */
#define PMT_SHAPE_TILES_F32 1      /* the build's tile counts, widths at run time, fp32 MFMAs (PMT_FORCE_TILES_F32, split read sets)  */
#define PMT_SHAPE_EXACT 2          /* the build's widths compiled in, fp32-equivalent products on the 16-bit matrix pipes             */
#define PMT_SHAPE_EXACT_BF16 3     /* the same widths with plain bf16 products (PMT_FORCE_EXACT_BF16; not a parity mode)              */
#define PMT_SHAPE_EXACT_DROPOUT 4  /* PMT_SHAPE_EXACT carrying a training step's dropout masks (chosen per batch, never by pmt_shape_id) */
#define PMT_SHAPE_TILES 6          /* the build's tile counts, widths at run time, on the 16-bit matrix pipes                         */
/* PmtModel.force_shape */
#define PMT_FORCE_AUTO 0
#define PMT_FORCE_TILES_F32 1      /* at most PMT_SHAPE_TILES_F32                                    */
#define PMT_FORCE_ANY 2            /* PMT_SHAPE_ANY                                                  */
#define PMT_FORCE_EXACT_BF16 3     /* PMT_SHAPE_EXACT_BF16 where PMT_SHAPE_EXACT applies             */
#define PMT_FORCE_FWD_BF16X3 5     /* the exact-width FORWARD on three bf16 pieces; auto otherwise   */
int pmt_shape_info(int32_t* nine);
int pmt_shape_id(const struct PmtModel* m);
/* The shape a model WOULD fill, whatever this build's: nine = (NTF, NTR, NTD, NTE, F, R, D, H, E) and PMT_OK when some build of the
 * library can run the model on tile-exact instances -- the read MLP starts and the reducer ends with a Linear, each keeps one tile
 * count in between, no skip block is deeper than two layers, no tile count exceeds eight -- else PMT_E_UNSUPPORTED (the generic
 * instance).  The same in every build (pmt_host.hip); pmt_shape_id compares its result with pmt_shape_info, and
 * permutect_amd/engine/instances.py names the library to pick or build after it. */
int pmt_model_shape(const struct PmtModel* m, int32_t* nine);
/* The compile-time limits of THIS build of the library: four[0] widest register-resident activation (PMT_MAX_WIDTH: 64; the wide
 * build `libpermutect_amd_wide.so` -- csrc/Makefile `make wide`, generic instances only -- 128), [1] largest d_ffn / 2, [2] floats of
 * one stash slot, [3] waves per workgroup of the read-set kernels.  permutect_amd/engine/instances.py loads the wide build for a
 * model with a layer wider than the default build's limit (the reference takes any width: architecture/mlp.py:32-67). */
int pmt_limits(int32_t* four);

/* A hash of the sources THIS build of the library was compiled from (16 hex digits and a terminating 0 into `out`; returns the
 * number of characters written, PMT_E_INVALID if `capacity` < 17).  The default library and every per-shape / wide build of one tree
 * carry the same id; permutect_amd/engine/instances.py refuses (and rebuilds) a per-shape library left over from other sources. */
int pmt_build_id(char* out, int32_t capacity);

/* sizeof() of the ABI structs as compiled into the library, for binding self-checks:
 * 0 PmtModel, 1 PmtBatch, 2 PmtOutputs, 3 PmtOutputGrads, 4 PmtAdamW, 5 PmtLinear, 6 PmtOp, 7 PmtMlp, 8 PmtBlock, 9 PmtHead,
 * 10 PmtPhiProgram, 11 PmtLossArgs, 12 PmtDownsample, 13 PmtRecordArgs, 14 PmtBalanceArgs, 15 PmtEvalArgs, 16 PmtPosteriorRows,
 * 17 PmtPosteriorParams, 18 PmtPruneArgs, 19 PmtPruneStats, 20 PmtWorstArgs, 21 PmtPosteriorEvalArgs, 22 PmtAnnotateArgs,
 * 23 PmtPreprocessArgs, 24 PmtSiteKeysArgs, 25 PmtVcfArgs */
int pmt_struct_bytes(int which);

/* Validates a descriptor against the kernels' limits. */
int pmt_model_check(const PmtModel* model);

/* Materialised parametrizations ("phi"): the reference registers torch parametrizations on a few small tensors
 * (reference architecture/feature_clustering.py:41-75, exponentially_modified_gaussian.py:66-75, gated_mlp.py:196-201,
 * euclidean_transformation.py:14-16); one segment per tensor maps theta[theta_off ...] (the `.original` leaf) to
 * phi[phi_off ...] (the value the kernels consume). */
#define PMT_PHI_EXP 0           /* phi = exp(theta)                                        (PositiveNumber)          */
#define PMT_PHI_BOUNDED 1       /* phi = p1 * sigmoid(theta) + p0                          (BoundedNumber)           */
#define PMT_PHI_UNIT_ROWS 2     /* every row x of [rows][cols]: x / |x|                    (UnitVector)              */
#define PMT_PHI_LOG_SOFTMAX 3   /* log_softmax of every row                                (LogWeights)              */
#define PMT_PHI_ORTHOGONAL 4    /* base @ expm(tril(X) - tril(X)^T), X = theta [n][n]      (torch orthogonal, matrix_exp map,
                                   use_trivialization; base == NULL means identity)                              */
#define PMT_MAX_PHI_SEGS 48
#define PMT_MAX_ORTHO_DIM 32
typedef struct PmtPhiSeg {
    int32_t kind, theta_off, phi_off, rows, cols, reserved;
    float p0, p1;
    int32_t base_rs, base_cs;   /* ORTHOGONAL: element strides of `base` (torch keeps it as a transposed view) */
    const float* base;          /* ORTHOGONAL: device base matrix, base[i][k] = base[i * base_rs + k * base_cs] */
} PmtPhiSeg;
typedef struct PmtPhiProgram {
    int32_t n_segs, reserved;
    PmtPhiSeg seg[PMT_MAX_PHI_SEGS];
} PmtPhiProgram;

/* phi <- parametrizations(theta): one launch, one workgroup per segment.  Replaces the forward of
 * torch.nn.utils.parametrize for the tensors above (~60 tiny launches per step through torch). */
int pmt_phi_forward(const PmtPhiProgram* prog, const float* theta, float* phi, void* stream);
/* grad_theta[segment's leaf] += J^T grad_phi: one launch.  Replaces autograd through the parametrizations (the adjoint of
 * matrix_exp alone is ~100 launches through torch). */
int pmt_phi_backward(const PmtPhiProgram* prog, const float* theta, const float* phi, const float* grad_phi,
                     float* grad_theta, void* stream);

/* One integer column of a batch as the caller holds it: element i at ptr + i * stride elements of elem_bytes (4: int32, 8: int64)
 * -- a column of Batch.int_tensor (int64, row stride), a DownsampledBatch's own counts (int32, dense).  ptr NULL = all zeros. */
typedef struct PmtIntColumn {
    const void* ptr;
    int64_t stride;
    int32_t elem_bytes, reserved;
} PmtIntColumn;

/* The (source, label, variant type, ref-count bin, alt-count bin) cell of a variant (reference data/batch.py:228-230,
 * data/count_binning.py:9-26): what the balancer's and the downsampler's tables are indexed by.
 * The caller's contract (the columns live on the device, no entry point can look at them): label in 0 .. 2, variant type in
 * 0 .. num_variant_types - 1, ref count >= 0, alt count >= 1, source >= 0.  A value outside lands in another cell's arithmetic -- where the
 * reference raises -- and is not diagnosed.  (An alt count of 0 would also differ from the reference: C division truncates (0 - 1) / skip
 * to bin 0, the reference floors it to -1.)  A source >= num_sources, with the rest in range, is beyond every table and is passed over:
 * see the entry points. */
typedef struct PmtBinning {
    int32_t num_sources, num_variant_types, num_ref_bins, num_alt_bins, count_bin_skip, max_ref_count, max_alt_count, reserved;
} PmtBinning;

/* Read downsampling of a training batch (reference data/batch.py:389-439, training/downsampler.py:105-123). */
typedef struct PmtDownsample {
    int32_t num_variants;
    int32_t reference_alt_gather;   /* 1: reproduce the reference's un-offset alt gather; 0: the intended rows */
    uint64_t seed;                  /* counter-based generator: decisions are a function of (seed, row) */
    int64_t force_random;           /* the reference's randint(0, 100): alt read  end - (force_random % count) - 1  is always kept */
    const int32_t* ref_offsets;     /* [B+1] exclusive scans of the PARENT batch's counts (pmt_scan_counts) */
    const int32_t* alt_offsets;
    const float* ref_weights_b4;    /* [B][4] mixture weights over the Beta shapes (1,1) (1,5) (5,1) (5,5), or NULL = uniform */
    const float* alt_weights_b4;
    const float* ref_fracs_in;      /* [B] keep fractions given by the caller (then no fractions are drawn), or NULL */
    const float* alt_fracs_in;
    /* The mixture weights looked up by the kernel itself (then *_weights_b4 are NULL): the Downsampler's tables [S][3][V][R][A][4]
     * (exp of its log-weights, reference training/downsampler.py:105-112) indexed by the variant's cell -- its label, variant type and
     * source columns and the bins of its PARENT counts (the offsets above).  Replaces ~25 torch launches per training step. */
    const float* ref_weight_table;
    const float* alt_weight_table;
    PmtIntColumn labels, variant_types, sources;
    PmtBinning bins;
} PmtDownsample;
/* Launch 1: draw the keep fractions (unless given) and count the kept reads per variant. */
int pmt_downsample_counts(const PmtDownsample* args, float* ref_fracs, float* alt_fracs, int32_t* new_ref_counts,
                          int32_t* new_alt_counts, void* stream);
/* Launch 2 (after the exclusive scans of the new counts): the gather index PmtBatch.read_index consumes; kept rows in
 * ascending order, all kept ref rows of all variants then all kept alt rows, like the reference's read_indices. */
int pmt_downsample_index(const PmtDownsample* args, const float* ref_fracs, const float* alt_fracs,
                         const int32_t* new_ref_offsets, const int32_t* new_alt_offsets, int64_t* read_index, void* stream);

/* The one-off fit of the downsampler's mixture weights before training (reference training/downsampler.py:125-158,
 * `optimize_downsampling_balance`: AdamW steps through torch on tensors of a few thousand floats) as ONE persistent launch: a
 * wavefront per (source, label, variant type) cell -- the loss is a sum over cells and AdamW is element-wise, so the 15 S cells are
 * independent problems of 160 unknowns -- runs all `steps` iterations with its logits, moments, counts and the two transition tables
 * in registers; global memory is read at the start and written at the end.  No atomics and nothing between workgroups: run-to-run
 * bit-identical.  Plain fp32; the loss and gradient are those of the torch fit (permutect_amd/training/downsampler.py), the AdamW is
 * torch.optim.AdamW's (fresh moments, bias corrections from the step number in double precision).
 *   counts_slvra [S][3][5][4][5]; ref_trans_kry [4][4][4], alt_trans_haz [4][5][5]: the module's binned transition tables;
 *   ref_logits_slvrak / alt_logits_slvrah [S][3][5][4][5][4]: the `.original` tensors, starting point in, fitted logits out;
 *   loss_before_after (optional) [15 S][2]: per cell the loss at the starting point and after the last step (0 for a cell without data,
 *   whose logits -- like those of an entry with a zero count -- see the weight decay only).
 * steps == 0 writes the losses only.  steps < 0 or > PMT_FIT_MAX_STEPS, num_sources < 1 or a NULL table / logits / counts:
 * PMT_E_INVALID, nothing launched. */
#define PMT_FIT_MAX_STEPS 200000    /* the reference runs 10 000; a launch is `steps` dependent iterations of a few microseconds */
int pmt_downsample_fit(const float* counts_slvra, int32_t num_sources, const float* ref_trans_kry, const float* alt_trans_haz,
                       float* ref_logits_slvrak, float* alt_logits_slvrah, int32_t steps, double lr, double beta1, double beta2,
                       double eps, double weight_decay, float* loss_before_after, void* stream);

/* The fit of the artifact allele-fraction spectra after refinement (reference architecture/spectra/artifact_spectra.py:58-75,
 * `ArtifactSpectra.fit`, called from tools/refine_artifact_model.py:46-52: epochs of batch-64 torch.optim.Adam steps on 30 parameters,
 * ~30 ATen ops each) as ONE persistent launch.  The loss of a step is minus the mean over its minibatch of the beta-binomial
 * log-likelihoods (utils/stats_utils.py:28-40) under the (alpha, beta) of each row's (depth bin, variant type) cell, and Adam is
 * element-wise, so the 3 x 5 cells are independent chains over one minibatch schedule: a wavefront per cell runs all
 * epochs * ceil(n / batch_size) steps with its two raw parameters and their moments in registers.  Only the gradient is evaluated
 * (digamma differences; no lgamma).  No atomics and nothing between workgroups: run-to-run bit-identical.
 *   variant_types, depths, alt_counts [n]: the rows in the order the minibatches are cut from them (step t of an epoch takes rows
 *   [t * batch_size, min((t + 1) * batch_size, n)); a short last batch divides by its own length).  Depth bin = (depth >= 10) +
 *   (depth >= 20).  A row whose type is outside 0 .. 4 belongs to no cell; 0 <= alt count <= depth is the caller's to check.
 *   log_alpha_dv, log_beta_dv [3][5]: the `.original` tensors of the exp parametrization (parameterizations.py:45-55), starting point
 *   in, fitted values out.  Fresh moments; lr, beta1, beta2, eps are torch.optim.Adam's, no weight decay, nothing clipped
 *   (misc_utils.py:125-129 is given no parameters to clip).  A cell without rows keeps its bits.
 * n == 0 or epochs == 0: PMT_OK, nothing launched or written.  A NULL array, n < 0, batch_size < 1 or epochs < 0: PMT_E_INVALID,
 * nothing launched. */
int pmt_spectra_fit(const int32_t* variant_types, const int32_t* depths, const int32_t* alt_counts, int32_t n, float* log_alpha_dv,
                    float* log_beta_dv, int32_t batch_size, int32_t epochs, double lr, double beta1, double beta2, double eps,
                    void* stream);

/* The posterior model (reference architecture/posterior_model.py:69-157, posterior_model_priors.py:129-145,
 * spectra/posterior_model_spectra.py:18-124, somatic_spectrum.py:72-96, normal_artifact_spectrum.py:37-58; this package's torch form:
 * architecture/posterior_model.py): per candidate the log priors, the tumor and normal log-likelihoods and the log posteriors of the five
 * calls (enums.Call: 0 somatic, 1 artifact, 2 seq error, 3 germline, 4 normal artifact), and the spectra's fit by minibatch Adam.  A lane
 * per candidate; everything between the 48 bytes of a row and its outputs stays in registers.
 *   rows: the candidates as device-resident columns of length n (permutect_amd/architecture/posterior_model.py: PosteriorRows).
 *   contexts: ((i0 * 5 + i1) * 5 + i2) * 5 + i3 of the four centre bases of the haplotype row (left flank, ref, right flank, alt).
 *   A variant type outside 0 .. 4 or a context outside 0 .. 624 is clamped into range (never an address out of bounds); counts are the
 *   caller's to check (0 <= alt <= depth).
 *   params.raw [PMT_POSTERIOR_RAW]: the `.original` tensors of the spectra, in this order:
 *      0 ..  4  somatic cell fractions before the sigmoid          5 ..  9  somatic weight logits (before log_softmax)
 *     10 .. 24  tumor artifact log alpha [3 depth bins][5 types]   25 .. 39  tumor artifact log beta
 *     40 .. 54  normal spectrum log alpha [3][5]                   55 .. 69  normal spectrum log beta
 *     70 .. 74  mean-multiplier logits [5] (before the sigmoid)    75 .. 79  log concentrations [5]
 *   params.log_priors_vc [5 types][5 calls], params.snv_log_priors_rrra [625] (read where use_context != 0 and the row is an SNV). */
#define PMT_POSTERIOR_RAW 80
#define PMT_POSTERIOR_PARTIAL 128
typedef struct PmtPosteriorRows {
    int64_t n;
    const int32_t *variant_types, *depths, *alt_counts, *normal_depths, *normal_alt_counts, *contexts;
    const float *seq_error_log_lks, *normal_seq_error_log_lks, *allele_frequencies, *mafs, *normal_mafs, *artifact_logits;
} PmtPosteriorRows;
typedef struct PmtPosteriorParams {
    const float *log_priors_vc, *snv_log_priors_rrra, *raw;
    int32_t use_context, no_germline, has_het_beta;
    float het_beta;
} PmtPosteriorParams;
/* One launch: the four [count][5] tensors of `log_posterior_and_ingredients` for rows [first, first + count); any output may be NULL.
 * A NULL struct, column or parameter array, first < 0, count < 0 or first + count > n: PMT_E_INVALID, nothing launched.  count == 0:
 * PMT_OK, nothing written. */
int pmt_posterior_forward(const PmtPosteriorRows* rows, int64_t first, int64_t count, const PmtPosteriorParams* params, float* log_priors_bc,
                          float* spectra_log_lks_bc, float* normal_log_lks_bc, float* log_posteriors_bc, void* stream);
/* One minibatch's E step and gradient: for rows [first, first + count) the same quantities and, in the same pass, analytically, the
 * gradient of -(1 / count) sum_b logsumexp_c(log_posteriors_bc) with respect to the 80 raw values, the softmax of every row added into
 * totals[variant type][call], and sum_b of the log evidence.  Nothing per candidate is written: workgroup w of `num_partial_rows` walks
 * its rows grid-stride and leaves partials[w][PMT_POSTERIOR_PARTIAL]: 0 .. 79 the gradient's share, 80 .. 104 the totals' [5][5],
 * 105 the log evidence, the rest 0.  The sums inside a workgroup are taken in a fixed order (no atomics): run-to-run bit-identical.
 * Invalid as above, or partials NULL, or num_partial_rows < 1: PMT_E_INVALID.  count == 0: PMT_OK, nothing written. */
int pmt_posterior_step(const PmtPosteriorRows* rows, int64_t first, int64_t count, const PmtPosteriorParams* params, float* partials,
                       int32_t num_partial_rows, void* stream);
/* One workgroup: sums the partial rows in row order, applies torch.optim.Adam's update number `step` (1-based; bias corrections in
 * double precision; no weight decay, nothing clipped) to raw / adam_m / adam_v [PMT_POSTERIOR_RAW], adds the 25 totals into
 * totals_tc [5][5] and the summed log evidence into *loss_sum.  A NULL pointer, num_partial_rows < 1, count < 0 or step < 1:
 * PMT_E_INVALID.  count == 0: PMT_OK, nothing written. */
int pmt_posterior_update(const float* partials, int32_t num_partial_rows, int64_t count, float* raw, float* adam_m, float* adam_v, int64_t step,
                         double lr, double beta1, double beta2, double eps, float* totals_tc, double* loss_sum, void* stream);
/* pmt_posterior_step with the E step of the context-dependent SNV priors in the same pass (reference posterior_model_priors.py:116-123,
 * `increment_somatic_snv_context_totals_rrra`): the same kernel body under a compile-time flag, the same arguments, the same `partials`
 * bit for bit, and for every row of variant type 0 (SNV, after the clamp above) llrintf(p_somatic * 2^30) -- p_somatic the row's float
 * posterior of the somatic call, the value that goes into totals[0][0] -- added into somatic_snv_fixed_rrra[context] (625 bins, the
 * caller zeroes them before an epoch) with a 64-bit integer vector atomic.  Integer adds commute: the bins are the same bits from run to
 * run and for any num_partial_rows, without a second pass.  A bin holds at most rows * 2^30: fewer than 2^33 SNV rows per epoch.  A
 * context outside 0 .. 624 is clamped like everywhere else, so nothing is added outside the 625 bins.  The number of SNV rows per bin
 * (the reference's snv_context_totals_rrra) is data alone and the caller's to count.
 * Invalid as pmt_posterior_step, or somatic_snv_fixed_rrra NULL: PMT_E_INVALID, nothing launched. */
#define PMT_CONTEXT_FIXED_ONE (1ll << 30)
int pmt_posterior_step_context(const PmtPosteriorRows* rows, int64_t first, int64_t count, const PmtPosteriorParams* params, float* partials,
                               int32_t num_partial_rows, unsigned long long* somatic_snv_fixed_rrra, void* stream);

/* A filtering run scored against truth labels (reference tools/filter_variants.py:381-411, :534-588: `EvaluationMetrics.record_batch(...,
 * use_original_counts=True)` of the error logit, `AccuracyMetrics.record_with_sources_and_logits` of the cached artifact logit by
 * most-confident call, the correctness decision tree and the mistakes): one pass over rows [first, first + count), a lane per candidate,
 * the posterior of pmt_posterior_forward in double (csrc/pmt_posterior_device.hpp: po_row), everything tallied into INTEGER tables.
 *   labels [n], filtered_in [n] (may be NULL): columns beside `rows`, read at first + i.  The per-row outputs [count] (each may be NULL)
 *   are written at i = 0 .. count - 1, like pmt_posterior_forward's.
 * Per row, p_c = softmax of the five log posteriors in double:
 *   error_prob = 1 - p[passing_call], written as float; error_logit = log(c / (1 - c)) with c = 0.5 + 0.9999999 (error_prob - 0.5)
 *   (reference utils/math_utils.py:26-28), evaluated in double, written as float; a logit x falls into bin
 *   floor(min(max(x, -10), 10) + 10) of 21 (reference data/count_binning.py:14-45) -- x being the FLOAT that is written;
 *   most_confident_call = argmax_c p_c (the lowest index among equals), most_confident_prob = that p as float;
 *   filtered = filtered_in[first + i] != 0 where given, else error_prob (the float) > thresholds_v[type], strictly (reference :535-537);
 *   error_call = for a filtered row argmax over c != passing_call (lowest index among equals; reference :541-548), else -1;
 *   correctness (reference :559-589): 0 unknown (unlabeled rows, and what the reference leaves "unknown"), 1 true-positive,
 *   2 true-negative-artifact, 3 false-negative-artifact, 4 false-positive;
 *   count bins from the ORIGINAL counts (reference data/batch.py:72-77): ref bin = min(max(depth - alt, 0), 10) / 3, alt bin =
 *   (min(max(alt, 1), 15) - 1) / 3.  The reference's floor division gives bin -1 for alt = 0 and for depth < alt (an index in front
 *   of its table); here both are CLAMPED into bin 0.  The variant type is clamped into 0 .. 4 like everywhere else.
 *   A row is INVALID when one of its five log posteriors or of their softmax is NaN, its cached artifact logit is NaN or its label is outside 0 .. 2
 *   (enums.Label: 0 artifact, 1 variant, 2 unlabeled): it adds 1 to `invalid`, is tallied nowhere else, and its per-row outputs are
 *   NaN (floats), -1 (ints) and 0 (filtered_out_b).
 * tables [PMT_EVAL_TABLE_WORDS] of 64-bit words, ADDED into (the caller zeroes them once and may call in slices):
 *   PMT_EVAL_TRUTH_HIST  [3 L][5 V][4 R][5 A][21 G]     labeled rows (label != 2) by label, type, ref bin, alt bin, ERROR-logit bin: 1 each
 *   PMT_EVAL_CALL_HIST   [5 C][3 L][5 V][4 R][5 A][21 G] every valid row by most-confident call, ..., bin of its CACHED ARTIFACT logit:
 *                        llrint(most_confident_prob (the float) * 2^30) each (PMT_CONTEXT_FIXED_ONE, as pmt_posterior_step_context)
 *   PMT_EVAL_CONFUSION   [5 V][3 L][2]                   every valid row by type, label, filtered
 *   PMT_EVAL_MISTAKES    [5 C][5 V]                      labeled rows called wrongly (filtered with label variant, passed with label
 *                        artifact) under their bad call: error_call if filtered, else passing_call (the reference writes Call.SOMATIC
 *                        there in germline mode too, under a TODO; in somatic mode the two agree)
 *   PMT_EVAL_INVALID     [1]
 * Every add is an integer add, so the tables' bits depend neither on the grid nor on slicing, arrival order or the run.  Persistent
 * workgroups walk the rows grid-stride; the small tables are counted in a private LDS copy and added once per workgroup, call_hist's
 * equal keys are summed within a wavefront before one 64-bit vector atomic.  num_workgroups: 0 = the library's choice.
 * A NULL struct, column, labels, thresholds_v, tables or parameter array, passing_call other than 0 or 3, num_workgroups < 0, first < 0,
 * count < 0 or first + count > n: PMT_E_INVALID, nothing launched.  count == 0: PMT_OK, nothing written. */
#define PMT_EVAL_LABELS 3
#define PMT_EVAL_REF_BINS 4
#define PMT_EVAL_ALT_BINS 5
#define PMT_EVAL_LOGIT_BINS 21
#define PMT_EVAL_CELLS (PMT_EVAL_LABELS * 5 * PMT_EVAL_REF_BINS * PMT_EVAL_ALT_BINS * PMT_EVAL_LOGIT_BINS) /* 6300 */
#define PMT_EVAL_TRUTH_HIST 0
#define PMT_EVAL_CALL_HIST (PMT_EVAL_TRUTH_HIST + PMT_EVAL_CELLS)
#define PMT_EVAL_CONFUSION (PMT_EVAL_CALL_HIST + 5 * PMT_EVAL_CELLS)
#define PMT_EVAL_MISTAKES (PMT_EVAL_CONFUSION + 5 * PMT_EVAL_LABELS * 2)
#define PMT_EVAL_INVALID (PMT_EVAL_MISTAKES + 5 * 5)
#define PMT_EVAL_TABLE_WORDS (PMT_EVAL_INVALID + 1) /* 37856 */
typedef struct PmtPosteriorEvalArgs {
    const int32_t* labels;
    const float* thresholds_v; /* [5] error-probability threshold per variant type */
    const uint8_t* filtered_in;
    float *error_probs_b, *error_logits_b;
    int32_t* most_confident_call_b;
    float* most_confident_prob_b;
    uint8_t* filtered_out_b;
    int32_t *error_call_b, *correctness_b;
    unsigned long long* tables;
    int32_t passing_call; /* 0 somatic, 3 germline (germline mode) */
    int32_t num_workgroups;
} PmtPosteriorEvalArgs;
int pmt_posterior_evaluate(const PmtPosteriorRows* rows, int64_t first, int64_t count, const PmtPosteriorParams* params,
                           const PmtPosteriorEvalArgs* args, void* stream);

/* The M step of the context-dependent SNV priors (reference posterior_model_priors.py:158-222) as ONE persistent launch of one
 * wavefront.  The reference fits its generative model of per-context mutation rates by pymc's mean-field ADVI and reports the mean of
 * 1000 draws: stochastic, unseeded, not reproducible.  This is a DETERMINISTIC estimator of the SAME generative model, not ADVI, and
 * claims no parity with ADVI's numbers: the maximiser of the model's log joint with every prior density taken in its unconstrained
 * coordinate (logit for the Beta, log for the Gammas, softmax basis for the Dirichlets), in which the mode of each conjugate piece is
 * its posterior mean.
 *   cells: substitution s = 0 .. 11 (ref * 4 + alt without the four ref == alt entries, A>C = 0 .. T>G = 11), flanks c = left * 4 + right;
 *   cell (s, c) is rrra[left][ref][right][alt] of the 5 x 5 x 5 x 5 tables (bins with a deletion code, index 4, are dropped).
 *   k_sc = rint(somatic_snv_fixed_rrra / 2^30) and n_sc = rint(snv_context_totals_rrra + ratio * sum(totals_tc) / 64), both in float
 *   (to even), as the reference rounds its float32 totals (:158-171); k is capped at n.
 *   unknowns (207): u, R = sigmoid(u); a = log kappa_s, b = log kappa_c; x[12], theta_s = softmax(x); y[12][16], theta_s. = softmax(y[s]);
 *   rate p_sc = R 12 theta_s 16 theta_sc, log p capped at log(1 - 1e-6).
 *   F = sum_sc [k log p + (n - k) log(1 - p)] + log R + 1e6 log(1 - R) + 4 a - 5 kappa_s + 4 b - 5 kappa_c
 *     + lgamma(12 kappa_s) - 12 lgamma(kappa_s) + kappa_s sum_s log theta_s + 12 (lgamma(16 kappa_c) - 16 lgamma(kappa_c)) + kappa_c sum_sc log theta_sc
 *   (Beta(1, 1e6), Gamma(4, 5) twice, Dirichlet(kappa_s 1_12), twelve Dirichlet(kappa_c 1_16), Binomial), maximised by `steps` steps of
 *   torch.optim.Adam on -F / max(sum k, 1) from x = y = 0, a = b = log 0.8, u = logit((sum k + 1) / (sum n + 1e6 + 1)) with the learning
 *   rate lr0 (1 - t / steps) at step t = 0 .. steps - 1 (fresh moments, no weight decay).  Only the analytic gradient is evaluated.
 *   snv_log_priors_rrra [625]: log p_sc of the last iterate into the 192 SNV entries; the other 433 keep their bits.
 *   diagnostics [PMT_CONTEXT_FIT_DIAG] (may be NULL): 0 the last step's largest |dF / d unknown| / max(sum k, 1) (what Adam saw), 1 sum k,
 *   2 kappa_s, 3 kappa_c, then n_sc [12][16] and k_sc [12][16] as the kernel rounded them.
 * Everything is read on the device (nothing is read back); no LDS, no barrier, no atomics: run-to-run bit-identical.  A cell with
 * n = 0, all k = 0 and ratio = 0 are ordinary inputs.  A NULL array other than diagnostics, steps < 1 or > PMT_FIT_MAX_STEPS, lr0 or
 * ratio negative or not finite, lr0 == 0: PMT_E_INVALID, nothing launched. */
#define PMT_CONTEXT_FIT_DIAG (4 + 2 * 192)
int pmt_context_priors_fit(const unsigned long long* somatic_snv_fixed_rrra, const int64_t* snv_context_totals_rrra, const float* totals_tc,
                           double ratio, float* snv_log_priors_rrra, int32_t steps, double lr0, double beta1, double beta2, double eps,
                           float* diagnostics, void* stream);

/* Per-variant losses (reference architecture/artifact_model.py:267-325). */
typedef struct PmtLossArgs {
    int32_t num_variants, num_clusters, num_sources, reserved;
    float max_outlier_logit;        /* constants.MAX_OUTLIER_LOGIT: the outlier logit is clipped from above */
    float max_alt_count;            /* constants.MAX_ALT_COUNT: alt-count target = alt_count / max_alt_count */
    const float* logits_b;          /* [B]      capped artifact logit (PmtOutputs.logits_b) */
    const float* logits_bk;         /* [B][K+2] (PmtOutputs.logits_bk) */
    const float* alt_count_raw;     /* [B]      output of the alt-count adversary's MLP (before the sigmoid) */
    const float* source_logits;     /* [B][S]   output of the source adversary's MLP, or NULL (num_sources == 1) */
    const int64_t* labels;          /* Label per variant (0 artifact, 1 variant, 2 unlabeled), element stride label_stride */
    int64_t label_stride;
    const int64_t* alt_counts;      /* element stride alt_count_stride */
    int64_t alt_count_stride;
    const int64_t* sources;         /* source index per variant (NULL if num_sources == 1), element stride source_stride */
    int64_t source_stride;
    const float* weights;           /* [B] BatchOutput.weights */
    const float* source_weights;    /* [B] BatchOutput.source_weights */
} PmtLossArgs;
typedef struct PmtLossOutputs {     /* forward: the five per-variant loss vectors; backward: their upstream gradients (NULL = 0) */
    float* supervised_b;
    float* unsupervised_b;
    float* alt_count_b;
    float* source_b;
    float* total_b;                 /* weights * (supervised + unsupervised + alt_count) + source_weights * source */
} PmtLossOutputs;
typedef struct PmtLossInputGrads {
    float* d_logits_b;              /* [B]      */
    float* d_logits_bk;             /* [B][K+2] */
    float* d_alt_count_raw;         /* [B]      */
    float* d_source_logits;         /* [B][S] or NULL */
} PmtLossInputGrads;
/* One launch each; replace ~85 elementwise torch launches per training step (BCEWithLogits, clip, logsumexp, sigmoid, MSE,
 * softmax, products and their autograd). */
int pmt_losses_forward(const PmtLossArgs* args, const PmtLossOutputs* out, void* stream);
int pmt_losses_backward(const PmtLossArgs* args, const PmtLossOutputs* grad_out, const PmtLossInputGrads* grad_in, void* stream);

/* Loss bookkeeping (reference training/loss_recorder.py:15-24, metrics/loss_metrics.py:50-54): adds one step's losses into
 * six histograms [6][num_bins] = (primary totals, primary counts, alt-count totals, alt-count counts, source totals,
 * source counts), each a flattened [S][3][V][R][A] tensor indexed by source, label, variant type, ref-count bin,
 * alt-count bin (reference data/count_binning.py:61-66, data/batch.py:228-230).  One launch instead of 8 index_add_. */
typedef struct PmtRecordArgs {
    int32_t num_variants, num_bins;                 /* num_bins = S * 3 * V * R * A */
    int32_t num_variant_types, num_ref_bins, num_alt_bins, count_bin_skip, max_ref_count, max_alt_count;
    PmtIntColumn labels, variant_types, sources, ref_counts, alt_counts;   /* (sources.ptr NULL = source 0; int32 or int64 columns as the batch holds them) */
    const float* weights;         /* [B] BatchOutput.weights */
    const float* source_weights;  /* [B] */
    const float* supervised_b;    /* [B] the four loss vectors of pmt_losses_forward */
    const float* unsupervised_b;
    const float* alt_count_b;
    const float* source_b;
} PmtRecordArgs;
int pmt_record_losses(const PmtRecordArgs* args, float* histograms, void* stream);

/* Rank pruning of mislabeled data (reference tools/prune_dataset.py:30-164): from the artifact probabilities of ONE forward sweep, kept in
 * device memory, the confidences, the confusion counts, the error rates, the two quantile thresholds and the list of the rows that stay.
 * The reference sweeps the data three times and walks `.tolist()` of every batch in Python after each.
 *   art_probs [n]: sigmoid of the capped artifact logit, row i of the dataset at i.  labels: the dataset's own Label column (0 artifact,
 *   1 variant; every other value is unlabeled: skipped by the statistics, always kept by the selection).  CLASS 1 below is the artifact
 *   label, class 0 the non-artifact label, as the reference's confusion matrix numbers them; a row's AGREEMENT probability is p under
 *   an artifact label and 1 - p (fp32) under the other.
 *   label_art_frac: artifacts / (artifacts + variants) of the label marginal (prune_dataset.py:183-186).
 *   levels_given != 0: the quantile levels are `levels` [0 non-artifact, 1 artifact] instead of the inverse error rates, so that the
 *   selection can be driven alone; the stages before it still run and fill the struct, and a degenerate confusion matrix is then no
 *   refusal. */
typedef struct PmtPruneArgs {
    int64_t n;
    const float* art_probs;
    PmtIntColumn labels;
    double label_art_frac;
    double levels[2];
    int32_t levels_given, reserved;
} PmtPruneArgs;
/* bits of PmtPruneStats.status: what the reference answers with ZeroDivisionError or torch.quantile's errors */
#define PMT_PRUNE_NO_ARTIFACT 1         /* no row labeled artifact (or label_art_frac == 0) */
#define PMT_PRUNE_NO_NONARTIFACT 2      /* no row labeled non-artifact (or label_art_frac == 1) */
#define PMT_PRUNE_CONFUSION_COLUMN 4    /* a column of the confusion matrix sums to zero */
#define PMT_PRUNE_RATES_SUM_TO_ONE 8    /* 1 - art_error_rate - nonart_error_rate == 0 */
#define PMT_PRUNE_LEVEL_RANGE 16        /* a quantile level is NaN or outside [0, 1] */
/* Every intermediate of the chain, index [0] the non-artifact class and [1] the artifact class throughout.  (The reference names its
 * error rates the other way round: its `art_error_rate`, confusion[0][1] / column 1, is error_rate[1]; its `inv_art_error_rate`, the
 * level of the ARTIFACT class's quantile, is inv_error_rate[1].) */
typedef struct PmtPruneStats {
    double confidence_sum[2];   /* sum of the agreement probabilities of the class (prune_dataset.py:57-58) */
    int64_t count[2];           /* labeled rows of the class */
    double confidence[2];       /* sum / (count + 1e-4): StreamingAverage.get, misc_utils.py:83-105 */
    int64_t confusion[2][2];    /* [label class][1]: p >= (float)confidence[1]; [label class][0]: 1 - p >= (float)confidence[0]  (:70-91) */
    double error_rate[2];       /* [1] = confusion[0][1] / (confusion[0][1] + confusion[1][1]), [0] = confusion[1][0] / (column 0)  (:93-94) */
    double inv_error_rate[2];   /* the quantile levels (:100-109, or `levels`) */
    float threshold[2];         /* quantile of the class's agreement probabilities at its level (:120-121); NaN when status != 0 */
    int32_t status, reserved;
} PmtPruneStats;
/* Bytes of the scratch buffer both calls below take for n rows (any alignment of 8).  Its contents mean nothing between calls. */
size_t pmt_prune_scratch_bytes(int64_t n);
/* `calculate_pruning_thresholds` (prune_dataset.py:30-129) in one call of nine short launches (behind two memsets) on `stream`, each reading what the one
 * before left in device memory; nothing waits for the device and no workgroup waits for another.  Sums: the agreement probabilities in
 * double, a partial per workgroup folded in workgroup order.  Counts and histograms: integer atomics.  So run-to-run bit-identical.
 * The quantiles are exact order statistics by radix selection on the bits of the agreement probability (a non-negative float orders as
 * its bit pattern), 8 bits a pass, both classes and both neighbours floor(rank), ceil(rank) in the same four passes, and then ATen's
 * arithmetic (aten/src/ATen/native/Sorting.cpp quantile_compute, Lerp.h): the level rounded to fp32, rank = level * (count - 1) in fp32,
 * weight = rank - floor(rank), lerp = weight < 0.5 ? fma(weight, hi - lo, lo) : fma(-(hi - lo), 1 - weight, hi) -- bit for bit
 * torch.quantile's answer on the CPU for a class of up to 2^24 rows; beyond that, where torch refuses, rank and weight in double and
 * lo + weight * (hi - lo) in double, rounded once.
 * `stats` (device) is written whole.  A degenerate input sets `status` and leaves both thresholds NaN; nothing is divided by zero and
 * no rank is looked up.  n == 0: PMT_OK, status = NO_ARTIFACT | NO_NONARTIFACT | CONFUSION_COLUMN.  A NULL struct, stats or scratch, n < 0, art_probs or
 * labels NULL with n > 0, or a label width other than 4 or 8: PMT_E_INVALID, nothing launched. */
int pmt_prune_thresholds(const PmtPruneArgs* args, PmtPruneStats* stats, void* scratch, void* stream);
/* `generated_pruned_data_for_fold`'s rule (prune_dataset.py:133-164) over all n rows: a row goes iff it is labeled artifact and
 * p < art_threshold, or labeled non-artifact and 1 - p < nonart_threshold (fp32).  The rows that stay, as ascending int64 indices, into
 * kept_ids [n] and their number into *kept_count (device): an ordered stream compaction in three launches (count per workgroup, scan,
 * scatter).  NaN thresholds keep everything; `levels`, `label_art_frac` are not read.  n == 0: *kept_count = 0. */
int pmt_prune_select(const PmtPruneArgs* args, float art_threshold, float nonart_threshold, int64_t* kept_ids, int64_t* kept_count,
                     void* scratch, void* stream);

/* The worst offenders of an evaluation pass (reference training/model_training.py:232-268, :294-303): for every (true label, alt-count
 * bin) the `queue_size` labeled variants that the model contradicts most confidently.  The reference walks `.tolist()` of every batch in
 * Python, builds a Datum per row and keeps a PriorityQueue per key; here the queues are a TABLE in device memory and a batch is two
 * launches.
 *   A row is WRONG iff (label == 0 (artifact) and logit < 0) or (label == 1 (variant) and logit > 0): unlabeled rows, logit == 0 and NaN
 *   logits never are.  Its confidence is |logit| (its fp32 bits order as the value: never zero, never NaN); its alt bin is
 *   (alt_count - 1) / 3, UNCAPPED; its key is label * num_alt_keys + bin; its identity is (contig, position, ref code, alt code) from
 *   columns 9 .. 15 of its int row: contig = column 9, the three others pairs of int16 decoded as the reference does,
 *   65535 * (hi + 32768) + (lo + 32768) (reference data/datum.py:28,46-48: 65535, not 65536), in 32 bits.
 *   THE ORDER of a key's slots: confidence descending, then contig (signed), position, ref code, alt code (unsigned) ascending.  Rows equal
 *   in all five are kept as duplicates.  Each key keeps the first queue_size rows of that order of everything ever recorded.
 * The table, 32-bit words (pmt_worst_table_bytes), K = 2 * num_alt_keys keys:
 *   [0, 16) the header: words 0-1 (uint64) the WRONG rows whose alt bin lies outside [0, num_alt_keys) (counted, otherwise ignored),
 *           word 2 (int32) the largest alt count of ANY row seen, word 3 zero, words 4-5 / 6-7 (uint64) the wrong rows of label 0 / 1
 *           (those outside the table included), words 8-15 zero;
 *   [16, 16 + K) the fill count of every key;
 *   then [K][queue_size][5] the slots: confidence bits, contig, position, ref code, alt code.
 * It is kept in CANONICAL FORM: every key's slots in the order above, unused slots zero -- so its bytes are a function of the MULTISET of
 * recorded rows alone: the same for any grid, any arrival order, any cut of the rows into batches, and from run to run.  A table of
 * zeros is the empty table. */
typedef struct PmtWorstArgs {
    int32_t num_variants, queue_size;          /* queue_size 1 .. PMT_WORST_MAX_QUEUE */
    int32_t num_alt_keys, int_elem_bytes;      /* alt bins per label; bytes of an element of int_rows: 2, 4 or 8 */
    PmtIntColumn labels, alt_counts;           /* alt_counts: the counts the model saw (a DownsampledBatch's own) */
    const void* int_rows;                      /* element (i, c) at int_rows + (i * int_row_stride + c) elements; columns 9 .. 15 are read */
    int64_t int_row_stride;
    const float* logits_b;
    int64_t scratch_bytes;                     /* what `scratch` holds: checked against pmt_worst_scratch_bytes(num_variants, ...) */
} PmtWorstArgs;
#define PMT_WORST_MAX_QUEUE 1024
#define PMT_WORST_HEADER_WORDS 16
size_t pmt_worst_table_bytes(int32_t queue_size, int32_t num_alt_keys);
/* Bytes of the scratch of pmt_worst_record for batches of up to max_variants rows (0 for arguments out of range).  Its contents mean
 * nothing between calls and need no initialisation. */
size_t pmt_worst_scratch_bytes(int64_t max_variants, int32_t queue_size, int32_t num_alt_keys);
/* Records one batch: TWO launches on `stream`, no memset, nothing waits for the device, no workgroup waits for another.
 *   1. a grid over the rows: predicate, key, and ONE compare of the confidence bits against the key's current cut (its last slot, once
 *      the key is full; a row equal to the cut goes on: identity may place it in front).  Each workgroup writes the survivors of its own
 *      1024 rows, and their number, to its own segment of `scratch`; the header's counts by integer atomics.
 *   2. a workgroup per key: gathers the key's survivors from every segment, sorts them with the kept slots in LDS (bitonic, the five-word
 *      order above) -- in several passes of up to 2048 records when there are more, never truncating -- and writes the first queue_size
 *      back in canonical form.  A key without survivors is left alone.
 * num_variants == 0: PMT_OK, nothing launched.  queue_size outside 1 .. 1024: PMT_E_UNSUPPORTED.  A NULL pointer, num_variants < 0,
 * num_alt_keys < 1, a column width other than 4 / 8 or a row element other than 2 / 4 / 8 bytes: PMT_E_INVALID.  scratch_bytes too
 * small: PMT_E_WORKSPACE.  Nothing is launched in any of these cases. */
int pmt_worst_record(const PmtWorstArgs* args, void* table, void* scratch, void* stream);
/* table <- the table of the union of both multisets: ONE launch, a workgroup per key (both keys' slots sorted together in LDS), the
 * header's counts added and its largest alt count the larger.  `other` is only read and must not be `table` (PMT_E_INVALID); `scratch`
 * is not used and may be NULL. */
int pmt_worst_merge(void* table, const void* other, int32_t queue_size, int32_t num_alt_keys, void* scratch, void* stream);

/* The site annotation of filter_variants (reference data/memory_mapped_data.py:131-175 `generate_vcf_annotated_data`, fed by
 * tools/filter_variants.py:167-182 `get_segmentation` and misc_utils.py `encode`): every candidate gets its population allele frequency
 * from the input VCF and its tumor / normal minor-allele fraction from two segmentations, and is dropped when the VCF has no record of
 * it or Mutect2 gave it a trusted filter.  The reference keeps a dict of strings per VCF record and two IntervalTrees and builds a Datum
 * per candidate; here the host sorts three tables once and ONE launch, a lane per candidate, looks every candidate up in all three.
 *   A candidate's identity is columns 9 .. 15 of its int row (as PmtWorstArgs; first_column .. first_column + 6 of what is passed): contig = column 9, position / ref code / alt code =
 *   65535 * (hi + 32768) + (lo + 32768) in 32 bits.  Its LOCUS is (contig & 0xFFFFFFFF) << 32 | position.  Its ALLELE KEY reproduces
 *   `truncate(trim(ref, alt).alt)` of the decoded strings: base-5 digits peeled off each code least significant first while the code is
 *   non-zero (a digit other than 1, 2, 3 counts as 4: bases5_as_base_string), trimmed from the top while both lengths exceed 1 and the
 *   top digits agree, the lowest 13 alt digits re-encoded (A=1 C=2 G=3 T=4, first base least significant) -- below 5^13; an empty alt
 *   gives 0, which no site has.
 *   The site table: n_sites rows sorted ascending by (site_locus, site_alt), keys distinct.  Found: keep = !site_excluded,
 *   allele_frequency = site_af.  Not found: keep = 0, allele_frequency = 0.
 *   A segment table: n rows sorted ascending by start key ((contig & 0xFFFFFFFF) << 32 | start), non-overlapping; stop is the plain
 *   coordinate; a segment covers start <= position < stop.  The answer is the maf of the last segment whose start key is at or before
 *   the candidate's locus when that segment's contig is the candidate's and position < stop, else 0.5.
 * Every element of the four outputs is written.  counters (six uint64, ADDED to: the caller zeroes them): kept, excluded (found with
 * the excluded flag), unmatched, unknown contig (never touched by the kernel: the host's check owns its meaning), maf hits, normal-maf
 * hits -- integer atomics, one per non-zero counter per workgroup, so all outputs are bit-identical for any grid and from run to run. */
typedef struct PmtAnnotateArgs {
    int64_t num_candidates;                    /* up to 2^31 - 1 */
    const void* int_rows;                      /* element (i, c) at int_rows + (i * int_row_stride + c) elements */
    int64_t int_row_stride;
    int32_t int_elem_bytes, first_column;      /* 2, 4 or 8; where CONTIG stands in a row: 9 for whole int rows, 0 for columns 9 .. 15 alone */
    int32_t threads_hint, reserved;            /* workgroup size 64 / 128 / 256 / 512 / 1024, 0 = 256 */
    int64_t n_sites;
    const uint64_t* site_locus;                /* [n_sites] */
    const uint32_t* site_alt;
    const float* site_af;
    const uint8_t* site_excluded;
    int64_t n_segments, n_normal_segments;
    const uint64_t* seg_start;                 /* [n_segments] */
    const uint64_t* seg_stop;
    const float* seg_maf;
    const uint64_t* normal_seg_start;          /* [n_normal_segments] */
    const uint64_t* normal_seg_stop;
    const float* normal_seg_maf;
    float* allele_frequencies;                 /* [num_candidates] out */
    float* mafs;
    float* normal_mafs;
    uint8_t* keep;
    uint64_t* counters;                        /* [6] added to */
} PmtAnnotateArgs;
/* One ordinary launch on `stream`; no allocation, no synchronisation, no host read-back.  num_candidates == 0: PMT_OK, nothing launched
 * (no output, counter or row pointer is looked at).  A NULL struct, output, counters or int_rows, num_candidates < 0 or beyond 2^31 - 1, a table size < 0 or beyond 2^31 - 1, a NULL array of a
 * non-empty table, an element width other than 2 / 4 / 8, first_column < 0 or a row shorter than first_column + 7, or a threads_hint not listed: PMT_E_INVALID, nothing launched. */
int pmt_annotate_sites(const PmtAnnotateArgs* args, void* stream);

/* The filtered VCF of filter_variants (reference tools/filter_variants.py:369-617 `apply_filtering_to_vcf`): the reference keeps a dict
 * of PosteriorResults keyed by the string `contig:pos:alt` and, per cyvcf2 record, looks it up, formats 21 numbers with "{:.3f}" and
 * joins a set of filter names.  Here the VCF's data lines lie on the device as bytes beside a table of numbers per line (what
 * permutect_amd/data/vcf_text.py reads), and four entries do the rest; the caller sorts between the first and the second and turns the
 * lengths into starts between the third and the fourth.  INTEGER ARITHMETIC ONLY: every output byte is the same for any grid, any
 * slab and from run to run.
 *   THE RULE.  A record's key is (CHROM, POS as written, truncate(trim(REF, ALT[0]).alt)) as a 64-bit locus and a 32-bit allele key,
 *   the candidates' keys being those of pmt_annotate_sites.  Records with one key match each on their own; of candidates with one key
 *   the LAST in dataset order wins (the reference's dict overwrites).  A record without PMT_VCF_HAS_KEY never matches.
 *   FILTER is a set: those of `contamination`, `slippage` that the record's own FILTER column holds; for a record that matches row r
 *   with filtered[r] != 0, the lower-case name of the error call: the call with the largest float32 posterior probability among the
 *   four that are not `passing_call`, the lowest index among equal maxima; for a record that matches nothing and carries
 *   PMT_VCF_ZERO_ALT_DEPTH, `seq_error`.  It is written in ONE order -- contamination, slippage, then somatic, artifact, seq_error,
 *   germline, normal_artifact -- joined by `;`, and as PASS when empty.
 *   INFO of a matched record gets `;POST=p0,..,p4;PRIOR=..;SPECLL=..;ARTLOD=x;NORMLL=..` appended (values [r, 0 .. 20] in this order);
 *   an INFO column that is `.` is replaced by that text without its leading `;`.  Every other byte of the line is copied.
 *   A NUMBER is Python's "{:.3f}".format(float(x)) of the float32 x = +-m * 2^e: q = round_half_even(m * 1000 * 2^e) -- a shift for
 *   e >= 0, a shift and one compare of the remainder with the half for -64 < e < 0, 0 below -- printed with four digits at least and a
 *   point before the last three, `-` whenever the sign bit is set; `nan`, `inf`, `-inf`.  A finite |x| >= 2^53 is NOT formatted: it
 *   takes no bytes and is counted; the caller refuses to write such a file.
 * counters (PMT_VCF_COUNTERS uint64, ADDED to by pmt_vcf_plan: the caller zeroes them): matched, unmatched, zero alt depth, passed
 * (written as PASS), records carrying each of the five call names, records with a trusted filter kept, matched records whose own
 * Variation differs from their candidate's, unformattable values -- integer atomics, one per non-zero counter per workgroup. */
#define PMT_VCF_CONTAMINATION 1
#define PMT_VCF_SLIPPAGE 2
#define PMT_VCF_HAS_KEY 4
#define PMT_VCF_INFO_DOT 8
#define PMT_VCF_VERBATIM 16        /* a line that is no record (blank, or `#` behind the header): copied as it stands */
#define PMT_VCF_ZERO_ALT_DEPTH 32
#define PMT_VCF_COUNTERS 12
#define PMT_VCF_VALUES 21
typedef struct PmtSiteKeysArgs {
    int64_t num_candidates;                    /* up to 2^31 - 1 */
    const void* int_rows;                      /* as in PmtAnnotateArgs */
    int64_t int_row_stride;
    int32_t int_elem_bytes, first_column;
    int32_t threads_hint, reserved;            /* workgroup size 64 / 128 / 256 / 512 / 1024, 0 = 256 */
    uint64_t* locus;                           /* [num_candidates] out */
    uint32_t* allele_key;                      /* [num_candidates] out */
} PmtSiteKeysArgs;
typedef struct PmtVcfArgs {
    int64_t num_records;                       /* lines behind the header, up to 2^31 - 1 */
    int64_t first_record, count;               /* pmt_vcf_write: the slab's records [first_record, first_record + count) */
    int32_t threads_hint, passing_call;        /* workgroup size as above; 0 .. 4 */
    const int64_t* line_start;                 /* [num_records + 1] byte offset of every line in the text; the last: its end */
    const int32_t* filter_begin;               /* [num_records] offsets inside the line: the FILTER column's begin, */
    const int32_t* filter_end;                 /*   its end (the tab in front of INFO) */
    const int32_t* info_end;                   /*   and the INFO column's end */
    const uint64_t* rec_locus;                 /* [num_records] */
    const uint32_t* rec_key;
    const uint8_t* rec_flags;                  /* PMT_VCF_* */
    const uint8_t* rec_variation;              /* the record's own Variation: len(ALT[0]) - len(REF) */
    int64_t num_candidates;                    /* up to 2^31 - 1 */
    const uint64_t* cand_locus;                /* [num_candidates] ascending by (locus, key, row) */
    const uint32_t* cand_key;
    const int64_t* cand_row;                   /* the dataset row of every sorted entry */
    const float* values;                       /* [num_candidates, 21] by dataset row */
    const uint8_t* filtered;                   /* [num_candidates] */
    const uint8_t* variant_types;              /* [num_candidates] */
    int32_t* matched;                          /* [num_records] out of match, in of plan and write: the row or -1 */
    uint8_t* mask;                             /* [num_records] out of plan, in of write: bit 0 contamination, 1 slippage, 2 + c call c */
    int8_t* error_call;                        /* [num_records] out of plan: the error call or -1 */
    int64_t* out_length;                       /* [num_records] out of plan: the bytes of the output line */
    uint64_t* counters;                        /* [PMT_VCF_COUNTERS] added to by plan */
    const int64_t* out_start;                  /* [num_records + 1] in of write: the exclusive sums of out_length */
    const uint8_t* text;                       /* in of write: text byte t stands at text[t - text_base], text_base <= t < text_base + text_bytes */
    int64_t text_base, text_bytes;
    uint8_t* out;                              /* out of write: output byte o goes to out[o - out_base], likewise */
    int64_t out_base, out_bytes;
} PmtVcfArgs;
/* Each entry: ordinary launches on `stream`; no allocation, no synchronisation, no host read-back.  A count of 0 (candidates for
 * pmt_site_keys, records for match and plan, `count` for write): PMT_OK, nothing launched.  A NULL struct or needed pointer, a size < 0
 * or beyond 2^31 - 1, a threads_hint not listed, passing_call outside 0 .. 4, an element width other than 2 / 4 / 8, a row shorter than
 * first_column + 7, a slab outside the records, or negative text / out sizes: PMT_E_INVALID, nothing launched.
 *   pmt_site_keys: a lane per candidate, identity columns -> locus and allele key.
 *   pmt_vcf_match: a lane per record; ceil(log2(num_candidates + 1)) probes of the sorted keys, every lane the same number.
 *   pmt_vcf_plan: a lane per record: mask, error_call, out_length, counters.  Needs `matched`.
 *   pmt_vcf_write: a wavefront per record of the slab: lanes 0 .. 20 format a value each, a prefix sum places them, then all lanes copy
 *   the line's pieces, consecutive lanes on consecutive bytes.  No byte outside text[0, text_bytes) is read, none outside
 *   out[0, out_bytes) written. */
int pmt_site_keys(const PmtSiteKeysArgs* args, void* stream);
int pmt_vcf_match(const PmtVcfArgs* args, void* stream);
int pmt_vcf_plan(const PmtVcfArgs* args, void* stream);
int pmt_vcf_write(const PmtVcfArgs* args, void* stream);

/* The normalisation of preprocess_dataset (reference data/plain_text_data.py:205-479: `normalized_data_generator`,
 * `make_read_quantile_transform`, `normalize_raw_data_list`; sklearn's QuantileTransformer and numpy's nanpercentile / interp behind
 * them).  The reference builds a Datum per variant, stacks a chunk's reads, fits one QuantileTransformer per chunk on the fragment
 * length (raw read column 6) of the chunk's REF reads and walks the chunk once more with np.median per variant.  Here the raw arrays of
 * a slab of whole chunks lie on the device and two entries do the rest.
 *   Raw arrays (what permutect_amd/data/plain_text_data.py reads from the text): int rows [num_data, int_row_stride] int16 (REF_COUNT,
 *   ALT_COUNT, ORIGINAL_DEPTH, ORIGINAL_ALT_COUNT = columns 0, 1, 5, 6), float rows [num_data, 17] float16 bits (six scalars, eleven
 *   info numbers), reads [num_reads, 9 + k] float16 bits (k = num_error_columns), read_start [num_data + 1] CSR offsets (per datum its
 *   ref rows, then its alt rows), chunk_of [num_data] the chunk of every datum, 0 <= chunk < num_chunks.
 *   The fit (:238-264, sklearn _dense_fit): per chunk, counts [num_chunks, 65536] tallies the ref reads' column 6 by its 16-bit
 *   pattern made order-preserving (sign set: 0xFFFF - bits, else bits + 0x8000; -0 counts as +0, a NaN is left out as nanpercentile
 *   leaves it out) with 32-bit integer atomics; one workgroup per chunk scans its table and takes, for i < nq = min(100, n), the order
 *   statistics around (n - 1) * ((r_i * 100) / 100), r = linspace(0, 1, nq), interpolates them as numpy's _lerp does (the difference of
 *   the two float16 neighbours is itself a float16; a + d * t, and b - d * (1 - t) where t >= 0.5; in double, nothing fused) and applies
 *   the running maximum.  quantiles [num_chunks, 100] (entries from nq on are NaN), ref_reads [num_chunks] = n.  ALL ref reads count:
 *   the reference's fit subsamples 10 000 of them with an unseeded generator beyond that number, and is identical up to it.
 *   The reads (:381-453): out_reads [num_reads, 12]: seven bytes of 10 + 3k bits, first bit highest as np.packbits packs them; four
 *   bytes of tanh(x / 20) of raw columns 4, 5, 7, 8 and one of the quantile-transformed column 6, each clip(v * 32 + 128, 0, 255)
 *   truncated, with every float16 rounding point of the reference's chain: the quotient, the tanh (double, rounded once), the product,
 *   the sum.  The transform is sklearn's _transform_col: np.interp's rule in both directions in double (nothing fused), the uniform
 *   value rounded to float16, 1 / 0 at the bounds (float16(x +- float16(1e-7)) against the end quantiles), then ppf_table: the
 *   clipped normal quantile as float16 bits for every float16 pattern 0 .. 0x3C00 of the uniform value.  A NaN in column 6 gives byte 0.
 *   The float rows (:293-379, :455-476): out_floats [num_data, 59 + 3k] float16 bits: the six scalars, 37 indicator / scaled columns
 *   and the quality feature from lgamma_table (torch.lgamma of every int16 value v as float32 at [v + 32768]), the medians of the five
 *   float columns and the means of the 10 + 3k boolean columns over the datum's alt reads (np.median: the float16 mean of the two
 *   middle values of an even count; np.mean of booleans: a double).
 * fault [1] int32 (zeroed by the entry): 1 + the largest index of a datum whose counts the kernels refuse -- more than 15 alt reads,
 * none at all, a negative ref count, or read_start not in step with them; such a datum's float row is not written. */
#define PMT_PREPROCESS_QUANTILES 100
#define PMT_PREPROCESS_KEYS 65536
#define PMT_PREPROCESS_PPF 15361
#define PMT_PREPROCESS_MAX_ALT 15
#define PMT_PREPROCESS_READ_BYTES 12
typedef struct PmtPreprocessArgs {
    int64_t num_data, num_reads;               /* each up to 2^31 - 1 */
    int64_t int_row_stride;                    /* in elements, >= 7 */
    int32_t num_chunks, num_error_columns;     /* k: 13, 14 or 15 (10 + 3k bits fill seven bytes) */
    int32_t threads_hint, reserved;            /* workgroup size of the per-read and per-datum kernels: 64 / 128 / 256 / 512, 0 = 256 */
    const int16_t* int_rows;
    const uint16_t* float_rows;                /* [num_data, 17] */
    const uint16_t* reads;                     /* [num_reads, 9 + k] */
    const int64_t* read_start;                 /* [num_data + 1] */
    const int32_t* chunk_of;                   /* [num_data] */
    uint32_t* counts;                          /* [num_chunks, 65536] workspace of the fit (zeroed by it) */
    double* quantiles;                         /* [num_chunks, 100]: out of the fit, in of the normalisation */
    int64_t* ref_reads;                        /* [num_chunks]: likewise */
    const float* lgamma_table;                 /* [65536] */
    const uint16_t* ppf_table;                 /* [15361] */
    uint8_t* out_reads;                        /* [num_reads, 12] */
    uint16_t* out_floats;                      /* [num_data, 59 + 3k] */
    int32_t* fault;                            /* [1] */
} PmtPreprocessArgs;
/* Three launches on `stream` (a memset of the table, the tally over the reads, a workgroup per chunk); nothing is read back.  Needs
 * int_rows, reads, read_start, chunk_of, counts, quantiles, ref_reads.  A chunk without a ref read gets n = 0 and a row of NaN: the
 * caller refuses such a slab before it calls (the reference dies inside sklearn).  num_data == 0: PMT_OK, nothing launched. */
int pmt_preprocess_fit(const PmtPreprocessArgs* args, void* stream);
/* Two launches on `stream` (a lane per read; a lane per datum), then ONE word read back after a synchronise of `stream`: PMT_E_CAPACITY
 * when `fault` is set (above).  Needs every pointer but counts.  num_data == 0: PMT_OK, nothing launched.
 * Both entries: a NULL struct or needed pointer, sizes < 0 or beyond 2^31 - 1, num_chunks < 1, k outside 13 .. 15, a row stride below 7
 * or a threads_hint not listed: PMT_E_INVALID, nothing launched.  Bit-identical for any workgroup size and from run to run. */
int pmt_preprocess_normalize(const PmtPreprocessArgs* args, void* stream);

/* The tallies of an evaluation step (reference metrics/evaluation_metrics.py:49-66 -> AccuracyMetrics, metrics/loss_metrics.py:226-243;
 * training/model_training.py:204-228 runs it three times per parent batch after every validation epoch): the weights of the LABELED
 * variants over (source, label, variant type, ref-count bin, alt-count bin, LOGIT bin) and, per label, the weight called artifact / not
 * and the weighted logit sum -- one launch for ~30 tensor ops.  `flat`: [2 epoch types][nhist] histograms, then [2][3 labels][3] statistics
 * (training/loss_recorder.py: EvaluationCounts.flat).  The logit bin is floor((clamp(logit, min_logit, max_logit) - min_logit) /
 * logit_bin_skip) exactly, taken as floor(clamp(logit)) and integer arithmetic (in float32 the subtraction rounds a logit just below a
 * bin boundary onto it).  nhist must be the product of the dimensions: PMT_E_INVALID otherwise. */
typedef struct PmtEvalArgs {
    int32_t num_variants, epoch_index;              /* 0: training data, 1: validation data */
    int32_t num_logit_bins, min_logit, max_logit, logit_bin_skip;   /* reference data/count_binning.py:14-26 */
    PmtBinning bins;
    PmtIntColumn labels, variant_types, sources, ref_counts, alt_counts;
    const float* logits_b;
    const float* weights_b;
    int64_t nhist;                                  /* S * 3 * V * R * A * num_logit_bins */
} PmtEvalArgs;
int pmt_record_evaluation(const PmtEvalArgs* args, float* flat, void* stream);

/* The balancer's step (reference training/balancer.py:55-119 `process_batch_and_compute_weights`): running counts per cell, pseudo-counts
 * of the unlabeled data from the model's artifact probability, the weight tables re-derived from them (when `recompute`: the reference
 * does it every DATA_BEFORE_RECOMPUTE variants) and this batch's weights looked up -- ~60 torch launches per training step in two:
 *   launch 1: counts[cell] += 1; unlabeled variants: pseudo_counts[cell as artifact] += p, [cell as variant] += 1 - p
 *             (p = sigmoid(logits_b); a workgroup's additions are joined in LDS first);
 *   launch 2: tables_out = recompute ? att * tables_in + (1 - att) * clip((1 + ratio^-+1) / 2, 0.01, 100) : tables_in with
 *             ratio = (counts[artifact] + 0.01) / (counts[variant] + 0.01) per cell (every workgroup derives the tables it reads from,
 *             workgroup 0 stores them), then weights_b = labeled ? weights[cell] : p * unlabeled_weights[cell as artifact] +
 *             (1 - p) * unlabeled_weights[cell as variant], and source_weights_b = weights_b * source_weights[source]
 *             (BatchOutput.weights / .source_weights of reference artifact_model.py:285-288).
 * tables_in and tables_out must be different buffers when recompute != 0 (the caller swaps them): PMT_E_INVALID otherwise.
 * A variant whose source is >= num_sources adds to no table and gets weights_b = source_weights_b = 1.  A source without a variant
 * so far has source weight inf after a recomputation (total / 0, as in the reference).  num_variants == 0: PMT_OK, nothing launched and
 * nothing written, whatever `recompute` says.  num_sources beyond 16: PMT_E_INVALID; tables beyond 2048 floats (seven sources of the
 * production bins): PMT_E_UNSUPPORTED. */
typedef struct PmtBalanceArgs {
    int32_t num_variants, recompute;
    float attenuation;                  /* ATTENUATION_PER_DATUM ^ (variants since the last recomputation) */
    int32_t reserved;
    PmtBinning bins;
    PmtIntColumn labels, variant_types, sources, ref_counts, alt_counts;
    const float* logits_b;              /* [B] capped artifact logits of this batch */
    float* counts;                      /* [S][3][V][R][A] running counts (added to) */
    float* pseudo_counts;
    const float* weights_in;            /* the three tables before this step: [S][3][V][R][A], the same, [S] */
    const float* unlabeled_weights_in;
    const float* source_weights_in;
    float* weights_out;                 /* ... after it */
    float* unlabeled_weights_out;
    float* source_weights_out;
    float* weights_b;                   /* [B] out */
    float* source_weights_b;            /* [B] out: weights_b * the source's weight */
} PmtBalanceArgs;
int pmt_balance_step(const PmtBalanceArgs* args, void* stream);

/* The float rows of the posterior hand-off, one launch per batch (reference tools/filter_variants.py:302-320 builds a Datum per
 * variant in Python: `set(CACHED_ARTIFACT_LOGIT, logit)` stores the logit through the float16 scalar array, `set_info_1d(embedding)`
 * replaces the info columns by the float32 embedding, data/datum.py:199-211).  Row i of the batch becomes row dest_ids[i] (NULL: i)
 * of `block`: columns [0, n_scalars) = the batch's float columns rounded through float16, column logit_col = float16(logits_b[i]);
 * columns [n_scalars, n_scalars + e) = features_be[i].  Replaces five torch launches per batch in tools/posterior_data.py. */
int pmt_posterior_rows(const float* float_rows, int64_t float_stride, int32_t n_scalars, int32_t logit_col, const float* logits_b,
                       const float* features_be, int32_t e, const int64_t* dest_ids, int32_t n, float* block, int64_t block_stride,
                       void* stream);

/* The group planners (csrc/pmt_plan.hip; the packing rule they all share: csrc/pmt_plan.hpp).
 * Partition variants into register-resident groups: greedy over consecutive variants so that each group has
 * <= PMT_GROUP_MAX_SETS sets and its tiles fit the workgroup: ref tiles and alt tiles go to disjoint waves, two per wave,
 * i.e. ceil(ceil(ref/16) / 2) + ceil(ceil(alt/16) / 2) <= PMT_GROUP_WAVES (so never more than PMT_GROUP_TILES tiles).  Counts are HOST arrays
 * (upper bounds are fine: a DownsampledBatch reuses its parent's plan).  group_start / group_tile_base must hold
 * num_variants + 1 ints.  Returns the number of groups, or PMT_E_CAPACITY if one variant alone exceeds a group
 * (*bad_variant receives its index). */
int pmt_plan_groups(const int32_t* ref_counts, const int32_t* alt_counts, int32_t num_variants,
                    int32_t* group_start, int32_t* group_tile_base, int32_t* bad_variant);

/* pmt_plan_groups on the DEVICE, from exclusive scans of the counts that live there (a DownsampledBatch's: how many reads it keeps is
 * decided by pmt_downsample_counts and never comes to the host): two small launches, stream-ordered.  The batch is cut into
 * pmt_plan_device_chunks(num_variants) chunks of consecutive variants, each packed next-fit like pmt_plan_groups (a chunk boundary closes
 * a group).  group_start / group_tile_base: device, capacity + 1 ints; num_groups_dev: device, [1] -- PmtBatch.num_groups_dev of the
 * launches that use the plan, whose PmtBatch.num_groups is then `capacity` (the grid).  capacity >= the groups of ANY plan of larger
 * counts in the same order + the number of chunks is always enough; an overflow, or a read set beyond one workgroup, sets
 * PMT_FAULT_PLAN in *fault (may be NULL).  The reference has no counterpart (its ATen kernels need no plan). */
int pmt_plan_groups_device(const int32_t* ref_offsets, const int32_t* alt_offsets, int32_t num_variants, int32_t* group_start,
                           int32_t* group_tile_base, int32_t capacity, int32_t* num_groups_dev, int32_t* fault, int32_t* scratch,
                           void* stream);   /* scratch: device, 2 * pmt_plan_device_chunks(num_variants) ints (contents irrelevant) */
int pmt_plan_device_chunks(int32_t num_variants);

/* An order of the batch's variants in which pmt_plan_groups packs fuller groups (a workgroup costs the same full or not, so
 * the number of groups is what a batch costs): the group under construction takes, out of the next `window` unplaced
 * variants, the first that still fits.  order[i] (host, num_variants ints) = the variant to put at position i of the batch.
 * The reference composes batches in random order (data/reads_dataset.py:141-196), so any order is as good to it. */
int pmt_pack_order(const int32_t* ref_counts, const int32_t* alt_counts, int32_t num_variants, int32_t window, int32_t* order);
/* The same for consecutive batches of `batch` variants (the batches of a dataset chunk) in one call, on `threads` host
 * threads: order[k * batch + i] = position in the whole array of the variant to put at place i of batch k. */
int pmt_pack_order_batches(const int32_t* ref_counts, const int32_t* alt_counts, int32_t num_variants, int32_t batch,
                           int32_t window, int32_t threads, int32_t* order);

/* Like pmt_plan_groups, but a variant whose reads exceed one workgroup is split over several groups (each a run of whole
 * tiles of its ref rows and / or alt rows).  span: host [max_groups][6] (PmtBatch.group_span), tile_base: host
 * [max_groups + 1].  *needs_layered is set when some group covers only part of a read set (then only pmt_forward_layered
 * can run the batch).  Returns the number of groups or PMT_E_WORKSPACE if max_groups is too small. */
int pmt_plan_groups_split(const int32_t* ref_counts, const int32_t* alt_counts, int32_t num_variants, int32_t* span,
                          int32_t* tile_base, int32_t max_groups, int32_t* needs_layered);

/* Floats of scratch pmt_forward_layered needs. */
size_t pmt_layered_scratch_floats(const PmtModel* model, int64_t total_tiles, int32_t num_variants);

/* The forward for batches with read sets of ANY size (BASELINE config: 600 reads per variant): the same kernel, run as
 * num_blocks + 1 launches.  A read set couples its reads only through per-set sums (the gating mean fields of every block,
 * reference gated_mlp.py:236-239, and the head's sums, feature_clustering.py:111-113); launch s finishes block s - 1 from
 * the complete sums and starts block s, the sums accumulate in HBM with float atomics, activations rest in `scratch` between
 * launches, and a last launch finalises the per-set outputs.  Same results as pmt_forward on batches it accepts.
 * `stash` (optional) as in pmt_forward; pmt_backward_layered is its backward. */
int pmt_forward_layered(const PmtModel* model_host, const PmtModel* model_dev, const float* theta, const float* phi,
                        const float* packed, const PmtBatch* batch, const PmtOutputs* out, float* stash, float* scratch,
                        void* stream);

/* Floats of scratch pmt_backward_layered needs. */
size_t pmt_layered_backward_scratch_floats(const PmtModel* model, int64_t total_tiles, int32_t num_variants);

/* Backward of pmt_forward_layered (same arguments as pmt_backward plus `scratch`): num_blocks + 1 launches of the backward
 * kernel.  Going down the stack, a block's backward needs the per-set sums of d(gate) over ALL reads of the set before the
 * gradient can pass its first projection, so launch s finishes block L - s from the complete sums (accumulated in HBM by
 * launch s - 1) and starts block L - s - 1; the running gradient and the half-finished block's per-read state rest in
 * `scratch` between launches.  Per-set parameter terms are added by the group that holds the set's first alt read.
 * grad_variant_embed must be zeroed by the caller (several groups add to a row).  grad_partials / num_partials: as in
 * pmt_backward (the rows are folded once, after the last launch). */
int pmt_backward_layered(const PmtModel* model_host, const PmtModel* model_dev, const float* theta, const float* phi,
                         const float* packed, const PmtBatch* batch, const PmtOutputs* out, const PmtOutputGrads* dout,
                         const float* stash, float* scratch, float* grad_theta, float* grad_phi, float* grad_variant_embed,
                         float* grad_partials, int32_t num_partials, void* stream);

/* Bytes of activation stash a training forward needs for `total_tiles` tiles (group_tile_base[G]) and B variants. */
size_t pmt_stash_bytes(const PmtModel* model, int64_t total_tiles, int32_t num_variants);

/* ---- device entry points ---------------------------------------------------------------------------------- */

/* Re-pack natural-layout parameters (theta: the flat leaf buffer the optimizer updates; phi: materialised
 * parametrizations) into MFMA fragment order.  Run after every optimizer step.  `model_dev` is a device copy of
 * the descriptor. */
int pmt_pack_params(const PmtModel* model_host, const PmtModel* model_dev, const float* theta, const float* phi,
                    float* packed, void* stream);

/* Exclusive scans of per-variant counts (int32 or int64, device) into ref_offsets/alt_offsets [B+1].
 * Replaces the host-synchronising torch.sum(...).item() of reference artifact_model.py:241. */
int pmt_scan_counts(const void* ref_counts, const void* alt_counts, int32_t count_elem_bytes, int64_t count_stride,
                    int32_t num_variants, int32_t* ref_offsets, int32_t* alt_offsets, void* stream);

/* Gather index of a batch whose variants are rows of a dataset chunk resident in HBM: row_start[b] = first read row of
 * variant b inside the chunk (its ref rows, then its alt rows, as on disk: reference data/memory_mapped_data.py:39-40);
 * read_index[R] lists the chunk rows in batch order (all ref rows of all variants, then all alt rows: reference
 * data/batch.py:45-47) and is what PmtBatch.read_index consumes.  Replaces the per-Datum Python collate
 * (reference data/batch.py:41-62) and the re-upload of every read for every batch. */
int pmt_build_read_index(const int64_t* row_start, const int32_t* ref_offsets, const int32_t* alt_offsets,
                         int32_t num_variants, int64_t* read_index, void* stream);

/* Host-side staging copy for the dataset loader (reference data/reads_dataset.py:141-196 reads the memory map Datum by
 * Datum): copies `bytes` from src (a memory-mapped file or host array) to dst (a pinned staging buffer) with `threads`
 * worker threads, outside the Python GIL.  Pure host code, no HIP call. */
/* One batch composed on the device from a chunk of the dataset resident in HBM as it lies on disk (int16 / float16 per-variant
 * tables, CSR row starts): the batch's variants are rows ids[0 .. num_variants) of the chunk.  Writes the Batch's tables in the
 * reference's dtypes (data/batch.py:47-49: int64 [B][int_cols], float32 [B][float_cols]), the variants' first read rows, the
 * exclusive scans of the two count columns ([B + 1] each) and the gather index of the reads (all ref rows, then all alt rows;
 * sized by the caller: the batch's total reads).  Everything device memory; asynchronous on `stream`. */
int pmt_compose_batch(const int16_t* chunk_ints, int32_t int_cols, const void* chunk_floats_f16, int32_t float_cols,
                      const int64_t* chunk_row_start, const int64_t* ids, int32_t num_variants, int32_t ref_col, int32_t alt_col,
                      int64_t* int_tensor, float* float_tensor, int64_t* row_start, int32_t* ref_offsets, int32_t* alt_offsets,
                      int64_t* read_index, void* stream);
/* pmt_compose_batch with the scans of the counts supplied (device copies of pmt_prepare_chunk's `offsets` rows): one launch. */
int pmt_compose_batch_planned(const int16_t* chunk_ints, int32_t int_cols, const void* chunk_floats_f16, int32_t float_cols,
                              const int64_t* chunk_row_start, const int64_t* ids, int32_t num_variants,
                              const int32_t* ref_offsets, const int32_t* alt_offsets, int64_t* int_tensor, float* float_tensor,
                              int64_t* row_start, int64_t* read_index, void* stream);

int pmt_host_copy(void* dst, const void* src, size_t bytes, int32_t threads);
/* The same for `rows` rows of `row_bytes` bytes with bytes [zero_offset, zero_offset + zero_bytes) of every row cleared in the
 * same pass: the integer rows of the posterior hand-off (reference tools/filter_variants.py:305-308: the datum's own integer
 * array with REF_COUNT and ALT_COUNT set to zero). */
int pmt_host_copy_rows(void* dst, const void* src, int64_t rows, int64_t row_bytes, int64_t zero_offset, int64_t zero_bytes,
                       int32_t threads);
/* The host side of one chunk of the device chunk loader in ONE call (no Python, no GIL): the chunk's read counts, the order in
 * which its variants are consumed (optionally shuffled: Fisher-Yates on a splitmix64 stream seeded by `seed`; then ordered
 * inside every batch of `batch` variants by pmt_pack_order with `window`), and every batch's group plan (pmt_plan_groups).
 * Replaces the per-Datum bookkeeping of reference data/reads_dataset.py:141-196 + data/batch.py:41-62 for a whole chunk.
 *   ints: the dataset's int16 table (row_stride in elements), ref_col / alt_col: its REF_COUNT / ALT_COUNT columns
 *   ref_host, alt_host [n]: out; ids [n]: out, ids in consumption order (batch k = ids[k * batch, (k + 1) * batch))
 *   plans [plans_capacity ints]: out, per batch group_start (g + 1) then group_tile_base (g + 1), back to back
 *   batch_info [batches][4]: out, {offset in plans, groups, total tiles, total reads}
 * Returns the number of batches; PMT_E_CAPACITY if a read set exceeds one workgroup (plan such a chunk with
 * pmt_plan_groups_split); PMT_E_WORKSPACE if `plans` is too small (2 * (n + batches) ints always suffice). */
int pmt_prepare_chunk(const int16_t* ints, int64_t row_stride, int32_t ref_col, int32_t alt_col, int32_t n, int32_t shuffle,
                      uint64_t seed, int32_t batch, int32_t window, int32_t threads, int32_t* ref_host, int32_t* alt_host,
                      int64_t* ids, int32_t* plans, int64_t plans_capacity, int32_t* batch_info, int32_t* offsets);
/* (offsets: optional, host, [batches][2][batch + 1]: per batch the exclusive scans of its ref counts and of its alt counts in its
 *  consumption order -- what pmt_compose_batch_planned takes, so that composing a batch on the device is one launch) */

/* Fused read-set forward: decode -> read MLP -> concat -> L gated ref/alt blocks -> reducer -> rotation ->
 * clustering head + per-set sums.  Replaces ArtifactModel.calculate_features + FeatureClustering.calculate_logits
 * + RaggedSets.means_over_sets (reference artifact_model.py:239-297).  `stash` = NULL for inference; otherwise the
 * activations the backward pass re-reads are written there (pmt_stash_bytes). */
int pmt_forward(const PmtModel* model_host, const PmtModel* model_dev, const float* theta, const float* phi,
                const float* packed, const PmtBatch* batch, const PmtOutputs* out, float* stash, void* stream);

/* Fused backward of pmt_forward.  Accumulates into grad_theta / grad_phi (same layouts as theta / phi; the caller zeroes
 * them) and writes grad_variant_embed [B][E_v].  Replaces autograd over the same graph (reference misc_utils.py:127).
 * grad_partials (optional, device): [num_partials][PmtModel.emit_len] floats, ALL ZERO on entry and all zero again on return.
 * With it the kernel runs as min(groups, num_partials) persistent workgroups, each adding its weight-gradient blocks into its
 * OWN row with plain loads and stores, and a second small launch folds the rows into grad_theta / grad_phi; without it
 * (NULL / 0) every block goes out as global float atomics, whose throughput then costs a tenth of the kernel's time.  One
 * row per compute unit (256) is the intended size. */
int pmt_backward(const PmtModel* model_host, const PmtModel* model_dev, const float* theta, const float* phi,
                 const float* packed, const PmtBatch* batch, const PmtOutputs* out, const PmtOutputGrads* dout,
                 const float* stash, float* grad_theta, float* grad_phi, float* grad_variant_embed, float* grad_partials,
                 int32_t num_partials, void* stream);

/* The dropout mask of one linear's output as the kernels generate it (host computation, no GPU; pmt_dropout.hpp): out[r][f] =
 * 1 / (1 - p) where element (row0 + r, f) of the output of linear `lin` (index into PmtModel.lin) is kept under `seed`, else 0.
 * For the parity tests: the oracle applies exactly these masks (reference mlp.py:57-58 draws its own from torch's generator). */
int pmt_dropout_mask(uint64_t seed, float p, int32_t lin, int64_t row0, int64_t rows, int32_t width, float* out);

/* Row-wise MLP over N independent rows -- the per-variant branches: `which` = PMT_ROWS_INFO (info_embedding,
 * reference artifact_model.py:244), PMT_ROWS_ALT_COUNT (alt_count_predictor, :180-183, :276-279) or PMT_ROWS_SOURCE
 * (source_predictor, :267-274).  in: [n_rows] rows of in_dim floats with the given row stride (floats); out likewise, so a
 * result can be written straight into a column block of a wider matrix.  stash = NULL for inference, else
 * pmt_rows_stash_bytes() bytes that the backward pass re-reads. */
size_t pmt_rows_stash_bytes(const PmtModel* model, int which, int32_t n_rows);
int pmt_rows_forward(const PmtModel* model_host, const PmtModel* model_dev, int which, const float* theta,
                     const float* packed, const float* in, int64_t in_stride, int32_t n_rows, float* out,
                     int64_t out_stride, float* stash, uint64_t dropout_seed, void* stream);
/* (dropout_seed: as PmtBatch.dropout_seed; row r of the masks is row r of `in`.)
 * Backward of pmt_rows_forward: accumulates parameter gradients into grad_theta and, if d_in != NULL, writes
 * d_in = d_in_scale * dL/d(in)  (d_in_scale = -alpha implements the reference's gradient reversal,
 * gradient_reversal/functional.py:18-22).
 * `workspace` (optional, device, >= pmt_rows_workspace_floats(model, which) floats, ALL ZERO at the first use; every call
 * leaves it zero again; may be shared by the three MLPs if sized for the largest): the workgroups add their weight-gradient
 * blocks into replicas of the MLP's parameter range and a second launch sums the replicas into grad_theta.  With NULL every
 * workgroup adds to grad_theta itself: hundreds of float atomics per address at the same moment, which the L2 serialises. */
int pmt_rows_backward(const PmtModel* model_host, const PmtModel* model_dev, int which, const float* theta,
                      const float* packed, const float* in, int64_t in_stride, int32_t n_rows, const float* d_out,
                      int64_t d_out_stride, const float* stash, float* grad_theta, float* d_in, int64_t d_in_stride,
                      float d_in_scale, float* workspace, size_t workspace_floats, uint64_t dropout_seed, void* stream);
size_t pmt_rows_workspace_floats(const PmtModel* model_host, int which);

/* Haplotype CNN: haplotypes = device int64 [n][H] rows (values 0..4: A, C, G, T, indel; ref half then alt half,
 * reference data/batch.py:110-130) with the given row stride in elements; out = [n][cnn.out_dim] with row stride.
 * Replaces Batch.get_one_hot_haplotypes_bcs + DNASequenceConvolution.forward (artifact_model.py:245). */
int pmt_cnn_forward(const PmtModel* model_host, const PmtModel* model_dev, const float* theta, const float* packed,
                    const int64_t* haplotypes, int64_t hap_stride, int32_t n, float* out, int64_t out_stride, float* stash,
                    void* stream);
/* Floats per variant of the optional activation stash of a training forward (every layer output, as the backward keeps
 * them in LDS), or 0 when this model runs on kernels that recompute instead (then pass stash = NULL). */
size_t pmt_cnn_stash_floats(const PmtModel* model_host);
/* Backward: accumulates parameter gradients into grad_theta.  With `stash` (written by pmt_cnn_forward for the
 * same haplotypes and weights) the layer outputs are loaded; with NULL the forward is recomputed in LDS (a third of the
 * kernel's time).
 * `workspace` (optional, device, >= pmt_cnn_workspace_floats(model) floats, contents irrelevant before and after): the
 * workgroups store their weight-gradient sums as private rows and a second launch folds the rows into grad_theta.  With
 * NULL (or too small a workspace) every wave adds its sums with global float atomics: thousands of adds to each address
 * within a few microseconds, which the L2 serialises (half of the kernel's time at 65 536 variants). */
int pmt_cnn_backward(const PmtModel* model_host, const PmtModel* model_dev, const float* theta, const float* packed,
                     const int64_t* haplotypes, int64_t hap_stride, int32_t n, const float* d_out, int64_t d_out_stride,
                     const float* stash, float* grad_theta, float* workspace, size_t workspace_floats, void* stream);
/* Floats of workspace pmt_cnn_backward can use for this model on the current device (0: its kernels for this model use atomics). */
size_t pmt_cnn_workspace_floats(const PmtModel* model_host);

/* The haplotype CNN with its `batch_norm` tokens on BATCH statistics (torch.nn.BatchNorm1d in train mode: eps 1e-5, affine), forward and
 * backward.  `cnn_host` / `cnn_dev`: the TRAINING descriptor -- the stack of model->cnn with its PMT_CNN_BATCHNORM layers kept, the
 * convolutions carrying the same PmtLinear ids -- on the host and a copy of it in device memory; theta / packed are the UNFOLDED
 * parameters.  The statistics of BatchNorm k depend on those of every BatchNorm in front of it, so one call makes 2 K + 1 launches on
 * `stream` for K BatchNorms (per BatchNorm a pass that writes per-workgroup partial sums and a fold of them in fp64 in a fixed order, then
 * the full pass): no host synchronisation, no grid barrier, no float atomics in the statistics -- they are the same bits on every call.
 * `stats`: device, cnn_host->reserved[0] floats (PMT_CNN_BN_STATS per channel); written by the forward, read and completed by the backward
 * of the same haplotypes and weights.  `workspace`: device, >= pmt_cnn_bn_workspace_floats(cnn_host, n) floats, contents irrelevant.
 * The backward recomputes the forward in LDS and ADDS every parameter gradient (the BatchNorms' weight / bias included) to grad_theta:
 * its full pass sums the convolutions' and the linear's gradients in a zeroed private row per workgroup inside `workspace` (the span of
 * those parameters in the flat buffer; the layers' w_src / b_src must be their PmtLinear's) and a fold adds the rows in workgroup order --
 * a fill and a launch more, and the gradients, like the statistics, are the same bits on every call.
 * PMT_E_INVALID when a BatchNorm would see a single value per channel (n = 1 in front of a length-1 layer: torch raises ValueError),
 * PMT_E_UNSUPPORTED when not even one variant fits the LDS budget. */
int pmt_cnn_bn_forward(const PmtModel* model_host, const PmtModel* model_dev, const PmtCnn* cnn_host, const PmtCnn* cnn_dev,
                       const float* theta, const float* packed, const int64_t* haplotypes, int64_t hap_stride, int32_t n, float* out,
                       int64_t out_stride, float* stats, float* workspace, size_t workspace_floats, void* stream);
int pmt_cnn_bn_backward(const PmtModel* model_host, const PmtModel* model_dev, const PmtCnn* cnn_host, const PmtCnn* cnn_dev,
                        const float* theta, const float* packed, const int64_t* haplotypes, int64_t hap_stride, int32_t n,
                        const float* d_out, int64_t d_out_stride, float* stats, float* grad_theta, float* workspace,
                        size_t workspace_floats, void* stream);
size_t pmt_cnn_bn_workspace_floats(const PmtCnn* cnn_host, int32_t n);

/* The same computation in STEPS, for batch statistics over the union of several processes' batches (data parallel: R ranks, every rank
 * its own n >= 1 variants).  A collective cannot go between the launches of one call and the library knows nothing of collectives, so
 * the caller drives, per BatchNorm `layer` (its index in cnn_host->layers) in dependency order -- ascending in the forward, descending in
 * the backward:
 *   1. pmt_cnn_bn_forward_moments / _backward_moments: the statistics (sums) pass of that BatchNorm and a fold of THIS rank's
 *      per-workgroup partials, in fp64 and in the fold's fixed order, into `moments`: double[3][C] in device memory, C = the layer's
 *      channels.  Row 0: the values this rank saw per channel, n * in_len.  Row 1: forward sum n_i m_i (= the sum of the values),
 *      backward sum dy.  Row 2: forward the M2 about this rank's OWN mean, backward sum dy xhat.  Two launches.
 *   2. the caller's exchange: `moments` of every rank, in rank order, as double[ranks][3][C] (with every other slot zero beforehand a SUM
 *      all-reduce is that gather: x + 0 is exact).
 *   3. pmt_cnn_bn_merge: one launch, a thread per channel walking the ranks in order, fp64, no atomics -- the same bits on every rank.
 *      backward == 0:  N = sum cnt_r,  mean = (sum sum_r) / N,  M2 = sum_r [M2_r + cnt_r (sum_r / cnt_r - mean)^2] over ranks with
 *      cnt_r > 0;  stores mean, rstd = 1 / sqrt(M2 / N + eps), unbiased variance M2 / (N - 1) into `stats` where the one-call form does.
 *      backward == 1:  c1 = sum_r (sum dy)_r / N, c2 = sum_r (sum dy xhat)_r / N into `stats`, and ONLY slot `rank`'s own sum dy /
 *      sum dy xhat added to grad_theta at b_src / w_src (the gradient all-reduce sums the ranks afterwards).
 *      `n`: this rank's variants, for the checks alone.
 * then pmt_cnn_bn_forward_full / _backward_full: the last launch of the one-call form, given a complete `stats` buffer.
 * With ranks == 1 the steps give the bits of pmt_cnn_bn_forward / _backward (sum / N is the same expression, the cross term exactly 0).
 * K BatchNorms: 3 K + 1 launches each way (the backward's full pass: its fill and fold more).  `workspace` as above.  PMT_E_INVALID: n < 1, a `layer` that is no PMT_CNN_BATCHNORM of the
 * descriptor, rank outside [0, ranks), and ranks == 1 with n * in_len < 2 (a single value per channel has no variance; with more ranks
 * every rank holds a value and the union holds at least two). */
int pmt_cnn_bn_forward_moments(const PmtModel* model_host, const PmtModel* model_dev, const PmtCnn* cnn_host, const PmtCnn* cnn_dev,
                               const float* theta, const float* packed, const int64_t* haplotypes, int64_t hap_stride, int32_t n,
                               int32_t layer, const float* stats, double* moments, float* workspace, size_t workspace_floats, void* stream);
int pmt_cnn_bn_backward_moments(const PmtModel* model_host, const PmtModel* model_dev, const PmtCnn* cnn_host, const PmtCnn* cnn_dev,
                                const float* theta, const float* packed, const int64_t* haplotypes, int64_t hap_stride, int32_t n,
                                int32_t layer, const float* d_out, int64_t d_out_stride, const float* stats, double* moments,
                                float* workspace, size_t workspace_floats, void* stream);
int pmt_cnn_bn_merge(const PmtModel* model_host, const PmtCnn* cnn_host, int32_t layer, int32_t n, const double* moments, int32_t ranks,
                     int32_t rank, int32_t backward, float* stats, float* grad_theta, void* stream);
int pmt_cnn_bn_forward_full(const PmtModel* model_host, const PmtModel* model_dev, const PmtCnn* cnn_host, const PmtCnn* cnn_dev,
                            const float* theta, const float* packed, const int64_t* haplotypes, int64_t hap_stride, int32_t n, float* out,
                            int64_t out_stride, const float* stats, void* stream);
int pmt_cnn_bn_backward_full(const PmtModel* model_host, const PmtModel* model_dev, const PmtCnn* cnn_host, const PmtCnn* cnn_dev,
                             const float* theta, const float* packed, const int64_t* haplotypes, int64_t hap_stride, int32_t n,
                             const float* d_out, int64_t d_out_stride, const float* stats, float* grad_theta, float* workspace,
                             size_t workspace_floats, void* stream);

/* Global-norm clip + AdamW over the flat parameter buffer, one launch sequence, no host sync.
 * Replaces nn.utils.clip_grad_norm_(max_norm=1.0) + torch.optim.AdamW.step (reference misc_utils.py:128-129).
 * `scratch` holds >= 1024 floats: a launch writes one partial sum per workgroup (at most 256, one per 1024 elements) to its
 * first slots and, with PMT_STEP_ON_DEVICE, increments the int32 at PMT_STEP_SLOT; nothing else.  grad_norm_out (device,
 * optional) receives the pre-clip global L2 norm.  max_grad_norm <= 0: no clipping.  n = 0 launches nothing: theta, the
 * moments, grad_norm_out and, with PMT_STEP_ON_DEVICE, the step slot are left as they are (an empty update is not a step). */
int pmt_clip_adamw(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                   const PmtAdamW* hyper, float* scratch, float* grad_norm_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PERMUTECT_AMD_H */
