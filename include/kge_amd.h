/*
 * kge_amd.h -- C ABI of the MI355X (gfx950) KGE scoring engine.
 *
 * This is the drop-in boundary of the hot path.  The
 * reference (uma-pi1/kge, "LibKGE") has no native code; its boundary for this
 * path is the index-level Python API of KgeModel.  Every entry point below
 * replaces one reference function and cites it (paths relative to the
 * reference tree):
 *
 *   kge_score_spo      KgeModel.score_spo        kge/model/kge_model.py:663-680
 *   kge_score_sp       KgeModel.score_sp         kge/model/kge_model.py:682-702
 *   kge_score_po       KgeModel.score_po         kge/model/kge_model.py:704-725
 *   kge_score_sp_po    KgeModel.score_sp_po      kge/model/kge_model.py:749-789
 *   kge_score_emb      RelationalScorer.score_emb kge/model/kge_model.py:151-213
 *                      (ComplEx complex.py:18-43, DistMult distmult.py:13-25,
 *                       TransE transe.py:15-37, RotatE rotate.py:20-69)
 *   kge_score_neg      BatchNegativeSample.score (impl "triple")
 *                                                kge/util/sampler.py:263-306
 *   kge_rank_counts    EntityRankingJob._filter_and_rank /
 *                      _get_ranks_and_num_ties   kge/job/eval_entity_ranking.py:533-596
 *   kge_score_*_bwd    autograd backward of the above (implicit in the
 *                      reference: train_1vsAll.py:70,81; train_KvsAll.py:293;
 *                      train_negative_sampling.py:161)
 *
 * Conventions
 *   - plain C: pointers + sizes, no C++/torch types.  All pointers are DEVICE
 *     pointers (HBM) unless the name says host.  The library never allocates
 *     or frees device memory and keeps no global state: outputs and
 *     workspaces are caller-provided.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *     All work is enqueued on that stream; calls are asynchronous and
 *     re-entrant.
 *   - every function returns KGE_OK (0) or a negative kge_status; nothing
 *     throws across the ABI.  kge_status_string() gives a static message.
 *   - embedding tables are row-major [rows, dim] with leading dimension `ld`
 *     (elements); element type f32 or bf16.  All scores are f32.
 *   - index vectors may be int32 or int64 with an element stride (the
 *     reference trainers pass stride-3 views triples[:,0] of an [n,3] tensor:
 *     kge/job/train_1vsAll.py:64; eval passes int32: eval_entity_ranking.py:164).
 *   - ComplEx/RotatE entity rows are [real half | imaginary half]
 *     (complex.py:24-27, rotate.py:24-25); RotatE relation rows hold dim/2
 *     phases in radians (rotate.py:28,88-93).
 *   - arithmetic is specified operation by operation in DESIGN.md ("canonical
 *     arithmetic"); the f32 paths are bit-reproducible against oracle/.
 */
#ifndef KGE_AMD_H
#define KGE_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KGE_AMD_ABI_VERSION 1

typedef enum kge_status {
  KGE_OK = 0,
  KGE_ERR_INVALID_ARG = -1,   /* NULL pointer, negative size, bad enum          */
  KGE_ERR_UNSUPPORTED = -2,   /* valid request this build has no kernel for     */
  KGE_ERR_LAUNCH = -3,        /* hipLaunchKernel / hip runtime error            */
  KGE_ERR_NO_DEVICE = -4,     /* no gfx950 device visible                       */
  KGE_ERR_WORKSPACE = -5      /* caller workspace too small                     */
} kge_status;

typedef enum kge_scorer {
  KGE_COMPLEX = 0,            /* kge/model/complex.py                            */
  KGE_DISTMULT = 1,           /* kge/model/distmult.py                           */
  KGE_TRANSE = 2,             /* kge/model/transe.py                             */
  KGE_ROTATE = 3,             /* kge/model/rotate.py                             */
  KGE_TRANSH = 4,             /* kge/model/transh.py (float32 tables, l_norm 1 / 2; the entries listed under
                                 "TransH" below -- every other entry answers KGE_ERR_UNSUPPORTED)             */
  KGE_RESCAL = 5              /* kge/model/rescal.py (float32 tables, dim <= KGE_RESCAL_MAX_DIM; the entries listed
                                 under "RESCAL" below -- every other entry answers KGE_ERR_UNSUPPORTED)       */
} kge_scorer;

typedef enum kge_dtype { KGE_F32 = 0, KGE_BF16 = 1 } kge_dtype;
typedef enum kge_itype { KGE_I32 = 0, KGE_I64 = 1 } kge_itype;

/* combine modes of RelationalScorer.score_emb (kge_model.py:151-213) */
typedef enum kge_combine {
  KGE_SPO = 0, KGE_SP_ = 1, KGE_PO_ = 2,
  KGE_SP_PO = 3               /* both blocks of KgeModel.score_sp_po (prepared-query entry points only) */
} kge_combine;

/* Entity + relation lookup tables (LookupEmbedder._embeddings.weight,
 * kge/model/embedder/lookup_embedder.py:44-46). */
typedef struct kge_tables {
  const void* ent;            /* [num_ent, dim]      */
  const void* rel;            /* [num_rel, rel_dim]  */
  int32_t dtype;              /* kge_dtype of both tables                        */
  int32_t scorer;             /* kge_scorer                                      */
  int64_t num_ent;
  int64_t num_rel;
  int64_t dim;                /* entity embedding size d                         */
  int64_t rel_dim;            /* d, except RotatE: d/2, TransH: 2 d, RESCAL: d*d */
  int64_t ent_ld;             /* leading dimensions in elements                  */
  int64_t rel_ld;
  float l_norm;               /* TransE/RotatE `l_norm` option (transe.yaml:11)  */
  int32_t flags;              /* kge_flags, 0 = default                           */
} kge_tables;

/* Per-call kernel selection (no global state).  Default: fastest kernel.        */
typedef enum kge_flags {
  KGE_FLAG_EXACT = 1,         /* ComplEx/DistMult on bf16 tables: use the bit-reproducible
                                 f32-chain kernel instead of the bf16 MFMA kernel            */
  KGE_FLAG_NO_MFMA = 2,       /* f32 ComplEx/DistMult: VALU fmaf chain instead of the f32
                                 MFMA (same bits; used to cross-check the MFMA mapping)      */
                              /* (4, 8: retired with the tile-per-workgroup kernels v1 and v2 -- bf16 tables of a
                                 dim outside {128, 256, 512} run the f32 chain; the bits are ignored)       */
  KGE_FLAG_BF16_V3 = 16,      /* bf16 ComplEx/DistMult with a workspace: the single-role
                                 kernel (v3) instead of the loader/consumer kernel (v4)      */
  KGE_FLAG_SPLIT_QUERY = 32   /* bf16 ComplEx/DistMult scoring: the query vector q = s (x) r is NOT rounded
                                 to one bf16 but carried as q_hi + q_lo (two bf16 pieces, two MFMA chains,
                                 one f32 add): products stay exact, only the f32 summation order differs from
                                 f32 arithmetic on the same bf16 tables (+ a 2^-17 relative residue of q for
                                 ComplEx, none for DistMult): f32-level parity at about half the speed of the
                                 single-pass kernel instead of the seventh the f32 kernels run at.  (KGE_FLAG_EXACT
                                 is something else: the single-pass semantics -- q rounded to bf16 -- as an
                                 order-specified f32 chain.)  Evaluation
                                 (rank parity with the reference: eval_entity_ranking.py:590-595 ties at
                                 rtol 1e-4) wants this; training does not.  Applies to kge_score_sp / _po /
                                 _sp_po / _emb / _emb_sp_po and the prepared-query entry points; shapes the
                                 matrix-core kernel does not take run the f32 chain on the widened tables with
                                 an unrounded query (bit-exact f32 arithmetic on the table values).            */
} kge_flags;
/* Bits 8..15 of `flags`: number of compute units the persistent bf16 scoring kernel leaves
 * free (it launches one workgroup per remaining CU), so that kernels on other streams -- the
 * RCCL kernels of an overlapped exchange -- run beside it.  0 = all.  */
/* kge_ce_sp_po_fwd(_sum) / kge_ce_sp_po_bwd_accum(_sum) only -- the caller's promise that the backward call follows
 * the forward call with the SAME tables, index vectors, n and workspace, and that no other call used that workspace in
 * between (a captured training step; kge_amd.model checks it with a per-workspace generation count): the forward then
 * also leaves the gradient products' query matrix in the workspace and the backward starts from the forward's query
 * fragments instead of building them again (one launch less per step).  Without the promise kept the backward reads
 * stale fragments: set it on BOTH calls or on neither. */
#define KGE_FLAG_CE_KEEP_QUERIES (1 << 16)
#define KGE_FLAG_RESERVE_CUS_SHIFT 8
#define KGE_FLAG_RESERVE_CUS(n) (((n) & 255) << KGE_FLAG_RESERVE_CUS_SHIFT)

/* An index vector: element i is ptr[i*stride] of type itype.
 * ptr == NULL means the identity 0,1,2,... (used for "all entities") -- or, as the `targets` of kge_score_sp / _po /
 * _sp_po only, the contiguous range start, start+1, ..., start+m-1 (0 <= start, start + m <= num_ent): the entity chunk
 * the reference's EntityRankingJob scores against, passed there as torch.arange(chunk_start, chunk_end)
 * (kge/job/eval_entity_ranking.py:216-229) -- the kernels stream rows [start, start + m) of the table itself, no index
 * is read.  `start` must be 0 with a non-NULL ptr and everywhere else. */
typedef struct kge_index {
  const void* ptr;
  int32_t itype;              /* kge_itype */
  int32_t start;              /* see above; 0 otherwise (until round 6 this field was `reserved`, always 0) */
  int64_t stride;             /* in elements */
} kge_index;

/* ---- TransH (KGE_TRANSH; kge/model/transh.py:11-118; csrc/transh.hip, csrc/transh_device.hpp) -------------------
 * Tables: float32; a relation row is [d_r | w_r] (translation, then hyperplane normal: the reference's
 * torch.chunk(p_emb, 2, dim=1)), rel_dim == 2 * dim (anything else: KGE_ERR_INVALID_ARG); l_norm > 0, of which 1 and 2
 * have a kernel (other p, bf16 tables, dim > 1024: KGE_ERR_UNSUPPORTED).  With w^ = w / max(||w||_2, 1e-12)
 * (F.normalize), P e = e - (w^ . e) w^ and eps = 1e-6 added to every component (F.pairwise_distance):
 *   kge_score_spo, kge_score_sp, kge_score_neg (both slots)   score = -|| (P s + d_r) - P o + eps ||_p
 *   kge_score_po                                              score = -|| (P o - d_r) - P s + eps ||_p
 * A score is a pure function of its three rows and l_norm -- the same bits from every entry point that scores the
 * triple in the same form, whatever n, m, the targets' kind (all, range, list), the layout or the launch; a zero w row
 * gives w^ = 0 (the eps-shifted TransE distance), never NaN.  Nothing of size n * m * dim is built (the reference's
 * score_emb materialises [m, n, dim]: transh.py:39-78).  kge_score_sp / _po / _sp_po ignore the workspace.
 * Entry points that take KGE_TRANSH: kge_score_spo, kge_score_sp, kge_score_po, kge_score_sp_po, kge_score_neg,
 * kge_score_pairs_bwd (no float atomics: two runs give the same bits), kge_score_spo_bwd, kge_score_spo_bwd_accum,
 * kge_score_neg_bwd_accum.  The backward entry points RECOMPUTE ||v|| for l_norm 2: `scores` is not read and may be
 * NULL.  Every other entry point that takes kge_tables returns KGE_ERR_UNSUPPORTED for a TransH table and launches
 * nothing (its *_bytes query returns 0). */

/* ---- RESCAL (KGE_RESCAL; kge/model/rescal.py:9-52; csrc/rescal.hip, csrc/rescal_device.hpp) ----------------------
 * Tables: float32; a relation row is the mixing matrix M_p, row-major d x d (rescal.py:25: p_emb.view(-1, d, d)),
 * rel_dim == dim * dim (anything else: KGE_ERR_INVALID_ARG); l_norm is ignored.  bf16 tables and
 * dim > KGE_RESCAL_MAX_DIM: KGE_ERR_UNSUPPORTED.  score(s, p, o) = s^T M_p o, computed in two stages:
 *   query       sp_ / spo / neg slot 2:  q_b = sum_a s_a M[a][b]   (q = M^T s)
 *               _po / neg slot 0:        q_a = sum_b M[a][b] o_b   (q = M o)
 *               a sum of K = dim terms: term k goes to partial sum (k / 4) mod 8, every partial sum is an fma chain in
 *               ascending k from +0, and the eight are added as ((p0 + p4) + (p2 + p6)) + ((p1 + p5) + (p3 + p7)).
 *               q is a pure function of its two rows: the same bits from kge_rescal_queries and from every scoring
 *               entry, whatever n, the index type or stride, the table pitch or alignment and the launch.
 *   contraction kge_score_sp / _po / _sp_po: the float32 chain of the ComplEx / DistMult pair kernels over (q, target) --
 *               bit-equal to kge_score_emb(KGE_DISTMULT float32, KGE_SP_ / KGE_PO_, q, ones, target rows), with and
 *               without KGE_FLAG_NO_MFMA.  kge_score_spo / kge_score_neg: the row-wise summation of kge_score_spo over
 *               (q, the other row) -- bit-equal to kge_score_emb(KGE_DISTMULT, KGE_SPO, q, ones, rows); q stays on chip.
 * kge_score_neg, slot 0 (the subject varies): q' = M_p o_i is built ONCE per positive and every sampled subject s' is
 * scored as q' . s'.  The reference's order for this triple is (s'^T M_p) . o, a d x d product per sample: the same
 * real number, a different rounding -- inside the float64 bound of the triple, not bit-equal to kge_score_spo.  Slot 2
 * IS bit-equal to kge_score_spo on the expanded triples.
 * Workspace: kge_score_sp / _po / _sp_po build their queries in the caller's workspace (kge_score_workspace_bytes(t, n):
 * two blocks of n * dim floats and one row of ones; kge_score_sp / _po use the first block); NULL or too small with
 * n * m > 0: KGE_ERR_WORKSPACE.  No zeroing needed.  kge_score_pairs_bwd likewise (kge_score_bwd_workspace_bytes).
 * Entry points that take KGE_RESCAL: kge_score_spo, kge_score_sp, kge_score_po, kge_score_sp_po, kge_score_neg,
 * kge_score_pairs_bwd (no float atomics: two runs give the same bits; g_p is [n, dim * dim]), kge_score_spo_bwd,
 * kge_score_spo_bwd_accum, kge_score_neg_bwd_accum (grad_rel is [num_rel, dim * dim]; float atomics), and
 * kge_rescal_queries.  `scores` of the backward entries is not read and may be NULL.  Every other entry point that
 * takes kge_tables returns KGE_ERR_UNSUPPORTED for a RESCAL table and launches nothing (its *_bytes query returns 0). */
#define KGE_RESCAL_MAX_DIM 256

/* ---- Relational Tucker3 (kge/model/relational_tucker3.py, kge/model/embedder/tucker3_relation_embedder.py;
 * csrc/tucker3.hip, csrc/tucker3_device.hpp) ---------------------------------------------------------------------------
 * relational_tucker3 is RESCAL whose mixing matrices are projected from a small base table: with base rows B [num_rel,
 * base_dim] and the projection weight W [dim * dim, base_dim] (torch.nn.Linear(base_dim, dim * dim, bias=False).weight),
 *   M_p = (B[p] @ W^T).view(dim, dim),    out[i][j] = sum_{k < base_dim} B[idx_i][k] * W[j][k],   j < dim * dim.
 * The projected rows are a KGE_RESCAL relation table (rel_dim == dim * dim): there is no scorer of its own.
 * Canonical arithmetic: ONE fused multiply-add chain per element, ascending k, from +0 --
 *   acc = +0;  acc = fma(B[idx_i][k], W[j][k], acc)  for k = 0 .. base_dim - 1
 * -- exactly base_dim operations (no zero padding).  An element of `out` is a pure function of its B row and its W row:
 * the same bits whatever n, num_rel, the row's position in the call, the index type / stride / range form, the pitch or
 * 16-byte alignment of any operand, and the launch.
 * Gate: dtype != KGE_F32, dim > KGE_RESCAL_MAX_DIM or base_dim > KGE_TUCKER3_MAX_BASE_DIM: KGE_ERR_UNSUPPORTED before
 * any launch (the *_bytes queries return 0); every base_dim >= 1 up to the cap works.  NULL tables, non-positive sizes,
 * base_ld < base_dim, proj_ld < base_dim, output pitches below their widths: KGE_ERR_INVALID_ARG. */
#define KGE_TUCKER3_MAX_BASE_DIM 1024

typedef struct kge_tucker3 {
  const void* base;           /* B [num_rel, base_dim], row-major                 */
  const void* proj;           /* W [dim * dim, base_dim], row-major               */
  int32_t dtype;              /* kge_dtype of both: KGE_F32                       */
  int32_t reserved_;          /* 0                                                */
  int64_t num_rel;
  int64_t dim;                /* entity embedding size d                          */
  int64_t base_dim;           /* d_r                                              */
  int64_t base_ld;            /* leading dimensions in elements                   */
  int64_t proj_ld;
} kge_tucker3;

/* out[i * out_ld + j] as above, i < n, out_ld >= dim * dim.  idx: a kge_index over base rows; ptr == NULL is the
 * contiguous range start, start + 1, ..., start + n - 1 (0 <= start, start + n <= num_rel): "all relations" is the range
 * 0 .. num_rel.  kge_tucker3_project_bytes: n * dim * dim floats (0 for a gated table).  n == 0: KGE_OK, nothing is
 * launched. */
int64_t kge_tucker3_project_bytes(const kge_tucker3* t, int64_t n);
int kge_tucker3_project(const kge_tucker3* t, kge_index idx, int64_t n, float* out, int64_t out_ld, void* stream);

/* Backward of the projection from g_out [n, dim * dim] (g_ld >= dim * dim):
 *   g_brows [n, base_dim]        = g_out * W           (row i belongs to base row idx_i: the caller scatters it)
 *   g_w     [dim * dim, base_dim] = g_out^T * B[idx]
 * on the float32 matrix cores (the gradient products of kge_score_pairs_bwd), plain stores, no float atomics: two runs
 * give the same bits.  The bits depend on the shape and, per output, on whether it is dense (ld == base_dim) and 16-byte
 * aligned (the split-K form of the product is taken only then); any pitch and alignment is accepted.  Either output may
 * be NULL (not computed).  The library allocates nothing: split-K partials and
 * the gathered base rows go to `workspace` (kge_tucker3_project_bwd_workspace_bytes(t, n); no zeroing needed); NULL or
 * too small with n > 0: KGE_ERR_WORKSPACE. */
int64_t kge_tucker3_project_bwd_workspace_bytes(const kge_tucker3* t, int64_t n);
int kge_tucker3_project_bwd(const kge_tucker3* t, kge_index idx, int64_t n, const float* g_out, int64_t g_ld,
                            float* g_brows, int64_t g_brows_ld, float* g_w, int64_t g_w_ld, void* workspace,
                            int64_t workspace_bytes, void* stream);

/* ---- ConvE (kge/model/conve.py:9-101; csrc/conve.hip, csrc/conve_device.hpp) -------------------------------------------
 * ConvE puts a small network between the (s, p) rows and the contraction with the entity table (conve.py:75-93).  In
 * eval mode that network is a fixed function of two rows; kge_conve_queries runs it and writes AUGMENTED query rows
 *   q' = [1.0f | x],   d + 1 floats,   x = the network's output for (s, p),   d = h * w,
 * so that score(s, p, o) = q' . ent[o] over the WHOLE entity row of d + 1 floats: the 1.0f meets the bias column (column 0
 * of an entity row).  There is no ConvE scorer and nothing ConvE in kge_tables: the contraction is the float32 DistMult
 * arithmetic through kge_score_emb(KGE_DISTMULT, KGE_SP_ / KGE_SPO, q', rows of ones, entity rows) and its backward
 * kge_score_emb_bwd.  The reference adds the bias AFTER the product (conve.py:99); the augmented form is the same real
 * number with a different rounding, inside the float64 bound of the score -- not bit-equal to the reference's order.
 * Eval-mode semantics only (running statistics, no dropout), in this order; Ho = 2 h - fs + 2 pad + 1,
 * Wo = w - fs + 2 pad + 1, F = 32 * Ho * Wo:
 *   1 gather    ent[s][1:] and rel[p][1:] as two h x w images stacked to 2 h x w, the subject on top (conve.py:82-84)
 *   2 conv      32 channels, fs x fs, stride 1, zero padding: ONE fma chain per output, taps in ascending (ky, kx),
 *               from conv_b[c] or +0; a tap in the padding enters no fma                       (conve.py:85)
 *   3 bn1       (v - bn1_mean[c]) * rsq,  rsq = 1 / sqrt(bn1_var[c] + bn1_eps): one add, one correctly rounded sqrt,
 *               one correctly rounded division; no affine                                      (conve.py:86)
 *   4 ReLU      v > 0 ? v : +0                                                                 (conve.py:87)
 *   5 flatten   channel-major: feature c * Ho * Wo + y * Wo + x                                (conve.py:89)
 *   6 proj      x_j = sum_k feature_k proj_w[j][k] + proj_b[j].  Summation order: 32 channel partials P_c, each one fma
 *               chain from +0 over the channel's positions k = y * Wo + x in groups of eight -- within group g the order
 *               is 8g, 8g+4, 8g+1, 8g+5, 8g+2, 8g+6, 8g+3, 8g+7 (the chain of v_mfma_f32_32x32x2_f32; positions past
 *               Ho * Wo in the last group are zeros on both sides) -- then (((P_0 + P_1) + P_2) + ... + P_31) + proj_b[j]
 *               by plain additions in a fixed order; no float atomics: two runs give the same bits   (conve.py:90)
 *   7 bn2       as 3 with bn2_mean[j], bn2_var[j], bn2_eps                                     (conve.py:92)
 *   8 ReLU                                                                                     (conve.py:93)
 *   9 write     q[i][1 + j] = the result, q[i][0] = 1.0f; nothing else of q is touched (q_ld > d + 1: a pitched q)
 * A query row is a pure function of its two table rows and the network: the same bits whatever n, the row's position in
 * the call, the index type or stride, the pitches, 16-byte alignment and the launch geometry.
 * Gate, before any launch (kge_conve_workspace_bytes returns 0):
 *   KGE_ERR_INVALID_ARG   NULL net or pointers (conv_b only with has_conv_bias), h, w < 1, padding < 0, proj_ld < F,
 *                         ent_ld / rel_ld / q_ld < d + 1, n < 0, NULL q or tables with n > 0, a malformed index
 *   KGE_ERR_UNSUPPORTED   filter_size outside 1..5, padding > 2 (stride is 1 by construction), Ho < 1, Wo < 1,
 *                         h * w > KGE_CONVE_MAX_DIM, or a channel slice that does not fit the LDS plan: the kernel holds
 *                         32 rows x (Ho * Wo rounded up to a multiple of 8, + 1) floats, and that row length must be at
 *                         most KGE_CONVE_MAX_SLICE floats (128 KiB)
 *   KGE_ERR_WORKSPACE     workspace NULL or below kge_conve_workspace_bytes(net, n) = 32 * n * d floats (the channel
 *                         partials; no zeroing needed, every float of it is written before it is read)
 * n == 0: KGE_OK, nothing is launched.  Every KGE_ERR_INVALID_ARG condition, the call's own arguments included, is
 * reported in front of KGE_ERR_UNSUPPORTED.  A slice above 48 KiB asks the runtime for its LDS once per device; a
 * runtime that refuses what the gate allows is KGE_ERR_LAUNCH. */
#define KGE_CONVE_MAX_DIM 1024
#define KGE_CONVE_MAX_SLICE 1024

typedef struct kge_conve_net {
  int32_t h;                  /* image height and width of one embedding: d = h * w (conve.py:17-42)  */
  int32_t w;
  int32_t filter_size;        /* fs                                                                   */
  int32_t padding;            /* pad                                                                  */
  int32_t has_conv_bias;      /* 0: conv_b is not read and may be NULL                                */
  int32_t reserved_;          /* 0                                                                    */
  const float* conv_w;        /* convolution.weight [32, 1, fs, fs], contiguous                       */
  const float* conv_b;        /* convolution.bias [32] or NULL                                        */
  const float* bn1_mean;      /* bn1.running_mean [32]                                                */
  const float* bn1_var;       /* bn1.running_var [32]                                                 */
  const float* proj_w;        /* projection.weight [d, F], row-major, pitch proj_ld                   */
  int64_t proj_ld;
  const float* proj_b;        /* projection.bias [d]                                                  */
  const float* bn2_mean;      /* bn2.running_mean [d]                                                 */
  const float* bn2_var;       /* bn2.running_var [d]                                                  */
  float bn1_eps;
  float bn2_eps;
} kge_conve_net;

/* q[i * q_ld + :] = [1.0f | network(ent[s_i], rel[p_i])], i < n, q_ld >= d + 1 ("ConvE" above: conve.py:75-93).
 * ent / rel: float32 tables whose rows hold d + 1 floats (column 0 of an entity row is its bias; column 0 of a relation
 * row is never read), pitches ent_ld / rel_ld in floats. */
int64_t kge_conve_workspace_bytes(const kge_conve_net* net, int64_t n);
int kge_conve_queries(const kge_conve_net* net, const float* ent, int64_t ent_ld, const float* rel, int64_t rel_ld,
                      kge_index s, kge_index p, int64_t n, float* q, int64_t q_ld, void* workspace,
                      int64_t workspace_bytes, void* stream);

/* ---- library ---------------------------------------------------------- */
int kge_abi_version(void);
const char* kge_status_string(int status);
/* Number of gfx950 devices visible to the HIP runtime (0 if none). */
int kge_device_count(void);

/* ---- index-level scoring (fused gather + score) ------------------------ */

/* Optional device workspace for the scoring calls below.  The library never allocates:
 * a caller that passes `workspace_bytes >= kge_score_workspace_bytes(t, n)` lets the
 * bf16 ComplEx/DistMult path build the n query vectors ONCE -- cooperatively inside the one
 * scoring kernel: a few workgroups build, publish through the workspace, all workgroups
 * consume -- instead of once per workgroup.  workspace == NULL (or too small) selects the
 * path where every workgroup builds its own copy.  Results are identical bit for bit.  The
 * workspace must be ZEROED ONCE (hipMemset) before its first use and left to the library from
 * then on: besides scratch it holds the builders' flag lines and a "degraded" word.  A consumer
 * workgroup waits for its builders only for a bounded time (they may not be running: other
 * streams' kernels, a second process, CU masking); after a time-out it builds its own query
 * vectors and sets that word to a count of launches; the next few thousand calls on the workspace
 * skip the hand-off (slower, never wrong, never a hang), then it is tried again (non-zero garbage
 * in a fresh workspace has the same effect, for as long as it takes to count it down).  The
 * workspace is only accessed during a call (stream order; calls may be captured into a hipGraph
 * and replayed) and must not be shared by calls that may run concurrently on different streams;
 * 16-byte aligned.  ONE workspace may serve calls with different n (size it for the largest): the
 * control block -- flag lines and the degraded word -- lies at its start, at an offset that does not
 * depend on n; the query vectors follow.  The same holds for the workspaces of the fused-loss entry points below. */
int64_t kge_score_workspace_bytes(const kge_tables* t, int64_t n);

/* RESCAL queries ("RESCAL" above): q[i * q_ld + :] = M_{p_i}^T ent[a_i] (dir = KGE_SP_) or M_{p_i} ent[a_i] (KGE_PO_),
 * dim floats per row, q_ld >= dim -- the dense query rows the scoring entries contract with the targets (the same
 * bits).  kge_rescal_queries_bytes: n * dim floats; 0 for a table the entry does not take.  Every scorer but KGE_RESCAL:
 * KGE_ERR_UNSUPPORTED.  n == 0: KGE_OK, nothing is launched. */
int64_t kge_rescal_queries_bytes(const kge_tables* t, int64_t n);
int kge_rescal_queries(const kge_tables* t, int dir, kge_index a, kge_index p, int64_t n, float* q, int64_t q_ld,
                       void* stream);

/* out[i] = score(s[i], p[i], o[i]), i < n.        KgeModel.score_spo */
int kge_score_spo(const kge_tables* t, kge_index s, kge_index p, kge_index o,
                  int64_t n, float* out, void* stream);

/* out[i*ldo + j] = score(s[i], p[i], targets[j]), j < m.  KgeModel.score_sp
 * targets.ptr == NULL: all entities, m must equal t->num_ent. */
int kge_score_sp(const kge_tables* t, kge_index s, kge_index p, int64_t n,
                 kge_index targets, int64_t m, float* out, int64_t ldo,
                 void* workspace, int64_t workspace_bytes, void* stream);

/* out[i*ldo + j] = score(targets[j], p[i], o[i]).  KgeModel.score_po */
int kge_score_po(const kge_tables* t, kge_index p, kge_index o, int64_t n,
                 kge_index targets, int64_t m, float* out, int64_t ldo,
                 void* workspace, int64_t workspace_bytes, void* stream);

/* out[i*ldo + j] = sp score, out[i*ldo + m + j] = po score (j < m); ldo >= 2m.
 * KgeModel.score_sp_po (cat of score_sp and score_po over one entity subset). */
int kge_score_sp_po(const kge_tables* t, kge_index s, kge_index p, kge_index o,
                    int64_t n, kge_index targets, int64_t m, float* out,
                    int64_t ldo, void* workspace, int64_t workspace_bytes,
                    void* stream);

/* ---- prepared queries: the query build taken out of the scoring launch -------------------------------
 * KgeModel.score_sp / score_po / score_sp_po (kge/model/kge_model.py:682-789) compute, per call,
 * q_i = embed(s_i) (x) embed(p_i) (complex.py:30-37, distmult.py:17-21: the "sp_" / "_po" halves of score_emb) and
 * then q . E^T.  Inside ONE launch the first half is a chain of five dependent memory round trips before the
 * first score can be stored -- 40 % of a launch at the FB15k-237 shape.  A caller that knows its
 * batches ahead (EntityRankingJob._evaluate iterates a DataLoader: eval_entity_ranking.py:158-170; so does every
 * training epoch) can take it off the critical path:
 *
 *   kge_build_queries(batch 0)                               -- one small launch, once
 *   kge_score_queries(batch k, next = batch k + 1) ...       -- ONE launch per batch: scores batch k from its
 *                                                               prepared queries, while workgroups on the compute
 *                                                               units the launch leaves idle build batch k + 1's
 *
 * `queries` is an opaque device buffer of kge_queries_bytes(t, combine, n) bytes (16-byte aligned; bf16 MFMA
 * operand fragments of the n query vectors; with KGE_FLAG_SPLIT_QUERY the q_hi and q_lo pieces), valid for the
 * tables, flags, combine and n it was built with; the caller double-buffers (`next->queries` must differ from
 * `queries`).  combine: KGE_SP_ (s, p given; o ignored), KGE_PO_ (p, o given; s ignored) or KGE_SP_PO (all three;
 * out[i, :m] = sp scores, out[i, b2:b2+m] = po scores, b2 = block2_offset or m).  Scores are bit-identical to kge_score_sp / _po /
 * _sp_po on the same tables and flags.  bf16 ComplEx / DistMult, dim 256 / 512; otherwise KGE_ERR_UNSUPPORTED.
 * No workspace, no flags to zero, no co-residency requirement: capture-safe, any n. */
typedef struct kge_next_queries {
  kge_index s, p, o;          /* the next batch (as for kge_build_queries)                       */
  int64_t n;                  /* 0: nothing to build                                             */
  void* queries;              /* destination, kge_queries_bytes(t, combine, n) bytes             */
  int64_t queries_bytes;
} kge_next_queries;
int64_t kge_queries_bytes(const kge_tables* t, int combine, int64_t n);
int kge_build_queries(const kge_tables* t, int combine, kge_index s, kge_index p, kge_index o,
                      int64_t n, void* queries, int64_t queries_bytes, void* stream);
/* block2_offset (KGE_SP_PO only): column at which the po block of a row starts, >= m and <= ldo - m; 0 = m
 * (the reference's cat layout).  With ldo and block2_offset multiples of 8 floats on a 32-byte aligned `out`
 * every store of the kernel covers whole 32-byte memory sectors (8 % per launch at the
 * FB15k-237 shape, 28 % on a Wikidata5M shard). */
int kge_score_queries(const kge_tables* t, int combine, const void* queries, int64_t n,
                      kge_index targets, int64_t m, float* out, int64_t ldo, int64_t block2_offset,
                      const kge_next_queries* next /* may be NULL */, void* stream);

/* GROUPS of batches in one launch.  A caller that iterates a split knows more than the next batch: an epoch's
 * DataLoader (kge/job/train_1vsAll.py:31-41) or EntityRankingJob._evaluate's loop (eval_entity_ranking.py:143-229)
 * can hand over `num_batches` equally shaped batches at once.  The scoring launch is then ONE persistent kernel that
 * streams the table through every compute unit once per batch and writes batch l's block at out + l * out_stride
 * (floats; each block laid out as kge_score_queries lays out its one): the launch gap, the cold start of a launch and
 * the compute units a single batch's grid cannot fill are paid once per group, not once per batch.
 *   kge_build_queries_multi   batch l = rows [l n, (l + 1) n) of s / p / o; its fragments at queries + l *
 *                             queries_stride (bytes; a multiple of 16, >= kge_queries_bytes(t, combine, n));
 *   kge_score_queries_multi   scores the group; `next` (may be NULL) describes the NEXT group -- num_batches batches of
 *                             next->n rows each, index vectors of num_batches * next->n entries, fragments next_stride
 *                             bytes apart in next->queries -- built by the same launch behind its last unit.
 *                             The next group's fragments are complete when the launch is complete.  At dim 512 the
 *                             workgroups that finish their scores early claim the build's slices through a counter
 *                             pair the library keeps per stream (launches of one stream are serial and leave it at 0;
 *                             DESIGN.md 37); a launch on a stream that is being captured builds a fixed slice per
 *                             workgroup instead (a captured launch may be replayed on any stream).  The same fragments.
 * Scores are bit-identical to num_batches kge_score_queries calls.  bf16 ComplEx / DistMult at dim 512 against all
 * entities; anything else KGE_ERR_UNSUPPORTED (loop over kge_score_queries instead). */
int kge_build_queries_multi(const kge_tables* t, int combine, kge_index s, kge_index p, kge_index o, int64_t n,
                            int64_t num_batches, void* queries, int64_t queries_stride, int64_t queries_bytes,
                            void* stream);
int kge_score_queries_multi(const kge_tables* t, int combine, const void* queries, int64_t queries_stride, int64_t n,
                            int64_t num_batches, kge_index targets, int64_t m, float* out, int64_t out_stride,
                            int64_t ldo, int64_t block2_offset, const kge_next_queries* next /* may be NULL */,
                            int64_t next_stride, void* stream);

/* Negative-sampling scores, the "triple" implementation without building the
 * [n*K,3] index tensor: slot 0/2 = corrupt s / o.
 * out[i*ldo + k] = score of triple i with slot replaced by neg[i*neg_ld + k].
 * BatchNegativeSample.score, kge/util/sampler.py:291-306. */
int kge_score_neg(const kge_tables* t, kge_index s, kge_index p, kge_index o,
                  int64_t n, int slot, const void* neg, int32_t neg_itype,
                  int64_t neg_ld, int64_t num_neg, float* out, int64_t ldo,
                  void* stream);

/* Negative-sampling scores with SHARED samples (negative_sampling.shared: true): the [n, K] block of
 * NaiveSharedNegativeSample.score / DefaultSharedNegativeSample.score, kge/util/sampler.py:428-463, 537-578
 * (and, for the "triple" implementation TransE / RotatE are forced to, of samples() at sampler.py:412-426, 503-535
 * scored through BatchNegativeSample.score, sampler.py:291-306), K = num_unique + num_repeat:
 *   out[i*ldo + c], c < num_unique   score of triple i with `slot` (0 / 2) replaced by unique[c] -- by the spare
 *                                    unique[num_unique] where drop != NULL and drop[i] == c
 *   out[i*ldo + num_unique + r]      = column repeat[r] (< num_unique) of the same row
 * drop == NULL: naive sharing, `unique` has num_unique ids.  drop != NULL: default sharing, `unique` has
 * num_unique + 1 ids (the last is the spare), drop[i] in [0, num_unique], drop[i] == num_unique uses no spare.
 * repeat may be NULL when num_repeat == 0.  Every target row is fetched once per workgroup (32 positives x 32
 * columns) and shared from LDS; the scores are bit-identical to kge_score_neg on the materialised samples; nothing
 * outside [n, K] is written.  Rows too wide for the LDS tile (f32 dim > 1024, bf16 dim > 2048): KGE_ERR_UNSUPPORTED. */
int kge_score_neg_shared(const kge_tables* t, kge_index s, kge_index p, kge_index o, int64_t n, int slot,
                         const void* unique, int32_t unique_itype, int64_t num_unique, const int64_t* drop,
                         const int64_t* repeat, int64_t num_repeat, float* out, int64_t ldo, void* stream);

/* Relation prediction: KgeModel.score_so, kge/model/kge_model.py:727-747.  out[i*ldo + j] = score of (s[i], rels[j],
 * o[i]): n (s, o) pairs against m relations -- rels.ptr == NULL: all of them, m == t->num_rel; else the listed ids
 * (they may repeat and need not be sorted).  The reference composes these scores from three repeats to [n*m, dim] and
 * the spo scorer (the generic "s_o" fallback of RelationalScorer.score_emb, kge_model.py:202-209); here a workgroup
 * stages a tile of relation rows once in LDS (RotatE: cos / sin of the phases, evaluated once per staged row) and
 * its pairs walk them from registers.  Every score has the bits kge_score_spo stores for the same triple; nothing
 * outside [n, m] is written.  ComplEx, DistMult, TransE and RotatE on float32 / bf16 tables; other scorers and rows
 * too wide for the LDS tile (f32 dim > 1024, bf16 dim > 2048): KGE_ERR_UNSUPPORTED.  n == 0 or m == 0: KGE_OK, nothing
 * is launched.  rels.ptr == NULL with m != t->num_rel, negative sizes, ldo < m: KGE_ERR_INVALID_ARG.  workspace:
 * kge_score_so_workspace_bytes(t, n, m) bytes of device scratch (currently 0 for every shape: pass NULL); less than
 * that: KGE_ERR_WORKSPACE. */
int64_t kge_score_so_workspace_bytes(const kge_tables* t, int64_t n, int64_t m);
int kge_score_so(const kge_tables* t, kge_index s, kge_index o, int64_t n, kge_index rels, int64_t m, float* out,
                 int64_t ldo, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- embedding-level scoring (dense inputs, no gather) ----------------- */
/* RelationalScorer.score_emb.  `t` supplies scorer, dtype, dim, rel_dim and
 * l_norm only (t->ent/rel ignored).  SPO: all three [n, *] -> out[n];
 * SP_: s,p [n,*], o [m,dim] -> out[n,m]; PO_: p,o [n,*], s [m,dim] -> out[n,m]. */
int kge_score_emb(const kge_tables* t, int combine, const void* s_emb,
                  int64_t s_ld, const void* p_emb, int64_t p_ld,
                  const void* o_emb, int64_t o_ld, int64_t n, int64_t m,
                  float* out, int64_t ldo, void* workspace,
                  int64_t workspace_bytes, void* stream);

/* score_sp_po on dense rows (KgeModel.score_sp_po, kge/model/kge_model.py:749-789, after its
 * embed() calls): s_emb / p_emb / o_emb are the n query rows, tgt_emb the m target rows;
 * out[i, :m] = sp_ scores, out[i, m:2m] = _po scores (ldo >= 2m), one two-sided launch when the
 * bf16 matrix-core kernel applies (workspace as for kge_score_sp_po).  Used by the entity-sharded
 * path, whose query rows arrive by all-gather. */
int kge_score_emb_sp_po(const kge_tables* t, const void* s_emb, int64_t s_ld, const void* p_emb,
                        int64_t p_ld, const void* o_emb, int64_t o_ld, int64_t n,
                        const void* tgt_emb, int64_t tgt_ld, int64_t m, float* out, int64_t ldo,
                        void* workspace, int64_t workspace_bytes, void* stream);
/* The same with the _po block `block2_offset` (>= m) floats behind the sp_ block of a row instead of right behind it
 * (ldo >= block2_offset + m): with both blocks on whole 256-byte lines -- block2_offset = a padded pitch, ldo twice
 * that -- the direct-store kernel takes its aligned store path (the per-rank launch of the sharded step). */
int kge_score_emb_sp_po_blocks(const kge_tables* t, const void* s_emb, int64_t s_ld, const void* p_emb,
                               int64_t p_ld, const void* o_emb, int64_t o_ld, int64_t n,
                               const void* tgt_emb, int64_t tgt_ld, int64_t m, float* out, int64_t ldo,
                               int64_t block2_offset, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- ranking ------------------------------------------------------------ */
/* For each row i of scores[n, c] (leading dim lds) and its true score:
 *   x = NaN -> -inf; filtered columns -> -inf; t = NaN -> -inf
 *   close   = (x == t) || (isfinite(|x-t|) && |x-t| <= atol + |rtol*t|)
 *   ties[i] += #close ;  rank[i] += #(x > t && !close)
 * Filtered columns of row i are lbl_col[lbl_rowptr[i] .. lbl_rowptr[i+1]) minus
 * col_offset; entries outside [0,c) and the entry equal to true_col[i] (global
 * id, may be NULL) are ignored.  Columns must be unique within a row.
 * lbl_rowptr == NULL: raw ranking.  rank/ties are int64 and ACCUMULATED
 * (counts are additive over entity chunks: eval_entity_ranking.py:310-313).
 * EntityRankingJob._filter_and_rank + _get_ranks_and_num_ties,
 * kge/job/eval_entity_ranking.py:533-596. */
int kge_rank_counts(const float* scores, int64_t lds, int64_t n, int64_t c,
                    const float* true_scores, const int64_t* lbl_rowptr,
                    const int64_t* lbl_col, int64_t col_offset,
                    const int64_t* true_col, float atol, float rtol,
                    int64_t* rank, int64_t* ties, void* stream);

/* ---- evaluation without host round trips --------------- */
/* The filter index of a set of splits lives on the device as sorted arrays:
 *   sorted_keys[num_keys]   unique keys (s*num_rel + p for the sp index, p*num_ent + o for po)
 *   starts[num_keys + 1]    range of key k in the index's value array
 *   values[...]             the known answers of each key, unique per key
 * (replaces the numba dict KvsAllIndex, kge/indexing.py:10-194).
 *
 * kge_filter_lookup: begin[i], end[i] = range of key a[i]*mult + b[i] (0, 0 if absent): what
 * get_sp_po_coords_from_spo_batch (kge/job/util.py:6-29) + _collate
 * (eval_entity_ranking.py:77-101) look up per batch on the host. */
int kge_filter_lookup(const int64_t* sorted_keys, int64_t num_keys, const int64_t* starts,
                      kge_index a, kge_index b, int64_t mult, int64_t n, int64_t* begin,
                      int64_t* end, void* stream);

/* Up to KGE_MAX_FILTER_QUERIES lookups in ONE launch: an evaluation batch needs four (the (s, p) and the
 * (p, o) keys of the filtered and of the filtered-with-test index), each a few dependent round trips of pure
 * latency on its own. */
#define KGE_MAX_FILTER_QUERIES 4
typedef struct kge_filter_query {
  const int64_t* sorted_keys;
  int64_t num_keys;
  const int64_t* starts;
  kge_index a, b;
  int64_t mult;
  int64_t* begin;
  int64_t* end;
} kge_filter_query;
int kge_filter_lookup_multi(const kge_filter_query* queries, int num_queries, int64_t n, void* stream);

/* kge_rank_counts for the raw ranking and `num_filters` (<= KGE_MAX_FILTERS) filtered
 * rankings from ONE scan of the scores: rank/ties are [num_filters + 1][n] int64, row 0 raw,
 * row k + 1 filtered by the columns lbl_col[k][lbl_begin[k][i] .. lbl_end[k][i]) of row i
 * (global ids, minus col_offset; the one equal to true_col[i] stays).  ACCUMULATED over
 * entity chunks.  lbl_begin / lbl_end / lbl_col are HOST arrays of device pointers.
 * eval_entity_ranking.py:233-313 runs _filter_and_rank once per ranking. */
#define KGE_MAX_FILTERS 4
int kge_rank_counts_multi(const float* scores, int64_t lds, int64_t n, int64_t c,
                          const float* true_scores, int num_filters,
                          const int64_t* const* lbl_begin, const int64_t* const* lbl_end,
                          const int64_t* const* lbl_col, int64_t col_offset,
                          const int64_t* true_col, float atol, float rtol, int64_t* rank,
                          int64_t* ties, void* stream);

/* Scoring and rank counting in ONE kernel: the counts kge_score_sp_po + kge_rank_counts_multi produce for the
 * entity slice [col_begin, col_begin + m) (bit for bit: the same score chains, the same tie arithmetic),
 * without the [n, 2m] score matrix ever being written or read -- EntityRankingJob._evaluate's
 * score_sp_po -> _filter_and_rank -> _get_ranks_and_num_ties (eval_entity_ranking.py:227-313) per entity chunk.
 *   true_sp[i] / true_po[i]   score of triple i as the sp_ / _po scoring sees it (an element of the score
 *                             matrix: e.g. the diagonal of kge_score_sp_po against targets = o resp. s);
 *   sp_* / po_*               num_filters (<= 2) filter sets per direction, as for kge_rank_counts_multi:
 *                             HOST arrays of device pointers; columns are global entity ids, the row's own
 *                             o[i] (sp_) / s[i] (_po) is never filtered;
 *   rank_* / ties_*           [num_filters + 1][ld] int64, row 0 raw, ACCUMULATED (over entity chunks);
 *   filter_bits               >= kge_score_rank_bits_bytes(n, m, num_filters) bytes, 8-byte aligned, ZEROED ONCE
 *                             before its first use: the call sets one bit per filtered (row, column), counts,
 *                             and clears the same words again (all-zero between calls);
 *   workspace                 as for kge_score_sp_po (kge_score_workspace_bytes(t, n)).
 * KGE_ERR_UNSUPPORTED (tables other than bf16 ComplEx / DistMult with dim 256 / 512, a launch the
 * loader/consumer kernel declines): use kge_score_sp_po + kge_rank_counts_multi. */
int64_t kge_score_rank_bits_bytes(int64_t n, int64_t m, int num_filters);
int kge_score_rank_sp_po(const kge_tables* t, kge_index s, kge_index p, kge_index o, int64_t n,
                         int64_t col_begin, int64_t m, const float* true_sp, const float* true_po,
                         int num_filters, const int64_t* const* sp_begin, const int64_t* const* sp_end,
                         const int64_t* const* sp_col, const int64_t* const* po_begin,
                         const int64_t* const* po_end, const int64_t* const* po_col, float atol, float rtol,
                         int64_t* rank_sp, int64_t* ties_sp, int64_t* rank_po, int64_t* ties_po, int64_t ld,
                         void* filter_bits, int64_t filter_bits_bytes, void* workspace,
                         int64_t workspace_bytes, void* stream);

/* Band-and-rescore: the counts of kge_score_rank_sp_po / kge_eval_batch under KGE_FLAG_SPLIT_QUERY --
 * the parity-compliant evaluation mode, EntityRankingJob._get_ranks_and_num_ties' tie band honoured on full-precision
 * query vectors (eval_entity_ranking.py:571-596) -- at close to the price of the SINGLE-PASS counting kernel.  The
 * single-pass score x_hi is the hi half of the split score x = fl(x_hi + x_lo), and |x_lo| <= ||q_lo_i|| * max_j ||t_j||:
 * with row i's tolerance widened by that bound, a score outside the widened band compares with the true score the same
 * way under x_hi and under x.  Launch 1 (the single-pass counting kernel on the q_hi fragments) counts those and LISTS
 * the (row, column) pairs inside the band -- per wave, no atomics --; launch 2 gathers the listed columns' table rows,
 * scores them with both chains (the bits the split kernel counts) and finishes the counts.  Identical (rank, ties) to
 * the split kernel by construction and by test WHEN NO PAIR WAS DROPPED; on a trained model (true scores in the tail of
 * their rows) ~2e-5 of the pairs are listed, on random tables ~1.5 % -- far more than the lists hold.
 *   table_max_norm  [1] device float: kge_table_max_row_norm of the scored rows [col_begin, col_begin + m);
 *   list            device scratch, 16-byte aligned, >= kge_rank_band_list_bytes(n) bytes, ZEROED ONCE by the caller
 *                   before the first call (the calls leave every list empty); 255 pairs per wave and 256-row chunk;
 *   status          [2] device uint32 or NULL, zeroed by the caller: [0] += pairs listed, [1] += pairs DROPPED because
 *                   a wave's list was full (sticky).
 * status[1] != 0 means some call's counts are INCOMPLETE: the caller must redo those batches without `band` (the
 * evaluator reads the words once at the end of a run -- no host wait per batch -- and falls back to the split kernel
 * for the run; it also probes the first batch and drops the band when it lists too much: nothing to gain there).
 * band == NULL: the plain entry points.  KGE_ERR_INVALID_ARG: band without KGE_FLAG_SPLIT_QUERY, missing pieces;
 * KGE_ERR_WORKSPACE: list too small for n; KGE_ERR_UNSUPPORTED as for kge_score_rank_sp_po. */
typedef struct kge_rank_band {
  const float* table_max_norm;
  void* list;
  int64_t list_bytes;
  uint32_t* status;
} kge_rank_band;
int64_t kge_rank_band_list_bytes(int64_t n);
/* 1.001 x the largest Euclidean norm of the rows [row_begin, row_begin + m) of the bf16 entity table, into out[0]
 * (device).  Once per table state (an evaluation run), not per batch. */
int kge_table_max_row_norm(const kge_tables* t, int64_t row_begin, int64_t m, float* out, void* stream);
int kge_score_rank_sp_po_band(const kge_tables* t, kge_index s, kge_index p, kge_index o, int64_t n,
                              int64_t col_begin, int64_t m, const float* true_sp, const float* true_po,
                              int num_filters, const int64_t* const* sp_begin, const int64_t* const* sp_end,
                              const int64_t* const* sp_col, const int64_t* const* po_begin,
                              const int64_t* const* po_end, const int64_t* const* po_col, float atol, float rtol,
                              int64_t* rank_sp, int64_t* ties_sp, int64_t* rank_po, int64_t* ties_po, int64_t ld,
                              void* filter_bits, int64_t filter_bits_bytes, void* workspace,
                              int64_t workspace_bytes, void* stream, const kge_rank_band* band);

/* The same for dense query rows (the row-sharded multi-GPU path: s / p / o rows come out of the exchange, the
 * scored rows tgt_emb[m] are this rank's shard, whose global entity ids start at col_begin; s_ids / o_ids =
 * the global ids of the rows' true subject / object, which the filters never remove).  Counts of the shard's
 * columns only: the caller sums them over the ranks (one int64 all-reduce). */
int kge_score_rank_emb_sp_po(const kge_tables* t, const void* s_emb, int64_t s_ld, const void* p_emb,
                             int64_t p_ld, const void* o_emb, int64_t o_ld, kge_index s_ids, kge_index o_ids,
                             int64_t n, const void* tgt_emb, int64_t tgt_ld, int64_t col_begin, int64_t m,
                             const float* true_sp, const float* true_po, int num_filters,
                             const int64_t* const* sp_begin, const int64_t* const* sp_end,
                             const int64_t* const* sp_col, const int64_t* const* po_begin,
                             const int64_t* const* po_end, const int64_t* const* po_col, float atol, float rtol,
                             int64_t* rank_sp, int64_t* ties_sp, int64_t* rank_po, int64_t* ties_po, int64_t ld,
                             void* filter_bits, int64_t filter_bits_bytes, void* workspace,
                             int64_t workspace_bytes, void* stream);

/* One evaluation batch of EntityRankingJob._evaluate (eval_entity_ranking.py:103-481: label lookup, score_sp_po,
 * _filter_and_rank per ranking, _get_ranks, hist_all) against ALL entities in FOUR launches, one call:
 *   (1) the filter ranges of the batch's (s, p) / (p, o) keys in up to two filter indexes (kge_filter_lookup's
 *       search) and one bit per filtered (row, column) -- the row's own o / s never --, plus the target list (o | s);
 *   (2) the true scores: the batch against its own targets (kge_score_sp_po on 2 n target rows), diagonals kept;
 *   (3) scoring + counting (kge_score_rank_sp_po's kernels: no [n, 2E] score matrix);
 *   (4) the bits cleared again, tie policy + rank histograms of both directions (kge_rank_hist), counters zeroed.
 * counts: int64 [2 (o | s)][2 (rank | ties)][num_filters + 1][n], ALL-ZERO on entry and again on return; hist:
 * float [num_filters + 1][ldh] accumulated (row 0 raw); ranks_o / ranks_s: int64 [num_filters + 1][n] or NULL;
 * filter_bits: as for kge_score_rank_sp_po (>= kge_score_rank_bits_bytes(n, num_entities, num_filters) bytes, ZEROED
 * ONCE before its first use, all-zero between calls); scratch: kge_eval_batch_scratch_bytes(t, n, num_filters) bytes,
 * 16-byte aligned, contents irrelevant; workspace as for kge_score_sp_po.  KGE_ERR_UNSUPPORTED: tables without a
 * counting kernel (see kge_score_rank_sp_po) -- nothing was counted, nothing left behind.  No host wait. */
typedef struct kge_eval_filter {
  const int64_t* sp_keys;   int64_t sp_num_keys; const int64_t* sp_starts; const int64_t* sp_values;  /* key s*R + p -> o's */
  const int64_t* po_keys;   int64_t po_num_keys; const int64_t* po_starts; const int64_t* po_values;  /* key p*E + o -> s's */
} kge_eval_filter;
int64_t kge_eval_batch_scratch_bytes(const kge_tables* t, int64_t n, int num_filters);
int kge_eval_batch(const kge_tables* t, kge_index s, kge_index p, kge_index o, int64_t n, int num_filters,
                   const kge_eval_filter* filters, float atol, float rtol, int tie_policy, int64_t* counts,
                   float* hist, int64_t ldh, int64_t* ranks_o, int64_t* ranks_s, void* filter_bits,
                   int64_t filter_bits_bytes, void* scratch, int64_t scratch_bytes, void* workspace,
                   int64_t workspace_bytes, void* stream);

/* kge_eval_batch with band-and-rescore in step (3) (see kge_score_rank_sp_po_band); band == NULL: kge_eval_batch. */
int kge_eval_batch_band(const kge_tables* t, kge_index s, kge_index p, kge_index o, int64_t n, int num_filters,
                        const kge_eval_filter* filters, float atol, float rtol, int tie_policy, int64_t* counts,
                        float* hist, int64_t ldh, int64_t* ranks_o, int64_t* ranks_s, void* filter_bits,
                        int64_t filter_bits_bytes, void* scratch, int64_t scratch_bytes, void* workspace,
                        int64_t workspace_bytes, void* stream, const kge_rank_band* band);

/* hist[m*ldh + r] += 1.0f with r = rank of the tie policy, for all [num_rankings][n] counts;
 * ranks_out (may be NULL) receives r.  EntityRankingJob._get_ranks (:598-618) + hist_all
 * (:665-687); the float32 histogram is the reference's. */
enum { KGE_TIES_ROUNDED_MEAN = 0, KGE_TIES_BEST = 1, KGE_TIES_WORST = 2 };
int kge_rank_hist(const int64_t* rank, const int64_t* ties, int num_rankings, int64_t n,
                  int tie_policy, float* hist, int64_t ldh, int64_t num_ent,
                  int64_t* ranks_out, void* stream);

/* ---- filtered top-k link prediction (topk.hip) ---------------------------- */
/* The k best entities of (s_i, p_i, ?) (dir = KGE_SP_, a = s) or (?, p_i, o_i) (dir = KGE_PO_, a = o: the direction
 * codes of kge_ce_fwd) among the entity rows [col_begin, col_begin + m), the columns of up to two filter sets left
 * out, without the [n, m] score matrix.  It replaces, in the reference, KgeModel.score_sp / score_po
 * (kge/model/kge_model.py:682-725), the masking of EntityRankingJob._filter_and_rank
 * (kge/job/eval_entity_ranking.py:233-313: known answers set to -inf) and torch.topk over the masked row.
 *   scores      the canonical chain: every score has the bits kge_score_sp / kge_score_po store for the
 *               same tables -- float32 tables, TransE / RotatE at either dtype, bf16 ComplEx / DistMult as under
 *               KGE_FLAG_EXACT (the entry always takes the exact chain, whatever the flag says);
 *   order       descending canonical score (NaN counts as -inf, -0.0 as +0.0), equal scores by ASCENDING entity id:
 *               every element of the result is determined (torch.topk leaves the order among equal scores open);
 *   f_*         num_filters (<= 2) filter sets as for kge_rank_counts_multi: HOST arrays of device pointers, row i's
 *               columns are f_col[k][f_begin[k][i] .. f_end[k][i]) (global entity ids; ids outside the scored slice are
 *               ignored).  A column listed in ANY set is left out -- except keep[i] (keep.ptr == NULL: no exception);
 *   out_val     [n][ld] float32, out_idx [n][ld] int64, ld >= k: the first k entries of a row are written, nothing
 *               else.  A row with fewer than k columns left is padded with (-inf, -1) BEHIND its real columns (a real
 *               column whose score is -inf or NaN is listed, as -inf, in its id order, ahead of the padding);
 *   workspace   >= kge_topk_workspace_bytes(t, n, m, k, num_filters) bytes, 16-byte aligned, contents irrelevant: the
 *               call zeroes the filter bits it uses itself and leaves nothing the caller has to preserve.
 * The result is a pure function of the arguments: it does not depend on how the launch cuts the columns into groups.
 * Stream-ordered, no host wait.  KGE_ERR_INVALID_ARG: k < 1, k > KGE_TOPK_MAX, ld < k, NULL outputs with n > 0,
 * m >= 2^32, a slice outside the table, a missing filter pointer; KGE_ERR_WORKSPACE: workspace too small or misaligned;
 * KGE_ERR_UNSUPPORTED: KGE_FLAG_SPLIT_QUERY / KGE_FLAG_BF16_V3 in the tables' flags, num_filters > 2.  n == 0 or
 * m == 0: KGE_OK (m == 0: every row is padding). */
enum { KGE_TOPK_MAX = 128 };
int64_t kge_topk_workspace_bytes(const kge_tables* t, int64_t n, int64_t m, int k, int num_filters);
int kge_topk(const kge_tables* t, int dir, kge_index a, kge_index p, int64_t n, int64_t col_begin, int64_t m, int k,
             int num_filters, const int64_t* const* f_begin, const int64_t* const* f_end,
             const int64_t* const* f_col, kge_index keep, float* out_val, int64_t* out_idx, int64_t ld,
             void* workspace, int64_t workspace_bytes, void* stream);

/* ---- LookupEmbedder.embed ------------------------------------------------ */
/* ent_out[i, :] = ent[ent_idx[i], :] (n_ent rows, leading dimension ent_ldo elements) and
 * rel_out[i, :] = rel[rel_idx[i], :] in ONE launch (table dtype; rows of 16-byte multiples).
 * kge/model/embedder/lookup_embedder.py:96-105.  The scoring entry points gather on the fly
 * and never need this; the entity-sharded path does: a rank gathers the query rows it owns
 * before the single all-gather of a batch.  Either count may be 0. */
int kge_embed(const kge_tables* t, kge_index ent_idx, int64_t n_ent, void* ent_out,
              int64_t ent_ldo, kge_index rel_idx, int64_t n_rel, void* rel_out,
              int64_t rel_ldo, void* stream);

/* BCEWithLogitsKgeLoss over the [n, c = 1 + K] score block of one negative-sampling slot (kge/util/loss.py:136-189 on
 * the block TrainingJobNegativeSampling._process_subbatch assembles, train_negative_sampling.py:120-151: column 0 the
 * positive, columns 1.. its negatives), forward and gradient in one pass:
 *   kind 0 "bce": sum_j l(x_j, y_j);  1 "bce_mean": (l(x_0, 1) + sum_{j>=1} l(x_j, 0) / K) / 2;
 *   2 "bce_self_adversarial": (l(x_0, 1) + sum_{j>=1} w_j l(x_j, 0)) / 2, w = softmax_j(temperature * x_j), not
 *   differentiated -- x = score + offset (train.loss_arg), l = torch.nn.BCEWithLogitsLoss's element.
 * loss_rows[i] = row i's term (the job's loss is their sum, divided by the batch size by the job);
 * grad (may be NULL) [n, c], leading dimension ldg: d (sum_i loss_rows[i]) / d scores[i, j]. */
int kge_ns_bce_loss(const float* scores, int64_t ld, int64_t n, int64_t c, int kind, float offset, float temperature,
                    float* loss_rows, float* grad, int64_t ldg, void* stream);

/* Every negative-sampling loss of LibKGE over one slot's scores, the positive and its negatives as TWO pieces: row i
 * has x_0 = pos[i * pos_stride] and x_j = neg[i * neg_ld + j - 1], j = 1..K (a contiguous [n, 1 + K] block is the
 * special case pos = scores, pos_stride = ld, neg = scores + 1, neg_ld = ld).  Forward and gradient in one launch, one
 * wave per row, no atomics (two runs give the same bits):
 *   kinds 0-2  the arithmetic of kge_ns_bce_loss, arg = offset                         kge/util/loss.py:153-186
 *   kind 3 "kl"              lse_j(x_j) - x_0: KLDivWithSoftmaxKgeLoss on the label matrix "column 0 is 1"
 *                            (0 log 0 = 0); d / d x_j = softmax(x)_j - [j = 0]         kge/util/loss.py:198-213
 *   kind 4 "margin_ranking"  sum_{j>=1} clamp_min(-(x_0 - x_j) + arg, 0), arg = the margin (train.loss_arg), in
 *                            float32 in torch's order; the subgradient is torch's: a negative with v_j >= 0 (the exact
 *                            tie v_j = 0 INCLUDED) gets 1, the positive minus their count   kge/util/loss.py:236-252
 *   kind 5 "soft_margin"     sum_j log(1 + exp(-t_j x_j)), t_0 = 1, t_j = -1, as max(z, 0) + log1p(exp(-|z|)): finite
 *                            where the reference's float32 log(1 + exp(z)) overflows (z >~ 89);
 *                            d / d x_j = -t_j sigmoid(-t_j x_j)                        kge/util/loss.py:221-224
 *   kind 6 "se"              sum_j (x_j - y_j)^2, y_0 = 1, y_j = 0; d / d x_j = 2 (x_j - y_j)   kge/util/loss.py:272-274
 * arg is ignored by kinds 3, 5 and 6, temperature by all but kind 2.
 * loss_rows[i] = row i's term (the job's loss is their sum).  g_pos / g_neg: both NULL (no gradient) or both set:
 * g_pos[i * g_pos_stride] = d (sum loss_rows) / d x_0 of row i, g_neg[i * g_neg_ld + j - 1] = ... / d x_j.
 * KGE_ERR_INVALID_ARG: K < 1, an unknown kind, a NULL piece, one gradient pointer without the other, a leading
 * dimension below K; n == 0 is KGE_OK. */
int kge_ns_loss(const float* pos, int64_t pos_stride, const float* neg, int64_t neg_ld, int64_t n, int64_t K, int kind,
                float arg, float temperature, float* loss_rows, float* g_pos, int64_t g_pos_stride, float* g_neg,
                int64_t g_neg_ld, void* stream);

/* The negative samples of one slot drawn ON THE DEVICE (KgeSampler.sample, kge/util/sampler.py:80-137, with
 * _filter_and_resample*, :163-196 / 700-752): one launch draws, filters and redraws.
 *   out[i * ld + k], i < n, k < K  = the draw of the first attempt t = 0, 1, 2, ... that is NOT among the known answers
 *   of row i's key a[i] * mult + b[i] in the filter index (sorted_keys / starts / values as for kge_filter_lookup; a key
 *   absent from the index has no known answers).  Rejection sampling: the same distribution as the reference's resample
 *   loop -- uniform, or frequency weighted, over the non-positives.
 * Random numbers: Philox4x32-10, counter based, no state, no library.  One block r0..r3 per (row, column, attempt):
 *   key = (seed low 32, seed high 32),  counter = (k, i, t, (uint32)call * 4 + slot)
 *   uniform (alias_prob == alias_idx == NULL):  id = umul64hi((r0 << 32) | r1, vocab)
 *   frequency (alias tables [vocab]):  bucket = umul64hi((r0 << 32) | r1, vocab), u = (r2 >> 8) * 2^-24,
 *                                      id = u < alias_prob[bucket] ? bucket : alias_idx[bucket]
 * so a draw is a pure function of (seed, call, slot, i, k, t): two runs give the same bits, whatever the launch.
 * sorted_keys == NULL: unfiltered (starts, values, a, b, mult ignored; every first draw is kept).
 * A column stops after KGE_NEG_SAMPLE_MAX_ATTEMPTS attempts and keeps its last draw (a key whose answers cover the
 * vocabulary: the reference never returns).  stats (NULL or int32 [n, 2]): stats[i * 2] = row i's number of rejected
 * attempts (the kept draw of a capped column included), stats[i * 2 + 1] = its columns that hit the cap; plain
 * stores, no atomics.
 * slot: 0 (subject) or 2 (object); it only enters the counter -- the caller passes the matching index and key columns
 * (slot 0: the po index, a = p, b = o, mult = num_ent; slot 2: the sp index, a = s, b = p, mult = num_rel).
 * n == 0 or K == 0: KGE_OK, nothing written; nothing outside [n, K] is written when ld > K.
 * KGE_ERR_INVALID_ARG: vocab < 1, slot 1 (the relation slot) or any other slot, one alias pointer without the other,
 * sorted_keys without starts / values / a / b, ld < K, out NULL; n or K above 2^32: KGE_ERR_UNSUPPORTED. */
#define KGE_NEG_SAMPLE_MAX_ATTEMPTS 256
int kge_neg_sample(int64_t n, int64_t K, int64_t vocab, int slot, uint64_t seed, uint64_t call,
                   const float* alias_prob, const int64_t* alias_idx,
                   const int64_t* sorted_keys, int64_t num_keys, const int64_t* starts, const int64_t* values,
                   kge_index a, kge_index b, int64_t mult,
                   int64_t* out, int64_t ld, int32_t* stats, void* stream);

/* A KvsAll batch built ON THE DEVICE from the batch's example numbers: what TrainingJobKvsAll's collate function does
 * on the host (kge/job/train_KvsAll.py:118-201, a Python loop over the examples) plus the cut of its label_coords into
 * one CSR per query type that the fused KvsAll losses read (kge_kl_* / kge_bce_* and their _dist / _f32 forms), padded
 * or not.  The index arrays never change during training and stay on the device; integer work only, no atomics.
 *
 * types[t], t < num_types (1..3), ordered as the job's query_types: the KvsAllIndex of the type -- keys int64 [M_t, 2],
 *   offsets int64 [M_t + 1], values int64 [offsets[M_t]], all on the device -- with
 *     last        the example number right after the type's last example (query_last_example: type t owns
 *                 [types[t-1].last, types[t].last), type 0 starts at 0; M_t = last - previous last)
 *     target_col  the triple column its labels go to: 2 for sp_, 1 for s_o, 0 for _po; its two key columns go to the
 *                 remaining triple columns in S, P, O order (train_KvsAll.py:165-170)
 * examples  int64 [n] on the device: the batch; a number may occur more than once.  A number outside
 *           [0, types[num_types-1].last) is read as the nearest valid one (nothing is read out of bounds).
 * nnz_cap   the label entries the batch form holds; the caller computes the batch's label count on the host from its own
 *           copy of the offsets.  Label positions >= nnz_cap are copied to neither form.
 *
 * Batch form (queries, query_type, label_coords, triples: all four or none; the last two may be NULL when nnz_cap == 0)
 * -- the collate function's dictionary:
 *   queries int64 [n, 2], query_type int64 [n], label_coords int32 [nnz_cap, 2] = (batch row, label), triples int64
 *   [nnz_cap, 3]; rows in batch order, the labels of a row in index order.  Entries at label positions >= the batch's
 *   label count are left as they are.
 * Typed form (typed == NULL or [num_types]; ids, rowptr, col required -- ids / col may be NULL at capacity 0 --, weight
 * and rows optional, each type its own):
 *   ids int64 [rows_cap, 2], rowptr int64 [rows_cap + 1], col int64 [lab_cap], weight float32 [rows_cap], rows int64
 *   [rows_cap].  The real rows are the type's batch rows in batch order with their labels in index order, weight =
 *   `weight`, rows = the batch row.  The remaining rows are padding: ids (0, 0), ONE label 0 each (rowptr goes on in
 *   steps of 1), weight 0, rows -1; col is 0 beyond the real labels.  rows_cap == n_t and lab_cap == nnz_t: the exact
 *   CSR.
 * counts (NULL or int64 [3 * num_types]): per type n_t, nnz_t, fits; fits = 1 iff n_t <= rows_cap and
 *   nnz_t + (rows_cap - n_t) <= lab_cap (1 without a typed form).  The contents of the typed outputs of a type with
 *   fits == 0 are unspecified; nothing is written outside any output's stated extent in any case.
 * workspace: device scratch of kge_kvsall_collate_workspace_bytes(n) = 8 * (2 n + 4) bytes, 8-byte aligned (too small:
 *   KGE_ERR_WORKSPACE).
 * Two launches on `stream` (the scans in one workgroup, then the label copy); no allocation, no host wait, capturable.
 * Rows without labels (offsets[e] == offsets[e + 1]) are legal.  n == 0: KGE_OK, nothing written.
 * KGE_ERR_INVALID_ARG: num_types outside 1..3, a NULL index array, last values that decrease or no example at all, a
 * target_col outside 0..2, negative sizes or capacities, examples / workspace NULL, a batch or typed form given in part.
 * The scans run in ONE workgroup: n > KGE_KVSALL_COLLATE_MAX_N (2^20) is KGE_ERR_UNSUPPORTED, as is nnz_cap >= 2^31
 * (label_coords is int32). */
#define KGE_KVSALL_COLLATE_MAX_N (1 << 20)
typedef struct kge_kvsall_index {
  const int64_t* keys;
  const int64_t* offsets;
  const int64_t* values;
  int64_t last;
  int32_t target_col;
  int32_t reserved_; /* 0 */
} kge_kvsall_index;
typedef struct kge_kvsall_typed {
  int64_t* ids;
  int64_t* rowptr;
  int64_t* col;
  float* weight;
  int64_t* rows;
  int64_t rows_cap;
  int64_t lab_cap;
} kge_kvsall_typed;
int64_t kge_kvsall_collate_workspace_bytes(int64_t n);
int kge_kvsall_collate(const kge_kvsall_index* types, int num_types, const int64_t* examples, int64_t n, int64_t nnz_cap,
                       int64_t* queries, int64_t* query_type, int32_t* label_coords, int64_t* triples,
                       const kge_kvsall_typed* typed, float weight, int64_t* counts, void* workspace,
                       int64_t workspace_bytes, void* stream);

/* The two row moves of the entity-sharded exchange (kge_amd/sharded.py: ShardedEntityTable.exchange_rows),
 * the id arithmetic evaluated inside the kernel, one launch each:
 *   kge_shard_gather   t->ent = THIS RANK's rows [lo, lo + t->num_ent) of the entity table.  For j < num_ids (1 or 2
 *                      id vectors of GLOBAL entity ids, e.g. the s and the o column of a batch), i < n:
 *                        send[(j*n + i) * send_ld ..] = t->ent[clamp(ids[j][i] - lo, 0, t->num_ent - 1)]
 *                      (an id this rank does not own reads some local row: that entry of the rank's block is never
 *                      picked) and, if rel_out != NULL, rel_out[i] = t->rel[rel_idx[i]] (replicated relation table).
 *   kge_shard_pick     after the all-gather of the ranks' blocks (`gathered` = world x [num_ids * n] rows, leading
 *                      dimension ld):  rows[j*n + i] = gathered[(ids[j][i] / shard_rows) * num_ids * n + j*n + i],
 *                      the owner's copy of every row (shard_rows = ceil(E / world), the rows per rank).
 * dtype: kge_dtype of the rows.  Rows must be 16-byte multiples on 16-byte aligned pitches (KGE_ERR_UNSUPPORTED). */
int kge_shard_gather(const kge_tables* t, int64_t lo, const kge_index* ids, int num_ids, int64_t n, void* send,
                     int64_t send_ld, kge_index rel_idx, void* rel_out, int64_t rel_ldo, void* stream);
int kge_shard_pick(const void* gathered, int64_t ld, int dtype, int64_t dim, int64_t shard_rows, int world,
                   const kge_index* ids, int num_ids, int64_t n, void* rows, int64_t rows_ld, void* stream);

/* ---- 1vsAll loss fused with the scoring ---------------- */
/* loss_rows[i] = logsumexp_j score(i, j) - score(i, label[i]),  lse[i] = logsumexp_j score(i, j),
 * j over ALL entities; score(i, .) = the kge_score_sp row (dir = KGE_SP_, a = s, label = o) or
 * the kge_score_po row (dir = KGE_PO_, a = o, label = s).  sum_i loss_rows[i] is what
 * TrainingJob1vsAll computes with the default `train.loss: kl`: score_sp / score_po
 * (kge/job/train_1vsAll.py:64, 75) followed by KLDivWithSoftmaxKgeLoss with index labels =
 * CrossEntropyLoss(reduction="sum") (kge/util/loss.py:192-207, train_1vsAll.py:65, 76).
 * The [n, num_ent] score matrix is never written: the scoring kernel folds every tile into a
 * per-row running (max, sum exp).  The scores inside are bit-identical to kge_score_sp /
 * kge_score_po on the same tables.
 *
 * A label outside [0, num_ent) gives loss_rows[i] = NaN (the reference raises an index error).
 *
 * kge_ce_bwd: gradients of sum_i g_i * loss_rows[i] (g_i = g_rows[i], or g_scalar if g_rows is
 * NULL -- the reference's 1 / batch_size), laid out as for kge_score_pairs_bwd:
 *   g_a [n, dim], g_p [n, rel_dim], g_tgt [num_ent, dim]   (f32, OVERWRITTEN)
 * The kernel recomputes the score tiles, writes d loss / d score in bf16 to the workspace and
 * runs the two gradient products of the mixed-precision backward on it.
 *
 * ComplEx / DistMult, bf16 tables, dim in {128, 256, 512}; anything else:
 * KGE_ERR_UNSUPPORTED (compose kge_score_sp + the loss instead).  Both calls need
 * `workspace_bytes >= kge_ce_workspace_bytes(t, n)` of 256-byte aligned device scratch (no
 * initialisation; stream-ordered use; not shared by concurrent calls).  Not capturable into a
 * hipGraph (the gradient products go through hipBLASLt). */
int64_t kge_ce_workspace_bytes(const kge_tables* t, int64_t n);
int kge_ce_fwd(const kge_tables* t, int dir, kge_index a, kge_index p, kge_index label,
               int64_t n, float* loss_rows, float* lse, void* workspace,
               int64_t workspace_bytes, void* stream);
int kge_ce_bwd(const kge_tables* t, int dir, kge_index a, kge_index p, kge_index label,
               int64_t n, const float* lse, const float* g_rows, float g_scalar, float* g_a,
               float* g_p, float* g_tgt, void* workspace, int64_t workspace_bytes,
               void* stream);

/* ---- the same loss for the distance scorers on float32 tables ---------------- */
/* kge_ce_dist_fwd / kge_ce_dist_bwd: loss_rows, lse and the gradients exactly as kge_ce_fwd / kge_ce_bwd define
 * them, for TransE and RotatE (transe.py:18-34, rotate.py:30-64) with l_norm 1 or 2 on float32 tables: the step of
 * TrainingJob1vsAll (kge/job/train_1vsAll.py:64-81) with KLDivWithSoftmaxKgeLoss on index labels
 * (kge/util/loss.py:192-207) without an [n, num_ent] matrix.  The forward folds every score tile into a per-row
 * running (max, sum exp) and merges the partial results in a fixed order (no atomics: the same bits on every run);
 * every score inside is bit-identical to kge_score_sp / kge_score_po on the same tables.  The backward walks the
 * entity columns in chunks: the scoring kernels write one [n, chunk] block of scores into the workspace, the
 * gradient kernels form d loss / d score from it, lse and label while they read it.
 *   g_rows, g_scalar, g_a [n, dim], g_p [n, rel_dim], g_tgt [num_ent, dim]: as for kge_ce_bwd (f32, OVERWRITTEN).
 *   A label outside [0, num_ent) gives loss_rows[i] = NaN.
 * kge_ce_dist_workspace_bytes(t, n, chunk_cols): chunk_cols = columns per chunk of the backward, a multiple of 64
 * (>= 64), or 0 = the library's default (a score chunk of at most 32 MB, at least 64 columns, clamped to num_ent
 * rounded up to 64); returns 0 for tables the calls do not take.  The workspace holds the forward's records
 * (12 bytes per row and column group, at most 256 groups), an [n, dim] buffer and the [n, chunk] score block:
 * 256-byte aligned device scratch, no initialisation, stream-ordered use, not shared by concurrent calls.  The
 * backward derives its chunk width from `workspace_bytes` (any size from chunk_cols = 64 up is valid: a smaller
 * workspace only means more chunks; below that, and for the forward below its records, KGE_ERR_WORKSPACE).
 * ComplEx / DistMult, bf16 tables or another l_norm: KGE_ERR_UNSUPPORTED, nothing is launched.  No allocation, no
 * host wait, no library call: both are stream-ordered and capturable into a hipGraph. */
int64_t kge_ce_dist_workspace_bytes(const kge_tables* t, int64_t n, int64_t chunk_cols);
int kge_ce_dist_fwd(const kge_tables* t, int dir, kge_index a, kge_index p, kge_index label,
                    int64_t n, float* loss_rows, float* lse, void* workspace,
                    int64_t workspace_bytes, void* stream);
int kge_ce_dist_bwd(const kge_tables* t, int dir, kge_index a, kge_index p, kge_index label,
                    int64_t n, const float* lse, const float* g_rows, float g_scalar, float* g_a,
                    float* g_p, float* g_tgt, void* workspace, int64_t workspace_bytes,
                    void* stream);

/* ---- the same loss for ComplEx / DistMult on FLOAT32 tables -------------------- */
/* kge_ce_f32_fwd / kge_ce_f32_bwd: loss_rows, lse and the gradients exactly as kge_ce_fwd / kge_ce_bwd define them, for
 * ComplEx and DistMult (complex.py:30-39, distmult.py:15-21) on float32 tables -- the reference's own precision: the
 * step of TrainingJob1vsAll (kge/job/train_1vsAll.py:64-81) with KLDivWithSoftmaxKgeLoss on index labels
 * (kge/util/loss.py:192-207) without an [n, num_ent] matrix.  The forward is the exact f32 matrix-core scoring kernel
 * with a fold epilogue: every score inside is bit-identical to kge_score_sp / kge_score_po on the same tables, one
 * (max, sum exp, label score) record per row and column group is merged in a fixed order (no atomics: the same bits
 * on every run).  The backward walks the entity columns in chunks: per chunk the scoring kernel writes
 * d loss / d score [n, chunk] into the workspace, and the two f32 matrix-core products of kge_score_pairs_bwd turn
 * it into the chunk's rows of g_tgt (OVERWRITTEN: bit-equal whatever the chunk width) and a further addend of the
 * query-side gradient, summed in chunk order, then split-K order (no float atomics).
 *   g_rows, g_scalar, g_a [n, dim], g_p [n, rel_dim], g_tgt [num_ent, dim]: as for kge_ce_bwd (f32, OVERWRITTEN).
 *   A label outside [0, num_ent) gives loss_rows[i] = NaN.
 * kge_ce_f32_workspace_bytes(t, n, chunk_cols) (train_1vsAll.py:64-81, loss.py:192-207): chunk_cols = columns per
 * chunk of the backward, a multiple of 128 (>= 128), or 0 = the library's default (a gradient chunk of at most 32 MB,
 * at least 128 columns, clamped to num_ent rounded up to 128); returns more than 0 only for ComplEx / DistMult,
 * KGE_F32 tables, dim % 8 == 0, rel_dim == dim and 16-byte aligned rows (base pointers and row pitches).  The
 * workspace holds the forward's records (12 bytes per row and column group, at most 256 groups), two [n, dim]
 * buffers, at most 8 MB of split-K partials and the [n, chunk] gradient block: 256-byte aligned device scratch, no
 * initialisation, stream-ordered use, not shared by concurrent calls.  The backward derives its chunk width from
 * `workspace_bytes` (any size from chunk_cols = 128 up is valid; below that, and for the forward below its records,
 * KGE_ERR_WORKSPACE).
 * kge_ce_f32_fwd (train_1vsAll.py:64-81, loss.py:192-207: the two loss values of a batch) and
 * kge_ce_f32_bwd (train_1vsAll.py:64-81, loss.py:192-207 under loss_value.backward(): their gradients):
 * other scorers, bf16 tables or another layout: KGE_ERR_UNSUPPORTED, nothing is launched.  No allocation, no host
 * wait, no library call: both are stream-ordered and capturable into a hipGraph. */
int64_t kge_ce_f32_workspace_bytes(const kge_tables* t, int64_t n, int64_t chunk_cols);
int kge_ce_f32_fwd(const kge_tables* t, int dir, kge_index a, kge_index p, kge_index label,
                   int64_t n, float* loss_rows, float* lse, void* workspace,
                   int64_t workspace_bytes, void* stream);
int kge_ce_f32_bwd(const kge_tables* t, int dir, kge_index a, kge_index p, kge_index label,
                   int64_t n, const float* lse, const float* g_rows, float g_scalar, float* g_a,
                   float* g_p, float* g_tgt, void* workspace, int64_t workspace_bytes,
                   void* stream);

/* The same pair with DENSE query rows (a_rows [n, dim], p_rows [n, rel_dim], row-major, bf16) scored
 * against ALL rows of t->ent: the per-shard step of entity-sharded 1vsAll training:
 * the query rows of a batch come out of the exchange between the shards, t->ent is this rank's shard,
 * `label[i]` is the LOCAL row id of row i's true entity or any value outside [0, t->num_ent) (also a
 * NULL vector) if another shard owns it -- loss_rows[i] is then NaN and lse[i] the shard's log-sum-exp;
 * the caller merges the shards' lse and the owner's score and passes the GLOBAL lse to the backward,
 * which returns this shard's part of the query-row gradients (g_a, g_p: summed over the shards by the
 * caller) and the gradient of its own rows (g_tgt).  Workspace as for kge_ce_fwd. */
int kge_ce_emb_fwd(const kge_tables* t, int dir, const void* a_rows, int64_t a_ld, const void* p_rows,
                   int64_t p_ld, kge_index label, int64_t n, float* loss_rows, float* lse,
                   void* workspace, int64_t workspace_bytes, void* stream);
int kge_ce_emb_bwd(const kge_tables* t, int dir, const void* a_rows, int64_t a_ld, const void* p_rows,
                   int64_t p_ld, kge_index label, int64_t n, const float* lse, const float* g_rows,
                   float g_scalar, float* g_a, float* g_p, float* g_tgt, void* workspace,
                   int64_t workspace_bytes, void* stream);

/* KvsAll training over an entity-SHARDED table (BASELINE configs[3]; TrainingJobKvsAll._process_subbatch,
 * kge/job/train_KvsAll.py:216-294, with the entity table row-sharded as SURVEY.md 8e lays out): kge_kl_weighted_fwd /
 * _bwd and kge_bce_fwd / _bwd with DENSE query rows (a_rows [n, dim], p_rows [n, rel_dim]: they come out of the
 * exchange between the shards) against ALL rows of t->ent = this rank's shard, whose rows are the GLOBAL entity ids
 * [col_lo, col_lo + t->num_ent).  lbl_col holds GLOBAL ids: labels outside the shard are skipped (another rank adds
 * them), so that
 *   kl:   loss_rows[i] = lse_shard[i] - w_i * sum_{labels of row i IN this shard} score;  the caller merges the shards'
 *         lse (log-sum-exp) and sums the label terms; the backward takes the GLOBAL lse;
 *   bce:  loss_rows[i] = this shard's part of the sum over all entities: the caller adds the shards' values.
 * Gradients as kge_ce_emb_bwd: g_a / g_p = this shard's part of the query-row gradients, g_tgt = the shard's rows. */
int kge_kl_weighted_emb_fwd(const kge_tables* t, int dir, const void* a_rows, int64_t a_ld, const void* p_rows,
                            int64_t p_ld, int64_t n, const int64_t* lbl_rowptr, const int64_t* lbl_col, int64_t col_lo,
                            const float* label_weight, float* loss_rows, float* lse, void* workspace,
                            int64_t workspace_bytes, void* stream);
int kge_kl_weighted_emb_bwd(const kge_tables* t, int dir, const void* a_rows, int64_t a_ld, const void* p_rows,
                            int64_t p_ld, int64_t n, const int64_t* lbl_rowptr, const int64_t* lbl_col, int64_t col_lo,
                            const float* label_weight, const float* label_bias /* [n] or NULL */, const float* lse,
                            const float* g_rows, float g_scalar, float* g_a, float* g_p, float* g_tgt, void* workspace,
                            int64_t workspace_bytes, void* stream);
int kge_bce_emb_fwd(const kge_tables* t, int dir, const void* a_rows, int64_t a_ld, const void* p_rows, int64_t p_ld,
                    int64_t n, const int64_t* lbl_rowptr, const int64_t* lbl_col, int64_t col_lo, float offset,
                    float* loss_rows, void* workspace, int64_t workspace_bytes, void* stream);
int kge_bce_emb_bwd(const kge_tables* t, int dir, const void* a_rows, int64_t a_ld, const void* p_rows, int64_t p_ld,
                    int64_t n, const int64_t* lbl_rowptr, const int64_t* lbl_col, int64_t col_lo, float offset,
                    const float* g_rows, float g_scalar, float* g_a, float* g_p, float* g_tgt, void* workspace,
                    int64_t workspace_bytes, void* stream);

/* Both directions of a 1vsAll batch at once (train_1vsAll.py:64-81 in one pass): rows [0, n) of
 * loss_rows / lse / g_rows are the (s, p, ?) queries with labels o, rows [n, 2n) the (?, p, o)
 * queries with labels s.  One scoring launch for both sides; the gradient products run once
 * over the 2n rows.  kge_ce_sp_po_bwd: g_a [2n, dim] (rows [0, n): gradient of the s rows,
 * [n, 2n): of the o rows), g_p [2n, rel_dim], g_tgt [num_ent, dim], OVERWRITTEN.  Values equal
 * the two one-sided calls up to f32 summation order (the same scores; the log-sum-exp merges a
 * different split of the columns, the products sum over 2n rows).
 * Workspace: kge_ce_sp_po_workspace_bytes(t, n). */
int64_t kge_ce_sp_po_workspace_bytes(const kge_tables* t, int64_t n);
int kge_ce_sp_po_fwd(const kge_tables* t, kge_index s, kge_index p, kge_index o, int64_t n,
                     float* loss_rows, float* lse, void* workspace, int64_t workspace_bytes,
                     void* stream);
int kge_ce_sp_po_bwd(const kge_tables* t, kge_index s, kge_index p, kge_index o, int64_t n,
                     const float* lse, const float* g_rows, float g_scalar, float* g_a,
                     float* g_p, float* g_tgt, void* workspace, int64_t workspace_bytes,
                     void* stream);

/* kge_ce_sp_po_bwd with the scatter-add of the row gradients done by the library:
 * grad_ent [num_ent, dim] and grad_rel [num_rel, rel_dim] (contiguous f32, OVERWRITTEN) receive the
 * complete gradients of both tables -- what autograd accumulates into `.grad` for the reference
 * (the dense target gradient, plus the gathered s / o rows, plus the gathered relation rows). */
int kge_ce_sp_po_bwd_accum(const kge_tables* t, kge_index s, kge_index p, kge_index o, int64_t n,
                           const float* lse, const float* g_rows, float g_scalar,
                           float* grad_ent, float* grad_rel, void* workspace,
                           int64_t workspace_bytes, void* stream);

/* The batch loss as ONE device scalar, for a training step that is captured into a hipGraph and replayed
 * (kge_amd/train_graph.py): TrainingJob1vsAll sums the rows and divides by the batch size
 * (kge/job/train_1vsAll.py:64-82, kge/util/loss.py:192-207 reduction "sum"), three more launches and as many
 * autograd nodes around the two calls above.  kge_ce_sp_po_fwd_sum: kge_ce_sp_po_fwd, and in the same launches
 *   loss_sum[0] = scale * scale_dev[0] * sum_i loss_rows[i]      (scale_dev == NULL: factor 1; device float)
 * summed in a fixed order (bitwise reproducible).  kge_ce_sp_po_bwd_accum_sum: kge_ce_sp_po_bwd_accum with the
 * SAME gradient for every row, g = scale * g_dev[0] * scale_dev[0] (NULL: factor 1) -- the upstream gradient of
 * loss_sum and the scale as device scalars: nothing of the step is a host value, so a replay follows both.
 * The workspace's control block (its first 33,024 bytes: flags of the cooperative build, the arrival counter of the
 * summing launch) must be ZERO before
 * the first call with a given workspace; every call leaves them zero.  A control block that was never cleared gives a
 * wrong loss_sum on every call. */
int kge_ce_sp_po_fwd_sum(const kge_tables* t, kge_index s, kge_index p, kge_index o, int64_t n,
                         float* loss_rows, float* lse, const float* scale_dev, float scale,
                         float* loss_sum, void* workspace, int64_t workspace_bytes, void* stream);
int kge_ce_sp_po_bwd_accum_sum(const kge_tables* t, kge_index s, kge_index p, kge_index o, int64_t n,
                               const float* lse, const float* g_dev, const float* scale_dev, float scale,
                               float* grad_ent, float* grad_rel, void* workspace,
                               int64_t workspace_bytes, void* stream);

/* KvsAll variant: KL divergence of softmax(score(i, .)) from the row's normalised multi-hot
 * labels, lbl_col[lbl_rowptr[i] .. lbl_rowptr[i+1]) (int64 CSR on the device, entity ids unique
 * per row), y_ij = 1/k_i:
 *   loss_rows[i] = lse[i] - (1/k_i) sum_{j in labels_i} score(i, j) - log k_i     (0 if k_i = 0)
 * = KLDivWithSoftmaxKgeLoss with a label matrix, no label smoothing (kge/util/loss.py:208-213),
 * as TrainingJobKvsAll computes it for sp_ / _po queries (kge/job/train_KvsAll.py:244-294).
 * The label scores use the same operands as the matrix-core kernel (query vector rounded to
 * bf16, exact products, f32 accumulation) in a different f32 summation order.  kge_kl_bwd:
 * gradients of sum_i g_i * loss_rows[i], outputs as kge_ce_bwd.  Same support matrix and
 * workspace as kge_ce_fwd / kge_ce_bwd. */
int kge_kl_fwd(const kge_tables* t, int dir, kge_index a, kge_index p, int64_t n,
               const int64_t* lbl_rowptr, const int64_t* lbl_col, float* loss_rows, float* lse,
               void* workspace, int64_t workspace_bytes, void* stream);
int kge_kl_bwd(const kge_tables* t, int dir, kge_index a, kge_index p, int64_t n,
               const int64_t* lbl_rowptr, const int64_t* lbl_col, const float* lse,
               const float* g_rows, float g_scalar, float* g_a, float* g_p, float* g_tgt,
               void* workspace, int64_t workspace_bytes, void* stream);

/* The pair with a per-row LABEL WEIGHT w_i instead of 1/k_i -- what KvsAll label smoothing
 * (kge/job/train_KvsAll.py:34-49, 262-270: labels = (1 - eps) * labels + 1/E, then normalised) needs
 * from the fused kernels:
 *   loss_rows[i] = lse[i] - w_i * sum_{j in labels_i} score(i, j)              (rows without labels: lse[i])
 *   d / d score(i, j) of sum_i g_i loss_rows[i] = g_i * (softmax_ij - w_i [j in labels_i])
 *   (kge_kl_weighted_bwd with label_bias b != NULL: g_i * (softmax_ij - b_i - w_i [j in labels_i]), i.e. the
 *   gradient of loss_rows[i] - b_i * sum_j score(i, j): the uniform term below, taken inside the kernel)
 * With Z_i = (1 - eps) k_i + 1, a_i = ((1 - eps) + 1/E) / Z_i, b_i = (1/E) / Z_i the smoothed loss of row i is
 *   loss_rows[i] (w_i = a_i - b_i)  -  b_i * sum_j score(i, j)  +  k_i a_i log a_i + (E - k_i) b_i log b_i;
 * the middle term is linear in the entity table (sum_j score(i, j) = score of row i against the table's
 * column sum): kge_amd.model adds it and the constant on the host side of the ABI. */
int kge_kl_weighted_fwd(const kge_tables* t, int dir, kge_index a, kge_index p, int64_t n,
                        const int64_t* lbl_rowptr, const int64_t* lbl_col, const float* label_weight,
                        float* loss_rows, float* lse, void* workspace, int64_t workspace_bytes,
                        void* stream);
int kge_kl_weighted_bwd(const kge_tables* t, int dir, kge_index a, kge_index p, int64_t n,
                        const int64_t* lbl_rowptr, const int64_t* lbl_col, const float* label_weight,
                        const float* label_bias /* [n] or NULL */, const float* lse, const float* g_rows,
                        float g_scalar, float* g_a, float* g_p,
                        float* g_tgt, void* workspace, int64_t workspace_bytes, void* stream);

/* Binary cross entropy with logits against the rows' multi-hot labels (CSR as for kge_kl_fwd), summed
 * over ALL entities:  loss_rows[i] = sum_j BCEWithLogits(score(i, j) + offset, y_ij), y_ij = 1 on
 * the labels = BCEWithLogitsKgeLoss with bce_type None (kge/util/loss.py:137-159; `offset` =
 * train.loss_arg), as TrainingJobKvsAll / TrainingJob1vsAll use it with train.loss: bce.
 * kge_bce_bwd: gradients of sum_i g_i * loss_rows[i] (d/d score = sigmoid(score + offset) - y),
 * outputs as kge_ce_bwd.  Same support matrix and workspace as kge_ce_fwd / kge_ce_bwd. */
int kge_bce_fwd(const kge_tables* t, int dir, kge_index a, kge_index p, int64_t n,
                const int64_t* lbl_rowptr, const int64_t* lbl_col, float offset,
                float* loss_rows, void* workspace, int64_t workspace_bytes, void* stream);
int kge_bce_bwd(const kge_tables* t, int dir, kge_index a, kge_index p, int64_t n,
                const int64_t* lbl_rowptr, const int64_t* lbl_col, float offset,
                const float* g_rows, float g_scalar, float* g_a, float* g_p, float* g_tgt,
                void* workspace, int64_t workspace_bytes, void* stream);

/* ---- the KvsAll losses for the distance scorers on float32 tables ------------- */
/* kge_kl_dist_fwd / _bwd and kge_bce_dist_fwd / _bwd: the losses of kge_kl_fwd / kge_kl_weighted_fwd and kge_bce_fwd
 * above, for TransE and RotatE with l_norm 1 or 2 on float32 tables, without an [n, num_ent] matrix: the step of
 * TrainingJobKvsAll for sp_ / _po queries (kge/job/train_KvsAll.py:216-294) with KLDivWithSoftmaxKgeLoss on a label
 * matrix (kge/util/loss.py:192-213) or BCEWithLogitsKgeLoss with bce_type None (kge/util/loss.py:137-159), built on
 * the kernels of kge_ce_dist_fwd / kge_ce_dist_bwd.
 *   kl, label_weight == NULL:  loss_rows[i] = lse[i] - (1/k_i) sum_{j in labels_i} score(i, j) - log k_i   (0 if k_i = 0)
 *   kl, label_weight [n]:      loss_rows[i] = lse[i] - w_i sum_{j in labels_i} score(i, j)      (k_i = 0: lse[i])
 *   bce:  loss_rows[i] = sum over ALL entities j of max(x, 0) - x y_ij + log1p(exp(-|x|)),  x = score(i, j) + offset
 *   d / d score(i, j) of sum_i g_i loss_rows[i]:  kl  g_i (softmax_ij - w_i [j in labels_i])   (w_i = 1/k_i without a
 *   weight, and then 0 for a row without labels);  bce  g_i (sigmoid(score(i, j) + offset) - [j in labels_i])
 * No label-smoothing bias term (kge_kl_weighted_bwd's label_bias): the uniform term of smoothed labels is not linear
 * in the table for a distance scorer.
 * Labels: lbl_col[lbl_rowptr[i] .. lbl_rowptr[i+1]), an int64 CSR on the device, entity ids unique per row, in ANY
 * order within a row.  A label outside [0, num_ent) gives loss_rows[i] = NaN and leaves the other rows (and lse)
 * untouched; the backward ignores it.  The forward folds every score tile into a per-row running (max, sum exp) (kl)
 * or sum of softplus (bce) and merges the partial results in a fixed order; the label scores are summed in CSR order:
 * no atomics, the same bits on every run.  Every score inside -- the label scores too -- is bit-identical to
 * kge_score_sp / kge_score_po on the same tables.  The backward walks the entity columns in chunks as
 * kge_ce_dist_bwd does; a bit mask of n x chunk bits per chunk (set from the CSR with atomic OR) says which columns
 * are labels.
 *   g_rows, g_scalar, g_a [n, dim], g_p [n, rel_dim], g_tgt [num_ent, dim]: as for kge_ce_dist_bwd (f32, OVERWRITTEN).
 * kge_multilabel_dist_workspace_bytes(t, n, chunk_cols): chunk_cols as for kge_ce_dist_workspace_bytes; returns 0 for
 * tables the calls do not take.  The workspace holds the forward's records (12 bytes per row and column group, at most
 * 256 groups; the backward keeps two floats per row there), an [n, dim] buffer, the [n, chunk] score block and
 * n x chunk / 8 bytes of label bits: 256-byte aligned device scratch, no initialisation, stream-ordered use, not shared
 * by concurrent calls.  The backward derives its chunk width from `workspace_bytes` (any size from chunk_cols = 64 up
 * is valid; below that, and for the forward below its records, KGE_ERR_WORKSPACE) and leaves the label bits all zero.
 * Row count limits as for kge_ce_dist_*.  ComplEx / DistMult, bf16 tables or another l_norm: KGE_ERR_UNSUPPORTED,
 * nothing is launched.  No allocation, no host wait, no library call: all four are stream-ordered and capturable into
 * a hipGraph. */
int64_t kge_multilabel_dist_workspace_bytes(const kge_tables* t, int64_t n, int64_t chunk_cols);
int kge_kl_dist_fwd(const kge_tables* t, int dir, kge_index a, kge_index p, int64_t n,
                    const int64_t* lbl_rowptr, const int64_t* lbl_col,
                    const float* label_weight /* [n] or NULL */, float* loss_rows, float* lse,
                    void* workspace, int64_t workspace_bytes, void* stream);
int kge_kl_dist_bwd(const kge_tables* t, int dir, kge_index a, kge_index p, int64_t n,
                    const int64_t* lbl_rowptr, const int64_t* lbl_col,
                    const float* label_weight /* [n] or NULL */, const float* lse, const float* g_rows,
                    float g_scalar, float* g_a, float* g_p, float* g_tgt, void* workspace,
                    int64_t workspace_bytes, void* stream);
int kge_bce_dist_fwd(const kge_tables* t, int dir, kge_index a, kge_index p, int64_t n,
                     const int64_t* lbl_rowptr, const int64_t* lbl_col, float offset, float* loss_rows,
                     void* workspace, int64_t workspace_bytes, void* stream);
int kge_bce_dist_bwd(const kge_tables* t, int dir, kge_index a, kge_index p, int64_t n,
                     const int64_t* lbl_rowptr, const int64_t* lbl_col, float offset, const float* g_rows,
                     float g_scalar, float* g_a, float* g_p, float* g_tgt, void* workspace,
                     int64_t workspace_bytes, void* stream);

/* ---- the KvsAll losses for ComplEx / DistMult on float32 tables ---------------- */
/* kge_kl_f32_fwd / _bwd and kge_bce_f32_fwd / _bwd: the losses of kge_kl_fwd / kge_kl_weighted_fwd /
 * kge_kl_weighted_bwd and kge_bce_fwd / kge_bce_bwd above, for ComplEx and DistMult (complex.py:30-39,
 * distmult.py:15-21) on float32 tables -- the reference's own precision -- without an [n, num_ent] matrix: the step of
 * TrainingJobKvsAll for sp_ / _po queries (kge/job/train_KvsAll.py:216-294) with KLDivWithSoftmaxKgeLoss on a label
 * matrix (kge/util/loss.py:192-213) or BCEWithLogitsKgeLoss with bce_type None (kge/util/loss.py:137-159), built on
 * the kernels of kge_ce_f32_fwd / kge_ce_f32_bwd and the label machinery of kge_kl_dist_*.
 *   kl, label_weight == NULL:  loss_rows[i] = lse[i] - (1/k_i) sum_{j in labels_i} score(i, j) - log k_i   (0 if k_i = 0)
 *   kl, label_weight [n]:      loss_rows[i] = lse[i] - w_i sum_{j in labels_i} score(i, j)      (k_i = 0: lse[i])
 *   bce:  loss_rows[i] = sum over ALL entities j of max(x, 0) - x y_ij + log1p(exp(-|x|)),  x = score(i, j) + offset
 *   d / d score(i, j) of sum_i g_i loss_rows[i]:  kl  g_i (softmax_ij - b_i - w_i [j in labels_i])   (w_i = 1/k_i
 *   without a weight, and then g_i = 0 for a row without labels; b_i = label_bias[i], 0 for label_bias == NULL: the
 *   uniform term of smoothed labels as for kge_kl_weighted_bwd -- these scores are linear in the target row, so
 *   KvsAll label smoothing (train_KvsAll.py:34-49, 262-270) stays on this path);
 *   bce  g_i (sigmoid(score(i, j) + offset) - [j in labels_i])
 * Labels: lbl_col[lbl_rowptr[i] .. lbl_rowptr[i+1]), an int64 CSR on the device, entity ids unique per row, in ANY
 * order within a row.  A label outside [0, num_ent) gives loss_rows[i] = NaN and leaves the other rows (and lse)
 * untouched; the backward ignores it.  The forward is the exact f32 matrix-core scoring kernel with a fold epilogue
 * (kl: a per-row running (max, sum exp); bce: a sum of softplus): every score of the dense part is bit-identical to
 * kge_score_sp / kge_score_po, the partial results are merged in a fixed order, and lse is BIT-EQUAL to
 * kge_ce_f32_fwd's on the same tables and queries.  The label scores are f32 dot products of the query vector (the
 * Q of kge_score_pairs_bwd) with the label's row: the same operands as the matrix-core kernel in a different f32
 * summation order; they are summed in CSR order.  No float atomics: the same bits on every run.  The backward walks
 * the entity columns in chunks as kge_ce_f32_bwd does (g_tgt OVERWRITTEN, bit-equal whatever the chunk width; the
 * query-side gradient summed in chunk order, then split-K order); a bit mask of n x chunk bits per chunk (set from the
 * CSR with atomic OR) says which columns are labels.
 *   g_rows, g_scalar, g_a [n, dim], g_p [n, rel_dim], g_tgt [num_ent, dim]: as for kge_ce_f32_bwd (f32, OVERWRITTEN;
 *   n = 0: g_tgt is zero-filled).
 * kge_multilabel_f32_workspace_bytes(t, n, chunk_cols) (train_KvsAll.py:216-294): chunk_cols and the support matrix as
 * for kge_ce_f32_workspace_bytes (ComplEx / DistMult, KGE_F32, dim % 8 == 0, rel_dim == dim, 16-byte aligned rows;
 * otherwise 0).  The workspace is kge_ce_f32's layout -- records | [n, dim] | [n, dim] (the query matrix Q) | split-K
 * partials | the [n, chunk] gradient block -- plus n x chunk / 8 bytes of label bits, each part rounded up to 256
 * bytes: 256-byte aligned device scratch, no initialisation, stream-ordered use, not shared by concurrent calls.  The
 * FORWARD needs the records and the two [n, dim] buffers (it writes Q where the backward keeps it):
 *   align256(12 n G) + 2 align256(4 n dim),  G = the column groups of kge_ce_f32_fwd (at most 256);
 * the BACKWARD derives its chunk width from `workspace_bytes` and needs at least
 *   kge_multilabel_f32_workspace_bytes(t, n, 128);
 * below these, KGE_ERR_WORKSPACE.  The backward leaves the label bits all zero.
 * kge_kl_f32_fwd (train_KvsAll.py:274-294, loss.py:192-213: the kl loss values of a query type),
 * kge_bce_f32_fwd (train_KvsAll.py:274-294, loss.py:137-159: the bce loss values of a query type),
 * kge_kl_f32_bwd (train_KvsAll.py:274-294, loss.py:192-213 under loss_value.backward(): their gradients) and
 * kge_bce_f32_bwd (train_KvsAll.py:274-294, loss.py:137-159 under loss_value.backward()): other scorers, bf16 tables
 * or another layout: KGE_ERR_UNSUPPORTED, nothing is launched.  No allocation, no host wait, no library call, no float
 * atomics: all four are stream-ordered and capturable into a hipGraph. */
int64_t kge_multilabel_f32_workspace_bytes(const kge_tables* t, int64_t n, int64_t chunk_cols);
int kge_kl_f32_fwd(const kge_tables* t, int dir, kge_index a, kge_index p, int64_t n,
                   const int64_t* lbl_rowptr, const int64_t* lbl_col,
                   const float* label_weight /* [n] or NULL */, float* loss_rows, float* lse,
                   void* workspace, int64_t workspace_bytes, void* stream);
int kge_kl_f32_bwd(const kge_tables* t, int dir, kge_index a, kge_index p, int64_t n,
                   const int64_t* lbl_rowptr, const int64_t* lbl_col,
                   const float* label_weight /* [n] or NULL */, const float* label_bias /* [n] or NULL */,
                   const float* lse, const float* g_rows, float g_scalar, float* g_a, float* g_p,
                   float* g_tgt, void* workspace, int64_t workspace_bytes, void* stream);
int kge_bce_f32_fwd(const kge_tables* t, int dir, kge_index a, kge_index p, int64_t n,
                    const int64_t* lbl_rowptr, const int64_t* lbl_col, float offset, float* loss_rows,
                    void* workspace, int64_t workspace_bytes, void* stream);
int kge_bce_f32_bwd(const kge_tables* t, int dir, kge_index a, kge_index p, int64_t n,
                    const int64_t* lbl_rowptr, const int64_t* lbl_col, float offset, const float* g_rows,
                    float g_scalar, float* g_a, float* g_p, float* g_tgt, void* workspace,
                    int64_t workspace_bytes, void* stream);

/* Both query types of a KvsAll batch, backward, with COMPLETE table gradients.  TrainingJobKvsAll scores the sp_ and
 * the _po queries of a batch one after the other and back-propagates each loss on its own
 * (kge/job/train_KvsAll.py:274-294): two d loss / d score passes, four gradient products, and autograd's index_add and
 * accumulation passes over the [num_ent, dim] gradient between them.  Here each type's pass (that of kge_kl_bwd /
 * kge_bce_bwd, no label smoothing) fills its rows of one gradient matrix and the two products run once over the
 * n_sp + n_po rows: grad_ent [num_ent, dim] and grad_rel [num_rel, rel_dim] (contiguous f32, OVERWRITTEN) receive what
 * `.grad` holds after the reference's two backward calls -- the dense target gradient of both types plus the
 * gathered entity and relation rows' gradients (float atomics: equal up to their order).
 *   sp: a = subjects, p = relations of the sp_ queries; po: a = OBJECTS, p = relations of the _po queries;
 *   lse: kge_kl_fwd's (KGE_LOSS_KL; unused for KGE_LOSS_BCE); g_rows / g_scalar / g_dev: upstream gradient of loss_rows;
 *   offset: kge_bce_fwd's (KGE_LOSS_BCE).  Either side may be empty (n = 0).
 * Workspace: kge_multilabel2_workspace_bytes(t, n_sp, n_po) (0: unsupported tables), 256-byte aligned, zeroed once. */
#define KGE_LOSS_KL 0
#define KGE_LOSS_BCE 1
typedef struct kge_label_queries {
  kge_index a, p;
  int64_t n;
  const int64_t* lbl_rowptr;   /* [n + 1] */
  const int64_t* lbl_col;
  const float* lse;            /* [n] or NULL (bce) */
  const float* g_rows;         /* [n] or NULL: g_scalar (x g_dev[0]) for every row */
  float g_scalar;
  const float* g_dev;          /* [1] device float or NULL: the upstream gradient of a SUMMED loss (a captured step
                                * holds no host value: kge_ce_sp_po_bwd_accum_sum) */
} kge_label_queries;
int64_t kge_multilabel2_workspace_bytes(const kge_tables* t, int64_t n_sp, int64_t n_po);
int kge_multilabel2_bwd_accum(const kge_tables* t, int loss, float offset, const kge_label_queries* sp,
                              const kge_label_queries* po, float* grad_ent, float* grad_rel,
                              void* workspace, int64_t workspace_bytes, void* stream);

/* ---- optimizer step over a table ---------------------- */
/* One dense Adagrad step on `count` contiguous f32 elements (16-byte aligned arrays), in place:
 *   g = grad + weight_decay * param (if weight_decay != 0);  state_sum += g*g;
 *   param += (minus_clr * g) / (sqrt(state_sum) + eps)
 * with minus_clr = -lr / (1 + (step - 1) * lr_decay): torch.optim.Adagrad's update
 * (the optimizer LibKGE creates by default, kge/util/optimizer.py:15-20; config-default.yaml
 * train.optimizer), one pass instead of five element-wise kernels.  bf16_copy != NULL: also
 * writes RNE(param) there (8-byte aligned) -- the table copies the bf16 scoring kernels read. */
int kge_adagrad_step(float* param, const float* grad, float* state_sum, int64_t count,
                     float minus_clr, float weight_decay, float eps, void* bf16_copy,
                     void* stream);

/* kge_adagrad_step on up to KGE_ADAGRAD_MAX_SEGS tables in ONE launch (the entity and the relation table of a
 * training step; kge/job/train.py:471-474 optimizer.step() over all parameters): the same arithmetic per
 * element, one launch latency instead of one per parameter. */
#define KGE_ADAGRAD_MAX_SEGS 8
typedef struct kge_adagrad_seg {
  float* param;
  const float* grad;
  float* state_sum;
  void* bf16_copy;      /* or NULL */
  int64_t count;
  float minus_clr, weight_decay, eps;
} kge_adagrad_seg;
int kge_adagrad_step_multi(const kge_adagrad_seg* segs, int num_segs, void* stream);

/* kge_adagrad_step_multi with the embedders' UNWEIGHTED penalty terms folded into the pass
 * (LookupEmbedder.penalty, kge/model/embedder/lookup_embedder.py:122-147, back-propagated by TrainingJob.run_epoch
 * between the batch and optimizer.step(), kge/job/train.py:417-436): segment j adds the gradient of
 *   kind 1 (regularize lp):          weight / p * sum |x|^p             (p = 1, 2, 3)   -> weight * sign(x) |x|^(p-1)
 *   kind 2 (regularize n3, complex): weight / 3 * sum |z|^3, |z| = sqrt(re^2 + im^2 + 1e-14), im = col + row_dim / 2
 * to grad before the update (grad itself is not written), and adds sum |x|^p (sum |z|^3) of the PRE-step parameters
 * to *value (a device double the caller zeroed; the term the reference's trace shows is weight / p times it).
 * `weight` is the gradient's factor: regularize_weight, doubled for an entity embedder shared by the subject and
 * object slot (kge_model.py:620-625).  kind 0: the plain step.  kind 2 needs count % row_dim == 0 and
 * row_dim % 8 == 0.  pens == NULL: kge_adagrad_step_multi. */
typedef struct kge_penalty_seg {
  int32_t kind, p;
  float weight;
  int64_t row_dim;
  double* value;        /* [1] device, or NULL for kind 0 */
} kge_penalty_seg;
int kge_adagrad_step_multi_penalty(const kge_adagrad_seg* segs, const kge_penalty_seg* pens, int num_segs,
                                   void* stream);

/* One dense Adam step (torch.optim.Adam, amsgrad / maximize off) on `count` contiguous f32 elements,
 * in place, one pass:  g = grad + weight_decay * param (if != 0);  exp_avg += (g - exp_avg)(1 - beta1);
 * exp_avg_sq = exp_avg_sq * beta2 + (1 - beta2) g g;
 * param -= step_size * exp_avg / (sqrt(exp_avg_sq) / bias_correction2_sqrt + eps),
 * step_size = lr / (1 - beta1^t), bias_correction2_sqrt = sqrt(1 - beta2^t) computed by the caller
 * (kge/util/optimizer.py:15-20 with train.optimizer.default.type: Adam).  bf16_copy as above. */
int kge_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t count,
                  float step_size, float bias_correction2_sqrt, double beta1, double beta2,
                  float weight_decay, float eps, void* bf16_copy, void* stream);

/* kge_adam_step on up to KGE_ADAM_MAX_SEGS tables in ONE launch, with the step count kept on the device
 * (kge/job/train.py:471-474 optimizer.step() over all parameters; kge/util/optimizer.py:15-20 with
 * train.optimizer.default.type: Adam).  kge_adam_step takes lr / (1 - beta1^t) and sqrt(1 - beta2^t) from the host: a
 * captured step would replay the values of the capture step for ever.  Here every parameter has a clock record in
 * device memory; a one-workgroup kernel in front of the update advances the records of the call's non-empty segments,
 * in float64 with IEEE division and square root:
 *   t += 1;  beta1_pow *= beta1;  beta2_pow *= beta2;
 *   step_size = (float)(lr / (1 - beta1_pow));  bias_correction2_sqrt = (float)sqrt(1 - beta2_pow)
 * and the update reads the two floats of its segment's record; per element it is kge_adam_step's arithmetic, operation
 * for operation (the same bits, given the same two floats).  A fresh record is {T, beta1^T, beta2^T, 0, 0}, written by
 * the caller: T = 0 at the start, T = the restored step count after a checkpoint was loaded.  lr and the betas are
 * launch arguments: a caller that replays a captured call must capture again when they change.
 *
 * pens != NULL: the embedders' penalty terms folded into the pass as in kge_adagrad_step_multi_penalty -- the term's
 * gradient is added to grad (in registers; grad is not written) before weight decay and the moments, and sum |x|^p
 * (sum |z|^3) of the PRE-step parameters is added to *value.  A segment of kind 0 is the plain update.
 *
 * KGE_ERR_INVALID_ARG: num_segs outside 0..KGE_ADAM_MAX_SEGS; count < 0; a NULL (non-empty segment) or not 16-byte
 * aligned param, grad, exp_avg or exp_avg_sq; a bf16_copy that is not 8-byte aligned; a NULL (non-empty segment) or not
 * 8-byte aligned clock; two non-empty segments with the same clock; beta1 or beta2 outside [0, 1); a penalty kind
 * other than 0, 1, 2; kind != 0 with a NULL or misaligned value; kind 2 with count % row_dim != 0 or row_dim % 8 != 0.
 * KGE_ERR_UNSUPPORTED: kind 1 with p outside 1..3; more than 2^31 - 1 workgroups.  num_segs == 0, or every segment
 * empty: KGE_OK, no launch, no clock advances.  An empty segment among non-empty ones: its clock does not advance. */
#define KGE_ADAM_MAX_SEGS 8
typedef struct kge_adam_clock {
  int64_t t;
  double beta1_pow, beta2_pow;
  float step_size, bias_correction2_sqrt;
} kge_adam_clock;
typedef struct kge_adam_seg {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  void* bf16_copy;            /* or NULL */
  kge_adam_clock* clock;      /* device */
  int64_t count;
  double lr, beta1, beta2;
  float weight_decay, eps;
} kge_adam_seg;
int kge_adam_step_multi(const kge_adam_seg* segs, const kge_penalty_seg* pens /* or NULL */, int num_segs,
                        void* stream);

/* Row-sparse Adagrad step: only the `num_rows` listed rows (unique ids, int64) of a [*, dim] table
 * have a gradient, grad_rows[r, :] belonging to row rows[r] -- torch.optim.Adagrad's update for the
 * sparse gradients of lookup_embedder.sparse: True (kge/model/embedder/lookup_embedder.yaml:78-81):
 *   state_sum[row] += g*g;  param[row] += minus_clr * g / (sqrt(state_sum[row]) + eps).
 * Untouched rows are neither read nor written.  bf16_copy: the same rows of the bf16 table copy. */
int kge_adagrad_step_rows(float* param, int64_t param_ld, const float* grad_rows, int64_t grad_ld,
                          float* state_sum, int64_t sum_ld, const int64_t* rows, int64_t num_rows,
                          int64_t dim, float minus_clr, float eps, void* bf16_copy, int64_t copy_ld,
                          void* stream);

/* ---- Adagrad over the rows a batch touched (csrc/touched.hip) --------------------------------
 * The step of TrainingJob.run_epoch (kge/job/train.py:452-474: zero_grad, backward, optimizer.step) without a pass over
 * the whole table: the backward accumulates into a PERSISTENT dense gradient buffer and marks the rows it adds to in a
 * bitmap; the step visits the marked rows only, and leaves buffer and bitmap zero for the next batch.  The row-wise
 * update of kge/model/embedder/lookup_embedder.yaml:78-81 (`sparse: True`) needs a coalesced sparse gradient, which
 * the fused backward kernels never produce; this one needs a bit per row.
 *
 * Bytes of the bitmap of a table of num_rows rows: 4 * ceil(num_rows / 32), rounded up to 16.  Bit r % 32 of the
 * 32-bit word r / 32 means that row r has a gradient.  (train.py:452-474, lookup_embedder.yaml:78-81) */
int64_t kge_touched_bitmap_bytes(int64_t num_rows);

/* Sets the bit of every id of an [n, k] block: element (i, j) is ids.ptr[(i * ld + j) * ids.stride], int32 or int64
 * (k = 1, ld = 1: a plain index vector, e.g. the stride-3 triples[:, 0]).  Ordinary global atomic OR: duplicates are
 * fine, calls on one bitmap may follow each other in any order.  An id outside [0, num_rows) sets nothing.  Nothing is
 * read on the host (capturable); n * k == 0: KGE_OK without a launch.  What is marked is what the backward of
 * train.py:452-474 would give a gradient row under lookup_embedder.yaml:78-81's sparse embeddings.
 * KGE_ERR_INVALID_ARG: n, k or num_rows < 0, ld < k, a NULL bitmap or ids.ptr (n * k > 0), an ids.itype other than
 * int32 / int64, ids.stride < 1, ids.start != 0. */
int kge_touched_mark(kge_index ids, int64_t n, int64_t k, int64_t ld, int64_t num_rows, uint32_t* bitmap,
                     void* stream);

/* For every set bit r of `bitmap` (bits of rows >= num_rows are ignored) the arithmetic of kge_adagrad_step_multi with
 * weight_decay == 0 on row r, operation for operation:
 *   state_sum[r] += g*g;  param[r] = param[r] + (minus_clr * g) / (sqrt(state_sum[r]) + eps);  bf16_copy[r] = bf16(param[r])
 * then zeros are stored over grad[r, 0:dim] and, once all rows of a word are done, over the word.  On return the
 * bitmap is all zero, and grad is all zero provided it was zero outside the marked rows on entry.  Rows whose bit is
 * clear are neither read nor written, in any of the four arrays.  A dense Adagrad step (train.py:452-474 with
 * torch.optim.Adagrad) leaves a row whose gradient is zero bit for bit as it was, so this is that step; there is no
 * weight decay here because it would move untouched rows (lookup_embedder.yaml:78-81's sparse route has none either).
 * Every shape is taken: four floats per lane when dim % 4 == 0, param, grad and state_sum are 16-byte aligned with
 * pitches % 4 == 0 (and bf16_copy, if given, 8-byte aligned with copy_ld % 4 == 0), one float per lane otherwise.
 * KGE_ERR_INVALID_ARG: num_rows or dim < 0, dim > 2^31 - 1, a pitch < dim, a NULL param, grad, state_sum or bitmap
 * (num_rows > 0).  KGE_ERR_UNSUPPORTED: more than 2^31 - 1 workgroups (256 rows each). */
int kge_adagrad_step_touched(float* param, int64_t param_ld, float* grad, int64_t grad_ld, float* state_sum,
                             int64_t sum_ld, uint32_t* bitmap, int64_t num_rows, int64_t dim, float minus_clr,
                             float eps, void* bf16_copy, int64_t copy_ld, void* stream);

/* ---- SparseAdam over the rows a batch touched (csrc/touched.hip) -------------------------------
 * torch.optim.SparseAdam (kge/util/optimizer.py:15-20 with train.optimizer.default.type: SparseAdam and
 * lookup_embedder.yaml:78-81 `sparse: True`) on the rows whose bit is set in `bitmap` (kge_touched_mark; bits of rows
 * >= num_rows are ignored): the bitmap stands for the index set of the coalesced sparse gradient, the persistent dense
 * `grad` for its values.  A dense Adam step cannot be cut down to these rows -- its momentum moves rows that have no
 * gradient --; SparseAdam is DEFINED row-wise, so this is that optimizer.
 *
 * The clock.  `clock` is the parameter's kge_adam_clock record, the layout of kge_adam_step_multi.  A one-workgroup
 * kernel in front of the update advances it, in float64 with IEEE division and square root:
 *   t += 1;  beta1_pow *= beta1;  beta2_pow *= beta2;  root = sqrt(1 - beta2_pow)
 *   step_size = (float)((lr * root) / (1 - beta1_pow));  bias_correction2_sqrt = (float)root
 * For THIS entry the record's first float is SparseAdam's whole step size lr * sqrt(1 - beta2^t) / (1 - beta1^t) --
 * not Adam's lr / (1 - beta1^t) --, and the second float, sqrt(1 - beta2^t), is written for the record's readers but
 * not read by the update: SparseAdam's denominator is sqrt(exp_avg_sq) + eps, without the bias correction inside.  A
 * record must not be shared between this entry and kge_adam_step_multi.  A fresh record is {T, beta1^T, beta2^T, 0, 0}.
 * The clock advances ONCE PER CALL, whether or not any bit is set and also when num_rows == 0 (torch counts a step for
 * every step() call in which the parameter has a gradient, an empty one included); a call that returns an error
 * advances nothing.  The caller must NOT call this entry for a parameter torch would skip (`grad is None`: a step in
 * which no backward ran for the table), or the step counts part.
 *
 * The update.  For every set bit r < num_rows and every column of row r, in float32, every operation rounded on its
 * own (no fused multiply-add anywhere), with omb1 = (float)(1 - beta1), omb2 = (float)(1 - beta2) formed in double
 * and rounded once, g = grad[r], m = exp_avg[r], v = exp_avg_sq[r], p = param[r] -- torch's functional sparse_adam,
 * operation for operation:
 *   u1 = (g - m) * omb1             (grad_values.sub(old_exp_avg_values).mul_(1 - beta1))
 *   m  = m + u1                     (exp_avg.add_(...); the same bits as numer = u1 + m)
 *   u2 = (g * g - v) * omb2         (grad_values.pow(2).sub_(old_exp_avg_sq_values).mul_(1 - beta2))
 *   v  = v + u2                     (exp_avg_sq.add_(...); the same bits as u2 + v under the square root)
 *   d  = sqrt(v) + eps              (IEEE square root)
 *   p  = p + (-step_size) * (m / d) (IEEE division; the quotient, then the product, then the sum)
 * then bf16_copy[r] = bf16(p) (RNE) if a copy was given, zeros are stored over grad[r, 0:dim] and, once all rows of a
 * word are done, over the word.  On return the bitmap is all zero, and grad is all zero provided it was zero outside
 * the marked rows on entry.  Rows whose bit is clear are neither read nor written, in any of the five arrays.  A
 * marked row whose gradient is exactly zero STILL decays its moments and moves (m = m - m * omb1 ...): that is what
 * torch does with a row present in the sparse gradient, and what separates this from the Adagrad entry above.
 * Every shape is taken: four floats per lane when dim % 4 == 0, param, grad, exp_avg and exp_avg_sq are 16-byte
 * aligned with pitches % 4 == 0 (and bf16_copy, if given, 8-byte aligned with copy_ld % 4 == 0), one float per lane
 * otherwise.
 * KGE_ERR_INVALID_ARG: num_rows or dim < 0, dim > 2^31 - 1, a pitch < dim, a NULL param, grad, exp_avg, exp_avg_sq or
 * bitmap (num_rows > 0), a NULL or not 8-byte aligned clock (whatever num_rows), beta1 or beta2 outside [0, 1).
 * KGE_ERR_UNSUPPORTED: more than 2^31 - 1 workgroups (256 rows each); checked before the clock.
 * num_rows == 0: KGE_OK; the clock kernel is the one launch. */
int kge_sparse_adam_step_touched(float* param, int64_t param_ld, float* grad, int64_t grad_ld, float* exp_avg,
                                 int64_t avg_ld, float* exp_avg_sq, int64_t sq_ld, uint32_t* bitmap, int64_t num_rows,
                                 int64_t dim, kge_adam_clock* clock, double lr, double beta1, double beta2, float eps,
                                 void* bf16_copy, int64_t copy_ld, void* stream);

/* ---- frequency-weighted penalties in the optimizer's pass (csrc/wpenalty.hip) -----------------
 * LookupEmbedder.penalty with regularize_args.weighted: true (kge/model/embedder/lookup_embedder.py:148-173,
 * lookup_embedder.yaml `regularize_args.weighted`), called with the batch's indexes (kge_model.py:607-634).  With
 * m = len(indexes) and c_r = the occurrences of row r among them the term is
 *   weight / p / m * sum_r c_r * sum_j |x_rj|^p        (n3, complex: |z|^3, |z| = sqrt(re^2 + im^2 + 1e-14))
 * and its gradient (weight * c_r / m) * sign(x) |x|^(p-1)  (n3: (weight * c_r / m) * |z| * re, ... * im): a function of
 * the element and its row's count.  kge_penalty_count builds the counts on the device; the four entries below are the
 * existing updates with the term's gradient added in registers, the row factor being
 *   f_r = weight * ((float)counts[r] / (float)m)      -- one IEEE float32 division, then one float32 product
 * (counts[r] == m gives f_r == weight exactly).  A row whose count is 0 gets no penalty gradient -- nothing is added to
 * its gradient -- and adds nothing to the value.
 *
 * Index block of kge_penalty_count: as kge_touched_mark -- element (i, j) of an [n, k] block is
 * ids.ptr[(i * ld + j) * ids.stride], int32 or int64 (triples[:, 1]: k = 1, ld = 1, stride 3; two neighbouring columns of
 * an [n, 3] matrix: k = 2, ld = 3, stride 1; the S and the O column of [n, 3] triples are not such a block: two calls
 * on one count buffer, which is what a count of the concatenated vector is).  counts[id] += 1 per
 * occurrence by integer atomic add (exact, order-free: the same counts on every run); bitmap != NULL: the row's bit of
 * a touched-row bitmap is set as well.  An id outside [0, num_rows) does nothing.  Nothing is read on the host
 * (capturable); n * k == 0: KGE_OK without a launch.
 * KGE_ERR_INVALID_ARG: n, k or num_rows < 0, ld < k, a NULL or not 4-byte aligned counts, a NULL ids.ptr (n * k > 0), an
 * ids.itype other than int32 / int64, ids.stride < 1, ids.start != 0. */
int kge_penalty_count(kge_index ids, int64_t n, int64_t k, int64_t ld, int64_t num_rows, uint32_t* counts,
                      uint32_t* bitmap /* or NULL */, void* stream);

/* The weighted term of one table.  kind, p, row_dim: as kge_penalty_seg (0: none; 1: lp with p in 1..3; 2: n3 on a
 * complex space, row_dim % 8 == 0), but row_dim is needed for every kind != 0: it is what makes rows of the elements.
 * `weight`: regularize_weight, NOT doubled for a shared entity embedder (kge_model.py:612-621 passes the subject and
 * object indexes as one [n, 2] tensor).  `counts`: [num_rows] device words (kge_penalty_count), `m` = len(indexes) as
 * the reference divides by it (lookup_embedder.py:171): n for triples[:, P] and ALSO n for the [n, 2] entity block,
 * whose 2n entries are counted -- so a count may reach 2m.  A count of 2^24 or more (possible only with m >= 2^23
 * under two-column counting) is rounded to nearest even by (float)counts[r]: f_r then carries a third rounding.  *value (a device double the caller zeroed) receives
 *   sum_r counts[r] * sum_j |x_rj|^p    (n3: |z|^3)
 * of the PRE-step parameters: |x|^p per element in float32, the product with the count and every sum in float64; the
 * term the reference's trace shows is weight / p / m times it.
 * Clearing: the kernel stores zero over every count word it has read.  The dense entries read all num_rows words; the
 * touched-row entries the words of the marked rows -- `counts` must be zero outside the marked rows on entry, as the
 * gradient buffer must (kge_penalty_count given the bitmap marks what it counts).  Either way the buffer is all zero
 * after the step, ready for the next batch's counts. */
typedef struct kge_wpenalty_seg {
  int32_t kind, p;
  float weight;
  int64_t row_dim;
  double* value;          /* [1] device, or NULL for kind 0 */
  const uint32_t* counts; /* [count / row_dim] device (cleared by the step), or NULL for kind 0 */
  int64_t m;
} kge_wpenalty_seg;

/* kge_adagrad_step_multi_penalty (train.py:417-436: the term is back-propagated between the batch and
 * optimizer.step()) with weighted terms: per element exactly that entry's arithmetic with `weight` replaced by f_r of
 * the element's row.  Argument checks: those of kge_adagrad_step_multi_penalty, and for kind != 0
 * KGE_ERR_INVALID_ARG for row_dim <= 0, count % row_dim != 0, a NULL or not 4-byte aligned counts, m <= 0, a NULL pens;
 * KGE_ERR_UNSUPPORTED for m >= 2^24 (the float32 quotient's operands must be exact), row_dim > 2^28. */
int kge_adagrad_step_multi_wpenalty(const kge_adagrad_seg* segs, const kge_wpenalty_seg* pens, int num_segs,
                                    void* stream);

/* kge_adam_step_multi (device clock; optimizer.py:15-20 with train.optimizer.default.type: Adam) with weighted terms:
 * the PEN path's arithmetic with `weight` replaced by f_r.  Argument checks: those of kge_adam_step_multi, and the
 * weighted record's as above (pens must not be NULL).  Clocks advance as there. */
int kge_adam_step_multi_wpenalty(const kge_adam_seg* segs, const kge_wpenalty_seg* pens, int num_segs, void* stream);

/* kge_adagrad_step_touched (lookup_embedder.yaml:78-81's row-wise update) with g + f_r * ... in registers on the marked
 * rows, both on the four-floats-per-lane and on the scalar path.  The same clearing contract for grad and bitmap, and
 * the counts of the marked rows are cleared; rows whose bit is clear are neither read nor written, their count word
 * included.  pen->row_dim must equal dim.  Argument checks: those of kge_adagrad_step_touched, the weighted record's as
 * above, KGE_ERR_INVALID_ARG for a NULL pen or row_dim != dim (kind != 0). */
int kge_adagrad_step_touched_wpenalty(float* param, int64_t param_ld, float* grad, int64_t grad_ld, float* state_sum,
                                      int64_t sum_ld, uint32_t* bitmap, int64_t num_rows, int64_t dim, float minus_clr,
                                      float eps, void* bf16_copy, int64_t copy_ld, const kge_wpenalty_seg* pen,
                                      void* stream);

/* kge_sparse_adam_step_touched (optimizer.py:15-20 with type: SparseAdam) with g + f_r * ... in registers on the marked
 * rows; the clock, the clearing contract and the argument checks of that entry plus those of
 * kge_adagrad_step_touched_wpenalty. */
int kge_sparse_adam_step_touched_wpenalty(float* param, int64_t param_ld, float* grad, int64_t grad_ld, float* exp_avg,
                                          int64_t avg_ld, float* exp_avg_sq, int64_t sq_ld, uint32_t* bitmap,
                                          int64_t num_rows, int64_t dim, kge_adam_clock* clock, double lr, double beta1,
                                          double beta2, float eps, void* bf16_copy, int64_t copy_ld,
                                          const kge_wpenalty_seg* pen, void* stream);

/* ---- backward (autograd twins) ------------------------------------------ */
/* All gradients are f32 and OVERWRITTEN; tables/embeddings must be f32, except
 * kge_score_pairs_bwd for ComplEx/DistMult, which also takes bf16 tables (mixed-precision
 * training: gout rounded to bf16, both products on the bf16 matrix cores, f32 accumulation)
 * and then needs `workspace_bytes >= kge_score_bwd_workspace_bytes(t, n, m)` of 256-byte
 * aligned device scratch (0 / NULL for f32 tables).
 * `scores` is the forward output (needed by TransE/RotatE with l_norm != 1 to
 * recover the distance; may be NULL otherwise).
 *
 * kge_score_pairs_bwd: gradients of sum_ij gout[i,j]*score(i,j) for
 * kge_score_sp / kge_score_po (dir = KGE_SP_ / KGE_PO_):
 *   g_a   [n, dim]      grad of the gathered entity query rows (s for SP_, o for PO_)
 *   g_p   [n, rel_dim]  grad of the gathered relation rows
 *   g_tgt [m, dim]      grad of the target rows (dense; caller scatter-adds)
 * An empty side leaves zeros on the other: n == 0 writes g_tgt = 0, m == 0 writes g_a = g_p = 0. */
int64_t kge_score_bwd_workspace_bytes(const kge_tables* t, int64_t n, int64_t m);
int kge_score_pairs_bwd(const kge_tables* t, int dir, kge_index a, kge_index p,
                        int64_t n, kge_index targets, int64_t m,
                        const float* gout, int64_t ldg, const float* scores,
                        int64_t lds, float* g_a, float* g_p, float* g_tgt,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* Gradients of sum_i gout[i]*score(s_i,p_i,o_i): g_s,g_o [n,dim], g_p [n,rel_dim]. */
int kge_score_spo_bwd(const kge_tables* t, kge_index s, kge_index p,
                      kge_index o, int64_t n, const float* gout,
                      const float* scores, float* g_s, float* g_p, float* g_o,
                      void* stream);

/* The same gradients ACCUMULATED (float atomics) into dense table gradients grad_ent [num_ent,
 * dim] and grad_rel [num_rel, rel_dim] (caller zeroes or pre-loads them): what autograd's
 * scatter-add of the gathered rows produces, without the three [n, dim] row-gradient tensors.
 * Runs of equal s / p indices (negative sampling: n*K triples, s and p repeated K times in a
 * row, kge/util/sampler.py:291-306) are summed in registers first.  dim <= 1024. */
int kge_score_spo_bwd_accum(const kge_tables* t, kge_index s, kge_index p, kge_index o,
                            int64_t n, const float* gout, const float* scores,
                            float* grad_ent, int64_t grad_ent_ld, float* grad_rel,
                            int64_t grad_rel_ld, void* stream);

/* Backward of kge_score_neg (replaces autograd through BatchNegativeSample.score,
 * kge/util/sampler.py:263-306, called at kge/job/train_negative_sampling.py:142-163): gradients
 * of sum_{i,k} gout[i*ldg + k] * score(triple i with `slot` replaced by neg[i*neg_ld + k])
 * ACCUMULATED into the dense table gradients like kge_score_spo_bwd_accum.  The relation row and
 * the uncorrupted entity row of a positive are read once and their gradients summed in registers
 * over a chunk of clamp(n * num_neg / 8192, 4, 64) negatives; only the corrupted rows stream.  `scores` = the forward output [n, num_neg]
 * (row pitch lds; needed for TransE / RotatE with l_norm != 1, may be NULL otherwise).
 * f32 tables, dim <= 1024. */
int kge_score_neg_bwd_accum(const kge_tables* t, kge_index s, kge_index p, kge_index o,
                            int64_t n, int slot, const void* neg, int32_t neg_itype,
                            int64_t neg_ld, int64_t num_neg, const float* gout, int64_t ldg,
                            const float* scores, int64_t lds, float* grad_ent,
                            int64_t grad_ent_ld, float* grad_rel, int64_t grad_rel_ld,
                            void* stream);

/* ---- Embedder dropout inside the triple-wise kernels -----------------------------------------------------------------
 * LookupEmbedder._postprocess applies torch.nn.Dropout to every gathered row (kge/model/embedder/
 * lookup_embedder.py:96-105).  The entries below compute that mask inside the kernel from a counter-based generator: no
 * mask and no gathered row goes to memory, and a backward regenerates the mask of its forward from (seed, call).
 *
 * THE MASK (one definition; kge_amd/csrc/philox.hpp is its device form, tests/_dropout_ref.py its numpy restatement).
 * For a gathered row occurrence, element c of the row is DROPPED iff r < thr, where
 *   r       = word (c % 4) of Philox4x32-10(counter, key)        (the generator of kge_neg_sample)
 *   counter = (c / 4, occ, (uint32)call, role)                    role: 0 = the s row, 1 = the p row, 2 = the o row
 *   key     = (seed low 32, (seed high 32) ^ 0x44524F50)          (apart from kge_neg_sample's streams of the same seed)
 *   thr     = (uint32)floor(p * 2^32), computed in double          p = p_ent for entity rows, p_rel for relation rows
 * A kept element becomes x * scale with scale = 1.0f / (1.0f - p) (one float32 division on the host, one float32
 * multiply in the kernel); a dropped element becomes x * 0.0f: the value and sign torch.nn.Dropout produces.  p == 0 for
 * a table means thr = 0, scale = 1: that table's rows pass through untouched, bit for bit.  For RotatE the relation
 * mask lies on the rel_dim = dim / 2 phases.
 *
 * Occurrences:
 *   kge_score_spo_dropout    the three rows of triple i: occ = i, roles 0 / 1 / 2 (the law of the reference's three
 *                            embed() calls, kge_model.py:663-680)
 *   kge_score_neg_dropout    the two uncorrupted rows of positive i: occ = i, masked ONCE per positive (as score_sp /
 *                            score_po embed them once under `implementation: batch`, sampler.py:307-362); the corrupted
 *                            row of (i, k): role = slot, occ = i * num_neg + k (as under `implementation: triple`,
 *                            sampler.py:291-306).  The marginal law of every element is the reference's (kept with
 *                            probability 1 - p, scaled by 1 / (1 - p)); its own implementations differ in the joint law.
 *
 * KGE_ERR_UNSUPPORTED, nothing launched: an occurrence number or n * num_neg at or above 2^32; p_ent or p_rel outside
 * [0, 1), or both 0; bf16 tables; TransH and RESCAL tables; dim > 1024 (the scoring and backward entries).  A NULL
 * kge_dropout: KGE_ERR_INVALID_ARG.  A TransH or RESCAL table is declined in front of every other check, as by every
 * entry without such a kernel; otherwise every KGE_ERR_INVALID_ARG of the undropped entry is reported first. */
typedef struct kge_dropout {
  float p_ent, p_rel; /* drop probabilities of the entity / relation embedder, each in [0, 1), not both 0 */
  uint64_t seed;      /* the model's dropout seed                                                         */
  uint64_t call;      /* one number per fused call; the backward passes its forward's                     */
} kge_dropout;

/* embed() in training mode (lookup_embedder.py:96-105): out[i, :] = mask(table[idx[i], :]) for the occurrences
 * occ0 .. occ0 + n of `role` (0 / 1 / 2).  table: 0 = the entity table (p_ent), 1 = the relation table (p_rel).
 * out: float32 [n, dim or rel_dim], row pitch out_ld elements.  Useful on its own, and the device-side statement of the
 * mask.  The other table's probability may be 0 or not; the table's own may be 0 (a plain gather). */
int kge_embed_dropout(const kge_tables* t, int table, kge_index idx, int64_t n, int role, int64_t occ0,
                      const kge_dropout* dropout, float* out, int64_t out_ld, void* stream);

/* kge_score_spo / kge_score_neg (kge_model.py:663-680; sampler.py:263-306) on rows under the mask above, the dropout of
 * LookupEmbedder._postprocess (lookup_embedder.py:96-105) on every row the reference's embed() gathers.  The mask is
 * applied where a row chunk reaches the registers; everything after it is the arithmetic of the undropped kernel in the
 * same order: the scores carry the bits kge_score_spo / kge_score_neg return on tables that hold the masked rows.
 * float32 ComplEx, DistMult, TransE (every l_norm) and RotatE tables, dim <= 1024. */
int kge_score_spo_dropout(const kge_tables* t, kge_index s, kge_index p, kge_index o, int64_t n, float* out,
                          const kge_dropout* dropout, void* stream);
int kge_score_neg_dropout(const kge_tables* t, kge_index s, kge_index p, kge_index o, int64_t n, int slot,
                          const void* neg, int32_t neg_itype, int64_t neg_ld, int64_t num_neg, float* out, int64_t ldo,
                          const kge_dropout* dropout, void* stream);

/* kge_score_spo_bwd_accum / kge_score_neg_bwd_accum of the two entries above (lookup_embedder.py:96-105 backward;
 * sampler.py:263-306, train_negative_sampling.py:142-163): the masks of the forward's (seed, call) are regenerated, the
 * row gradients are evaluated on the masked rows, multiplied by the row's mask factor and accumulated into grad_ent /
 * grad_rel as the undropped entries do, with the same register summing of the fixed rows.  `scores`: the DROPOUT
 * forward's output.  A fully masked row still receives its (zero) atomics. */
int kge_score_spo_dropout_bwd_accum(const kge_tables* t, kge_index s, kge_index p, kge_index o, int64_t n,
                                    const float* gout, const float* scores, float* grad_ent, int64_t grad_ent_ld,
                                    float* grad_rel, int64_t grad_rel_ld, const kge_dropout* dropout, void* stream);
int kge_score_neg_dropout_bwd_accum(const kge_tables* t, kge_index s, kge_index p, kge_index o, int64_t n, int slot,
                                    const void* neg, int32_t neg_itype, int64_t neg_ld, int64_t num_neg,
                                    const float* gout, int64_t ldg, const float* scores, int64_t lds, float* grad_ent,
                                    int64_t grad_ent_ld, float* grad_rel, int64_t grad_rel_ld,
                                    const kge_dropout* dropout, void* stream);

/* The same backward with the [n, num_neg] occurrences SORTED by the entity they corrupt: `order` = int64 [n * num_neg]
 * (device), the positions i * num_neg + k in ascending neg[i, k] (any order among equal ids: kge_neg_order above).  kge_score_neg_bwd_accum issues one float atomic per element and occurrence into
 * grad_ent (262 M per slot at the WN18RR shape with 512 x 1000 negatives: 73 % of that training step); here a wave keeps
 * the running sum of an entity's gradient row in registers over consecutive occurrences and writes it where the entity
 * changes: ~num_entities / 32 + n * num_neg / 32 row flushes instead of n * num_neg.  Same sums in another order
 * (float rounding apart).  Worth the sort from a few occurrences per entity on.  rel_scratch (may be NULL): RotatE only,
 * num_rel x 2 rel_dim floats of scratch for the relations' cos / sin (computed once per call instead of per occurrence).  kge/util/sampler.py:263-306 backward,
 * called at kge/job/train_negative_sampling.py:161-163. */
/* `order` for the call below: a counting sort of the [n, num_neg] samples by entity id in two calls, no host wait
 * (capturable).  order == NULL: the histogram -- cursor[e] += the number of samples with id e (int64 [num_ent], zeroed
 * by the caller).  The caller turns it into exclusive prefix sums (a cumsum: the torch front end's), then order != NULL:
 * the scatter -- on return order[cursor_in[e] .. cursor_in[e + 1]) holds the positions i * num_neg + k of entity e's
 * samples in any order; cursor is clobbered. */
int kge_neg_order(const void* neg, int32_t neg_itype, int64_t neg_ld, int64_t n, int64_t num_neg,
                  int64_t num_ent, int64_t* cursor, int64_t* order, void* stream);
int kge_score_neg_bwd_accum_sorted(const kge_tables* t, kge_index s, kge_index p, kge_index o,
                                   int64_t n, int slot, const void* neg, int32_t neg_itype,
                                   int64_t neg_ld, int64_t num_neg, const int64_t* order,
                                   const float* gout, int64_t ldg, const float* scores, int64_t lds,
                                   float* grad_ent, int64_t grad_ent_ld, float* grad_rel,
                                   int64_t grad_rel_ld, float* rel_scratch, void* stream);

/* Backward of kge_score_neg_shared (replaces autograd through the sampler's indexing of the score matrix --
 * kge/util/sampler.py:450-460, 559-575 -- and through the scoring behind it, called at
 * kge/job/train_negative_sampling.py:142-163): gradients of sum_{i,c} gout[i*ldg + c] * out[i, c] ACCUMULATED into
 * the dense table gradients like kge_score_neg_bwd_accum.  gout is folded over the repeat columns and the drop rule
 * into one weight per (positive, physical row); a positive's relation / fixed entity row gradients are summed in
 * registers over a tile of 64 / NC physical rows, a physical row's gradient over a tile of 32 / NC positives (NC = 1,
 * 2, 4, 8 coordinate pairs per lane for ceil(dim / 2) <= 64, 128, 256, 512): one atomic row flush per (owner, tile),
 * none per occurrence.  `scores` = the forward output (row pitch lds; needed for TransE / RotatE with l_norm != 1 --
 * NULL there: KGE_ERR_INVALID_ARG --, may be NULL otherwise).  workspace: kge_score_neg_shared_workspace_bytes(t, n,
 * num_unique) bytes of device scratch, 16-byte aligned (sized for num_unique + 1 physical rows, with or without drop
 * indexes; less than the call needs: KGE_ERR_WORKSPACE).  f32 tables, dim <= 1024 (odd dims included); bf16 tables and
 * dim > 1024: KGE_ERR_UNSUPPORTED, gradients untouched.  n == 0 or num_unique + num_repeat == 0: KGE_OK, nothing is
 * touched.  Rows of grad_ent / grad_rel that only weightless pairs reach get +0.f added. */
int64_t kge_score_neg_shared_workspace_bytes(const kge_tables* t, int64_t n, int64_t num_unique);
int kge_score_neg_shared_bwd_accum(const kge_tables* t, kge_index s, kge_index p, kge_index o, int64_t n, int slot,
                                   const void* unique, int32_t unique_itype, int64_t num_unique, const int64_t* drop,
                                   const int64_t* repeat, int64_t num_repeat, const float* gout, int64_t ldg,
                                   const float* scores, int64_t lds, float* grad_ent, int64_t grad_ent_ld,
                                   float* grad_rel, int64_t grad_rel_ld, void* workspace, int64_t workspace_bytes,
                                   void* stream);

/* Backward of kge_score_so (replaces autograd through the three [n*m, dim] repeats of the reference's "s_o"
 * composition, kge/model/kge_model.py:727-747 and :202-209): gradients of sum_{i,j} gout[i*ldg + j] * out[i, j]
 * ACCUMULATED into the dense table gradients like kge_score_neg_shared_bwd_accum.  A pair's s and o row gradients are
 * summed in registers over a tile of 64 / NC relation rows, a relation entry's gradient over a tile of 32 / NC pairs
 * (NC = 1, 2, 4, 8 coordinate pairs per lane for ceil(dim / 2) <= 64, 128, 256, 512): one atomic row flush per (owner,
 * tile), none per (pair, relation) occurrence; s[i] == o[i], repeated pairs and repeated rels entries add up.
 * `scores` = the forward output (row pitch lds; needed for TransE / RotatE with l_norm != 1 -- NULL there:
 * KGE_ERR_INVALID_ARG --, may be NULL otherwise).  f32 tables, dim <= 1024 (odd dims included); bf16 tables and wider
 * dims: KGE_ERR_UNSUPPORTED, gradients untouched.  Rows no index names are not touched; rows that only zero weights
 * reach get +0.f added.  workspace: as kge_score_so. */
int kge_score_so_bwd_accum(const kge_tables* t, kge_index s, kge_index o, int64_t n, kge_index rels, int64_t m,
                           const float* gout, int64_t ldg, const float* scores, int64_t lds, float* grad_ent,
                           int64_t grad_ent_ld, float* grad_rel, int64_t grad_rel_ld, void* workspace,
                           int64_t workspace_bytes, void* stream);

/* Backward of kge_score_emb (dense embeddings).  SPO: g_s,g_o [n,dim], g_p [n,rel_dim].
 * SP_: g_s [n,dim], g_p [n,rel_dim], g_o [m,dim].  PO_: g_o [n,dim], g_p, g_s [m,dim]. */
int kge_score_emb_bwd(const kge_tables* t, int combine, const void* s_emb,
                      int64_t s_ld, const void* p_emb, int64_t p_ld,
                      const void* o_emb, int64_t o_ld, int64_t n, int64_t m,
                      const float* gout, int64_t ldg, const float* scores,
                      int64_t lds, float* g_s, float* g_p, float* g_o,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KGE_AMD_H */
