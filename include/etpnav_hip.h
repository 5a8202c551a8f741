/* etpnav_hip.h — C ABI of the MI355X-native ETPNav planner hot path (libetpnav_hip.so).
 *
 * The reference (MarSaKi/ETPNav) is 100 % Python/PyTorch and has no FFI; the "interface each entry point
 * replaces" is therefore the reference Python call site whose arithmetic it takes over (paths relative to
 * the reference root).  Every function:
 *   - takes raw device pointers (caller-owned, caller-allocated), plain integer sizes and a hipStream_t
 *     passed as void*; no torch / C++ types cross the boundary;
 *   - enqueues work on that stream and returns immediately (hipGraph-capturable: no allocation, no sync);
 *   - returns 0 on success, <0 for an invalid argument, >0 for a hipError_t; etp_last_error() gives text.
 * "T" below means the compute dtype selected by `dtype` (ETP_F32 parity mode, ETP_BF16 performance mode);
 * parameters, statistics, logits and losses are always fp32.
 */
#ifndef ETPNAV_HIP_H
#define ETPNAV_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ETP_OK 0
#define ETP_ERR_INVALID (-1)
#define ETP_ERR_STATE (-2)

#define ETP_F32 0
#define ETP_BF16 1

/* GEMM epilogue activations */
#define ETP_ACT_NONE 0
#define ETP_ACT_GELU 1      /* C = gelu_erf(v), aux Z = v            (BertIntermediate vilmodel_cmt.py:177-180) */
#define ETP_ACT_RELU 2      /* C = relu(v)                           (NextActionPrediction :654-655)           */
#define ETP_ACT_GELU_BWD 3  /* C = v * gelu_erf'(Z)                                                              */
#define ETP_ACT_RELU_BWD 4  /* C = v * (Z > 0)                                                                   */
/* Round 5: the GELU pair the planner's FFN blocks use.  The erf arithmetic made the GELU / GELU' epilogues VALU-bound (measured
 * with the arithmetic compiled out: FFN-up epilogue 8.2 -> 3.8 us, FFN dgrad 11.5 -> 5.5 us, profiles/r05_epilogue_valu.txt), and the
 * forward has everything the derivative needs in registers (cdf and exp(-v^2/2)): it saves gelu_erf'(v) instead of v, the backward
 * epilogue is a multiply.  Same stash footprint; nothing else reads the pre-activation. */
#define ETP_ACT_GELU_SAVEGRAD 5  /* C = gelu_erf(v), aux Z = gelu_erf'(v)   (bf16 mode: Z holds IEEE HALF values -- the      */
#define ETP_ACT_MUL_Z 6          /* C = v * Z                                derivative lies in [-0.13, 1.13], 11 bits > bf16's 8) */

typedef void* etp_stream_t; /* hipStream_t */

const char* etp_version(void);
const char* etp_last_error(void);

/* Run-time switches of the library (tile-class forcing for tests and A/B runs, schedule variants).  They are read from the
 * environment ONCE, at the first lookup (ETP_<NAME>), and afterwards change only through these calls -- no launch path calls
 * getenv (rounds 1-5 did, three times per GEMM launch).  `name` with or without the ETP_ prefix; value NULL or "" = unset.
 * The reference has no counterpart (its switches are Python config keys, vlnce_baselines/config/default.py); the names are listed
 * in csrc/options.h and every line bench.py prints carries the ones that are set (config.env_overrides). */
int etp_option_set(const char* name, const char* value);
int etp_option_get(const char* name, char* out, int cap);   /* length of the value (0 = unset), -1 = unknown switch */
int etp_option_list(char* out, int cap);                     /* "NAME=value\n" per set switch; returns the length needed */

/* ------------------------------------------------------------------------------------------------------
 * Per-operator entry points (one per implicit device op of SURVEY.md §2.1)
 * ---------------------------------------------------------------------------------------------------- */

/* C[m,n] = epi(alpha * sum_k A[m,k]*B[n,k]); replaces every nn.Linear / torch.matmul on the path
 * (vilmodel_cmt.py:108-110,117,133,151,178,190,326-328,335,348; common/transformer.py:138,140-142) and their
 * autograd backward (dgrad / wgrad).  trans_a/trans_b = 1 means the operand is stored [K][rows].
 *
 * The contract in one place (tests/test_gemm_kernels_gpu.py holds every kernel instance to it):
 *   v = alpha * sum_k A[m,k] B[n,k] + bias[n]     fp32 accumulation, alpha BEFORE the bias
 *   y = act(v)  [* Z for the backward forms]  + R[m,n]          R is added after the activation
 *   C = y (out_mode 0) | C + y, added in fp32 and rounded once (out_mode 1) | atomicAdd(C, y) (out_mode 2)
 * Written: C[m, n] for m < M, n < N, nothing else: columns N .. ldc - 1 of a row, rows beyond M and whatever surrounds a C that
 *   is a slice of a wider buffer are left alone (N % 8 != 0 takes a one-element-per-thread epilogue for that reason).  Z[m, n]
 *   for the same m, n under ETP_ACT_GELU (v, operand dtype) and ETP_ACT_GELU_SAVEGRAD (gelu'(v); IEEE half in bf16 mode).
 * Accumulated: C under out_mode 1 / 2; a_colsum[m] += sum_k A[m,k] ALWAYS accumulates, whatever out_mode says.
 * Read only: A, B, bias, R, Z under ETP_ACT_GELU_BWD / RELU_BWD (operand dtype) / MUL_Z (IEEE half in bf16 mode).
 * K == 0 is accepted: C = epi(0).
 * Alignment: A and B 16-byte aligned, lda / ldb and the A / B batch strides multiples of a 16-byte chunk (8 bf16, 4 fp32); a
 *   transposed operand's leading dimension covers its row count rounded up to that chunk.  C, R, Z and bias may sit anywhere:
 *   16-byte aligned bases with leading dimensions that are multiples of 8 (and N % 8 == 0) take the vectorised epilogue,
 *   everything else the scalar one, with equal results.
 * Which fields combine (everything else returns ETP_ERR_INVALID before anything is launched):
 *   (trans_a, trans_b) in {(0,0), (0,1), (1,1)};  dtype ETP_F32 needs c_dtype ETP_F32;
 *   out_mode 2 needs c_dtype ETP_F32;  ksplit > 1 needs out_mode 2 (the bias is added by the first split only);
 *   R, Z and an activation other than ETP_ACT_NONE need ksplit == 1 and batch == 1: every split would run the epilogue on its
 *     partial sum, and R / Z carry no batch stride;
 *   an activation other than ETP_ACT_NONE / ETP_ACT_RELU needs Z;
 *   a_colsum needs trans_a = trans_b = 1 and a reduction (per split) of whole 128-byte slabs, at least two of them. */
typedef struct etp_gemm_desc {
  const void* A; const void* B; void* C;
  int32_t M, N, K;
  int64_t lda, ldb, ldc;
  int32_t trans_a, trans_b;
  int32_t dtype;            /* operand dtype */
  int32_t c_dtype;          /* output dtype (ETP_F32 allowed with bf16 operands: weight gradients) */
  int32_t batch, batch_inner;               /* z -> (zo = z / batch_inner, zi = z % batch_inner) */
  int64_t sAo, sAi, sBo, sBi, sCo, sCi;     /* batch strides in elements */
  int32_t ksplit;           /* >1: split the reduction, needs out_mode 2 */
  float alpha;
  const float* bias;        /* [N] or NULL */
  const void* R; int64_t ldr; /* residual added after the activation, in the OUTPUT dtype (c_dtype: fp32 with bf16 operands and an
                               * fp32 C), or NULL; unsplit, unbatched products only */
  void* Z; int64_t ldz;     /* aux tensor for the activation epilogues, operand dtype (IEEE half for ETP_ACT_GELU_SAVEGRAD /
                             * ETP_ACT_MUL_Z in bf16 mode); unsplit, unbatched products only */
  int32_t act;              /* ETP_ACT_* */
  int32_t out_mode;         /* 0 store, 1 C += v, 2 atomicAdd (fp32 C) */
  float* a_colsum;          /* TN products (weight gradients) only, or NULL: a_colsum[m] += sum_k A[m,k] -- the bias gradient
                             * db = colsum(dY) fused into the dW = dY^T X product (K a multiple of the 128-byte slab, >= 2 slabs) */
} etp_gemm_desc;
int etp_gemm(const etp_gemm_desc* d, etp_stream_t stream);
/* n (<= 8) independent, unbatched, unsplit products of ONE (dtype, c_dtype, trans_a, trans_b) class in a single grid: the
 * four to seven weight gradients of one transformer layer (autograd of vilmodel_cmt.py:108-110,151,178,190,326-328), none
 * of which fills 256 CUs alone.  Every K must be a multiple of the 128-byte slab (64 bf16 / 32 fp32) and >= 2 slabs. */
int etp_gemm_group(const etp_gemm_desc* d, int n, etp_stream_t stream);
/* Host only, launches nothing and makes no HIP call: the name of the kernel instance etp_gemm(d) (n == 1) or etp_gemm_group(d, n)
 * (n > 1; the members re-sorted by K as the launch does) would run under the current switches, e.g. `gemm_dma<bf16,f32,TN,64x64,s3>`
 * or `mm32<bf16,bf16,NT,128x64,s3,k2>` -- family<operand dtype, C dtype, storage, tile, ring depth[, k2]>, the name the per-launch
 * profiler (etp_prof_report) and the phase probe report.  It runs the launch's own argument checks, instance selection and instance-list
 * lookup; pointers are only tested for NULL and alignment, never dereferenced.  Returns the name's length and writes the name, truncated to
 * `cap` bytes with the terminator (out may be NULL); where the launch would refuse the call, that same error code, with the same
 * etp_last_error. */
int etp_gemm_instance(const etp_gemm_desc* d, int n, char* out, int cap);

/* db[n] += sum_m dY[m,n]  (bias gradient of every nn.Linear).  db ACCUMULATES.  N % 4 == 0 and ld % 4 == 0; dy aligned to four
 * elements (8 bytes bf16, 16 bytes fp32); columns [N, ld) are never read.  Anything else: ETP_ERR_INVALID, nothing launched. */
int etp_colsum(int dtype, const void* dy, int64_t ld, float* db, int M, int N, etp_stream_t stream);

/* y = LayerNorm(x); stats[row] = {mean, rstd} (stats may be NULL).  x / y in `dtype`, gamma / beta / stats fp32.  H in {256, 512, 768,
 * 1024}.  x / y / dy / add / dx must be aligned to four elements (8 bytes bf16, 16 bytes fp32), gamma / beta to 16 bytes (every LayerNorm
 * entry point below checks the same and returns ETP_ERR_INVALID before anything is launched).  BertLayerNorm / nn.LayerNorm: vilmodel_cmt.py:59,147,186,459-478,
 * 571,656; common/transformer.py:144-145; common/ops.py:19-23. */
int etp_ln_fwd(int dtype, const void* x, const float* gamma, const float* beta, void* y, float* stats, int M, int H,
               float eps, etp_stream_t stream);
/* dx = LNbwd(dy) (+ add if non-NULL), OVERWRITTEN; dgamma / dbeta ACCUMULATED atomically -- pass both or neither (a mixed NULL pair
 * is refused).  stats: the forward's {mean, rstd} rows. */
int etp_ln_bwd(int dtype, const void* dy, const void* x, const float* stats, const float* gamma, const void* add, void* dx,
               float* dgamma, float* dbeta, int M, int H, etp_stream_t stream);

/* In-place masked row softmax over scores S[B,heads,Lq,ldS] (vilmodel_cmt.py:117-127,335-346,391-393,732-736):
 *   s += keymask(b,k) + (sp_w*dist[b,q,k] + sp_b);  mask_mode 0: (1-m)*-10000 (ops.py:25-34), 1: -inf (MHA key padding).
 * Columns [Lk, ldS) are written as 0. */
int etp_softmax_fwd(int dtype, void* S, const uint8_t* keymask, const float* dist, const float* sp_w, const float* sp_b,
                    int B, int heads, int Lq, int Lk, int ldS, int mask_mode, etp_stream_t stream);
int etp_softmax_bwd(int dtype, const void* P, void* dP, const float* dist, float* d_sp_w, float* d_sp_b, int B, int heads,
                    int Lq, int Lk, int ldS, etp_stream_t stream);

/* softmax(alpha*Q.K^T + mask)V for [B,heads] problems with head dim 64, head-interleaved row layouts
 * (BertSelfAttention / BertOutAttention / nn.MultiheadAttention).  P [B,heads,Lq,ldS] is the buffer the forward leaves for the
 * backward of the SAME shape/dtype: probabilities on the tile / batched-GEMM paths (fp32; bf16 with dist on an axis > 128),
 * and for bf16 otherwise only lse = rowmax + log(rowsum) (fp32, [B,heads,Lq] in the front of the buffer) -- the register-resident
 * (both axes <= 128) and streaming kernels recompute the probabilities in backward.  Callers must treat it as opaque.
 *
 * Contract (tests/test_attn_kernels_gpu.py holds every family to it against float64):
 *   - ctx, dQ, dK, dV are OVERWRITTEN; d_sp_w / d_sp_b ACCUMULATE (one atomicAdd per workgroup: their last bits depend on the order).
 *   - keymask NULL = every key valid.  mask_mode 0 adds -10000 to an invalid key's score, so a row whose keys are all invalid is the
 *     softmax of its unmasked scores.  Under mask_mode 1 a query row with NO valid key is OUTSIDE the contract: the register-resident,
 *     LDS-tile and batched-GEMM kernels return NaN there (exp(-inf - -inf): csrc/attn_rows.hip rows_fwd_kernel, `inv = 1.0f / sum`;
 *     csrc/norm.hip softmax_fwd_kernel), the streaming kernels 0 (csrc/attn.hip flash_fwd_kernel, `inv = l_run > 0 ? 1 / l_run : 0`).
 *     The model never forms such a row (every panorama has a view, every instruction a [CLS]).
 *   - Which kernel family runs (etp_attn_family; tried in this order):
 *       2 register-resident  bf16, Lq and Lk <= 128; Q / K / V 16-byte aligned, ldq / ldk / ldv / ldc multiples of 8, ldS >= 2;
 *                            sp_w and sp_b given whenever dist is (switch ATTN_ROWS)
 *       1 LDS-tile           Lq and Lk <= 128 (fp32: <= 64); Q / K / V 16-byte aligned; ldq / ldk / ldv / ldc / ldS multiples of
 *                            8 (bf16) or 4 (fp32) (switch ATTN_FUSED; ATTN_Q96 picks the 96 x 96 tile for 64 < Lq, Lk <= 96)
 *       3 streaming          bf16, Lq or Lk > 128, dist NULL; same alignment as 2, ldS >= 4 (switches ATTN_FLASH and ATTN_FUSED)
 *       0 batched-GEMM       everything else: fp32 beyond 64, bf16 with dist beyond 128, an operand or leading dimension that is
 *                            not aligned as above, a switch turned off.  Stores alpha*Q.K^T and dP in the operand dtype.
 *   - The backward re-derives the forward's family from the same descriptor (it decides what P holds), so the switches, the operand
 *     alignments and ctx / ldc must be the same for a forward and its backward; families 2 and 3 then also need 16-byte-aligned
 *     dctx / dQ / dK / dV rows and fail with ETP_ERR_INVALID otherwise. */
typedef struct etp_attn_desc {
  int32_t dtype, B, heads, Lq, Lk, ldS;
  const void* Q; int64_t ldq;   /* Q rows [B*Lq], head h at column h*64 */
  const void* K; int64_t ldk;
  const void* V; int64_t ldv;
  void* P;                      /* [B,heads,Lq,ldS] saved for etp_attn_bwd (opaque, see above) */
  void* ctx; int64_t ldc;       /* [B*Lq, heads*64] */
  const uint8_t* keymask;       /* [B,Lk] 1 = valid */
  int32_t mask_mode;
  const float* dist;            /* [B,Lq,Lk] or NULL (graph_sprels) */
  const float* sp_w; const float* sp_b;
  float alpha;
} etp_attn_desc;
int etp_attn_fwd(const etp_attn_desc* d, etp_stream_t stream);
/* Host only, launches nothing: the family etp_attn_fwd would run for `d` under the current switches -- 0 batched-GEMM, 1 LDS-tile,
 * 2 register-resident, 3 streaming (the same predicates in the same order, from the helper the dispatch itself uses); < 0 on error. */
int etp_attn_family(const etp_attn_desc* d);
/* Self-attention forward with the QKV PROJECTION folded in (round 6): Q / K / V of `d` (Lq == Lk, rows of one token block, e.g. the
 * three column blocks of a [B*L, 3*heads*64] stash) are OUTPUTS -- each (batch, head) workgroup computes
 *   [Q | K | V][b, l, h*64 : h*64+64] = x[b*L + l, :] . w_qkv[sec*heads*64 + h*64 + (0..63), :]^T + b_qkv     (sec = 0, 1, 2)
 * itself (BertSelfAttention.query / key / value, vilmodel_cmt.py:108-110; MHA in_proj_weight, common/transformer.py:138), stores them
 * (the backward's stash) and goes on with the attention, instead of reading the result of a GEMM launch.  x [B*L, heads*64] (row
 * stride ldx) and w_qkv [3*heads*64][ldw] in the operand dtype, b_qkv fp32 [3*heads*64] or NULL.  bf16, L <= 128, heads*64 == 768;
 * anything else returns ETP_ERR_INVALID and the caller issues etp_gemm + etp_attn_fwd.  Results equal that pair's (the projections
 * are rounded to bf16 exactly where the GEMM stored them). */
int etp_attn_fwd_qkv(const etp_attn_desc* d, const void* x, int64_t ldx, const void* w_qkv, int64_t ldw, const float* b_qkv,
                     etp_stream_t stream);
typedef struct etp_attn_bwd_desc {
  etp_attn_desc f;              /* same as forward; ctx / ldc MUST be the forward's output: the bf16 kernels keep only lse in P and
                                 * recompute from it (Lq or Lk > 128 also read ctx for D = rowsum(dO * O)) */
  const void* dctx; int64_t ldd;
  void* dP;                     /* scratch [B,heads,Lq,ldS] */
  void* dQ; int64_t lddq; void* dK; int64_t lddk; void* dV; int64_t lddv;
  float* d_sp_w; float* d_sp_b; /* accumulated, or NULL */
} etp_attn_bwd_desc;
int etp_attn_bwd(const etp_attn_bwd_desc* d, etp_stream_t stream);
/* The same two calls with PER-EPISODE K/V INDIRECTION (the batched rollout: T = B / kv_mod steps stacked along the batch axis share the
 * kv_mod instructions; the reference re-projects the same txt_embeds at every step, ss_trainer_ETP.py:819-822 -> BertOutAttention
 * vilmodel_cmt.py:326-348): K and V have kv_mod*Lk rows, keymask is [kv_mod, Lk], and stacked episode b reads instruction b % kv_mod
 * inside the kernels.  Q, ctx, P, dctx and dQ stay per stacked episode ([B*Lq] rows); B % kv_mod == 0.
 *   sum_steps == 0   dK / dV per stacked episode, B*Lk rows: the same bits as etp_attn_fwd / etp_attn_bwd on K, V and masks replicated
 *                    B / kv_mod times
 *   sum_steps == 1   dK / dV SUMMED over the B / kv_mod episodes of each instruction, kv_mod*Lk rows (what autograd accumulates into the
 *                    shared txt_embeds, ss_trainer_ETP.py:1055): the streaming dK/dV kernel keeps the sum in its fp32 accumulators and
 *                    rounds once.  Deterministic (no atomics).
 * Served by families 2 (register-resident; sum_steps == 0 only) and 3 (streaming) of etp_attn_family; any other family (fp32, dist
 * beyond 128, a switch turned off, unaligned operands), sum_steps == 1 on family 2 or B % kv_mod != 0 returns ETP_ERR_INVALID and
 * launches nothing. */
int etp_attn_fwd_kv(const etp_attn_desc* d, int kv_mod, etp_stream_t stream);
int etp_attn_bwd_kv(const etp_attn_bwd_desc* d, int kv_mod, int sum_steps, etp_stream_t stream);
/* The same backward with the OUT-PROJECTION's input gradient folded in (round 6): `d->dctx` is dL/d(dense output) [B*Lq, heads*64]
 * (row stride ldd) of BertSelfOutput.dense / BertOutAttention's output dense / MHA out_proj (vilmodel_cmt.py:150-154, 325-352;
 * common/transformer.py:138-142), `w_out` that projection's weight [heads*64 (out)][ldw] in the operand dtype; each (batch, head)
 * workgroup forms dctx[:, h*64:h*64+64] = dctx_in . w_out[:, h*64:h*64+64] itself instead of reading the result of a GEMM launch.
 * bf16 with both axes <= 128 and heads*64 == 768; anything else returns ETP_ERR_INVALID and the caller issues
 * etp_gemm + etp_attn_bwd.  Results equal that pair's (the tile is rounded to bf16 exactly where the GEMM stored it). */
int etp_attn_bwd_proj(const etp_attn_bwd_desc* d, const void* w_out, int64_t ldw, etp_stream_t stream);

/* Neighbourhood attention of the waypoint predictor (vlnce_baselines/waypoint_pred/transformer/waypoint_bert.py:49-90 under the mask
 * of waypoint_pred/utils.py:90-102, TRM_net.py:51-53,74-77), forward only -- the predictor is frozen and in eval()
 * (ss_trainer_ETP.py:201-202), so there is no dropout and nothing is saved for a backward:
 *   ctx[b*12 + i, h*64 : h*64+64] = sum_{o = -neighbor .. neighbor} softmax_o(alpha q_i . k_{(i+o) mod 12}) v_{(i+o) mod 12}
 * Q, K, V: head-interleaved rows [B*12, ld] in `dtype` (12 heads of 64 at column h*64; three slices of one [B*12, 2304] product
 * or separate buffers), ctx [B*12, ldc] in `dtype`.  Twelve tokens, twelve heads, head dimension 64 are fixed.  The reference adds
 * -10000 to the scores outside the window, which in fp32 equals leaving those keys out (exp(-10000 + d) == 0): they are not read.
 * fp32 scores, probabilities and accumulation whatever `dtype` is; ctx is rounded once, at its store.  Columns 768 .. ldc-1 of ctx are
 * left alone.
 * ETP_ERR_INVALID before anything is launched: neighbor outside 0 .. 5 (utils.py:91), B <= 0, an operand not aligned to four elements
 * (8 bytes bf16, 16 bytes fp32), a leading dimension below 768 or not a multiple of 4. */
int etp_ring_attn_fwd(int dtype, const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv, void* ctx,
                      int64_t ldc, int B, int neighbor, float alpha, etp_stream_t stream);

/* From heat-map logits to waypoint candidates, one workgroup per episode (vlnce_baselines/models/Policy_ViewSelection_ETP.py:220-239,
 * 247-282, 304-305, 313-314; waypoint_pred/utils.py:8-64).  logits [B,120,12] fp32 (angle x distance, already rolled by
 * HEATMAP_OFFSET, TRM_net.py:84-86):
 *   heat [B,120,12]      softmax over the 1 440 cells
 *   nms_map [B,120,12]   nms(wrap(heat), max_predictions = max_pred, sigma = (sigma_x, sigma_y)) without the two wrap rows.  The wrapped
 *                        map has 122 angle rows (row 0 = angle 119, row 121 = angle 0).  Each round takes the arg-max (lowest flat index
 *                        among equal values), records it and zeroes the cells with min(|x - x_mu|, |x - x_mu + 12|) <= sigma_x and
 *                        |y - y_mu| <= sigma_y, where x_mu = ix % 12 and y_mu = ix / 12 is a TRUE division (utils.py:55): the centre on
 *                        the angle axis is fractional.  A pick in a wrap row is lost with the row.
 *   cand_count [B]       int32, number of non-zero cells of nms_map (<= max_pred)
 *   cand_angle, cand_dist, cand_img_cw, cand_img_ccw [B,max_pred]   int32, the non-zero cells in row-major order: angle index, distance
 *                        index, ((angle+5)/10) % 12 (:263-264) and (12 - (angle+5)/10) % 12 (:313-314); -1 beyond the count
 * uniforms [B,max_pred] fp32 in [0,1) or NULL.  Non-NULL (in_train, :247-282): per candidate, the softmax over the 10 x 12 logits of its
 *   image sector (taken from the logits rolled back by 5) and one inverse-CDF draw -- the first index whose inclusive prefix sum, added
 *   serially in index order, exceeds u * total -- in place of torch.distributions.Categorical.sample (whose stream is not reproduced):
 *   samp_angle = act / 12 + pointer, samp_dist = act % 12, pointer = (sector-1)*10 + 5, or 0 for sector 0 (:275-280); -1 beyond the count.
 *   With uniforms NULL samp_angle / samp_dist may be NULL and are not written.
 * Plain stores only, no atomics: a second run returns the same bits.
 * ETP_ERR_INVALID before anything is launched: max_pred outside 1 .. 8, B <= 0, logits / heat / nms_map not 16-byte aligned, a table
 * not 4-byte aligned, uniforms without samp_angle / samp_dist. */
int etp_waypoint_tail(const float* logits, int B, int max_pred, float sigma_x, float sigma_y, const float* uniforms, float* heat,
                      float* nms_map, int32_t* cand_count, int32_t* cand_angle, int32_t* cand_dist, int32_t* cand_img_cw,
                      int32_t* cand_img_ccw, int32_t* samp_angle, int32_t* samp_dist, etp_stream_t stream);

/* Residual-stream convention: tensors that flow from one LayerNorm / residual add to the next are ALWAYS fp32 (as under
 * the reference's autocast, where LayerNorm and residual adds stay fp32); `*_lp` arguments are optional copies in the GEMM
 * operand dtype `dtype` for the next MFMA product (pass NULL in fp32 mode). */

/* LayerNorm on the fp32 stream: y (fp32, may be NULL) and/or y_lp (operand dtype, may be NULL). */
int etp_ln_stream_fwd(int dtype, const float* x, const float* gamma, const float* beta, float* y, void* y_lp, float* stats, int M,
                      int H, float eps, etp_stream_t stream);
int etp_ln_stream_bwd(int dtype, const float* dy, const float* x, const float* stats, const float* gamma, const float* add,
                      float* dx, void* dx_lp, float* dgamma, float* dbeta, int M, int H, etp_stream_t stream);
/* The same with the two-stage parameter-gradient reduction the planner uses: stage 1 (on `stream`) writes per-workgroup
 * column sums to `part` (etp_ln_bwd_part_bytes(M, H) bytes), stage 2 (on `reduce_stream`, ordered after stage 1 by the
 * caller when the streams differ) adds them into dgamma / dbeta.
 * etp_ln_bwd_part_bytes = 2*H*4 bytes per stage-1 workgroup: ceil(ceil(M/4) / rounds) workgroups, rounds = ceil(ceil(M/4) / cap), cap =
 * 1024 or the LNBWD_GRID switch clamped to [1, 1024].  Change the switch between the size query and the two stages and the sizes no
 * longer agree.  Stage 1 needs dgamma, dbeta and part non-NULL (it does not touch dgamma / dbeta); stage 2 only reads part. */
int64_t etp_ln_bwd_part_bytes(int M, int H);
int etp_ln_stream_bwd_stage1(int dtype, const float* dy, const float* x, const float* stats, const float* gamma, const float* add,
                             float* dx, void* dx_lp, float* dgamma, float* dbeta, float* part, int M, int H, etp_stream_t stream);
int etp_ln_part_reduce(const float* part, int M, int H, float* dgamma, float* dbeta, etp_stream_t reduce_stream);

/* BertEmbeddings.forward vilmodel_cmt.py:62-77 (eval): y = LN(word[id] + pos[l] + type[0]).
 * Forward: y, y_lp (may be NULL) and stats are OVERWRITTEN.  Backward: the parameter gradients dword / dpos / dtype0 / dgamma /
 * dbeta are ACCUMULATED (+=) into what the caller passes (zero them for a fresh gradient); the padding row 0 of dword is not
 * touched. */
int etp_text_embed_fwd(int dtype, const int64_t* ids, const float* word, const float* pos, const float* type0,
                       const float* gamma, const float* beta, float* y, void* y_lp, float* stats, int B, int L, int H, float eps,
                       etp_stream_t stream);
int etp_text_embed_bwd(int dtype, const float* dy, const int64_t* ids, const float* word, const float* pos,
                       const float* type0, const float* gamma, const float* stats, float* dword, float* dpos, float* dtype0,
                       float* dgamma, float* dbeta, int B, int L, int H, etp_stream_t stream);

/* Panorama view-embedding fuse, forward_panorama vilmodel_cmt.py:695-711:
 *   y = LN(LN_i(a) + LN_d(d) + LN_l(loc.Wl^T+bl) + nav_emb[nav] + type_emb[1]); a,d (dtype T) = MFMA projections of rgb/depth.
 * params / grads: 12 fp32 pointers in the order g_img,b_img,g_dep,b_dep,w_loc,bias_loc,g_loc,b_loc,nav_emb,type1,g_out,b_out.
 * stats: [M,8]; y / dy fp32; da, dd in dtype T.  d (and dd) may be NULL: no depth branch, stats columns 2-3 are not written
 * and grads[2] / grads[3] (g_dep, b_dep) are left untouched.
 * Backward: the twelve parameter gradients are ACCUMULATED (+=); the row outputs da / dd are OVERWRITTEN. */
int etp_pano_embed_fwd(int dtype, const void* a, const void* d, const float* loc, const int64_t* nav,
                       const float* const* params, float* y, float* stats, int M, int H, etp_stream_t stream);
int etp_pano_embed_bwd(int dtype, const float* dy, const void* a, const void* d, const float* loc, const int64_t* nav,
                       const float* stats, const float* const* params, float* const* grads, void* da, void* dd, int M, int H,
                       etp_stream_t stream);

/* forward_navigation vilmodel_cmt.py:728-730: x = img + step_emb[step] + LN(pos.Wp^T+bp)  (img, x, dx fp32; x_lp may be NULL).
 * Backward: d_step_emb (rows named by step_ids only), d_w_pos [H, pos_dim], d_b_pos, dgamma, dbeta are ACCUMULATED (+=). */
int etp_gmap_embed_fwd(int dtype, const float* img, const int64_t* step_ids, const float* pos, const float* step_emb,
                       const float* w_pos, const float* b_pos, const float* gamma, const float* beta, float* x, void* x_lp,
                       float* stats, int M, int H, int pos_dim, etp_stream_t stream);
int etp_gmap_embed_bwd(int dtype, const float* dx, const int64_t* step_ids, const float* pos, const float* w_pos,
                       const float* b_pos, const float* gamma, const float* stats, float* d_step_emb, float* d_w_pos,
                       float* d_b_pos, float* dgamma, float* dbeta, int M, int H, int pos_dim, etp_stream_t stream);

/* NextActionPrediction tail vilmodel_cmt.py:651-661 + masked_fill_ :742-744: logits = LN(r).w2 + b2, -inf where
 * visited or !valid; r = relu(x.W1^T+b1) from etp_gemm(ETP_ACT_RELU).  visited / valid may each be NULL (no such mask).
 * Backward: dgamma / dbeta / dw2 / db2 are ACCUMULATED (+=); the row output dz (gradient of the pre-ReLU input) is OVERWRITTEN,
 * exactly 0 on masked rows (whatever dlogits holds there) and where r == 0. */
int etp_sap_tail_fwd(int dtype, const void* r, const float* gamma, const float* beta, const float* w2, const float* b2,
                     const uint8_t* visited, const uint8_t* valid, float* logits, float* stats, int M, int H,
                     etp_stream_t stream);
int etp_sap_tail_bwd(int dtype, const float* dlogits, const void* r, const float* gamma, const float* beta, const float* w2,
                     const float* stats, const uint8_t* visited, const uint8_t* valid, void* dz, float* dgamma, float* dbeta,
                     float* dw2, float* db2, int M, int H, etp_stream_t stream);

/* F.cross_entropy(reduction='sum', ignore_index) ss_trainer_ETP.py:892 scaled by `scale` (:1055):
 * *loss = scale*sum_b nll_b (stored, not accumulated) ; dlogits = scale*(softmax - onehot) (0 on ignored rows); dlogits may
 * be NULL.  One workgroup; labels must be ignore_index or in [0, G); a -inf logit no label points at gets an exactly zero gradient;
 * with every row ignored *loss and dlogits are exactly 0. */
int etp_sap_ce(const float* logits, const int64_t* labels, float* loss, float* dlogits, int B, int G, float scale,
               int64_t ignore_index, etp_stream_t stream);

/* out[n,:] (+)= sum_{j in [ptr[n],ptr[n+1])} w[j]*src[idx[j],:] — node aggregation (ss_trainer_ETP.py:838-839,
 * graph_utils.py:272-276, pretrain vilmodel.py:585-619) and, with the transposed CSR, its backward.  src / out in `dtype` (bf16: the
 * row is accumulated in fp32 and rounded once), aligned to four elements; H in {256, 512, 768}; ptr has N + 1 entries; accumulate != 0
 * adds onto what out holds; rows >= N are not touched. */
int etp_gather_sum(int dtype, const void* src, const int32_t* ptr, const int32_t* idx, const float* w, void* out, int N, int H,
                   int accumulate, etp_stream_t stream);

/* Round-to-nearest-even (NaN stays NaN); src and dst 16-byte aligned, any n. */
int etp_cast_f32_to_bf16(const float* src, void* dst, int64_t n, etp_stream_t stream);
/* dst[i] = float(src[i]) * scale and p[i] *= scale: one fp32 rounding per element; scalar accesses, natural alignment, any n. */
int etp_cast_bf16_to_f32(const void* src, float* dst, int64_t n, float scale, etp_stream_t stream);
int etp_scale_f32(float* p, int64_t n, float scale, etp_stream_t stream);

/* Masked-LM loss over the vocabulary (pretrain_cmt.py:155-159: F.cross_entropy(reduction='none').mean() with scale = 1/Nm), one
 * workgroup per masked token.  logits fp32 [Nm, ldv], ldv >= V; columns >= V are padding and are never read.  labels [Nm] in [0, V)
 * (there is no ignore_index: the caller gathers the masked tokens).  dlogits [Nm, ldv] in `dtype` is OVERWRITTEN with
 * scale * (softmax - onehot), one rounding to bf16 where dtype is ETP_BF16, and exactly 0 in the padding columns and in a -inf column
 * no label points at.  *loss is ACCUMULATED (+= scale * nll of every row, one atomic per row: the order, and with it the last bits
 * of the sum, may change from run to run); the caller zeroes it (etp_memset_async).  Refused: NULL pointers, Nm <= 0, V <= 0,
 * ldv < V. */
int etp_vocab_ce(int dtype, const float* logits, const int64_t* labels, float* loss, void* dlogits, int Nm, int V, int ldv,
                 float scale, etp_stream_t stream);
/* d[i] <- d[i] * gelu'(z[i]), gelu'(x) = Phi(x) + x phi(x) (erf form, BertPredictionHeadTransform's activation), in place; d and z in
 * `dtype`, computed in fp32 with one rounding on the store; z is read only; scalar accesses, natural alignment, any n >= 0 (n = 0
 * launches nothing).  x phi(x) is formed as written: z = +-inf gives NaN, as torch's own GELU backward does. */
int etp_gelu_bwd(int dtype, void* d, const void* z, int64_t n, etp_stream_t stream);
/* dst[i] = sum_{t < steps} src[t * n + i], accumulated in fp32 in the order t = 0, 1, ... and rounded once to `dtype` (steps = 1 is a
 * bit-for-bit copy; the first addend is added onto +0).  Refused: NULL pointers, n % 4 != 0, steps <= 0, src or dst not 16-byte
 * aligned.  n = 0 launches nothing. */
int etp_sum_steps(int dtype, const void* src, void* dst, int64_t n, int steps, etp_stream_t stream);
/* dst[t * bytes + i] = src[i] for t < T, byte for byte in 16-byte vectors (the text K|V cache replicated for T stacked steps); src and
 * dst must not overlap.  Refused: NULL pointers, bytes % 16 != 0, src or dst not 16-byte aligned.  bytes = 0 or T = 0 launches
 * nothing. */
int etp_repeat_block(const void* src, void* dst, int64_t bytes, int T, etp_stream_t stream);
/* dst[i] = src[i], i < n, bit for bit (float4 body, scalar tail of n % 4 elements); src == dst or n = 0 launches nothing; otherwise
 * the buffers must not overlap.  Refused: NULL pointers, src or dst not 16-byte aligned. */
int etp_copy_f32(const float* src, float* dst, int64_t n, etp_stream_t stream);
/* dst[i] = (dtype) src[i]: fp32 -> the operand dtype in vectors of four (the panorama's RGB-feature conversion without its dropout).
 * ETP_F32: a bit-for-bit copy; ETP_BF16: round-to-nearest-even, NaN stays NaN.  Refused: NULL pointers, n % 4 != 0, src or dst not
 * 16-byte aligned.  n = 0 launches nothing. */
int etp_cast_f32_to(int dtype, const float* src, void* dst, int64_t n, etp_stream_t stream);
/* gen_seq_masks (common/ops.py:36-44): m1[b, v] = v < lens[b] ? 1 : 0 for b < B, v < V; m2 (nullable) receives the same bytes.  lens
 * int64 [B]; a length <= 0 gives a row of zeros, a length >= V a row of ones.  Refused: NULL lens / m1, B <= 0, V <= 0. */
int etp_seq_mask(const int64_t* lens, uint8_t* m1, uint8_t* m2, int B, int V, etp_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Fused AdamW over flat fp32 arenas.  Replaces, in ONE HBM pass per step: torch.optim.AdamW
 * (ss_trainer_ETP.py:213,505) or the pre-training AdamW (pretrain_src/pretrain_src/optim/adamw.py:53-112),
 * GradScaler.unscale_ + its non-finite check (ss_trainer_ETP.py:463,504-506), clip_grad_norm_, the autocast weight
 * casts of the next forward (etp_planner_refresh_weights) and optimizer.zero_grad().
 *   hf_style 0: torch.optim.AdamW      p *= 1 - lr*wd;  p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps)
 *   hf_style 1: optim/adamw.py         p -= lr*sqrt(bc2)/bc1 * m / (sqrt(v) + eps);  p -= lr*wd*p
 *   bc1 = 1-beta1^step, bc2 = 1-beta2^step (both 1 when correct_bias == 0); step counts from 1.
 *   g = grad * grad_scale * clip, clip = min(1, max_norm / (sqrt(*sumsq)*|grad_scale| + 1e-6)) when max_norm > 0.
 * decay_mask (nullable = decay everywhere, nothing frozen): one byte per 64 consecutive elements; bit 0 = apply weight_decay
 * (planner parameters start on 64-element boundaries, so any per-parameter grouping such as optim/misc.py:12-22 fits),
 * bit 1 = FROZEN block (requires_grad = False: fix_lang_embedding / fix_pano_embedding, vilmodel_cmt.py:675-682;
 * LanguageEncoder :422-424): p / m / v / shadow are left untouched, the gradient is still zeroed.
 * CHANGELOG (round 5 -> 6): until round 4 the byte meant "any non-zero value = decay".  The byte values are now 0 = no decay,
 * 1 = decay, 2 / 3 = frozen; every other non-zero value (0xFF, a bool stored as 255, ...) still means "decay" and never "frozen", so
 * the only value whose meaning changed for an old caller is exactly 2.
 * shadow (nullable): bf16 copy written for elements [0, n_shadow).  skip (nullable, device int32): non-zero -> leave
 * p/m/v/shadow untouched (GradScaler's skipped step); gradients are still zeroed when zero_grads != 0.
 * sumsq / skip are produced by etp_grad_sqnorm (both ACCUMULATE: zero them first).  n % 4 == 0, 16-byte aligned.
 * decay_mask holds ceil(n / 64) bytes: when n % 64 != 0 the last byte covers the partial block (the kernels read byte e >> 6 of element
 * e and nothing behind it).  n_shadow % 4 == 0 and 0 <= n_shadow <= n.  max_norm > 0 REQUIRES sumsq (it used to train unclipped without
 * a word when sumsq was NULL); 0 <= beta < 1; step >= 1 unless a device counter is given.  A refused call launches nothing.
 * zero_grads == 0 leaves the gradients as they are.  A frozen block's gradient is zeroed like any other. */
typedef struct {
  float lr, beta1, beta2, eps, weight_decay;
  int32_t step;
  int32_t hf_style;
  int32_t correct_bias;
  float grad_scale;
  float max_norm;
} etp_adamw_cfg;
int etp_adamw_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, void* shadow, int64_t n_shadow,
                   const uint8_t* decay_mask, int64_t n, const etp_adamw_cfg* cfg, const float* sumsq, const int32_t* skip,
                   int zero_grads, etp_stream_t stream);
/* The same with the optimizer's step count kept ON THE DEVICE: *step_counter is incremented only when the update is applied
 * (skip == NULL or *skip == 0) and the bias corrections use it -- GradScaler.step() does not call optimizer.step() on
 * overflow, so state['step'] must not advance on a skipped step (ss_trainer_ETP.py:504-506).  cfg->step is ignored.  The bias
 * corrections are then formed on the device in fp32 (powf): at beta2 = 0.999 and t = 1 that is a relative error of up to ~1e-4 in the
 * update (2^-24 * beta^t / (1 - beta^t)), against 1e-7 for etp_adamw_step, which forms them on the host in double. */
int etp_adamw_step_counted(float* params, float* grads, float* exp_avg, float* exp_avg_sq, void* shadow, int64_t n_shadow,
                           const uint8_t* decay_mask, int64_t n, const etp_adamw_cfg* cfg, const float* sumsq, const int32_t* skip,
                           int zero_grads, int32_t* step_counter, etp_stream_t stream);
/* *sumsq += sum g^2, *nonfinite += number of NaN / +-inf values (nonfinite may be NULL); n % 4 == 0, grads 16-byte aligned. */
int etp_grad_sqnorm(const float* grads, int64_t n, float* sumsq, int32_t* nonfinite, etp_stream_t stream);
/* The same, leaving out the blocks whose mask byte (layout of decay_mask above, ceil(n / 64) bytes) is 2 or 3: frozen parameters have no .grad in
 * the reference, so clip_grad_norm_ / GradScaler's non-finite scan never see them. */
int etp_grad_sqnorm_masked(const float* grads, int64_t n, const uint8_t* mask, float* sumsq, int32_t* nonfinite,
                           etp_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Planner engine: whole forward/backward of the three planner entry points over one flat parameter arena.
 * Replaces GlocalTextPathNavCMT.forward_txt / forward_panorama / forward_navigation (vilmodel_cmt.py:684-750)
 * and their autograd backward.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct etp_config {
  int32_t hidden, heads, inter;
  int32_t n_l, n_p, n_x;                 /* text / panorama / cross-modal layer counts (vlnbert_init.py:46-48) */
  int32_t vocab, max_pos, type_vocab;
  int32_t img_feat, dep_feat, ang_feat, max_steps;
  int32_t use_depth, use_sprels;
  float ln_eps;                          /* config.layer_norm_eps (1e-12 bert / 1e-5 xlm-r) */
  int32_t dtype;                         /* ETP_F32 | ETP_BF16 */
  int32_t use_lang2visn;                 /* pre-training variant (run_pt/r2r_model_config_dep.json use_lang2visn_attn): adds the
                                          * language-side x-layer weights (vilmodel.py:371-376) and the tied MLM head (:258-299) */
} etp_config;

typedef struct etp_param_info {
  char name[128];                        /* reference state-dict name */
  int32_t ndim; int64_t shape[2];
  int64_t offset;                        /* element offset in the fp32 arena (and grad arena, and bf16 shadow) */
} etp_param_info;

typedef struct etp_planner etp_planner;

etp_planner* etp_planner_create(const etp_config* cfg);      /* NULL on error */
void etp_planner_destroy(etp_planner* p);
int etp_planner_param_count(const etp_planner* p);
int etp_planner_param_info(const etp_planner* p, int i, etp_param_info* out);
int64_t etp_planner_arena_elems(const etp_planner* p);       /* total fp32 elements */
int64_t etp_planner_matrix_elems(const etp_planner* p);      /* leading region holding the GEMM weights */
/* params: fp32 master arena; shadow: bf16 copy of the matrix region (NULL in fp32 mode); grads: fp32 arena. */
int etp_planner_bind(etp_planner* p, float* params, void* shadow, float* grads);
/* Optional second stream for the backward entry points: weight-gradient GEMMs (leaves of the autograd graph) are issued
 * on `aux` after their dY producer and joined back before the call returns to `stream`, so they overlap the dgrad
 * chain (works eagerly and under hipGraph capture: the fork/join become graph edges).  NULL = single stream. */
int etp_planner_set_aux_stream(etp_planner* p, etp_stream_t aux);
/* Optional third stream for etp_nav_bwd: the d(txt_embeds) contributions of the text K/V projections (vilmodel_cmt.py:326-328,
 * M = B*L rows) accumulate on `aux2` beside the node chain.  NULL = main stream.  With lazy joins off (below) they are joined
 * back before the call returns.  With lazy >= 1, etp_nav_bwd returns with d_txt_embeds complete ONLY on `aux2`: it becomes
 * ordered into `stream` by the next etp_txt_bwd / etp_txt_bwd_range or etp_planner_join_aux ON THE SAME STREAM (the call
 * remembers which stream is owed the wait).  A caller that reads d_txt_embeds otherwise -- on another stream, with torch, on
 * the host -- must call etp_planner_join_aux(p, stream) with etp_nav_bwd's stream first. */
int etp_planner_set_aux2_stream(etp_planner* p, etp_stream_t aux2);
/* With an aux stream: lazy = 1 lets etp_nav_bwd* / etp_pano_bwd return WITHOUT joining their weight-gradient GEMMs back
 * (nothing downstream of them reads weight gradients), so the text backward does not wait for the navigation weight
 * gradients; the gradients are complete in `stream` order only after a later joining call: etp_txt_bwd / etp_txt_bwd_range
 * / etp_nav_kv_bwd (always join) or etp_planner_join_aux.  Default 0: every backward entry point joins before it returns.
 * Not only weight gradients are deferred: with an aux2 stream, lazy >= 1 also defers the join of etp_nav_bwd's d_txt_embeds
 * (see etp_planner_set_aux2_stream: in flight on `aux2` when the call returns, waited for by etp_txt_bwd(_range) and
 * etp_planner_join_aux on the same stream only).
 * lazy = 2: additionally etp_txt_bwd_range calls that stop above layer 0 do not join (the next range continues the chain). */
int etp_planner_set_lazy_join(etp_planner* p, int lazy);
/* on = 1: weight-gradient products STORE into the matrix region [0, etp_planner_matrix_elems) of the gradient arena instead of
 * accumulating (torch's `.grad +=`, the default): no fp32 read of the old gradient and no per-step zeroing of that region.
 * Valid when every weight matrix receives exactly one weight-gradient product between two optimizer steps (one rollout step
 * per optimizer step, as bench.py's unit of work); the vector / embedding-table tail still accumulates and must be zeroed. */
int etp_planner_set_grad_overwrite(etp_planner* p, int on);
int etp_planner_join_aux(etp_planner* p, etp_stream_t stream);
/* Training-mode dropout (all rates 0 = eval, the default).  Masks are a counter-based hash of (seed, site, element index):
 * nothing is stored, the backward entry points recompute the masks, so a backward call must see the same rates and seed as
 * its forward (the state is read at enqueue time; change it between calls freely).  Sites mirror the reference:
 *   p_hidden  nn.Dropout(hidden_dropout_prob): BertEmbeddings vilmodel_cmt.py:76, BertSelfOutput :152, BertOutput :191,
 *             BertXAttention output :363 (BertSelfOutput), panorama embedding :711, and the panorama
 *             TransformerEncoderLayer's dropout/dropout1/dropout2 + its MultiheadAttention dropout (common/ops.py:15,
 *             common/transformer.py:138-147,178-181);
 *   p_attn    attention_probs_dropout_prob on softmax probabilities (:127 self, :346 cross);
 *   p_head    ClsPrediction dropout (:657, pred_head_dropout_prob);
 *   p_env     the policy's drop_env on the RGB features (Policy_ViewSelection_ETP.py:102,345) fused into the operand
 *             cast of forward_panorama (0 = leave it to the caller, as the reference does).
 * Sequences beyond the fused attention kernels (Lq or Lk > 128; fp32 mode > 64, e.g. the 512-token RxR instruction) take
 * the batched-GEMM attention path, whose stash then carries a second probability buffer for the dropped copy. */
int etp_planner_set_dropout(etp_planner* p, float p_hidden, float p_attn, float p_head, float p_env, uint64_t seed);
/* Host-side view of the mask generator (tests, debugging): out_host[i] = multiplier (0 or 1/(1-p)) of element i (row-major
 * index into the site's tensor) at site (mode 1=txt 2=panorama 3=navigation, layer, slot) for step seed `seed`.  Slots:
 * 0 embedding output, 1 self-attention probabilities, 2 attention-output dense, 3 FFN-output dense, 4 FFN inner
 * (panorama layers), 5 cross-attention probabilities, 6 cross-attention-output dense, 7 SAP head, 8 drop_env.
 * Needs no GPU. */
int etp_dropout_multipliers(float p, uint64_t seed, int mode, int layer, int slot, int64_t n, float* out_host);
/* One dropout site at operator level: the five numbers of etp_dropout_multipliers.  The `_drop` entry points below are the plain
 * entry points of the same name with a trailing `const etp_drop_site*`; NULL or p == 0 is the plain call (the plain entry points
 * ARE these calls with NULL).  p in [0, 1), mode >= 0, layer >= 0, 0 <= slot < 16, otherwise ETP_ERR_INVALID and nothing is launched.
 * A backward call must name the site of its forward: the kernels regenerate the mask, none is stored.
 * Element index each kernel hands to the generator (the `i` of etp_dropout_multipliers), all 32-bit -- a site's tensor must stay
 * below 2^32 elements:
 *   text / panorama embedding, SAP tail   row * H + col of the [M, H] row tensor: y (forward) and dy (backward) of the two
 *                                         embeddings; the normalised row n of the SAP tail, forward and twice in its backward
 *                                         (dw2 += dl * dropout(n), dn = dl * w2 * mask)
 *   etp_ln_stream_bwd(_stage1)            row * H + col, on the operand copy dx_lp ONLY (dx, dgamma, dbeta stay undropped);
 *                                         refused unless dx_lp is given and is not dx
 *   etp_cast_f32_to                       the flat index
 *   etp_gemm                              row * N + col of the M x N product (never ldc), on the epilogue value: bias -> activation ->
 *                                         mask -> residual R -> store; Z of ETP_ACT_GELU_SAVEGRAD stays undropped, ETP_ACT_MUL_Z
 *                                         masks (alpha A B^T) * Z.  ksplit > 1 or batch > 1 with dropout is refused.
 *   etp_attn_*                            ((b * heads + h) * Lq + q) * Lk + key on the probabilities (never ldS): ctx = (P * mask) V,
 *                                         dV = (P * mask)^T dctx, dP = (dctx V^T) * mask; the stored P stays undropped.  The batched-GEMM
 *                                         family (etp_attn_family 0) writes the dropped copy to `Pd`, a second [B, heads, Lq, ldS]
 *                                         buffer the backward reads again; it refuses dropout without it.  The other families
 *                                         ignore `Pd`. */
typedef struct etp_drop_site { float p; uint64_t seed; int32_t mode, layer, slot; } etp_drop_site;
int etp_gemm_drop(const etp_gemm_desc* d, etp_stream_t stream, const etp_drop_site* drop);
int etp_attn_fwd_drop(const etp_attn_desc* d, etp_stream_t stream, void* Pd, const etp_drop_site* drop);
int etp_attn_bwd_drop(const etp_attn_bwd_desc* d, etp_stream_t stream, void* Pd, const etp_drop_site* drop);
int etp_attn_fwd_qkv_drop(const etp_attn_desc* d, const void* x, int64_t ldx, const void* w_qkv, int64_t ldw, const float* b_qkv,
                          etp_stream_t stream, const etp_drop_site* drop);
int etp_attn_bwd_proj_drop(const etp_attn_bwd_desc* d, const void* w_out, int64_t ldw, etp_stream_t stream, const etp_drop_site* drop);
int etp_ln_stream_bwd_drop(int dtype, const float* dy, const float* x, const float* stats, const float* gamma, const float* add,
                           float* dx, void* dx_lp, float* dgamma, float* dbeta, int M, int H, etp_stream_t stream,
                           const etp_drop_site* drop);
int etp_ln_stream_bwd_stage1_drop(int dtype, const float* dy, const float* x, const float* stats, const float* gamma,
                                  const float* add, float* dx, void* dx_lp, float* dgamma, float* dbeta, float* part, int M, int H,
                                  etp_stream_t stream, const etp_drop_site* drop);
int etp_text_embed_fwd_drop(int dtype, const int64_t* ids, const float* word, const float* pos, const float* type0,
                            const float* gamma, const float* beta, float* y, void* y_lp, float* stats, int B, int L, int H, float eps,
                            etp_stream_t stream, const etp_drop_site* drop);
int etp_text_embed_bwd_drop(int dtype, const float* dy, const int64_t* ids, const float* word, const float* pos, const float* type0,
                            const float* gamma, const float* stats, float* dword, float* dpos, float* dtype0, float* dgamma,
                            float* dbeta, int B, int L, int H, etp_stream_t stream, const etp_drop_site* drop);
int etp_pano_embed_fwd_drop(int dtype, const void* a, const void* d, const float* loc, const int64_t* nav, const float* const* params,
                            float* y, float* stats, int M, int H, etp_stream_t stream, const etp_drop_site* drop);
int etp_pano_embed_bwd_drop(int dtype, const float* dy, const void* a, const void* d, const float* loc, const int64_t* nav,
                            const float* stats, const float* const* params, float* const* grads, void* da, void* dd, int M, int H,
                            etp_stream_t stream, const etp_drop_site* drop);
int etp_sap_tail_fwd_drop(int dtype, const void* r, const float* gamma, const float* beta, const float* w2, const float* b2,
                          const uint8_t* visited, const uint8_t* valid, float* logits, float* stats, int M, int H,
                          etp_stream_t stream, const etp_drop_site* drop);
int etp_sap_tail_bwd_drop(int dtype, const float* dlogits, const void* r, const float* gamma, const float* beta, const float* w2,
                          const float* stats, const uint8_t* visited, const uint8_t* valid, void* dz, float* dgamma, float* dbeta,
                          float* dw2, float* db2, int M, int H, etp_stream_t stream, const etp_drop_site* drop);
int etp_cast_f32_to_drop(int dtype, const float* src, void* dst, int64_t n, etp_stream_t stream, const etp_drop_site* drop);
/* bf16 mode: refresh the bf16 shadow of the GEMM weights from the fp32 masters (autocast's per-step weight cast). */
int etp_planner_refresh_weights(etp_planner* p, etp_stream_t stream);
/* The same refresh for one consumer only, so a multi-stream step can put each cast on the stream that first needs it:
 * part 0 = text encoder (forward_txt), 1 = view projections + panorama encoder (forward_panorama), 2 = x-layers + SAP
 * head (forward_navigation).  The three parts tile the matrix region exactly. */
int etp_planner_refresh_part(etp_planner* p, int part, etp_stream_t stream);
/* bf16 shadow of the text encoder, layer 0 on `main` and layers >= 1 on `side`; the next etp_txt_fwd issued on `main` waits for
 * the side cast after its layer 0 (takes ~40 us of weight casting off the head of the dependent chain of a training step). */
int etp_planner_refresh_text_split(etp_planner* p, etp_stream_t main, etp_stream_t side);

/* ------------------------------------------------------------------------------------------------------
 * Waypoint predictor engine: BinaryDistPredictor_TRM.forward (vlnce_baselines/waypoint_pred/TRM_net.py:62-88, called first in
 * every rollout step, ss_trainer_ETP.py:825-830 -> Policy_ViewSelection_ETP.py:198-199) over one flat parameter arena.  Forward
 * only: the predictor is frozen and in eval() (ss_trainer_ETP.py:201-202,490,586,711).
 * ---------------------------------------------------------------------------------------------------- */
typedef struct etp_waypoint etp_waypoint;
etp_waypoint* etp_waypoint_create(int dtype);                /* ETP_F32 | ETP_BF16; NULL on error */
void etp_waypoint_destroy(etp_waypoint* w);
/* The parameter table: names are the keys of the reference module's state dict in its order (TRM_net.py:27-60), the two modules
 * the forward never uses (visual_merge, mergefeats_LayerNorm) included, so that a strict load sees every key.  offset: element
 * offset in the fp32 arena; the GEMM matrices lead it ([0, etp_waypoint_matrix_elems)) and have a bf16 shadow at the same offsets. */
int etp_waypoint_param_count(const etp_waypoint* w);
int etp_waypoint_param_info(const etp_waypoint* w, int i, etp_param_info* out);
int64_t etp_waypoint_arena_elems(const etp_waypoint* w);
int64_t etp_waypoint_matrix_elems(const etp_waypoint* w);
/* params: fp32 arena; shadow: bf16 copy of the matrix region (NULL in fp32 mode).  Both 256-byte aligned. */
int etp_waypoint_bind(etp_waypoint* w, float* params, void* shadow);
/* bf16 mode: shadow = bf16(params) over the matrix region (once after loading the checkpoint: the weights are frozen). */
int etp_waypoint_refresh_weights(etp_waypoint* w, etp_stream_t stream);
/* logits [B,120,12] fp32 (angle x distance, already rolled by HEATMAP_OFFSET = 5, TRM_net.py:83-86) from the depth encoder's
 * embeddings depth_feats [12*B, 2048] fp32 (nn.Flatten of [12*B,128,4,4], views of an episode in clockwise order; the rgb_feats
 * argument of the reference is ignored by it, TRM_net.py:65-72).  x = relu(fc(depth)); two post-LN BERT layers whose tokens attend
 * to their ring neighbours (etp_ring_attn_fwd, neighbor = TRM_NEIGHBOR = 1) with Q, K, V from one N = 2304 product; the two-layer
 * classifier; the roll.  Residual stream and LayerNorms fp32 in both modes; `dtype` selects the GEMM / attention operand precision.
 * ws: etp_waypoint_ws_bytes(w, B) bytes of caller-owned scratch, 256-byte aligned (one plan for the whole call).  18 launches in
 * fp32 mode, 20 in bf16 mode, whatever B is. */
int64_t etp_waypoint_ws_bytes(const etp_waypoint* w, int B);
int etp_waypoint_fwd(etp_waypoint* w, const float* depth_feats, int B, float* logits, void* ws, etp_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * CLIP ViT-B/32 view encoder: CLIPEncoder.forward (vlnce_baselines/models/encoders/resnet_encoders.py:244-278), the first GPU work of
 * every rollout step (`rgb_embedding = self.rgb_encoder(obs_view12)`, Policy_ViewSelection_ETP.py:138,195).  Forward only: the encoder
 * is frozen and in eval() (resnet_encoders.py:259-261).  S below is the image size: a multiple of 32 in 32 .. 224 (ViT-B/32: 224);
 * T = (S / 32)^2 + 1 tokens per image.  Every entry point returns ETP_ERR_INVALID before anything is launched for a NULL pointer, a
 * pointer not aligned to 16 bytes, S outside that set, or a non-positive image count.
 * ---------------------------------------------------------------------------------------------------- */
/* Replaces observations["rgb"].permute(0, 3, 1, 2), transforms.ConvertImageDtype(torch.float) and transforms.Normalize
 * (resnet_encoders.py:264-267,274-275), the unfold of conv1 (clip/model.py VisionTransformer.forward: stride = kernel = 32) and -- with
 * n_views == 12 -- the zero-filled rgb_batch and its 12 strided copies (Policy_ViewSelection_ETP.py:176-190).
 * views: host array of n_views device pointers to uint8 tensors.  n_views == 1: one tensor [B, S, S, 3], image b -> slot b.
 * n_views == 12: tensor a is view a of every episode, [B, S, S, 3]; view a of episode b -> slot (12 - a) % 12 + 12 b (clockwise order).
 * out [n_views B (S/32)^2, 3072] in `dtype`: row = slot (S/32)^2 + patch (row-major), column = c 1024 + ky 32 + kx (conv1.weight's own
 * order), value = (float(x) / 255 - mean[c]) / std[c] with each operation rounded in fp32 (bf16: then rounded to nearest even). */
int etp_clip_patch_rows(int dtype, const void* const* views, int n_views, int B, int S, void* out, etp_stream_t stream);
/* Replaces the class-token concatenation, `x + self.positional_embedding` and ln_pre (clip/model.py VisionTransformer.forward).
 * prod [N (T-1), 768] fp32 = patch rows . conv1.weight^T; class_embedding [768]; pos [T, 768]; x [N T, 768] fp32 (eps 1e-5 in CLIP). */
int etp_clip_tokens(const float* prod, const float* class_embedding, const float* pos, const float* gamma, const float* beta, float* x,
                    int N, int S, float eps, etp_stream_t stream);
/* Replaces QuickGELU (clip/model.py: x * torch.sigmoid(1.702 * x)) in place on n elements of `dtype`; n a positive multiple of 8.
 * -inf gives NaN and +inf gives +inf, as torch does. */
int etp_quick_gelu(int dtype, void* x, int64_t n, etp_stream_t stream);
/* Replaces `self.ln_post(x[:, 0, :])` (clip/model.py VisionTransformer.forward): row 0 of every image of x [N T, 768] fp32 ->
 * out [N, 768] in `dtype`. */
int etp_clip_cls_ln(int dtype, const float* x, const float* gamma, const float* beta, void* out, int N, int S, float eps,
                    etp_stream_t stream);

/* One parameter of a frozen encoder (rank <= 4).  name: CLIP: key of OpenAI CLIP's state dict without the leading "visual.";
 * depth: key of VlnResnetDepthEncoder.visual_encoder's state dict. */
typedef struct etp_tensor_info {
  char name[128];
  int32_t ndim; int64_t shape[4];
  int64_t offset;                        /* element offset in the fp32 arena (and, for the matrices, in the bf16 shadow / packed copy) */
} etp_tensor_info;
typedef etp_tensor_info etp_clip_tensor_info;

typedef struct etp_clip etp_clip;
/* dtype ETP_F32 | ETP_BF16 (GEMM / attention operand precision; the residual stream and the LayerNorms are fp32 in both);
 * image_size a multiple of 32 in 32 .. 224; layers 1 .. 12.  Width 768, 12 heads, patch 32, output 512 are fixed.  NULL on error. */
etp_clip* etp_clip_create(int dtype, int image_size, int layers);
void etp_clip_destroy(etp_clip* w);
/* The parameter table: OpenAI CLIP's visual.* keys in the order of its state dict, with its shapes (152 tensors, 87 849 216 parameters
 * at (224, 12)).  The GEMM matrices lead the arena ([0, etp_clip_matrix_elems)) and have a bf16 shadow at the same offsets; every
 * offset is a multiple of 64 elements. */
int etp_clip_param_count(const etp_clip* w);
int etp_clip_param_info(const etp_clip* w, int i, etp_clip_tensor_info* out);
int64_t etp_clip_arena_elems(const etp_clip* w);
int64_t etp_clip_matrix_elems(const etp_clip* w);
/* params: fp32 arena; shadow: bf16 copy of the matrix region (NULL in fp32 mode).  Both 256-byte aligned. */
int etp_clip_bind(etp_clip* w, float* params, void* shadow);
/* bf16 mode: shadow = bf16(params) over the matrix region (once after loading: the weights are frozen). */
int etp_clip_refresh_weights(etp_clip* w, etp_stream_t stream);
/* Replaces CLIPEncoder.forward (resnet_encoders.py:269-278 -> clip/model.py encode_image): views uint8 [N, S, S, 3] -> out [N, 512]
 * fp32.  ws: etp_clip_ws_bytes(w, N) bytes of caller-owned scratch, 256-byte aligned (one plan for the whole call).
 * 1 + 1 + 1 + 8 x layers + 2 launches, whatever N is. */
int64_t etp_clip_ws_bytes(const etp_clip* w, int N);
int etp_clip_fwd(etp_clip* w, const void* views, int N, float* out, void* ws, etp_stream_t stream);
/* The same on the rollout's 12 view tensors (host array of 12 device pointers, each uint8 [B, S, S, 3]): replaces the rgb half of
 * Policy_ViewSelection_ETP.py:176-195.  out [12 B, 512] in clockwise order; ws for N = 12 B. */
int etp_clip_fwd_views(etp_clip* w, const void* const* views, int B, float* out, void* ws, etp_stream_t stream);
/* Test aid: with a device buffer of 3 x N T x 768 fp32 installed, the following calls also copy the residual stream after ln_pre,
 * after layer 0 and after the last layer into it (three more launches).  NULL removes it. */
int etp_clip_set_probe(etp_clip* w, float* probe);

/* ------------------------------------------------------------------------------------------------------
 * DD-PPO ResNet-50 depth encoder: VlnResnetDepthEncoder.forward (vlnce_baselines/models/encoders/resnet_encoders.py:13-107; habitat-lab
 * rl/ddppo/policy/resnet.py and resnet_policy.py::ResNetEncoder with baseplanes 32, ngroups 16, no input normalisation,
 * spatial_output False), `depth_embedding = self.depth_encoder(obs_view12)` of every rollout step (Policy_ViewSelection_ETP.py:194).
 * Forward only: the encoder is frozen.  Activations are NHWC (a pixel's channels are contiguous).  Every entry point returns
 * ETP_ERR_INVALID before anything is launched for a NULL pointer, a pointer not aligned to 16 bytes, a size outside its set, or a tensor of
 * 2^31 elements or more.
 * ---------------------------------------------------------------------------------------------------- */
/* Replaces observations["depth"].permute(0, 3, 1, 2), F.avg_pool2d(x, 2) (resnet_policy.py ResNetEncoder.forward), backbone.conv1[0]
 * (Conv2d(1, bp, 7, stride 2, pad 3, no bias)) and -- with n_views == 12 -- the zero-filled depth_batch and its 12 strided copies
 * (Policy_ViewSelection_ETP.py:176-190).  views: host array of n_views device pointers to fp32 tensors.  n_views == 1: one tensor
 * [B, S, S, 1], image b -> slot b.  n_views == 12: tensor a is view a of every episode; view a of episode b -> slot (12 - a) % 12 + 12 b.
 * S a multiple of 64 in 64 .. 256, base_planes 16 | 32, weight [bp, 1, 7, 7] fp32, out [n_views B, S/4, S/4, bp] fp32 (pre-norm).
 * Pooled pixel = ((a + b) + (c + d)) * 0.25 over its 2x2 block (rows first); output = the 49 taps in (ky, kx) order, one fused
 * multiply-add each, zeros outside the pooled image. */
int etp_depth_stem(const void* const* views, int n_views, int B, int S, int base_planes, const float* weight, float* out,
                   etp_stream_t stream);
/* GroupNorm statistics of x [N, HW, C] fp32 (groups of consecutive channels, biased variance): stats [N, groups, 2] = mean,
 * 1 / sqrt(var + eps).  Two passes, the second around the mean; deterministic, no atomics.  C a multiple of 4, at most 2048; groups at
 * most 64. */
int etp_gn_stats(const float* x, float* stats, int N, int HW, int C, int groups, float eps, etp_stream_t stream);
/* y = ((x - mean) * rstd) * gamma + beta in fp32, + residual (fp32), ReLU when relu != 0, rounded once.  res_kind 0: none; 1: res is a
 * finished tensor [N, HW, C] in `dtype`; 2: res is a second pre-norm fp32 tensor normalised with stats2 / gamma2 / beta2 (the downsample
 * branch of a bottleneck block).  nchw == 0: out [N, HW, C] in `dtype`; nchw != 0: out [N, C, HW] fp32. */
int etp_gn_apply(int dtype, const float* x, const float* stats, const float* gamma, const float* beta, int res_kind, const void* res,
                 const float* stats2, const float* gamma2, const float* beta2, int relu, int nchw, void* out, int N, int HW, int C,
                 int groups, etp_stream_t stream);
/* MaxPool2d(3, stride 2, pad 1) on x [N, H, W, C] in `dtype` -> out [N, (H - 1) / 2 + 1, (W - 1) / 2 + 1, C].  Padding is -inf: taps
 * outside the image are skipped (equivalent to 0 behind a ReLU).  C a multiple of 8. */
int etp_maxpool3x3s2(int dtype, const void* x, void* out, int N, int H, int W, int C, etp_stream_t stream);
/* im2col: x [N, H, W, C] in `dtype` -> rows [N Ho Wo, k k C], column = (ky k + kx) C + c, zeros where the window leaves the image;
 * k 1 | 3, stride 1 | 2, pad (k - 1) / 2, Ho = (H + 2 pad - k) / stride + 1.  k == 1 with stride 2 is the row gather of the strided
 * downsample.  C a multiple of 8. */
int etp_conv_rows(int dtype, const void* x, void* out, int N, int H, int W, int C, int k, int stride, etp_stream_t stream);

typedef etp_tensor_info etp_depth_tensor_info;

typedef struct etp_depth etp_depth;
/* dtype ETP_F32 | ETP_BF16 (GEMM operand and activation precision; every product and every GroupNorm computes in fp32); image_size a
 * multiple of 64 in 64 .. 256; base_planes 16 | 32 (groups = base_planes / 2); blocks[4] each 1 .. 6.  The shipped network is
 * (256, 32, {3, 4, 6, 3}); the rest exists so that tests can be small.  Output channels Cc = round(2048 / (image_size / 64)^2).
 * NULL on error. */
etp_depth* etp_depth_create(int dtype, int image_size, int base_planes, const int* blocks);
void etp_depth_destroy(etp_depth* w);
/* The parameter table: the state dict's keys in its order, with its shapes (162 tensors, 7 069 408 parameters at the shipped size).  The
 * GEMM matrices (every convolution but the stem's) lead the arena ([0, etp_depth_matrix_elems)); every offset is a multiple of 64. */
int etp_depth_param_count(const etp_depth* w);
int etp_depth_param_info(const etp_depth* w, int i, etp_depth_tensor_info* out);
int64_t etp_depth_arena_elems(const etp_depth* w);
int64_t etp_depth_matrix_elems(const etp_depth* w);
int etp_depth_out_channels(const etp_depth* w);
/* params: fp32 arena; packed: etp_depth_matrix_elems elements of `dtype`, the GEMM-ready copy (both modes).  Both 256-byte aligned. */
int etp_depth_bind(etp_depth* w, float* params, void* packed);
/* packed = the matrices in `dtype` at the arena's offsets, 3x3 weights permuted from [Cout, Cin, 3, 3] to [Cout, ky, kx, Cin], 1x1 weights
 * as they are (one launch per matrix; needed once after loading: the weights are frozen). */
int etp_depth_refresh_weights(etp_depth* w, etp_stream_t stream);
/* Replaces VlnResnetDepthEncoder.forward (resnet_encoders.py:77-107): depth fp32 [N, S, S, 1] -> out [N, Cc, S/64, S/64] fp32, NCHW
 * ([N, 128, 4, 4] at the shipped size).  ws: etp_depth_ws_bytes(w, N) bytes of caller-owned scratch, 256-byte aligned (one plan for the
 * whole call, buffers reused across layers).  19 + 10 x (number of blocks) launches (179 at the shipped size), whatever N is; no
 * allocation, no synchronisation. */
int64_t etp_depth_ws_bytes(const etp_depth* w, int N);
int etp_depth_fwd(etp_depth* w, const float* depth, int N, float* out, void* ws, etp_stream_t stream);
/* The same on the rollout's 12 view tensors (host array of 12 device pointers, each fp32 [B, S, S, 1]): replaces the depth half of
 * Policy_ViewSelection_ETP.py:176-194.  out [12 B, Cc, S/64, S/64] in clockwise order; ws for N = 12 B. */
int etp_depth_fwd_views(etp_depth* w, const void* const* views, int B, float* out, void* ws, etp_stream_t stream);
/* Test aid: with a device buffer installed, the following calls also copy (as fp32, NHWC, back to back) the activations after the
 * max-pool [N, S/8, S/8, bp], after layer1 [N, S/8, S/8, 4 bp] and after layer4 [N, S/64, S/64, 32 bp] into it (three more launches).
 * NULL removes it. */
int etp_depth_set_probe(etp_depth* w, float* probe);

/* Activations that cross these entry points (txt_embeds, pano_embeds, gmap_img_fts, gmap_embeds and their gradients) are
 * fp32 in BOTH modes, as they are under the reference's autocast (outputs of fp32 LayerNorms); `dtype` only selects the
 * GEMM / attention operand precision inside. */
int64_t etp_txt_stash_bytes(const etp_planner* p, int B, int L);
int64_t etp_txt_ws_bytes(const etp_planner* p, int B, int L);
int etp_txt_fwd(etp_planner* p, const int64_t* txt_ids, const uint8_t* txt_masks, int B, int L, float* txt_embeds /*[B,L,H]*/,
                void* stash, etp_stream_t stream);
int etp_txt_bwd(etp_planner* p, const float* d_txt_embeds, const int64_t* txt_ids, const uint8_t* txt_masks, int B, int L,
                void* stash, void* ws, etp_stream_t stream);

/* Same, restricted to text layers [layer_lo, layer_hi) (call with descending ranges and the same ws: the running gradient is
 * kept in ws).  The first call (layer_hi = n_l) reads d_txt_embeds, the last (layer_lo = 0) also runs the embedding backward.
 * Lets a data-parallel caller all-reduce the gradients of finished layers while earlier layers are still in backward. */
int etp_txt_bwd_range(etp_planner* p, const float* d_txt_embeds, const int64_t* txt_ids, const uint8_t* txt_masks, int B, int L,
                      void* stash, void* ws, int layer_lo, int layer_hi, etp_stream_t stream);

int64_t etp_pano_stash_bytes(const etp_planner* p, int B, int V);
int64_t etp_pano_ws_bytes(const etp_planner* p, int B, int V);
int etp_pano_fwd(etp_planner* p, const float* rgb, const float* dep, const float* loc, const int64_t* nav_types,
                 const int64_t* view_lens, int B, int V, float* pano_embeds /*[B,V,H]*/, uint8_t* pano_masks /*[B,V]*/,
                 void* stash, etp_stream_t stream);
int etp_pano_bwd(etp_planner* p, const float* d_pano_embeds, const float* rgb, const float* dep, const float* loc,
                 const int64_t* nav_types, int B, int V, float* d_rgb /*[B,V,img_feat] or NULL*/, void* stash, void* ws,
                 etp_stream_t stream);

int64_t etp_nav_stash_bytes(const etp_planner* p, int B, int L, int G);
int64_t etp_nav_ws_bytes(const etp_planner* p, int B, int L, int G);
int etp_nav_fwd(etp_planner* p, const float* txt_embeds, const uint8_t* txt_masks, const int64_t* gmap_step_ids,
                const float* gmap_img_fts, const float* gmap_pos_fts, const uint8_t* gmap_masks,
                const uint8_t* gmap_visited_masks, const float* gmap_pair_dists, int B, int L, int G,
                float* gmap_embeds /*[B,G,H]*/, float* global_logits /*[B,G]*/, void* stash, etp_stream_t stream);
int etp_nav_bwd(etp_planner* p, const float* d_gmap_embeds /*or NULL*/, const float* d_logits /*or NULL*/,
                const float* txt_embeds, const uint8_t* txt_masks, const int64_t* gmap_step_ids, const float* gmap_pos_fts,
                const uint8_t* gmap_masks, const uint8_t* gmap_visited_masks, const float* gmap_pair_dists, int B, int L, int G,
                float* d_txt_embeds /*[B,L,H], overwritten*/, float* d_gmap_img_fts /*[B,G,H], overwritten*/, void* stash,
                void* ws, etp_stream_t stream);

/* Text K/V cache for rollouts.  The instruction is fixed for an episode, but BertOutAttention
 * (vilmodel_cmt.py:326-328) re-projects it to keys/values in every x-layer at every step (GraphLXRTXLayer :387-389 called
 * from the per-step loop ss_trainer_ETP.py:819-892).  Compute the projections once per episode batch and reuse them:
 *   etp_nav_kv_fwd   txt_embeds -> cache (caller-owned, etp_nav_kv_bytes): [bf16 text | K|V of x-layer 0 | ... ]
 *   etp_nav_fwd_kv   = etp_nav_fwd reading keys/values from the cache (identical results)
 *   etp_nav_bwd_kv   = etp_nav_bwd, except that dK|dV of each x-layer are WRITTEN to d_kv [n_x][B*L][2H] (operand dtype,
 *                      etp_nav_kv_grad_elems elements) instead of being projected back immediately
 *   etp_nav_kv_bwd   once per episode: d_kv summed over the steps -> gradients of the K/V weights and d_txt_embeds. */
int64_t etp_nav_kv_bytes(const etp_planner* p, int B, int L);
int64_t etp_nav_kv_grad_elems(const etp_planner* p, int B, int L);
int64_t etp_nav_kv_offset(const etp_planner* p, int B, int L);   /* byte offset of the K|V blocks (contiguous, layer-major) */
int etp_nav_kv_fwd(etp_planner* p, const float* txt_embeds, int B, int L, void* kv_cache, etp_stream_t stream);
int etp_nav_kv_bwd(etp_planner* p, const float* txt_embeds, const void* d_kv, int B, int L, const void* kv_cache,
                   float* d_txt_embeds /*[B,L,H], overwritten*/, etp_stream_t stream);
/* The cache under the batched rollout call (T steps stacked along the batch axis, episode t*Bt + b reads instruction b; the
 * reference re-projects the same instruction at every step, ss_trainer_ETP.py:819-822 -> vilmodel_cmt.py:326-328):
 *   etp_nav_kv_repeat     K|V blocks of a Bt-instruction cache replicated T times into a cache sized for T*Bt episodes
 *                         (etp_nav_kv_bytes(p, T*Bt, L)) -- a copy in place of T projections of the same rows
 *   etp_nav_kv_sum_steps  d_kv of the stacked call [n_x][T*Bt*L][2H] summed over the steps (fp32 accumulation) into
 *                         [n_x][Bt*L][2H], the operand of etp_nav_kv_bwd */
int etp_nav_kv_repeat(etp_planner* p, const void* kv_cache, int Bt, int L, int T, void* kv_cache_steps, etp_stream_t stream);
int etp_nav_kv_sum_steps(etp_planner* p, const void* d_kv_steps, int Bt, int L, int T, void* d_kv, etp_stream_t stream);
int etp_nav_fwd_kv(etp_planner* p, const void* kv_cache, const uint8_t* txt_masks, const int64_t* gmap_step_ids,
                   const float* gmap_img_fts, const float* gmap_pos_fts, const uint8_t* gmap_masks,
                   const uint8_t* gmap_visited_masks, const float* gmap_pair_dists, int B, int L, int G, float* gmap_embeds,
                   float* global_logits, void* stash, etp_stream_t stream);
int etp_nav_bwd_kv(etp_planner* p, const float* d_gmap_embeds /*or NULL*/, const float* d_logits /*or NULL*/,
                   const void* kv_cache, const uint8_t* txt_masks, const int64_t* gmap_step_ids, const float* gmap_pos_fts,
                   const uint8_t* gmap_masks, const uint8_t* gmap_visited_masks, const float* gmap_pair_dists, int B, int L,
                   int G, void* d_kv /*overwritten*/, float* d_gmap_img_fts, void* stash, void* ws, etp_stream_t stream);
/* The same two calls with PER-EPISODE INDIRECTION instead of the replicated copy (round 6; N1): B = T * Bt stacked episodes, `kv_cache`
 * (etp_nav_kv_bytes(p, Bt, L)) and `txt_masks` [Bt, L] hold the Bt instructions once, and episode e reads the keys / values / key mask
 * of instruction e % Bt inside the cross-attention kernels (vilmodel_cmt.py:326-328 with the same txt_embeds at every step,
 * ss_trainer_ETP.py:819-822).
 *   etp_nav_kv_steps_mode     host only, launches nothing: how this shape is served under the current switches, from the kernel family
 *                             of the cross-attention descriptor (etp_attn_family's helper):
 *                               0  no indirection (fp32, a switch off): use etp_nav_kv_repeat + the calls above
 *                               1  register-resident kernels (bf16, L and G <= 128): etp_nav_bwd_kv_steps, d_kv per stacked episode
 *                                  [n_x][B*L][2H], summed over the steps by the caller with etp_nav_kv_sum_steps
 *                               2  streaming kernels (bf16, L or G > 128, e.g. RxR's 512-token instructions): etp_nav_bwd_kv_steps_sum,
 *                                  d_kv [n_x][Bt*L][2H] already summed over the steps inside the dK/dV kernel (the sum autograd forms in
 *                                  the shared txt_embeds, ss_trainer_ETP.py:1055) -- no per-step gradient buffer, no reduction launch
 *   etp_nav_fwd_kv_steps      every shape whose mode is not 0; otherwise ETP_ERR_INVALID
 *   etp_nav_bwd_kv_steps      mode 1; mode 2 fails with ETP_ERR_INVALID and names etp_nav_bwd_kv_steps_sum
 *   etp_nav_bwd_kv_steps_sum  mode 2; the arguments of etp_nav_bwd_kv_steps except for the shape of d_kv */
int etp_nav_kv_steps_mode(const etp_planner* p, int B, int L, int G, int Bt);
int etp_nav_fwd_kv_steps(etp_planner* p, const void* kv_cache, const uint8_t* txt_masks, const int64_t* gmap_step_ids,
                         const float* gmap_img_fts, const float* gmap_pos_fts, const uint8_t* gmap_masks,
                         const uint8_t* gmap_visited_masks, const float* gmap_pair_dists, int B, int L, int G, int Bt,
                         float* gmap_embeds, float* global_logits, void* stash, etp_stream_t stream);
int etp_nav_bwd_kv_steps(etp_planner* p, const float* d_gmap_embeds /*or NULL*/, const float* d_logits /*or NULL*/,
                         const void* kv_cache, const uint8_t* txt_masks, const int64_t* gmap_step_ids, const float* gmap_pos_fts,
                         const uint8_t* gmap_masks, const uint8_t* gmap_visited_masks, const float* gmap_pair_dists, int B, int L,
                         int G, int Bt, void* d_kv /*[n_x][B*L][2H], overwritten*/, float* d_gmap_img_fts, void* stash, void* ws,
                         etp_stream_t stream);
int etp_nav_bwd_kv_steps_sum(etp_planner* p, const float* d_gmap_embeds /*or NULL*/, const float* d_logits /*or NULL*/,
                             const void* kv_cache, const uint8_t* txt_masks, const int64_t* gmap_step_ids, const float* gmap_pos_fts,
                             const uint8_t* gmap_masks, const uint8_t* gmap_visited_masks, const float* gmap_pair_dists, int B,
                             int L, int G, int Bt, void* d_kv /*[n_x][Bt*L][2H], overwritten*/, float* d_gmap_img_fts, void* stash,
                             void* ws, etp_stream_t stream);

/* Device-side graph-input assembly: everything RLTrainer._nav_gmap_variable computes on the host
 * besides the node embeddings (ss_trainer_ETP.py:344-417) -- all-pairs shortest paths over the visited-node graph
 * (GraphMap.update_graph's networkx Dijkstra, graph_utils.py:256-257), nearest front of each ghost (:259-270), the 7-d
 * position features of GraphMap.get_pos_fts (:278-322), step ids, masks and the pairwise distance matrix (:371-387) --
 * from compact per-episode arrays.  One workgroup per episode; <= 64 visited nodes and <= 192 ghosts per episode.
 *   node_pos [B,Nmax,3], node_step [B,Nmax], n_nodes [B], adj [B,Nmax,Nmax] (edge length, < 0 = no edge, symmetric),
 *   ghost_pos [B,Mmax,3] (ghost_aug_pos), n_ghost [B], front_ptr [B,Mmax+1] + front_idx [B,Fmax] (CSR per episode: node
 *   indices of each ghost's fronts, in the reference's list order), cur_node [B], cur_pos [B,3], cur_heading [B] (radians;
 *   heading_from_quaternion stays with the caller).  Outputs padded to G >= 1 + n_nodes + n_ghost entries per episode,
 *   ordered [stop], visited nodes, ghosts: gmap_step_ids [B,G] i64, gmap_masks / gmap_visited_masks [B,G] u8,
 *   gmap_pos_fts [B,G,7] f32, gmap_pair_dists [B,G,G] f32. */
int etp_gmap_assemble(const float* node_pos, const int32_t* node_step, const int32_t* n_nodes, const float* adj,
                      const float* ghost_pos, const int32_t* n_ghost, const int32_t* front_ptr, const int32_t* front_idx,
                      const int32_t* cur_node, const float* cur_pos, const float* cur_heading, int B, int Nmax, int Mmax,
                      int Fmax, int G, int64_t* gmap_step_ids, uint8_t* gmap_masks, uint8_t* gmap_visited_masks,
                      float* gmap_pos_fts, float* gmap_pair_dists, etp_stream_t stream);

/* RLTrainer._vp_feature_variable (ss_trainer_ETP.py:308-342): out[b] = [candidate-view features (K_b rows) ; panorama
 * views whose index is not a candidate's image, in index order], zero-padded to V rows; nav_types 1 for the candidate rows
 * (NULL to skip), view_lens[b] = K_b + #free views (NULL to skip).  cand_fts packed [sum K, F] with cand_ptr [B+1];
 * pano_fts [B,P,F] with pano_batch_stride = P*F, or one shared [P,F] table with stride 0 (pano_angle_fts); cand_mask [B,P]
 * (non-zero = the view is a candidate's image).  cand_fts is not read, and may be NULL, when sum K = 0.
 * PRECONDITION: V >= K_b + #free views for every episode (the caller sizes V from the batch maximum, graph_inputs.py).  With a
 * smaller V nothing is written out of bounds, but the rows of the episode beyond V are dropped while view_lens[b] still reports the
 * untruncated length: the outputs no longer describe each other, and no caller may rely on that case. */
int etp_vp_gather(const float* cand_fts, const int32_t* cand_ptr, const float* pano_fts, int64_t pano_batch_stride,
                  const uint8_t* cand_mask, int B, int P, int F, int V, float* out_fts, int64_t* nav_types, int64_t* view_lens,
                  etp_stream_t stream);

/* The rollout decision: from the node logits of forward_navigation to everything envs.step needs, in one launch
 * (vlnce_baselines/ss_trainer_ETP.py:880-977; GraphMap.shortest_path / front_to_ghost_dist / node_stop_scores,
 * vlnce_baselines/models/graph_utils.py:161,256,259-270).  One workgroup per episode b; n = n_nodes[b], m = n_ghost[b]:
 *   node_pos, n_nodes, adj, ghost_pos, n_ghost, front_ptr, front_idx, cur_node: the compact arrays of etp_gmap_assemble (same
 *     layout, same limits: Nmax <= 64, Mmax <= 192, so G <= 257); ghost arrays may be NULL when Mmax == 0.
 *   logits [B,G] fp32 (global_logits; entries past 1 + n + m are expected to be -inf, as the masks make them).
 *   slot [B]: the episode's row of stop_scores = its original environment index (the reference pops paused environments,
 *     :1036-1044; rows of other slots are never touched).  Slots of one call must differ.
 *   stop_scores [S,64] fp32, device resident for the whole rollout, -inf at its start: GraphMap.node_stop_scores.
 *   uniforms [B,2] fp32 in [0,1) or NULL; teacher [B] int64 or NULL; sample_ratio; force_stop (stepk == max_len - 1, :909).
 * Steps:
 *   1. p = softmax(logits[b]) in fp32 with the row maximum subtracted (expf; a -inf logit gives exactly 0); stop_prob = p[0]
 *      (:880-882).  The sum is a tree: <= 2 entries per thread, a 64-lane butterfly, four wave sums -- an addition chain of 10.
 *   2. greedy = arg-max of the logits, the LOWEST index among equal maxima (:900, torch's rule).
 *   3. action: uniforms NULL -> greedy.  Otherwise (:896-898) the inverse CDF at u0 = uniforms[b,0]: the first index whose inclusive
 *      prefix sum of p, added serially in index order, exceeds u0 * total (total = the same serial sum) -- the convention of
 *      etp_waypoint_tail; it reproduces the distribution of torch.distributions.Categorical, not its random stream -- clamped to the
 *      last index with p > 0; then, if teacher is given and u1 = uniforms[b,1] <= sample_ratio, the teacher label as it is
 *      (ignore_index included; labels outside int32 become INT32_MIN).
 *   4. stop_scores[slot[b], cur_node[b]] = stop_prob; stop_node = arg-max of stop_scores[slot[b], 0 .. n-1], the LOWEST index among
 *      equal maxima (np.argmax over the insertion-ordered dict, :911-913).
 *   5. stop if action == 0 or force_stop or m == 0 (:909).  Otherwise ghost = action - 1 - n and front = that ghost's nearest
 *      front, the FIRST minimum in list order (graph_utils.py:259-270), by the arithmetic etp_gmap_assemble uses (one shared device
 *      function).  A non-stop action outside [1 + n, 1 + n + m) sets ETP_DECIDE_ERR_ACTION.
 *   6. target = stop_node on a stop, front otherwise; path = the shortest path cur_node -> target over the visited-node graph
 *      without its first node (:916-917, 958-959; length 0 when target == cur_node); among equally short paths the predecessor with
 *      the lowest index wins at every node.  An unreachable target sets ETP_DECIDE_ERR_UNREACHABLE.
 * record [B, ETP_DECIDE_HDR + Nmax] int32, one contiguous row per episode:
 *   [0] action  [1] greedy action  [2] flags (ETP_DECIDE_*)  [3] stop node  [4] target node (-1: none)  [5] ghost (-1 on a stop)
 *   [6] path length  [7] the bits of stop_prob (fp32)  [8 ..] the path's node indices, -1 beyond its length.
 *   An episode whose n, m, cur_node, slot or fronts are out of range, or with 1 + n + m > G, gets ETP_DECIDE_ERR_INPUT, -1 in the
 *   other fields, and its table row is left alone.  The host raises on any error flag.
 * Plain stores only, no atomics: a second run from the same table state returns the same bits.
 * ETP_ERR_INVALID before anything is launched: B <= 0; G outside 1 .. 257, Nmax outside 1 .. 64, Mmax outside 0 .. 192; a NULL table
 * or S <= 0; a NULL required operand; uniforms without teacher while sample_ratio > 0; an fp32 / int32 operand not 4-byte aligned or
 * teacher not 8-byte aligned. */
#define ETP_DECIDE_HDR 8
#define ETP_DECIDE_STOP 1
#define ETP_DECIDE_ERR_ACTION 2
#define ETP_DECIDE_ERR_UNREACHABLE 4
#define ETP_DECIDE_ERR_INPUT 8
int etp_nav_decide(const float* logits, const float* node_pos, const int32_t* n_nodes, const float* adj, const float* ghost_pos,
                   const int32_t* n_ghost, const int32_t* front_ptr, const int32_t* front_idx, const int32_t* cur_node,
                   const int32_t* slot, const float* uniforms, const int64_t* teacher, float sample_ratio, int force_stop, int B,
                   int Nmax, int Mmax, int Fmax, int G, float* stop_scores, int S, int32_t* record, etp_stream_t stream);

/* The topological map on the device (csrc/gmap_update.hip): GraphMap.update_graph (vlnce_baselines/models/graph_utils.py:193-254)
 * with _localize (:163-175) and delete_ghost (:185-191; consume_ghost, vlnce_baselines/ss_trainer_ETP.py:976-977) in one launch, on
 * state that stays on the device.
 * state: S records of etp_gmap_slot_bytes() bytes, 16-byte aligned, one per ORIGINAL environment (the convention of etp_nav_decide's
 *   stop-score table); opaque apart from that stride.  A record holds <= 64 visited nodes, <= 192 ghosts and <= ETP_GMAP_FMAX absorbed
 *   candidates; positions and the ghosts' running sums and means are double.  etp_gmap_reset empties the n given slots (a slot must be
 *   reset before its first update; slots out of range are skipped).  A call never writes the record of a slot it was not given.
 * etp_gmap_update, one workgroup per episode b (slots of one call must differ):
 *   slot [B]; prev_node [B] (node index, -1: none); step_id [B]; cur_pos [B,3] f64; cur_heading [B] f32; cand_pos [B,Kmax,3] f64
 *   (estimate_cand_pos, :61-71, stays on the host: sin / cos there keep numpy's bits); n_cand [B] in 0 .. Kmax; cur_row [B] and
 *   cand_row [B,Kmax]: rows of the embedding store; del_ghost [B]: a ghost's index in the current order, or -1; noise [B,192,3] f64
 *   standard normals or NULL; loc_noise, merge_ghost, ghost_aug: GraphMap's constructor arguments.
 *   1. del_ghost >= 0: that ghost and everything it absorbed leave; the remaining ghosts keep their order.
 *   2. the visited node is appended (index n): position, step_id, cur_row; edge prev_node - n of Euclidean length (:199-202).
 *   3. every candidate in order (:208-246): the nearest visited node, the new one included (the FIRST minimum in insertion order, a
 *      distance below 10000); if its distance is <= loc_noise the edge (n, that node) is set to the distance between the two NODES.
 *      Otherwise, with merge_ghost, the nearest ghost MEAN by the same rule, the means as the previous candidate left them: the
 *      candidate joins it (sum += position, mean = sum / count, front n and the row appended; duplicate fronts are kept).  Otherwise
 *      a new ghost with id ghost_cnt++ at the end of the order.
 *   4. ghost_aug_pos = mean + clip(noise * (aug, 0, aug), +-aug) for every ghost when ghost_aug != 0 and noise is given (:248-254:
 *      the distribution of np.random.normal, not its stream), the mean otherwise.
 *   5. outputs, in BATCH order, fp32 / int32, padded as graph_inputs.pack_batch pads them, with the FIXED strides Nmax = 64, Mmax = 192,
 *      Fmax = ETP_GMAP_FMAX: node_pos [B,64,3], node_step [B,64], n_nodes [B], adj [B,64,64], ghost_pos [B,192,3] (the aug positions),
 *      n_ghost [B], front_ptr [B,193], front_idx [B,ETP_GMAP_FMAX], cur_node [B] (= the new node), cur_pos [B,3], cur_heading [B]:
 *      the operands of etp_gmap_assemble and etp_nav_decide.
 *   6. record [B, ETP_GMAP_HDR + Kmax] int32: [0] nodes  [1] ghosts  [2] flags (ETP_GMAP_ERR_*)  [3] the new node  [4] ghost_cnt
 *      [5] absorbed candidates held  [6] [7] 0;  then per candidate (kind << 24) | target: ETP_GMAP_EDGE with the node index,
 *      ETP_GMAP_NEW / ETP_GMAP_MERGED with the ghost's id; -1 beyond n_cand.
 *   Every operation on positions is one correctly rounded double operation in numpy's order (the file is compiled with contraction
 *   off): (dx*dx + dy*dy) + dz*dz, one sqrt, sum / count.  Edge lengths are rounded to fp32 once, when they are set.
 *   Before anything is changed, with n, m, f the slot's nodes, ghosts and absorbed candidates after the deletion: n + 1 > 64,
 *   m + n_cand > 192 or f + n_cand > ETP_GMAP_FMAX (as if nothing merged) gives ETP_GMAP_ERR_CAPACITY; a slot outside 0 .. S-1, n_cand
 *   outside 0 .. Kmax, prev_node outside -1 .. n-1, del_ghost outside -1 .. m-1 or a record whose counts are out of range gives
 *   ETP_GMAP_ERR_INPUT.  Either way the slot's record stays as it was, the flags go to record[b,2] and the episode's outputs are
 *   those of an empty map (n_nodes = n_ghost = 0).  Plain stores, no atomics: the same state and inputs give the same bits.
 *   ETP_ERR_INVALID before anything is launched: a NULL operand (noise excepted), B <= 0, S <= 0, Kmax outside 1 .. 16, a state not
 *   16-byte aligned, an fp64 operand not 8-byte or an fp32 / int32 operand not 4-byte aligned.
 * etp_gmap_embed_csr: the CSR of graph_inputs.pack_img_csr from the states (get_node_embeds, graph_utils.py:272-276;
 *   ss_trainer_ETP.py:360-365) in three launches, no atomics, no host synchronisation.  Forward, over the [B*G] padded entry list
 *   ([stop], nodes, ghosts, padding): ptr_f [B*G+1], idx_f / w_f (room for the sum of nodes + absorbed candidates; at most
 *   B * (64 + ETP_GMAP_FMAX)); a node is its row with weight 1, a ghost its absorbed rows in absorption order with weight 1/count.
 *   Transposed, over the store rows 0 .. R-1: ptr_b [R+1], idx_b / w_b with room for R entries (a store row has at most one owner
 *   among the episodes of the call; the owner map is built in idx_b / w_b and compacted in place).  status [B]: 0, or
 *   ETP_GMAP_ERR_CAPACITY when G < 1 + nodes + ghosts, ETP_GMAP_ERR_INPUT for a slot out of range or a record whose counts are out of
 *   range (never reset) -- either way the episode comes out empty and nothing of the record is indexed --,
 *   ETP_GMAP_ERR_ROW when a stored row lies outside 0 .. R-1 (it is replaced by row 0 with weight 0).  ETP_ERR_INVALID before
 *   anything is launched: a NULL or misaligned operand, B, S or R <= 0, G outside 1 .. 257. */
#define ETP_GMAP_FMAX 512
#define ETP_GMAP_HDR 8
#define ETP_GMAP_ERR_CAPACITY 1
#define ETP_GMAP_ERR_INPUT 2
#define ETP_GMAP_ERR_ROW 4
#define ETP_GMAP_EDGE 1
#define ETP_GMAP_NEW 2
#define ETP_GMAP_MERGED 3
int64_t etp_gmap_slot_bytes(void);
int etp_gmap_reset(void* state, int S, const int32_t* slots, int n, etp_stream_t stream);
int etp_gmap_update(void* state, int S, const int32_t* slot, const int32_t* prev_node, const int32_t* step_id, const double* cur_pos,
                    const float* cur_heading, const double* cand_pos, const int32_t* n_cand, const int32_t* cur_row,
                    const int32_t* cand_row, const int32_t* del_ghost, const double* noise, double loc_noise, int merge_ghost,
                    double ghost_aug, int B, int Kmax, float* node_pos, int32_t* node_step, int32_t* n_nodes, float* adj,
                    float* ghost_pos, int32_t* n_ghost, int32_t* front_ptr, int32_t* front_idx, int32_t* cur_node, float* cur_pos_out,
                    float* cur_heading_out, int32_t* record, etp_stream_t stream);
int etp_gmap_embed_csr(const void* state, int S, const int32_t* slot, int B, int G, int R, int32_t* ptr_f, int32_t* idx_f, float* w_f,
                       int32_t* ptr_b, int32_t* idx_b, float* w_b, int32_t* status, etp_stream_t stream);

/* The embedding store's rows from the panorama encoder's output (csrc/pano_store.hip): the masked panorama mean and the candidate
 * selection of vlnce_baselines/ss_trainer_ETP.py:838-839, 864-869, laid down as the rows that GraphMap.update_graph keeps
 * (vlnce_baselines/models/graph_utils.py:206,224,233) and that etp_gmap_update / etp_gmap_embed_csr / etp_gather_sum index.
 * etp_pano_store_fwd, one launch: pano_embeds [B,V,H] fp32 (etp_pano_fwd's output), pano_masks [B,V] u8, nav_types [B,V] int64,
 *   row_base [B] and n_cand [B] int32, store [R,H] fp32, status [B] int32.  For episode b
 *     store[row_base[b]]          = (sum of the views with pano_masks != 0, added in VIEW ORDER in fp32) / their count: one true
 *                                   division; views are selected by the mask, never multiplied by it, so a masked-out view may hold
 *                                   anything;
 *     store[row_base[b] + 1 + j]  = a bit copy of the j-th view with nav_types == 1, in view order (candidates need not come first).
 *   Rows are relative to the `store` pointer given; no other row is written.  status[b] = 0, or the OR of ETP_PSTORE_ERR_EMPTY (no
 *   unmasked view), ETP_PSTORE_ERR_MASKED (a candidate at a masked-out view), ETP_PSTORE_ERR_COUNT (the views with nav_types == 1
 *   are not n_cand[b] many), ETP_PSTORE_ERR_ROW (row_base[b] < 0 or row_base[b] + 1 + candidates > R); a flagged episode writes
 *   nothing to the store, and nothing is indexed by its values.  Episodes whose rows overlap are the caller's error.
 * etp_pano_store_bwd, one launch: d_store [R,H] with the same masks, types, bases and counts (bases relative to the d_store pointer
 *   given, so a block of the store's gradient goes with block-relative rows) ->
 *     d_pano_embeds[b,v] = (pano_masks[b,v] ? d_store[row_base[b]] / count_b : 0) + (nav_types[b,v] == 1 ? d_store[row_base[b] + 1 +
 *                          rank(v)] : 0), rank(v) = the candidates before view v; a candidate view receives both terms: the quotient
 *                          is rounded, then the sum.
 *   accumulate == 0: every element of d_pano_embeds is written, padded views and flagged episodes (the kernel derives the flags again;
 *   it takes no status) with exact zeros.  accumulate == 1: the value is added to what is there; flagged episodes are left alone.
 * Plain vector stores, no atomics, no scratch; the order of every sum is fixed by the data, so a second run gives the same bits.
 * ETP_ERR_INVALID before anything is launched: H not 256 / 512 / 768, V outside 1 .. 64, B < 1, R < 1, accumulate not 0 / 1, a NULL
 * operand, pano_embeds / store / d_store / d_pano_embeds not 16-byte aligned, nav_types not 8-byte or an int32 operand not 4-byte
 * aligned. */
#define ETP_PSTORE_ERR_EMPTY 1
#define ETP_PSTORE_ERR_MASKED 2
#define ETP_PSTORE_ERR_COUNT 4
#define ETP_PSTORE_ERR_ROW 8
int etp_pano_store_fwd(const float* pano_embeds, const uint8_t* pano_masks, const int64_t* nav_types, const int32_t* row_base,
                       const int32_t* n_cand, int B, int V, int H, float* store, int R, int32_t* status, etp_stream_t stream);
int etp_pano_store_bwd(const float* d_store, const uint8_t* pano_masks, const int64_t* nav_types, const int32_t* row_base,
                       const int32_t* n_cand, int B, int V, int H, int R, float* d_pano_embeds, int accumulate, etp_stream_t stream);

/* The panorama encoder's inputs from the waypoint head's candidate table (csrc/pano_inputs.hip): the end of ETP.forward(mode='waypoint')
 * (vlnce_baselines/models/Policy_ViewSelection_ETP.py:289-342) followed by RLTrainer._vp_feature_variable
 * (vlnce_baselines/ss_trainer_ETP.py:308-342), one launch, one wavefront per output row.
 *   rgb_embedding [12B, Frgb] and depth_embedding [12B, C, HW] fp32: the view encoders' outputs, CLOCKWISE (episode b's
 *   counter-clockwise view i is row b*12 + (12 - i) % 12, Policy_ViewSelection_ETP.py:182-190, 201-213).  cand_count: the count of
 *   episode b at cand_count[b * max_pred] (column 0 of row 0 of etp_waypoint_tail's table); cand_angle [B, max_pred]: the table's angle
 *   row (eval) or sampled-angle row (in_train); the distances play no part in these outputs.  cand_angle_tab [120,4] and
 *   pano_angle_tab [12,4] fp32: angle_feature_torch of the 120 heat-map angles and of the 12 panorama headings (:141-143), built once on
 *   the host -- the kernel has no transcendental.
 * For episode b with K = count, a_j = angle j, img(a) = 12 - (a + 5) / 10 with 12 -> 0 (:313-314), mask = the views img(a_j),
 * view_len = K + 12 - popcount(mask):
 *     row v < K             candidate v, in table order: view i = img(a_v), nav_types 1, loc_fts = cand_angle_tab[a_v];
 *     row K <= v < view_len the (v - K)-th view i of 0 .. 11 that is not in the mask: nav_types 0, loc_fts = pano_angle_tab[i];
 *       rgb_fts [B,V,Frgb]  a bit copy of rgb_embedding's row of view i (the 1 x 1 pool),
 *       dep_fts [B,V,C]     per channel the HW values of view i added in index order into one fp32 accumulator, then one division by HW;
 *     row v >= view_len     exact zeros in rgb_fts, dep_fts, loc_fts [B,V,4] and nav_types [B,V] (int64);
 *   view_lens [B] int64, cand_img [B, max_pred] int32 (img(a_j), -1 beyond K), status [B] int32.
 * status[b] = 0, or the OR of ETP_PINPUTS_ERR_COUNT (count outside 0 .. max_pred; the angles are then not read), ETP_PINPUTS_ERR_ANGLE (an
 * angle outside 0 .. 119), ETP_PINPUTS_ERR_VIEWS (view_len > V): a flagged episode writes its status and nothing else, and nothing is
 * indexed by its values.  Plain vector stores, no atomics, no LDS, no scratch; a second run gives the same bits.
 * ETP_ERR_INVALID before anything is launched: a NULL operand, B < 1, V < 12, max_pred < 1, Frgb < 4 or not a multiple of 4, C < 1,
 * HW < 1, rgb_embedding / depth_embedding / rgb_fts not 16-byte aligned, nav_types / view_lens not 8-byte or any other operand not
 * 4-byte aligned. */
#define ETP_PINPUTS_ERR_COUNT 1
#define ETP_PINPUTS_ERR_ANGLE 2
#define ETP_PINPUTS_ERR_VIEWS 4
int etp_pano_inputs(const float* rgb_embedding, const float* depth_embedding, const int32_t* cand_count, const int32_t* cand_angle,
                    const float* cand_angle_tab, const float* pano_angle_tab, int B, int V, int max_pred, int Frgb, int C, int HW,
                    float* rgb_fts, float* dep_fts, float* loc_fts, int64_t* nav_types, int64_t* view_lens, int32_t* cand_img,
                    int32_t* status, etp_stream_t stream);

/* A pre-training batch's device side from the resident view-feature store (csrc/traj_batch.hip; host side etpnav_amd/pretrain_data.py).
 * etp_traj_views, one launch, one wavefront per output row: R2RTextPathData.get_traj_pano_fts
 *   (pretrain_src/pretrain_src/data/dataset.py:483-526) plus the padding of sap_collate / mlm_collate (tasks.py:331-343) for R trajectory
 *   steps.  img_store [N, P, ld_img] and dep_store [N, P, ld_dep] fp32 (dep_store NULL: no depth, dep_fts NULL too, F_dep / ld_dep
 *   unread); per step r: pano_row [R] the store row, cand_count [R], cand_view [R, Kmax] view indices, cand_loc [R, Kmax, 4] the
 *   candidates' angle features (host); view_loc_tab [P, 4] the angle features of get_view_rel_angles(12).  All indices int32.
 *   For step r with k = count, mask = the views cand_view[r, 0 .. k-1], view_len = k + P - popcount(mask) (two candidates of one view
 *   free that view once, so view_len can exceed P):
 *     row v < k              candidate v, in table order: view i = cand_view[r, v], nav_types 1, loc_fts = cand_loc[r, v];
 *     row k <= v < view_len  the (v - k)-th view i of 0 .. P-1 that is not in the mask: nav_types 0, loc_fts = view_loc_tab[i];
 *       rgb_fts [R,V,F_img]  a bit copy of the first F_img columns of img_store[pano_row[r], i] (x[:, :image_feat_size]),
 *       dep_fts [R,V,F_dep]  likewise from dep_store;
 *     row v >= view_len      exact zeros in rgb_fts, dep_fts, loc_fts [R,V,4] and nav_types [R,V] (int64);
 *   view_lens [R] int64, status [R] int32 = 0, or the OR of ETP_TRAJ_ERR_COUNT (count outside 0 .. Kmax; the views are then not
 *   read), ETP_TRAJ_ERR_VIEW (a view index outside 0 .. P-1), ETP_TRAJ_ERR_ROW (pano_row outside 0 .. N-1), ETP_TRAJ_ERR_VIEWS
 *   (view_len > V): a flagged step writes its status and nothing else, and nothing is indexed by its values.
 *   ETP_ERR_INVALID before anything is launched: a NULL operand (dep_store and dep_fts only together), R, V or N < 1, Kmax or P outside
 *   1 .. 64, F_img (F_dep) < 4, not a multiple of 4 or > ld_img (ld_dep), ld_img (ld_dep) not a multiple of 4, img_store / dep_store /
 *   rgb_fts / dep_fts not 16-byte aligned, nav_types / view_lens not 8-byte or any other operand not 4-byte aligned.
 * etp_traj_pair_dists, one launch, one wavefront per output row: the double loop of get_gmap_inputs (dataset.py:316-320) plus the
 *   padding of tasks.py:350-355 for B samples.  dist_tab: dist_len float64, one n x n block per scan with entry [a][b] the Dijkstra
 *   distance from a to b; scan_off [B] int64 and scan_n [B] int32 the sample's block; gmap_idx [B, G] int32 the local viewpoint index
 *   (entry 0, [stop], is never looked up); gmap_len [B] int32.  For 1 <= i < j < len:
 *     gmap_pair_dists[b, i, j] = gmap_pair_dists[b, j, i] = (float)(dist_tab[off + idx_i * n + idx_j] / 30.0), evaluated in double and
 *     rounded once (the lookup is directional, as the reference's is); row 0, column 0, the diagonal and the padding are exact zeros;
 *   gmap_masks [B, G] u8 = (i < len).  status [B] int32 = 0, or ETP_TRAJ_ERR_LEN (gmap_len outside 1 .. G), ETP_TRAJ_ERR_SCAN (the
 *   block does not lie in the table), ETP_TRAJ_ERR_INDEX (an index of 1 .. len-1 outside 0 .. n-1): a flagged sample writes its status
 *   and nothing else.  ETP_ERR_INVALID before anything is launched: a NULL operand, B, G or dist_len < 1, dist_tab / scan_off not
 *   8-byte or scan_n / gmap_idx / gmap_len / gmap_pair_dists / status not 4-byte aligned.
 * Plain vector stores, no atomics, no LDS, no scratch; a second run gives the same bits. */
#define ETP_TRAJ_ERR_COUNT 1
#define ETP_TRAJ_ERR_VIEW 2
#define ETP_TRAJ_ERR_ROW 4
#define ETP_TRAJ_ERR_VIEWS 8
#define ETP_TRAJ_ERR_LEN 1
#define ETP_TRAJ_ERR_SCAN 2
#define ETP_TRAJ_ERR_INDEX 4
int etp_traj_views(const float* img_store, const float* dep_store, const int32_t* pano_row, const int32_t* cand_count,
                   const int32_t* cand_view, const float* cand_loc, const float* view_loc_tab, int R, int V, int Kmax, int P, int F_img,
                   int ld_img, int F_dep, int ld_dep, int N, float* rgb_fts, float* dep_fts, float* loc_fts, int64_t* nav_types,
                   int64_t* view_lens, int32_t* status, etp_stream_t stream);
int etp_traj_pair_dists(const double* dist_tab, int64_t dist_len, const int64_t* scan_off, const int32_t* scan_n, const int32_t* gmap_idx,
                        const int32_t* gmap_len, int B, int G, float* gmap_pair_dists, uint8_t* gmap_masks, int32_t* status,
                        etp_stream_t stream);

/* Trajectory node features straight from a batch's integer tables (csrc/traj_batch.hip): GlobalMapEncoder._aggregate_gmap_features
 * (pretrain_src/pretrain_src/model/vilmodel.py:585-619) and its backward, with the results of etp_gather_sum over
 * graph_inputs.pack_traj_csr's arrays, bit for bit, and no CSR.  One launch each, one wavefront per output row.
 *   pano [R*V, H] fp32: the panorama encoder's output for the R trajectory steps of B samples; sample b owns the steps
 *   step_off[b] .. step_off[b+1]-1 (step_off [B+1] int32).  Per step t: step_vp [R] int32 the viewpoint's id, view_lens [R] int64 its
 *   valid views n_t, cand_count [R] int32 and cand_vp [R, Kmax] int32 the ids its candidate slots name.  gmap_id [B, G] int32 the ids of
 *   the sample's nodes, gmap_len [B] int32 how many are listed.  An id is any int32 >= 0, distinct per viewpoint within a sample; -1 is
 *   the [stop] entry and padding; the ids of gmap_id[b, 1 .. len-1] are distinct.
 * etp_traj_nodes_fwd, node row (b, g) of gmap_img_fts [B*G, H]:
 *   g = 0 or g >= gmap_len[b]: exact zeros.
 *   the id equals step_vp of a step of sample b: with t the LAST such step, sum over the views j < n_t ascending of w * pano[t*V + j],
 *     w = (float)(1.0 / (double)n_t) (a later visit overwrites an earlier one, :603-607).
 *   otherwise every candidate slot (t, j), j < cand_count[t], whose cand_vp equals the id counts; the slots with j < n_t contribute
 *     w * pano[t*V + j] in the order t ascending, then j ascending, w = (float)(1.0 / (double)count): a slot beyond the valid views is a
 *     zero row of the reference (embeds * vp_masks, :599-600) that still counts in the mean.
 *   a listed node that is neither visited nor named: ETP_TRAJ_ERR_NODE, the row keeps what it held.
 * etp_traj_nodes_bwd, panorama row (t, j) of d_pano [R*V, H], t a step of sample b; at most two nodes read the row:
 *   (A) j < n_t, t is the last visit of step_vp[t] and that id is listed in gmap_id[b]: weight 1/n_t;
 *   (B) j < cand_count[t], j < n_t, cand_vp[t, j] is visited nowhere in the sample and is listed: weight 1/count;
 *   added in ascending node index; every other row is exact zeros.
 * Both accumulate acc = fma(w, x, acc) per element from +0 in the order stated, which is etp_gather_sum's operation.
 * status: forward [B*G] int32 per node row, backward [R] int32 per step (written by the wave of view 0) = 0, or the OR of
 *   ETP_TRAJ_ERR_STEPS (the sample's step range is not 0 <= step_off[b] < step_off[b+1] <= R; backward: also a step no sample owns),
 *   ETP_TRAJ_ERR_COUNT (a cand_count of the sample outside 0 .. Kmax), ETP_TRAJ_ERR_VIEWS (a view_lens of the sample outside 1 .. V),
 *   ETP_TRAJ_ERR_LEN (gmap_len[b] outside 1 .. G; it shares the value of ETP_TRAJ_ERR_COUNT, as in the two calls above) and, forward
 *   only, ETP_TRAJ_ERR_NODE.  A flagged wave writes its status word and leaves its row alone; nothing is indexed by an unchecked value.
 * ETP_ERR_INVALID before anything is launched: a NULL operand, H outside {256, 512, 768}, B, R, V or G < 1, Kmax outside 1 .. 64,
 *   B*G or R*V rows beyond the grid, pano / gmap_img_fts / d_gmap_img_fts / d_pano not 16-byte, view_lens not 8-byte or an int32 operand
 *   not 4-byte aligned.
 * Plain vector stores, no atomics, no LDS, no scratch; a second run gives the same bits. */
#define ETP_TRAJ_ERR_STEPS 16
#define ETP_TRAJ_ERR_NODE 32
int etp_traj_nodes_fwd(const float* pano, const int32_t* step_off, const int32_t* step_vp, const int64_t* view_lens,
                       const int32_t* cand_count, const int32_t* cand_vp, const int32_t* gmap_id, const int32_t* gmap_len, int B, int R,
                       int V, int Kmax, int G, int H, float* gmap_img_fts, int32_t* status, etp_stream_t stream);
int etp_traj_nodes_bwd(const float* d_gmap_img_fts, const int32_t* step_off, const int32_t* step_vp, const int64_t* view_lens,
                       const int32_t* cand_count, const int32_t* cand_vp, const int32_t* gmap_id, const int32_t* gmap_len, int B, int R,
                       int V, int Kmax, int G, int H, float* d_pano, int32_t* status, etp_stream_t stream);

/* The MLM task's masked-row selection on the device (csrc/traj_batch.hip): what _compute_masked_hidden and the label gather of
 * pretrain_cmt.py:141-163 select, as the index arrays etp_mlm_fwd / etp_mlm_eval / etp_mlm_bwd read -- the host build of
 * pretrain.MlmStep.__init__ (torch.nonzero, cumsum with a leading 0, labels[sel]) bit for bit, in one launch.
 *   txt_labels [n] int32, n = B*L: -1 = not masked, any other value a token id.
 *   rows [cap] int32: rows[j] = the flat index of the j-th entry != -1, ascending (sel_idx of etp_mlm_fwd).
 *   labels [cap] int64: labels[j] = that entry.
 *   ptr_t [n+1] int32: ptr_t[i] = the number of selected entries below i (the transposed CSR pointer of etp_mlm_bwd).
 *   status [2] int32: status[0] = 0 or the OR of ETP_MLM_ERR_COUNT (the count differs from n_expected) and ETP_MLM_ERR_LABEL (an
 *     entry below -1 or >= vocab); status[1] = the count.
 * n_expected is the count the caller sized the step for (the host knows it: mask_tokens runs there).  Whatever txt_labels holds,
 * after the launch every rows[j], j < n_expected, lies in [0, n), every labels[j] in [0, vocab), ptr_t is non-decreasing with
 * ptr_t[n] <= n_expected, and nothing at an index >= n_expected (<= cap) is written: a surplus entry is dropped, a short selection is
 * filled with row 0 / label 0, a label is clamped, ptr_t is clamped to n_expected.  A flagged launch is numerically meaningless
 * but no later kernel can take an out-of-range index from it.
 * ETP_ERR_INVALID before anything is launched: a NULL pointer, n outside 1 .. 2^20, vocab < 1, n_expected outside 0 .. cap, an int32
 * operand not 4-byte or labels not 8-byte aligned.
 * One workgroup walks n in chunks of 256; wave ballots, every wave derives the prefix of the waves below it for itself.  Plain
 * vector stores, no atomics, no LDS, no scratch; a second run gives the same bits. */
#define ETP_MLM_ERR_COUNT 1
#define ETP_MLM_ERR_LABEL 2
int etp_mlm_select(const int32_t* txt_labels, int n, int vocab, int n_expected, int cap, int32_t* rows, int32_t* ptr_t,
                   int64_t* labels, int32_t* status, etp_stream_t stream);

/* Pre-training MLM task for a planner created with cfg.use_lang2visn = 1:
 * GlocalTextPathCMT.forward_mlm (pretrain vilmodel.py:708-754): the text (output of etp_txt_fwd) attends to the graph-node
 * inputs gmap_img_fts + step + position embeddings through forward_lang2visn of every x-layer (:400-411), then
 * BertOnlyMLMHead (:258-299, decoder tied to the word embeddings) on the Nm masked positions and
 * *loss += scale * sum of token cross-entropies (pretrain_cmt.py:141-163; scale = 1/Nm for the reference's .mean()).
 * The masked positions are given as the CSR of a row gather (sel_ptr = 0..Nm, sel_idx = b*L + l, sel_w = 1) and, for the
 * backward, its transpose over the B*L rows.  etp_mlm_bwd returns d txt_embeds and d gmap_img_fts and accumulates every
 * parameter gradient, including the tied decoder's into the word-embedding gradient. */
int64_t etp_mlm_stash_bytes(const etp_planner* p, int B, int L, int G, int Nm);
int64_t etp_mlm_ws_bytes(const etp_planner* p, int B, int L, int G, int Nm);
int etp_mlm_fwd(etp_planner* p, const float* txt_embeds, const uint8_t* txt_masks, const int64_t* gmap_step_ids,
                const float* gmap_img_fts, const float* gmap_pos_fts, const uint8_t* gmap_masks, const int32_t* sel_ptr,
                const int32_t* sel_idx, const float* sel_w, const int64_t* labels, int B, int L, int G, int Nm, float scale,
                float* loss, void* stash, etp_stream_t stream);
int etp_mlm_bwd(etp_planner* p, const float* txt_embeds, const uint8_t* txt_masks, const int64_t* gmap_step_ids,
                const float* gmap_pos_fts, const uint8_t* gmap_masks, const int32_t* selT_ptr, const int32_t* selT_idx,
                const float* selT_w, int B, int L, int G, int Nm, float* d_txt_embeds, float* d_gmap_img_fts, void* stash,
                void* ws, etp_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Pre-training validation (pretrain_src/pretrain_src/train_r2r.py:335-444): the loss / arg-max tails of validate_mlm and
 * validate_sap and counters that stay on the device across batches (csrc/eval_tail.hip).  No atomics, every summation order is
 * fixed: a second run on the same inputs gives the same bits.  Tie and special-value semantics are torch's on the CPU: ties of the
 * maximum go to the lowest column, a label on a -inf logit gives nll = +inf, a row of only -inf gives pred 0 and a NaN nll.
 * PRECONDITION: no NaN in the logits.  Every entry refuses (ETP_ERR_INVALID, nothing launched) NULL pointers and counts < 1.
 * ---------------------------------------------------------------------------------------------------- */
/* what validate_mlm / validate_sap keep on the host (train_r2r.py:357-359, :418-420), on the device; 8-byte aligned */
typedef struct etp_eval_record {
  double loss_sum;     /* val_loss / val_gloss before the division */
  int64_t n_correct;   /* rows with label != ignore_index and pred == label */
  int64_t n_rows;      /* n_word / n_data: every row handed in, ignored ones included (labels.numel(), len(labels)) */
  int64_t n_counted;   /* rows whose label is not ignore_index */
} etp_eval_record;
/* F.cross_entropy(scores, labels, reduction='sum') and scores.max(dim=-1)[1] of train_r2r.py:365-367, per row: logits fp32 [Nm, ldv],
 * columns >= V are padding and are never read; labels [Nm] (there is no ignore_index: the caller gathers the masked tokens).  Writes
 * row_nll[r] = lse_r - logits[r, y_r] (fp32; NaN where y_r is outside [0, V), which is never used as an index) and row_pred[r]
 * (int32).  One workgroup per row; the row sum runs in etp_vocab_ce's order.  Refused besides: V < 1, ldv < V. */
int etp_vocab_eval(const float* logits, const int64_t* labels, int Nm, int V, int ldv, float* row_nll, int32_t* row_pred,
                   etp_stream_t stream);
/* F.cross_entropy(global_logits, labels, reduction='sum') and torch.argmax(global_logits, 1) of train_r2r.py:424-427, per row: logits
 * fp32 [B, G] with -inf entries; a row whose label is ignore_index writes nll = 0 (its pred is still the arg-max); any other label
 * outside [0, G) writes NaN.  One wavefront per row; max / sum / lse in etp_sap_ce's order. */
int etp_sap_eval(const float* logits, const int64_t* labels, int B, int G, int64_t ignore_index, float* row_nll, int32_t* row_pred,
                 etp_stream_t stream);
/* val_loss += loss.item(); n_correct += (pred == labels).sum().item(); n_word += labels.numel() of train_r2r.py:366-368 (:424-430 for
 * SAP) without the .item(): *acc += the n rows, in double, in an order fixed by the row index (one workgroup).  Rows whose label is
 * ignore_index add to n_rows only.  acc is device memory, 8-byte aligned, and is read and written by this launch alone. */
int etp_eval_accum(const float* row_nll, const int32_t* row_pred, const int64_t* labels, int n, int64_t ignore_index,
                   etp_eval_record* acc, etp_stream_t stream);
/* model(batch, task='mlm', compute_loss=False) of train_r2r.py:362 followed by the two launches above: etp_mlm_fwd's forward up to
 * the logits (the same code, the same stash plan), then etp_vocab_eval and etp_eval_accum (ignore_index -1, which a gathered label
 * never is).  Writes no dlogits and no loss.  row_nll [Nm] fp32, row_pred [Nm] int32.  Refused besides: a planner without
 * use_lang2visn, acc not 8-byte aligned. */
int etp_mlm_eval(etp_planner* p, const float* txt_embeds, const uint8_t* txt_masks, const int64_t* gmap_step_ids,
                 const float* gmap_img_fts, const float* gmap_pos_fts, const uint8_t* gmap_masks, const int32_t* sel_ptr,
                 const int32_t* sel_idx, const float* sel_w, const int64_t* labels, int B, int L, int G, int Nm, void* stash,
                 float* row_nll, int32_t* row_pred, etp_eval_record* acc, etp_stream_t stream);
/* Host only: where etp_mlm_fwd / etp_mlm_eval put the fp32 logits [Nm, *ldv] inside a stash of etp_mlm_stash_bytes -- the `scores`
 * of train_r2r.py:362 are its columns [0, vocab). */
int etp_mlm_stash_logits(const etp_planner* p, int B, int L, int G, int Nm, int64_t* byte_offset, int64_t* ldv);

/* ------------------------------------------------------------------------------------------------------
 * Pre-training log (pretrain_src/pretrain_src/train_r2r.py:229-317): what the loop tells the user while it trains, as small records
 * that stay on the device across steps and are read in one copy every log_steps optimizer steps (csrc/trainlog.hip) -- the
 * training-side twin of etp_eval_record.  Plain vector stores, no atomics of any kind, no scratch; every order of summation is
 * fixed, so a second run on the same inputs gives the same bits.  Every entry refuses (ETP_ERR_INVALID, nothing launched) NULL
 * pointers (those marked nullable excepted), misaligned operands and negative counts.
 * ---------------------------------------------------------------------------------------------------- */
/* one task's RunningMeter (utils/logger.py:68-94) and its three throughput counters (train_r2r.py:233-234, :246); 64 bytes,
 * little-endian, 8-byte aligned; starts as all zero bytes */
typedef struct etp_train_task_record {
  double run_loss;       /* RunningMeter._val; meaningless while n_values == 0 (the reference's None; .val reports 0) */
  double last_loss;      /* the value of the last call, taken or not */
  int64_t n_values;      /* calls whose smoothed value was taken */
  int64_t n_skipped;     /* calls whose smoothed value was NaN and was dropped (logger.py:80) */
  int64_t n_examples;    /* n_examples[name] (:233) */
  int64_t n_in_units;    /* n_in_units[name] (:234): the non-zero bytes of txt_masks, = batch['txt_lens'].sum() */
  int64_t n_loss_units;  /* n_loss_units[name] (:246): loss.size(0) before the mean */
  int64_t reserved;
} etp_train_task_record;
/* the optimizer steps' gradient norm (train_r2r.py:282-290); 64 bytes; starts as zero bytes with first_nonfinite_step = -1 */
typedef struct etp_train_step_record {
  double norm_last;               /* the last step's pre-clip grad_norm, an fp32 value as clip_grad_norm_ returns it */
  double norm_max;                /* over the finite steps */
  double norm_sum;                /* over the finite steps, added in double in step order */
  int64_t n_steps;
  int64_t n_nonfinite_steps;      /* steps whose norm was not finite or whose non-finite count was not zero */
  int64_t first_nonfinite_step;   /* the first such step counted from 1 (n_steps after it); -1 = none */
  int64_t reserved[2];
} etp_train_step_record;
/* task2loss[name](loss.item()) of train_r2r.py:259 without the .item(), and the counters of :233-234 and :246.  loss: the step's
 * device loss (one fp32, already divided by the accumulation steps as :250-252 logs it).  RunningMeter.__call__ (logger.py:77-81)
 * in Python's double arithmetic, bit for bit: value = (double)*loss; with no value taken yet val = value, otherwise
 * val = value*(1.0 - smooth) + run_loss*smooth -- 1.0 - smooth formed in double, two double products and one double sum, each rounded
 * on its own; a NaN val leaves run_loss alone and counts a skip, +-inf is taken.  The counters advance on every call, skipped or not:
 * n_examples and n_loss_units by the arguments, n_in_units by the number of non-zero bytes among txt_masks[0 .. n_mask_bytes) (the
 * step's staged bool tensor [B, L]; train_r2r.py:234 sums batch['txt_lens'], which the native batches do not carry).
 * Refused besides: smooth outside [0, 1).  One workgroup; rec is read and written by this launch alone. */
int etp_train_meter_loss(const float* loss, double smooth, const uint8_t* txt_masks, int64_t n_mask_bytes, int64_t n_examples,
                         int64_t n_loss_units, etp_train_task_record* rec, etp_stream_t stream);
/* grad_norm = clip_grad_norm_(model.parameters(), opts.grad_norm) of train_r2r.py:282-284 and its TB_LOGGER.add_scalar (:290) without
 * the host read: from the optimizer's sumsq (etp_grad_sqnorm / etp_tensor_report; one fp32) and nonfinite (one int32, nullable = 0),
 * launched behind the norm pass and before the pair is next zeroed.  grad_norm = (float)sqrt((double)*sumsq), the correctly rounded
 * fp32 root.  A step whose norm is not finite or whose count is not zero adds to n_nonfinite_steps and not to norm_max / norm_sum.
 * One thread. */
int etp_train_meter_step(const float* sumsq, const int32_t* nonfinite, etp_train_step_record* rec, etp_stream_t stream);

/* Per-tensor fingerprint of a float arena: (sum, abs-max, L2) of oracle/make_golden.py:69-73 per tensor -- the per-parameter norm
 * loop the reference keeps as commented-out debugging code (train_r2r.py:286-289) -- deterministic, in double, without a copy of the
 * arena to the host.  32 bytes, 8-byte aligned. */
typedef struct etp_tensor_record {
  double sum;          /* over the finite values, in double */
  double sumsq;        /* over the finite values; the square of a float is exact in double, only the additions round */
  float absmax;        /* over the finite values, exact */
  int32_t nonfinite;   /* NaN and +-inf values: counted, left out of the three others */
  int64_t reserved;    /* written as 0 */
} etp_tensor_record;
#define ETP_TENSOR_REPORT_CHUNK 16384      /* elements per stage-1 workgroup */
typedef struct etp_tensor_report_plan etp_tensor_report_plan;
/* A plan over n_seg segments [seg_off[s], seg_off[s] + seg_len[s]) of an arena of arena_len floats, in elements.  All arrays are HOST
 * pointers, validated here and uploaded once, at the plan's first etp_tensor_report (creating a plan needs no device).  include
 * (nullable = all): one byte per segment, non-zero = the segment enters the totals.  The plan owns the per-chunk partials, so one plan
 * serves one stream at a time.  Refused: n_seg <= 0, arena_len <= 0, an offset that is negative or no multiple of 4, a length < 1,
 * segments that do not ascend or that overlap, a segment that ends behind arena_len. */
int etp_tensor_report_create(const int64_t* seg_off, const int64_t* seg_len, const uint8_t* include, int n_seg, int64_t arena_len,
                             etp_tensor_report_plan** plan);
/* Host only: the number of stage-1 workgroups, sum over the segments of ceil(seg_len / ETP_TENSOR_REPORT_CHUNK); -1 for NULL. */
int64_t etp_tensor_report_chunks(const etp_tensor_report_plan* plan);
/* Three launches on `stream`.  Stage 1: one workgroup of 256 threads per chunk of at most ETP_TENSOR_REPORT_CHUNK elements, never
 * across a segment (binary search of the chunk prefix); 16-byte loads thread-strided in ascending order, the up to three elements
 * behind the last whole vector by threads 0 .. 2; the wave's shuffle tree; the four waves in wave order; one partial per chunk.
 * Stage 2: one wavefront per segment, lane l adds the partials l, l + 64, ... in chunk order, then the shuffle tree; writes
 * records_out[s].  Stage 3 (when sumsq_out or nonfinite_out is given; both nullable): one wavefront adds the records whose include
 * byte is non-zero, lane l the segments l, l + 64, ... in segment order, then the shuffle tree, and STORES (float)sum of sumsq and
 * the int32 non-finite total -- an etp_grad_sqnorm-compatible pair that needs no zeroing; with a non-zero total the float is a
 * quiet NaN.  Nothing outside the segments is read.  arena 16-byte, records_out 8-byte aligned; records_out [n_seg]. */
int etp_tensor_report(etp_tensor_report_plan* plan, const float* arena, etp_tensor_record* records_out, float* sumsq_out,
                      int32_t* nonfinite_out, etp_stream_t stream);
int etp_tensor_report_destroy(etp_tensor_report_plan* plan);

/* ------------------------------------------------------------------------------------------------------
 * Fine-tuning rollout loss (vlnce_baselines/ss_trainer_ETP.py:820, :892, :1055-1057): the imitation loss of one rollout, its
 * scale and the IL_loss log, kept on the device (csrc/rollout_loss.hip).  The divisor total_actions is known only when the last
 * environment has stopped, so it is no launch argument: the per-step launches advance a device record and the backward launches
 * read it.  Plain vector stores, no atomics, no scratch; every order of summation is fixed, so a second run on the same inputs gives
 * the same bits.  PRECONDITION: no NaN in the logits.  Every entry refuses (ETP_ERR_INVALID, nothing launched) NULL pointers (those
 * marked nullable excepted), B < 1, G < 1, misaligned operands (fp32 4 bytes; labels, record and log 8 bytes) and an output that
 * overlaps the record.
 * ---------------------------------------------------------------------------------------------------- */
/* one rollout's `loss` and `total_actions` (ss_trainer_ETP.py:795-796); 64 bytes, little-endian, 8-byte aligned; starts as zero bytes */
typedef struct etp_rollout_record {
  double loss_sum;       /* loss before the scaling of :1055: the rows' nll, added in double in row order, step after step */
  int64_t n_actions;     /* total_actions (:820): every row handed in, ignored ones included */
  int64_t n_counted;     /* rows whose label is not ignore_index */
  int64_t n_steps;       /* etp_rollout_ce_fwd calls */
  int64_t n_nonfinite;   /* counted rows whose nll is not finite (a label outside [0, G), a label on a -inf logit, a row of only -inf) */
  int64_t reserved[3];
} etp_rollout_record;
/* self.logs['IL_loss'] (:1057) as a running sum: np.mean over an interval is sum / n; 24 bytes, 8-byte aligned; starts as zero bytes */
typedef struct etp_rollout_log {
  double sum;            /* the rollouts' fp32 loss values, added in double in call order */
  int64_t n;             /* values added */
  int64_t n_nonfinite;   /* values that were not finite (they are added all the same, as np.mean would take them) */
} etp_rollout_log;
/* One step: loss += F.cross_entropy(nav_logits, teacher_actions, reduction='sum', ignore_index) (:892) and total_actions += B (:820).
 * logits fp32 [B, G] with -inf entries, labels [B].  Per row nll = lse - logits[y] with max / sum / lse in etp_sap_eval's order; an
 * ignored row contributes 0; any other label outside [0, G) gives NaN for its row, adds 1 to n_nonfinite and is never used as an
 * index.  rec->loss_sum += sum_b (double)nll_b, added in row order by one workgroup; n_actions += B; n_counted += the rows that are
 * not ignored; n_steps += 1.  The launch loops over the rows, so one call may take T stacked steps as (T*B) rows (n_steps still
 * advances by 1).  row_nll (nullable) [B] fp32 receives the rows' nll.  rec is read and written by this launch alone. */
int etp_rollout_ce_fwd(const float* logits, const int64_t* labels, int B, int G, int64_t ignore_index, etp_rollout_record* rec,
                       float* row_nll /*nullable*/, etp_stream_t stream);
/* loss = ml_weight * loss / total_actions (:1055): *loss = (float)((ml_weight * loss_sum) / (double)n_actions), the product and the
 * quotient in double, one rounding to fp32; n_actions == 0 gives exactly 0.  log (nullable): the same fp32 value is added to it --
 * self.logs['IL_loss'].append(loss.item()) (:1057) without the .item().  Refused besides: loss inside the record, a log that overlaps
 * either.  One thread. */
int etp_rollout_loss(const etp_rollout_record* rec, double ml_weight, float* loss, etp_rollout_log* log /*nullable*/,
                     etp_stream_t stream);
/* What autograd sends back into one step's nav_logits: dlogits = s * (softmax - onehot) with s = (float)(ml_weight /
 * (double)rec->n_actions) * *upstream (upstream nullable = 1; n_actions == 0 gives s = 0).  The scale is read from the device, so
 * total_actions is never copied to the host.  Ignored rows are exactly 0; a -inf logit that no label points at gets exactly 0, as in
 * etp_sap_ce; a row whose label is neither ignore_index nor a column is NaN.  dlogits fp32 [B, G].  One wavefront per row. */
int etp_rollout_ce_bwd(const float* logits, const int64_t* labels, int B, int G, int64_t ignore_index, const etp_rollout_record* rec,
                       double ml_weight, const float* upstream /*nullable: 1*/, float* dlogits, etp_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * hipGraph helpers (launch-bound inner loops are captured once and replayed) and timing.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct etp_graph etp_graph;
int etp_stream_create(etp_stream_t* out);
/* level < 0: the lowest priority the device offers (for leaf work such as weight gradients, so that the dependent chain's
 * workgroups are dispatched first whenever both wait for a CU), 0: default, > 0: highest. */
int etp_stream_create_prio(etp_stream_t* out, int level);
int etp_stream_destroy(etp_stream_t s);
int etp_stream_sync(etp_stream_t s);
/* make `to` wait for the work enqueued so far on `from` (fork / join of parallel branches; capturable) */
int etp_stream_after(etp_stream_t from, etp_stream_t to);
int etp_graph_begin(etp_stream_t s);
int etp_graph_end(etp_stream_t s, etp_graph** out);
/* ----------------------------------------------------------------------------------------------------
 * Data-parallel gradient mean: replaces DistributedDataParallel(self.policy.net) of
 * ss_trainer_ETP.py:208-212 / pretrain utils/misc.py:52-65 for the planner's flat gradient arena.  One communicator per
 * process (one process per GPU); RCCL over xGMI, bound at run time.  A bucket is reduced IN PLACE as reduce-scatter (sum) ->
 * 1/world scaling of the rank's own slice -> all-gather on a private communication stream ordered after `producer`.
 * comm_dtype ETP_F32 (default, DDP's numerics) or ETP_BF16 (opt-in: half the xGMI bytes, bf16 sums; needs
 * max_bucket_elems for the packed staging buffer).  Rank 0 creates the 128-byte id, the caller distributes it (any
 * out-of-band channel, e.g. torch.distributed's store) and every rank calls etp_allreduce_init with it.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct etp_comm etp_comm;
int etp_allreduce_unique_id(void* id_out_128_bytes);
int etp_allreduce_init(etp_comm** out, const void* unique_id, int rank, int world, int comm_dtype, int64_t max_bucket_elems);
int etp_allreduce_bucket_ready(etp_comm* c, float* grads, int64_t n, etp_stream_t producer);
/* The slice arithmetic etp_allreduce_bucket_ready applies to a bucket of n fp32 gradients over `world` ranks, as a pure host
 * function (no communicator, no GPU): out[0] = elements per rank slice, out[1] = elements covered by reduce-scatter + all-gather,
 * out[2] = tail elements that go through one all-reduce (fp32 transport only), out[3] = bf16 elements staged (bf16 transport only;
 * the pad [n, out[3]) is zeroed).  DDP's buckets (ss_trainer_ETP.py:208-212) have no counterpart of this: it exists so that the
 * multi-rank arithmetic can be unit-tested for worlds 2 / 4 / 8 on a one-GPU box. */
int etp_allreduce_plan(int64_t n, int world, int comm_dtype, int64_t* out);
int64_t etp_allreduce_staging_elems(int64_t max_bucket_elems, int world);
/* Row-sparse mean of a table gradient [n_rows, row_len] (the word-embedding table: a step touches <= B*L of its 30 522 /
 * 250 002 rows; DDP would all-reduce the dense table, ss_trainer_ETP.py:208-212).  ids[0, n_ids) = rows this rank touched (any
 * order, repeats allowed); `capacity` >= n_ids is the rank-INDEPENDENT block size (e.g. B * max_txt_len; the reference's collate
 * pads to the per-batch maximum, pretrain_src/pretrain_src/data/tasks.py:322-364, so the token count differs across ranks --
 * the capacity must not).  pack (repeats masked on the device) -> ncclAllGather of (ids, rows) -> scatter-add x 1/world, on the
 * communicator's own stream after `producer`: the same communicator and stream as the dense buckets. */
int etp_allreduce_gather_rows(etp_comm* c, float* table, int64_t n_rows, int64_t row_len, const int64_t* ids, int64_t n_ids,
                              int64_t capacity, etp_stream_t producer);
/* 1 when librccl can be bound in this process (ranks agree on it before any of them enters etp_allreduce_init) */
int etp_allreduce_available(void);
int etp_allreduce_wait(etp_comm* c, etp_stream_t consumer);
/* Host-side poll: 1 when everything issued on the communicator's stream has completed, 0 while work is in flight.  With
 * etp_allreduce_abort (ncclCommAbort; afterwards only etp_allreduce_destroy is valid) this lets a first-contact self-test give
 * up on a collective that never completes instead of blocking the job: etpnav_amd/dp.py NativeComm.self_test.  (DDP has no
 * counterpart; its watchdog is NCCL_ASYNC_ERROR_HANDLING inside torch.distributed, ss_trainer_ETP.py:208-212.) */
int etp_allreduce_idle(etp_comm* c);
int etp_allreduce_abort(etp_comm* c);
int etp_allreduce_destroy(etp_comm* c);
int etp_allreduce_rank(const etp_comm* c);
int etp_allreduce_world(const etp_comm* c);
etp_stream_t etp_allreduce_stream(const etp_comm* c);

/* Explicit graph construction (replaces stream capture for the three-stream step: hipStreamEndCapture crashes on ROCm 7.2
 * once two side streams joined a capture).  Between etp_rec_begin() and etp_rec_end() every entry point of this library
 * that takes a stream is RECORDED as hipGraph kernel / memset nodes instead of being issued: per-stream order and the event
 * edges of etp_stream_after / the planner's internal forks and joins become graph dependencies.  The result is launched,
 * timed and destroyed like a captured graph.  One recording at a time; record from one host thread. */
int etp_rec_begin(void);
int etp_rec_end(etp_graph** out, int64_t* n_kernels, int64_t* n_edges);
int etp_rec_abort(void);
int etp_graph_launch(etp_graph* g, etp_stream_t s);
int etp_graph_destroy(etp_graph* g);
/* Introspection of a graph built by etp_rec_end (host-side only; a captured graph returns ETP_ERR_INVALID).  A recording keeps its
 * nodes in creation order (kernel nodes, memset nodes, the empty join nodes of event records made right after waits) and a trace of
 * every call the recorder saw; both live until etp_graph_destroy.  None of it adds a node, an edge or an eager call.
 *   etp_graph_info      out[0..3] = nodes, trace rows, edges (as the runtime reports them), logical streams.
 *   etp_graph_trace     one row of 4 x int32 per recorded call, in call order: kind (0 kernel, 1 memset, 2 empty join node, 3 event
 *                       record, 4 stream wait), stream index (by first appearance), event index (by first appearance) or -1, node
 *                       index or -1.  A wait on an event that was never recorded inside the recording is traced too; the recorder
 *                       ignores it (outside the recording that event is complete).  cap = rows the buffer holds.
 *   etp_graph_edges     the edges hipGraphGetEdges reports, as creation indices (NOT the recorder's own dependency lists).
 *   etp_graph_node_name the kernel's name, or "memset" / "join".
 *   etp_graph_linearize a new graph of the same nodes with the same parameters whose only edges are order[i] -> order[i+1];
 *                       `order` must be a permutation of all n nodes, anything else returns ETP_ERR_INVALID.  The result keeps the
 *                       creation indices of `g` and is launched and destroyed like any etp_graph.  (tests/test_sched_gpu.py runs every
 *                       order the recorded dependencies allow this way: a missing edge shows as a wrong result, without a race.) */
int etp_graph_info(etp_graph* g, int64_t* out);
int etp_graph_trace(etp_graph* g, int32_t* rows, int64_t cap);
int etp_graph_edges(etp_graph* g, int32_t* from, int32_t* to, int64_t cap);
int etp_graph_node_name(etp_graph* g, int64_t i, char* buf, int cap);
int etp_graph_linearize(etp_graph* g, const int32_t* order, int64_t n, etp_graph** out);
/* memset of `bytes` bytes.  value == 0 with bytes % 4 == 0 and p 16-byte aligned: the library's own zeroing kernel (float4 body, scalar
 * tail; recorded as a kernel node); everything else: the runtime's memset.  bytes = 0 does nothing. */
int etp_memset_async(void* p, int value, int64_t bytes, etp_stream_t s);
/* HIP-event timing on the given stream: elapsed ms of `iters` graph replays. */
int etp_graph_time(etp_graph* g, etp_stream_t s, int iters, float* ms_out);

/* Per-launch HIP-event timing of the MFMA GEMM family (events recorded on the launch stream; eager launches only —
 * do not enable during graph capture).  etp_prof_report synchronises the recorded events and returns one entry per
 * kernel instantiation: launches, summed ms, summed algorithmic FLOPs and algorithmic bytes (A+B+C once). */
typedef struct etp_prof_entry {
  char name[96];
  int64_t launches;
  double ms, flops, bytes;
} etp_prof_entry;
/* Per-launch HIP-event timing of EVERY kernel the library issues (measurement aid, tools/chain_budget.py): one text line per
 * launch in launch order, "<us>\t<grid>\t<block>\t<stream>\t<kernel name>".  Events sit on the launch stream: issue the step on a
 * single stream when each pair should bracket its kernel alone. */
int etp_ktime_enable(int on);
int etp_ktime_reset(void);
int64_t etp_ktime_report(char* buf, int64_t cap);
int etp_prof_enable(int on);
int etp_prof_reset(void);
/* Bracket only launches whose name contains `name_part` (NULL / "" = all): with the step on its three streams every event pair is
 * a barrier packet the queues must process, so timing one kernel class in-step should not bracket the other 150 launches. */
int etp_prof_filter(const char* name_part);
/* Phase probe of the LDS-DMA GEMM kernels (measurement aid, tools/gemm_phase_probe.py; the reference has only host
 * time.time() counters, pretrain_src/pretrain_src/train_r2r.py:227,299-317).  With a device buffer of
 * max_launches x 4096 x 8 uint64 installed, every following eager GEMM launch of <= 4096 workgroups records per workgroup
 * { s_memrealtime at entry, at exit; s_memtime at entry, first slab visible, end of reduction, end of epilogue;
 *   XCC_ID << 32 | HW_ID; slabs } in launch order; etp_gemm_probe_meta names launch i (dims = grid, M, N, K).
 * dev_buf == NULL switches the probe off. */
int etp_gemm_probe_enable(uint64_t* dev_buf, int64_t max_launches);
int64_t etp_gemm_probe_count(void);
int etp_gemm_probe_meta(int64_t i, char* name, int cap, int32_t* dims);
int etp_prof_report(etp_prof_entry* out, int cap);
/* Device-side time stamp (measurement aid, tools/chain_waits.py): a one-thread kernel on `stream` stores s_memrealtime (100 MHz,
 * chip-wide) into *slot when the stream reaches it -- the un-profiled view of where a stream waits (the reference's single
 * backward, ss_trainer_ETP.py:504, has no joins of its own: every wait found is ours). */
int etp_stamp(uint64_t* slot, etp_stream_t stream);
/* Stamp sink: with a device buffer of `cap` uint64 installed, the planner entry points (and etp_stamp_mark, for the caller's own
 * points) append one such stamp per marked point of their issue order -- text / navigation / panorama layer boundaries, forks and
 * joins -- in enqueue order; etp_stamp_tag(i) names stamp i (tags: tools/chain_waits.py).  dev_buf == NULL removes the sink. */
int etp_stamp_sink(uint64_t* dev_buf, int64_t cap);
int64_t etp_stamp_count(void);
int etp_stamp_tag(int64_t i);
int etp_stamp_mark(etp_stream_t stream, int tag);

#ifdef __cplusplus
}
#endif
#endif /* ETPNAV_HIP_H */
