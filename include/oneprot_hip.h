/*
 * oneprot_hip.h -- C ABI of liboneprot_hip.so: the MI355X (gfx950) kernels behind the OneProt contrastive
 * alignment training step.
 *
 * The reference (klemens-floege/oneprot) is pure Python: it has no FFI of its own.  Its "plugin API" for this path
 * is the encoder/loss protocol used by OneProtLitModule (ref src/models/oneprot_module.py:67-108); the arithmetic is
 * delegated to torch/ATen and HF transformers.  Each entry point below replaces one such library call site and cites
 * it ("ref" = /root/reference, "hf" = transformers/models/esm/modeling_esm.py or .../bert/modeling_bert.py).
 * INTEGRATION.md shows the ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - plain pointers (device memory owned by the caller), sizes, and an opaque stream (hipStream_t passed as void*);
 *   - every function that takes a `stream` only enqueues work on it: no allocation, no synchronisation, graph-capturable (per-launch bookkeeping that
 *     a replayed graph must see advance -- work-queue heads, launch tags -- lives in caller-provided device memory and is advanced by the kernels themselves,
 *     see "sched workspace" below).  The exceptions say so: *_workspace*() / *_eligible() size queries, oneprot_alloc_uncached / oneprot_free_uncached (host
 *     allocation calls, for set-up code), oneprot_gemm_resid_ln8_error (a host-synchronous read for tests and end-of-epoch checks), and the test / tuning hooks;
 *   - return 0 on success, -1 invalid argument / unsupported shape, -2 launch failure.  Nothing throws;
 *   - "bf16" pointers are raw 16-bit bfloat16 storage; statistics, residual stream, losses and all parameter
 *     gradients are fp32;
 *   - workspaces are caller-provided; *_workspace() returns the byte count.
 */
#ifndef ONEPROT_HIP_H
#define ONEPROT_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int oneprot_abi_version(void);

/* ---------------- embeddings (hf modeling_esm.py:224-271; ref sequence_encoder.py:78) ---------------------------- */
/* x[b,l,:] = table[id] * 0.88/(1 - n_mask_b/n_valid_b); rows of <mask> and <pad> ids are zero. row_scale[b] (optional) keeps the factor. */
int oneprot_esm_embed_fwd(const int64_t* ids, const float* table, float* x, float* row_scale, int B, int L, int d, int vocab,
                          int pad_id, int mask_id, int token_dropout, void* stream);
size_t oneprot_esm_embed_bwd_workspace(int T, int d, int vocab);
int oneprot_esm_embed_bwd(const int64_t* ids, const float* dx, const float* row_scale, float* dtable, void* workspace, int B, int L, int d,
                          int vocab, int pad_id, int mask_id, int token_dropout, int accumulate, void* stream);
/* BERT: x = LN(word[id] + pos[l] + type[0])  (hf modeling_bert.py:53-108; ref text_encoder.py:59) */
int oneprot_bert_embed_fwd(const int64_t* ids, const float* word, const float* pos, const float* type0, const float* gamma, const float* beta,
                           float* x_f32, void* x_bf16, int B, int L, int d, int vocab, float eps, void* stream);

/* ---------------- LayerNorm (nn.LayerNorm: hf modeling_esm.py:429,518,552; ref base_encoder.py:153,158,162) ------ */
int oneprot_layernorm_fwd(const void* x, int x_is_bf16, const float* gamma, const float* beta, void* y_bf16, float* y_f32, float* mean,
                          float* rstd, int64_t T, int d, float eps, void* stream);
size_t oneprot_layernorm_bwd_workspace(int d);
/* dy_mode 0: bf16 [T,d]; 1: fp32 [T,d]; 2: dy[t] = dpool[t/L] * wrow[t].  dx = (add_to ? add_to : 0) + LN'(dy). */
int oneprot_layernorm_bwd(const void* dy, int dy_mode, const float* wrow, int L, const void* x, int x_is_bf16, const float* gamma,
                          const float* mean, const float* rstd, const float* add_to, float* dx, void* dx_bf16 /* optional bf16 copy of dx */,
                          float* dgamma, float* dbeta, void* workspace, int64_t T, int d, int accumulate_param_grads, void* stream);
/* final LayerNorm fused with pooling (ref base_encoder.py:109-126): mode 0 masked mean (CLS/EOS included), 1 CLS. */
int oneprot_lnpool_fwd(const float* x, const int64_t* ids, int pad_id, const float* gamma, const float* beta, float* pooled, float* mean,
                       float* rstd, float* wrow, void* hidden_bf16, float* hidden_f32, int B, int L, int d, float eps, int mode, void* stream);

/* pooling of an already-normalised hidden state (BERT): mode 0 masked mean, 1 CLS (ref base_encoder.py:109-126). */
int oneprot_pool_fwd(const float* x, const int64_t* ids, int pad_id, float* pooled, int B, int L, int d, int mode, void* stream);
/* its backward: g[b,l,:] = dpooled[b,:]/n_b on non-pad tokens (mode 0) or dpooled[b,:] at l=0 (mode 1), zero elsewhere; optional bf16 copy. */
int oneprot_pool_bwd(const float* dpooled, const int64_t* ids, int pad_id, float* g, void* g_bf16, int B, int L, int d, int mode, void* stream);
/* Embedding-table gradient for a large vocabulary (BertEmbeddings.word_embeddings, hf modeling_bert.py:53-108): `perm` = stable argsort of
 * the token ids, `seg_start[s]` / `seg_row[s]` = first sorted position / token id of run s; rows are added in sorted order (deterministic);
 * run with id == skip_row (padding_idx) is skipped; untouched rows must have been zeroed by the caller. */
int oneprot_embed_scatter_sorted(const float* dx, const int64_t* perm, const int64_t* seg_start, const int64_t* seg_row, int64_t n_tokens, int n_seg,
                                 int d, int skip_row, float* dtable, void* stream);
/* out[j] = sum_r x[r,j], fp32 [R,n] (position / token-type embedding gradients: sums over batch, then over positions). */
int oneprot_rowsum_f32(const float* x, float* out, int R, int64_t n, void* stream);

/* Attention1dPooling (ref base_encoder.py:40-103): pooled = sum_l softmax_l(x_l.w + b | padding -> -inf) x_l on an fp32 hidden state [B,L,d];
   attn [B,L] (optional in fwd, required by bwd).  bwd: dw [d], db [1], dx [B,L,d] (optional). */
int oneprot_attnpool_fwd(const float* x, const int64_t* ids, int pad_id, const float* w, const float* bias, float* pooled, float* attn, int B, int L,
                         int d, void* stream);
size_t oneprot_attnpool_bwd_workspace(int B, int d);
int oneprot_attnpool_bwd(const float* x, const float* attn, const float* w, const float* dpooled, float* dw, float* db, float* dx, void* workspace,
                         int B, int L, int d, void* stream);

/* ---------------- dense contractions on MFMA (nn.Linear call sites: hf modeling_esm.py:362-368,399-409,442-463) -- */
enum {
  ONEPROT_EPI_BF16 = 0,        /* out0 bf16 [M,N] = acc (+bias)                                                   */
  ONEPROT_EPI_F32 = 1,         /* out0 fp32 [M,N] = acc (+bias)                                                   */
  ONEPROT_EPI_BIAS_GELU = 2,   /* z = acc+bias; out0 bf16 = gelu_erf(z); out1 u8 [M,N] = gelu_erf'(z) as the code rint(192 g' + 25) (optional, for bwd) */
  ONEPROT_EPI_BIAS_RESID = 3,  /* out0 fp32 = acc + bias + resid fp32 (out0 may alias resid); out1 bf16 copy opt. */
  ONEPROT_EPI_QKV_ROPE = 4,    /* N = 3*H*hd: q=(acc+b)*q_scale -> rope -> out0 [B,H,L,hd]; k -> rope -> out1; v -> out2 */
  ONEPROT_EPI_GELU_BWD = 5     /* out0 bf16 = acc * g', g' = (aux - 25) / 192, aux u8 [M,N] = the codes saved by ONEPROT_EPI_BIAS_GELU  */
};
/* C[M,N] = A[M,K] * B[N,K]^T, A and B bf16 row-major with leading dims lda/ldb (elements), fp32 accumulation. */
int oneprot_gemm_bf16_nt(const void* A, const void* Bw, int64_t M, int N, int K, int lda, int ldb, int epilogue, const float* bias,
                         void* out0, void* out1, void* out2, const void* aux, const float* rope_cos, const float* rope_sin, float q_scale,
                         int L, int H, int hd, void* stream);
/* Full-row form for N = 640 with the FOLLOWING LayerNorm fused into the epilogue (hf modeling_esm.py:399-409 + :429 / :455-463 + :518 of the next
   layer): x_out fp32 [M,640] = A * W^T + bias + resid (x_out may alias resid); h_out bf16 [M,640] = LayerNorm(x_out; gamma, beta, eps); mean / rstd [M]
   (optional) as oneprot_layernorm_fwd would return them.  Wp = the weight packed by oneprot_gemm_ln_pack_weight (same byte count as W).
   Needs N == 640, M % 128 == 0, K % 64 == 0; -1 otherwise (callers then use oneprot_gemm_bf16_nt + oneprot_layernorm_fwd). */
int oneprot_gemm_ln_pack_weight(const void* W_bf16 /* [N,K] row-major */, void* Wp, int N, int K, void* stream);
int oneprot_gemm_bf16_nt_resid_ln(const void* A, const void* Wp, int64_t M, int N, int K, int lda, const float* bias, const float* resid, float* x_out,
                                  const float* gamma, const float* beta, float eps, void* h_out, float* mean, float* rstd, void* stream);
/* ---- sched workspace: device memory through which the persistent one-work-group-per-CU kernels hand out work at run time and keep per-launch
 * bookkeeping on the device (csrc/sched_ws.h: eight per-XCD queue heads, an arrival counter, a launch epoch, a sticky error word, and room for the partial
 * row statistics of oneprot_gemm_bf16_nt_resid_ln8 for up to M_max rows).  The caller owns it: oneprot_sched_workspace_bytes(M_max) bytes, 128-byte aligned,
 * zeroed ONCE (oneprot_sched_workspace_init: a memset enqueued on `stream`), then only ever touched by the kernels -- the last work-group to leave a launch
 * checks that the launch computed exactly the tiles it was given, resets the queue heads and advances the epoch, so a captured graph replays correctly.  One workspace serves one stream (launches that overlap in time must
 * not share one).  The statistics exchange crosses the XCDs' L2s: allocate the workspace with oneprot_alloc_uncached (hipExtMallocWithFlags(
 * hipDeviceMallocUncached); a host call like any allocation -- set-up code, never a launch path) and release it with oneprot_free_uncached. */
size_t oneprot_sched_workspace_bytes(int64_t M_max);
int oneprot_alloc_uncached(void** out, size_t bytes);
int oneprot_free_uncached(void* ptr);
int oneprot_sched_workspace_init(void* sched_ws, size_t bytes, void* stream);
/* Tiles of the persistent GEMM kernels drawn from the work queues of `sched_ws` instead of static per-work-group lists (NULL: static lists, the default).
 * With static lists a work-group that cannot start with the others -- another kernel (an RCCL channel of an overlapped gradient all-reduce, another process)
 * holds its CU -- runs its whole list after the others have finished: 1.47 x per launch whatever the number of CUs held.  With queues the running
 * work-groups share the tiles and late ones find the queue empty.  Results are bit-identical (which CU computes a tile changes no summation order).
 * Process-wide setting; the kernels of every stream then use this one workspace, so the streams must not overlap such launches. */
void oneprot_dynamic_tiles(void* sched_ws, size_t bytes);
/* diagnostic, host-synchronous: ticket draws that had not returned where the kernel first looked for them (each costs one drained operand prefetch; 0 expected) */
int oneprot_sched_late_draws(const void* sched_ws);
/* diagnostic, host-synchronous: launches completed on this workspace = its device-side epoch (-1: read failed) */
int64_t oneprot_sched_epoch(const void* sched_ws);
/* The same product with the row statistics completed ACROSS work-groups, for the launches whose K loop the full-row kernel above runs too slowly
 * (FFN-2, K = 4 d): x_out = resid + A W^T + bias (fp32; may alias resid) and h = LayerNorm(x_out) (bf16), by the 8-phase GEMM on 256 x 320 tiles; the
 * column tiles of a row panel exchange (mean, M2) partials through the sched workspace (hf modeling_esm.py:442-463 followed by :429 of the next layer or by
 * emb_layer_norm_after, sequence_encoder.py:76-81).  W as for oneprot_gemm_bf16_nt (not packed).  stats: fp32 [2][M] = mean | rstd, or NULL.
 * sched_ws / sched_ws_bytes: a sched workspace sized for at least M rows (-1 otherwise); the launch's tag comes from its device-side epoch.
 * oneprot_gemm_resid_ln8_eligible: 0 when (M, N, K) is not made of whole tiles this form serves (M % 256 == 0, N in {320, 640, 1280}, K % 128 == 0) -- the
 * caller runs oneprot_gemm_bf16_nt (ONEPROT_EPI_BIAS_RESID) + oneprot_layernorm_fwd --, 2 when it is and has the >= 192 tiles from which a persistent
 * work-group per CU pays, 1 when it is served but smaller (right, not faster: what the small-batch parity tests run).
 * FAILURE SEMANTICS.  A work-group waits, bounded, for the partials of the other column tiles of its row panel.  A wait that runs out (the partner work-group
 * never got a CU: fewer CUs free than the form needs) sets the workspace's sticky error word and the wave writes NaN into its rows of h, mean and rstd --
 * the next loss is NaN, not plausibly wrong -- and every later wait of that launch gives up at its first miss instead of spinning again.
 * oneprot_clip_coef(…, sched_ws, …) folds the word into the step's gradient norm on the device.  oneprot_gemm_resid_ln8_error: host-synchronous read of the
 * word (0 = clean; 1 = some launch on this workspace wrote NaN rows; 2 = a launch that drew its tiles from the work queues did not compute exactly the tiles it was
 * given -- a queue head that was not zero when it started: another stream sharing the workspace, a launch that never finished); _error_clear: enqueues its reset.  oneprot_gemm_resid_ln8_poll_bound: test hook, polls per wait
 * (default 2^20, about a second; < 0 restores it). */
int oneprot_gemm_resid_ln8_eligible(int64_t M, int N, int K);
int oneprot_gemm_resid_ln8_error(const void* sched_ws);
int oneprot_gemm_resid_ln8_error_clear(void* sched_ws, void* stream);
void oneprot_gemm_resid_ln8_poll_bound(int polls);
int oneprot_gemm_bf16_nt_resid_ln8(const void* A, const void* W, int64_t M, int N, int K, int lda, int ldb, const float* bias, const float* resid,
                                   float* x_out, const float* gamma, const float* beta, float eps, void* h_bf16, float* stats, void* sched_ws,
                                   size_t sched_ws_bytes, void* stream);
/* test / tuning hook: kernel form of oneprot_gemm_bf16_nt_resid_ln -- 0 (default): eight-wave work-groups on 128-row tiles, one per CU; 1: four-wave
   work-groups on 64-row tiles, two per CU (measured 5-9 % slower: kept as a tested variant).  Bit-identical results.  oneprot_gemm_ln_form_get: the current form. */
void oneprot_gemm_ln_form(int form);
int oneprot_gemm_ln_form_get(void);
/* test / tuning hook: force the kernel form of oneprot_gemm_bf16_nt (negative = heuristic; 0..8 per-tile block shapes, 17 / 19 / 20 = 1 / 3 / 4 with direct
 * stores, 32 (+ 64 * n) ping-pong, 40 / 41 / 42 the 8-phase forms: see csrc/gemm_nt.hip).  With any other id set, oneprot_gemm_bf16_nt returns OP_EINVAL. */
void oneprot_gemm_force_shape(int shape);
/* test / tuning hook: L2 super-tile of the per-tile kernels (sup_m row panels x sup_n column tiles per XCD at a time; <= 0 keeps a value). */
void oneprot_gemm_tune(int sup_m, int sup_n);
/* dW[N,K] (+)= dY[M,N]^T * X[M,K]  (contraction over the M tokens; split over workgroups, fp32 slabs in workspace);
   dbias[N] (+)= column sums of dY (optional, fused: an all-ones MFMA operand in the k-tile-0 workgroups). */
/* workspace bytes for an (N, K) weight gradient, for any M (the split count is capped by M inside the call, never raised). */
size_t oneprot_gemm_bf16_tn_workspace(int N, int K);
/* test / tuning hook: -1 = auto (default: the 8-phase 320 x 128 form where the problem is made of whole tiles, else 2), 0 = 64-token stages x2 (LDS-DMA ring),
   1 = 32-token stages x3, 2 = 64-token stages x2 with register-staged fill, 3 = 8-phase form where eligible (else 2). */
void oneprot_gemm_tn_variant(int v);
/* CUs left to co-resident kernels (the RCCL channels of a gradient all-reduce overlapped with the backward) when oneprot_gemm_bf16_tn cuts the token range into
   one-shot work items: at most (CUs - reserve) of them, so that none has to wait for a CU and run after the others (twice the launch time).  Changes the number of
   token splits, i.e. the (fixed) summation order.  Process-wide; default 0. */
void oneprot_cu_reserve(int cus);
/* workspace_bytes = size of `workspace`; -1 (invalid argument) when it is smaller than oneprot_gemm_bf16_tn_workspace(N, K). */
int oneprot_gemm_bf16_tn(const void* dY, const void* X, int64_t M, int N, int K, int ldy, int ldx, float* dW, float* dbias, void* workspace,
                         size_t workspace_bytes, int accumulate, void* stream);
/* The weight gradient above AND a LayerNorm backward over the same M token rows of width K in one launch, on disjoint CUs: the matrix work-groups leave half of the
   HBM rate unused, the row work-groups issue no MFMA, and neither waits for the other.  The LayerNorm half is oneprot_layernorm_bwd(dy bf16, x fp32) on
   [M, K]: dx = (add_to ? add_to : 0) + LN'(dy) (add_to may alias dx), optional bf16 copy -- both bit-identical to that entry point, row for row -- and
   dgamma / dbeta (optional, together) through ln_partial, at least ln_cus * 2 * K floats (oneprot_layernorm_bwd_workspace(K) bytes always suffice).
   ln_cus: the CUs (= work-groups) of the LayerNorm role, a multiple of 8 in [8, CUs - 64]; dW / dbias are then, bit for bit, those of oneprot_gemm_bf16_tn
   under oneprot_cu_reserve(ln_cus) (the process-wide reserve itself is not read).  Served: the 8-phase form with 256 x 320 tiles (K % 320 == 0, N % 64 == 0,
   N >= 256), M % 32 == 0, K <= 1280; anything else returns -1 before any launch and the caller keeps the two entry points. */
int oneprot_gemm_tn_ln_bwd_eligible(int64_t M, int N, int K);
int oneprot_gemm_tn_ln_bwd(const void* dY, const void* X, int64_t M, int N, int K, int ldy, int ldx, float* dW, float* dbias, void* workspace,
                           size_t workspace_bytes, int accumulate, const void* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                           const float* add_to, float* dx, void* dx_bf16, float* dgamma, float* dbeta, float* ln_partial, int accumulate_param_grads,
                           int ln_cus, void* stream);
/* fp32 GEMM for the small head / logits contractions (ref base_encoder.py:155,159,164; loss.py:91-99):
   C[M,N] = alpha * op(A) * op(B) (+ C if accumulate);  transA: A stored [K,M]; transB: B stored [K,N] else [N,K]. */
int oneprot_sgemm(const float* A, const float* B, float* C, int M, int N, int K, int transA, int b_is_kn, float alpha, int accumulate, void* stream);

/* ---------------- attention (hf modeling_esm.py:292-317,340-395) ------------------------------------------------- */
/* q = rotary(projection * hd^-1/2 * log2(e)) (what the QKV_ROPE epilogue writes when it is given q_scale = hd^-1/2 * log2 e: scores are in
   log2 units inside the kernels, so the softmax is exp2 without a multiply), k (rotated), v : bf16 [B,H,L,hd]; key_bias fp32 [B,L] (0 valid,
   -inf-like for padding); ctx bf16 [B*L, H*hd]; lse fp32 [B,H,L] (NATURAL log of the softmax denominator, incl. max). */
int oneprot_attn_fwd(const void* q, const void* k, const void* v, const float* key_bias, void* ctx, float* lse, int B, int H, int L, int hd,
                     void* stream);
/* dctx bf16 [B*L, H*hd] -> dqkv bf16 [B*L, 3*H*hd] = gradient w.r.t. the un-rotated, un-scaled q/k/v projections; q_scale here is the
   natural hd^-1/2 (the log2 e inside the stored q cancels in dq and is divided out of dk). */
size_t oneprot_attn_bwd_workspace(int B, int H, int L);
int oneprot_attn_bwd(const void* q, const void* k, const void* v, const float* key_bias, const void* ctx, const void* dctx, const float* lse,
                     const float* rope_cos, const float* rope_sin, float q_scale, void* dqkv, void* workspace, int B, int H, int L, int hd,
                     void* stream);
/* The forward with attention-probability dropout (hf modeling_bert.py BertSelfAttention: softmax -> nn.Dropout(attention_probs_dropout_prob) -> @ V;
   the reference leaves it active whenever the text tower is in train mode, text_encoder.py:59).  keep(b, h, q, k) is a pure function of
   (seed, stream_id, b*H+h, q, k) -- one integer hash per element, 16-bit threshold, kept probabilities scaled by the inverse keep probability;
   ctx = (keep * softmax / keep_prob) @ V, lse = that of the undropped softmax.  Same arguments as oneprot_attn_fwd otherwise. */
int oneprot_attn_fwd_dropout(const void* q, const void* k, const void* v, const float* key_bias, void* ctx, float* lse, int B, int H, int L, int hd,
                             float p, uint64_t seed, uint64_t stream_id, void* stream);
/* Its backward (the two split kernels; hd 16 / 32 / 64, any L): dV = (keep * P / keep_prob)^T dO, dS = P * (keep * dP / keep_prob - delta), the mask
   regenerated from the same (p, seed, stream_id).  Same arguments as oneprot_attn_bwd otherwise.
   In all three calls p becomes the 16-bit threshold thr16 = (unsigned)(p * 65536 + 0.5) in fp32: an element is kept iff the upper 16 bits of its hash are
   >= thr16, and kept values are scaled by 65536 / (65536 - thr16).  p < 2^-17 gives thr16 = 0, no dropout at all; p < 0, NaN, p >= 1 and any
   p >= 1 - 2^-17 (thr16 = 65536: nothing would be kept) are refused with OP_EINVAL, as is any other hd. */
int oneprot_attn_bwd_dropout(const void* q, const void* k, const void* v, const float* key_bias, const void* ctx, const void* dctx, const float* lse,
                             const float* rope_cos, const float* rope_sin, float q_scale, void* dqkv, void* workspace, int B, int H, int L, int hd,
                             float p, uint64_t seed, uint64_t stream_id, void* stream);
/* keep[B][H][L][L] (one byte each, 0 / 1): the mask the call above applies -- for tests and for a reference that is handed the mask. */
int oneprot_attn_dropout_keep(void* keep, int B, int H, int L, float p, uint64_t seed, uint64_t stream_id, void* stream);
/* Test / A-B hook: -1 automatic (default: by sequence length -- the split kernels up to L = 288, the 16-wave fused kernel up to 416, the
   8-wave fused kernel up to 512), 0 the two split kernels (dQ, then dK/dV), 1 the fused short-sequence kernel with 16 waves of 32 keys where
   eligible (L <= 512, hd <= 32: S, P, dP, dS formed once per tile; dQ summed in LDS in a fixed ticket order: deterministic like the split
   kernels), 2 the fused kernel with 8 waves of 64 keys (two key blocks per wave: Q / dO fragments read once per two tiles, one ticketed
   read-add-write of dQ per two tiles, deferred under the next step's MFMA chains). */
void oneprot_attn_force_bwd_path(int path);
/* Test / A-B hook for oneprot_attn_fwd: -1 automatic (default), 0 the round-1 kernel (per-tile running maximum), 1 the kernels without a row
   maximum (persistent LDS-DMA kernel for hd <= 32 and L <= 512, the chunked kernel otherwise; rows whose sums leave [2^-60, 2^60] are repeated
   with the running maximum), 2 the chunked kernel everywhere.  All three produce the same context / LSE up to the bf16 rounding of P. */
void oneprot_attn_force_fwd_path(int path);

/* ---------------- small fp32 feature ops (ref base_encoder.py:6-38, loss.py:103-114, oneprot_module.py:99-101) --- */
int oneprot_gelu_f32(const float* x, float* y, int64_t n, void* stream);
int oneprot_gelu_bwd_f32(const float* x, const float* dy, float* dx, int64_t n, void* stream);
/* y = scale * x / max(||x||, 1e-12) per row; inv_norm[r] saved for backward. */
int oneprot_l2norm_fwd(const float* x, float* y, float* inv_norm, int R, int D, float scale, void* stream);
/* dx = scale*inv_norm*(g - xhat*(xhat.g)), g = dy + l1_coef*sign(y)  (l1_coef = 0.01/(R*D) folds the L1 term's gradient). */
int oneprot_l2norm_bwd(const float* y, const float* dy, const float* inv_norm, float* dx, int R, int D, float scale, float l1_coef, void* stream);
/* Softmax cross-entropy over rows of logits [R,C] with label[r] = r + label_offset.  loss_sum += sum_r (lse_r - logit[r,label]) * row_weight;
   logits are overwritten with dlogits = (softmax - onehot) * row_weight. */
int oneprot_ce_fwd_bwd(float* logits, float* loss_sum, float* row_loss_ws /* R floats */, int R, int C, int label_offset, float row_weight, void* stream);
/* SigLIP block (ref loss.py:229-255) on logits [B,B] = scale*m@s^T: loss_sum += -sum logsigmoid(label*(logit+bias))/B with label +1 on the
   diagonal (-1 everywhere if negative_only); logits are overwritten with dloss/dlogit. */
int oneprot_siglip_fwd_bwd(float* logits, float* loss_sum, float* row_loss_ws /* B floats */, int B, float logit_bias, int negative_only, void* stream);
/* the same with the bias read from device memory (a learnable logit_bias tensor, ref loss.py:243-245; NULL = 0): no host synchronisation */
int oneprot_siglip_fwd_bwd_dev(float* logits, float* loss_sum, float* row_loss_ws /* B floats */, int B, const float* logit_bias_dev, int negative_only, void* stream);
/* retrieval ranks of the diagonal of logits [N,N] (ref retrieval_metric.py:83-102): rank_row[i] = #{j: logits[i][j] > logits[i][i]}, rank_col likewise on columns. */
int oneprot_diag_rank(const float* logits, int* rank_row, int* rank_col, int N, void* stream);
/* sum_abs += coef * sum |x|   (L1 feature regulariser, ref oneprot_module.py:101) */
int oneprot_abs_sum(const float* x, float* out_sum, void* workspace /* oneprot_sumsq_workspace() bytes */, int64_t n, float coef, void* stream);

/* out_sum += coef * sum x[i]*y[i]   (gradient of a tensor logit scale: sum(dlogits * logits) / scale, ref oneprot_module.py:142 feeds `log_logit_scale.exp()`) */
int oneprot_dot_f32(const float* x, const float* y, float* out_sum, void* workspace /* oneprot_sumsq_workspace() bytes */, int64_t n, float coef, void* stream);

/* dx (+)= coef * upstream[0] * sign(x); upstream is a device scalar (NULL = 1). */
int oneprot_l1_bwd(const float* x, float* dx, int64_t n, float coef, const float* upstream, int accumulate, void* stream);
int oneprot_scale_by_device_scalar(float* x, int64_t n, const float* s, void* stream);
/* bias[i] = ids[i]==pad ? -FLT_MAX : 0  (additive key-padding mask, hf masking_utils.create_bidirectional_mask) */
int oneprot_key_padding_bias(const int64_t* ids, float* bias, int64_t n, int pad_id, void* stream);

/* THE ELEMENT RULE of every Philox draw below (csrc/philox.h; host side and stream-id layout: oneprot_amd/rng.py): element e reads the 16-bit slice e & 7 --
   the low (even) or high (odd) half of word (e & 7) >> 1 -- of Philox4x32-10(counter = (e >> 3, stream_id), key = seed).  A dropout keeps e iff that slice
   >= thr = (unsigned)(p * 65536 + 0.5) in fp32 and scales kept values by 65536 / (65536 - thr); p < 0, NaN, p >= 1 and thr = 65536 are refused with OP_EINVAL.
   y = dropout(x) on a bf16 operand of n elements (n % 8 == 0) under that rule; the mask
   is a pure function of (seed, stream_id, element index) and is never stored.  Replaces the `lora_dropout` module peft 0.5.0
   applies to the adapter branch's input (ref src/models/components/sequence_encoder.py:61-74, text_encoder.py:39-52: LoraConfig(lora_dropout=...)).
   The generator is not torch's: same distribution, different stream. */
int oneprot_dropout_bf16(const void* x, void* y, int64_t n, float p, uint64_t seed, uint64_t stream_id, void* stream);
/* the same on fp32 (hidden-state dropout of the BERT tower: hf modeling_bert.py BertEmbeddings / BertSelfOutput / BertOutput); y may alias x. */
int oneprot_dropout_f32(const float* x, float* y, int64_t n, float p, uint64_t seed, uint64_t stream_id, void* stream);
/* y = resid + dropout(x): the dense output's dropout and the residual add that follows it in BertSelfOutput / BertOutput (hf modeling_bert.py) in one pass;
   the same mask as oneprot_dropout_f32 for the same (seed, stream_id); y may alias x or resid. */
int oneprot_dropout_add_f32(const float* x, const float* resid, float* y, int64_t n, float p, uint64_t seed, uint64_t stream_id, void* stream);
/* s = resid + dropout(x), then LayerNorm(s), one pass (hf modeling_bert.py:BertSelfOutput / BertOutput.forward: dense -> dropout -> LayerNorm(. + input);
 * the reference runs them whenever the text tower is in train mode, src/models/components/text_encoder.py:56-62).  Same mask as oneprot_dropout_add_f32 for
 * the same (seed, stream_id).  s_out (fp32 [T,d], the sum the LayerNorm backward needs) may be NULL; y_bf16 / y_f32 / mean / rstd as oneprot_layernorm_fwd;
 * d a multiple of 8, d <= 2048. */
int oneprot_dropout_add_layernorm_fwd(const float* x, const float* resid, float* s_out, const float* gamma, const float* beta, void* y_bf16, float* y_f32,
                                      float* mean, float* rstd, int64_t T, int d, float eps, float p, uint64_t seed, uint64_t stream_id, void* stream);
/* dx += mask(seed, stream_id) * dy / keep: the backward of the call above with the same (p, seed, stream_id), added into an existing bf16 gradient. */
int oneprot_dropout_bwd_add_bf16(const void* dy, void* dx, int64_t n, float p, uint64_t seed, uint64_t stream_id, void* stream);
/* the same into an fp32 gradient (the post-LN BERT tower keeps the layer-input gradient in fp32; ref text_encoder.py:39-52). */
int oneprot_dropout_bwd_add_f32(const void* dy, float* dx, int64_t n, float p, uint64_t seed, uint64_t stream_id, void* stream);

/* ---------------- optimiser (torch.optim.Adam, ref configs/model/default.yaml:2-6; clip: oneprot_module.py:106) -- */
/* sumsq[0] += sum x^2 (two-stage deterministic reduction through workspace of oneprot_sumsq_workspace() bytes). */
size_t oneprot_sumsq_workspace(void);
int oneprot_sumsq(const float* x, int64_t n, float* sumsq, void* workspace, void* stream);
/* coef[0] = min(1, max_norm / (sqrt(sumsq[0]) + 1e-6)); norm_out[0] = sqrt(sumsq[0]) */
int oneprot_clip_coef(const float* sumsq, float max_norm, float* coef, float* norm_out, const void* sched_ws /* optional: its error word turns norm and coef into NaN */, void* stream);
/* Adam step on a flat arena; g is multiplied by grad_scale[0] (device scalar, may be NULL) before use. step >= 1. */
int oneprot_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                      int step, const float* grad_scale, void* stream);

/* ---------------- casts ------------------------------------------------------------------------------------------ */
int oneprot_cast_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream);
int oneprot_transpose_cast_f32_to_bf16(const float* src, void* dst, int R, int C, void* stream);
/* the same for `count` matrices src + z*src_stride -> dst + z*dst_stride (strides in elements): one launch for a weight of every layer */
int oneprot_transpose_cast_f32_to_bf16_batched(const float* src, void* dst, int R, int C, int64_t src_stride, int64_t dst_stride, int count, void* stream);
size_t oneprot_colsum_workspace(int N);
int oneprot_colsum_bf16(const void* a, float* out, void* workspace, int64_t M, int N, int accumulate, void* stream);

/* ---------------- packed (variable-length) batches ------------------------------------------------------------------
 * A packed batch is a token stream: N sequences back to back, each with its own <cls> ... <eos>, in rows [cu_seqlens[b], cu_seqlens[b+1]) of
 * ids int64 [T_pad]; rows [cu_seqlens[N], T_pad) (the tail) hold pad ids.  cu_seqlens is int32 [N + 1] on the device.  Every row-wise kernel above
 * runs unchanged on the T_pad rows (the QKV GEMM with B = 1, L = T_pad, its rotary epilogue reading the per-token tables written below); these entry
 * points replace the layout-dependent ones.  The reference pads each batch instead (ref struct_token_dataset.py:87-88, collate with padding=True). */
/* embeddings (hf modeling_esm.py:224-271; ref sequence_encoder.py:78) with the token-dropout factor counted per sequence, kept per token in tok_scale
   [T_pad] (0 on the tail), plus the rotary tables gathered per token: cos_out / sin_out [T_pad, half] = rope_cos / rope_sin [n_pos, half] at the
   token's position within its sequence (hf modeling_esm.py:150-158 with positions restarting at 0 per sequence).  max_len <= n_pos. */
int oneprot_esm_embed_packed_fwd(const int64_t* ids, const int* cu_seqlens, const float* table, const float* rope_cos, const float* rope_sin, float* x,
                                 float* tok_scale, float* cos_out, float* sin_out, int N, int T_pad, int max_len, int d, int vocab, int half, int n_pos,
                                 int pad_id, int mask_id, int token_dropout, void* stream);
/* dtable (+)= per-token-scaled rows of dx; workspace: oneprot_esm_embed_bwd_workspace(T_pad, d, vocab).  Tail rows (pad ids) add nothing. */
int oneprot_esm_embed_packed_bwd(const int64_t* ids, const float* dx, const float* tok_scale, float* dtable, void* workspace, int T_pad, int d, int vocab,
                                 int pad_id, int mask_id, int token_dropout, int accumulate, void* stream);
/* attention over segments (hf modeling_esm.py:292-317, one softmax per sequence): q/k/v bf16 [H, T_pad, hd] (the QKV GEMM's head-major output
   with B = 1), work int32 [n_work][2] = (segment, 128-row block) items, longest segment first; ctx bf16 [T_pad, H*hd], lse fp32 [H, T_pad]
   (natural log); tail rows are written as 0.  hd 16 / 32 / 64, segments of 1 .. 1026 tokens. */
int oneprot_attn_varlen_fwd(const void* q, const void* k, const void* v, const int* cu_seqlens, const int* work, int n_work, void* ctx, float* lse,
                            int N, int T_pad, int H, int hd, void* stream);
size_t oneprot_attn_varlen_bwd_workspace(int H, int T_pad);
/* dqkv bf16 [T_pad, 3*H*hd] as oneprot_attn_bwd, the inverse rotary through the per-token tables of oneprot_esm_embed_packed_fwd; tail rows 0.
   Split dQ and dK/dV kernels, no atomics: deterministic. */
int oneprot_attn_varlen_bwd(const void* q, const void* k, const void* v, const int* cu_seqlens, const int* work, int n_work, const void* ctx,
                            const void* dctx, const float* lse, const float* rope_cos, const float* rope_sin, float q_scale, void* dqkv,
                            void* workspace, int N, int T_pad, int H, int hd, void* stream);
/* The same two calls with attention-probability dropout (hf modeling_bert.py BertSelfAttention: softmax -> dropout -> @ V, per sequence; ref
   text_encoder.py:54-62 runs the text tower in train mode, here on a packed batch of captions).  Element (query i, key j) of head h of segment s is
   kept iff the padded kernels keep element (i, j) of stream s * H + h: i, j are positions within the segment, s the segment's index in cu_seqlens (not
   its place in `work`).  A packed batch therefore drops exactly what oneprot_attn_fwd_dropout drops on the padded batch of the same sequences in the
   same order, and oneprot_attn_dropout_keep(keep, N, H, max_len, ...)[s, h, :n_s, :n_s] is its mask.  Row sum, LSE and delta are those of the undropped
   softmax.  p, seed, stream_id, hd and the rope tables (both NULL or both given) as oneprot_attn_fwd_dropout / oneprot_attn_bwd_dropout: OP_EINVAL
   and no launch otherwise. */
int oneprot_attn_varlen_fwd_dropout(const void* q, const void* k, const void* v, const int* cu_seqlens, const int* work, int n_work, void* ctx, float* lse,
                                    int N, int T_pad, int H, int hd, float p, uint64_t seed, uint64_t stream_id, void* stream);
int oneprot_attn_varlen_bwd_dropout(const void* q, const void* k, const void* v, const int* cu_seqlens, const int* work, int n_work, const void* ctx,
                                    const void* dctx, const float* lse, const float* rope_cos, const float* rope_sin, float q_scale, void* dqkv,
                                    void* workspace, int N, int T_pad, int H, int hd, float p, uint64_t seed, uint64_t stream_id, void* stream);
/* BERT embeddings on a packed stream (hf modeling_bert.py:53-108; ref text_encoder.py:54-62): row t = LN(word[id_t] + pos[t - start of t's segment] +
   type0), absolute positions restarting at every segment; tail rows take position 0 (finite).  pos is [n_pos, d]; every segment <= n_pos tokens (the
   caller checks: the kernel clamps the position).  d % 4 == 0, d <= 2048. */
int oneprot_bert_embed_packed_fwd(const int64_t* ids, const int* cu_seqlens, const float* word, const float* pos, const float* type0, const float* gamma,
                                  const float* beta, float* x_f32, void* x_bf16, int N, int T_pad, int d, int vocab, int n_pos, float eps, void* stream);
/* its position-table gradient (hf modeling_bert.py:53-108, position_embeddings; ref text_encoder.py:33 trains it when the tower is not frozen):
   dpos[l] = sum over the segments s with n_s > l of de[cu_seqlens[s] + l] for l < n_rows, segments in ascending order, no atomics (deterministic);
   rows no segment reaches are written as 0; the tail rows of de [T_pad, d] are never read. */
int oneprot_segment_possum_f32(const float* de, const int* cu_seqlens, float* dpos, int N, int T_pad, int n_rows, int d, void* stream);
/* pooling per segment without a LayerNorm in front (post-LN BERT; ref base_encoder.py:109-126 from text_encoder.py:54-62): mode 0 the mean over the
   segment's tokens != pad_id, 1 its first row: the rule of oneprot_pool_fwd.  x fp32 [T_pad, d] -> pooled [N, d]. */
int oneprot_pool_packed_fwd(const float* x, const int64_t* ids, const int* cu_seqlens, int pad_id, float* pooled, int N, int T_pad, int d, int mode,
                            void* stream);
/* its backward (ref base_encoder.py:109-126 under autograd): g fp32 [T_pad, d] (+ optional bf16 copy); tail rows exactly 0. */
int oneprot_pool_packed_bwd(const float* dpooled, const int64_t* ids, const int* cu_seqlens, int pad_id, float* g, void* g_bf16, int N, int T_pad, int d,
                            int mode, void* stream);
/* final LayerNorm fused with pooling per sequence (hf modeling_esm.py:552; ref base_encoder.py:109-126): mode 0 mean, 1 CLS; x fp32 [T_pad, d] ->
   pooled [N, d]; mean / rstd / wrow per stream row (wrow = 0 on the tail), hidden_f32 [T_pad, d] optional. */
int oneprot_lnpool_packed_fwd(const float* x, const int64_t* ids, const int* cu_seqlens, int pad_id, const float* gamma, const float* beta, float* pooled,
                              float* mean, float* rstd, float* wrow, float* hidden_f32, int N, int T_pad, int d, float eps, int mode, void* stream);
/* its backward: dx [T_pad, d] = LN'(dpooled[seq(t)] * wrow[t]) (exactly 0 on the tail), optional bf16 copy, dgamma / dbeta (workspace:
   oneprot_layernorm_bwd_workspace(d)). */
int oneprot_lnpool_packed_bwd(const float* dpooled, const int* cu_seqlens, const float* wrow, const float* x, const float* gamma, const float* mean,
                              const float* rstd, float* dx, void* dx_bf16, float* dgamma, float* dbeta, void* workspace, int N, int T_pad, int d,
                              void* stream);
/* Attention1dPooling per sequence (ref base_encoder.py:88-103): x fp32 [T_pad, d] (the normalised hidden state), attn [T_pad]; every sequence <= max_len. */
int oneprot_attnpool_packed_fwd(const float* x, const int64_t* ids, const int* cu_seqlens, int pad_id, const float* w, const float* bias, float* pooled,
                                float* attn, int N, int max_len, int d, void* stream);
/* its backward; dx (optional) [T_pad, d] with zero tail rows; workspace: oneprot_attnpool_bwd_workspace(N, d). */
int oneprot_attnpool_packed_bwd(const float* x, const float* attn, const int* cu_seqlens, const float* w, const float* dpooled, float* dw, float* db,
                                float* dx, void* workspace, int N, int T_pad, int max_len, int d, void* stream);

/* ---------------- retrieval without the N x N matrix (ref retrieval_metric.py:83-102, eval.py:158-184) --------------------------------------
 * S, M, Q, Db: fp32 row-major [rows, D], any D >= 1.  Every similarity is the k-ordered fp32 chain acc = fmaf(a_k, b_k, acc) from k = 0 (formed by
 * the fp32-input MFMA): the values of oneprot_sgemm with alpha = 1, bit for bit, so the ranks below equal those of oneprot_sgemm + oneprot_diag_rank. */
/* diag[i] = S_i . M_i, bit-equal to element (i, i) of the tiles of oneprot_sim_rank (ref retrieval_metric.py:86: the matching pair's similarity). */
int oneprot_sim_pair_dot(const float* S, const float* M, float* diag, int N, int D, void* stream);
/* The row slab [row0, row0 + rows) of S against all N rows of M (ref retrieval_metric.py:83-102: sort + position of the diagonal, here counted):
   rank_row[i] += #{ j : S_i . M_j > diag[i] } (complete for the slab's rows); rank_col[j] += #{ i in slab : S_i . M_j > diag[j] } (partial: summed over
   the slabs of a whole pass it is complete).  Strict >, int32 counts added with integer atomics (deterministic); the caller zeroes both before the first slab. */
int oneprot_sim_rank(const float* S, const float* M, const float* diag, int N, int D, int row0, int rows, int* rank_row, int* rank_col, void* stream);
/* oneprot_sim_rank with tie counts from the same tile values: rank_row / rank_col receive exactly what oneprot_sim_rank adds, and
   tie_row[i] += #{ j != i : S_i . M_j == diag[i] }, tie_col[j] += #{ i != j, i in slab : S_i . M_j == diag[j] } (the matching pair is left out by its index,
   not by its value; rows and columns past N count nothing).  rank + tie is the pessimistic rank.  The caller zeroes all four before the first slab. */
int oneprot_sim_rank_ties(const float* S, const float* M, const float* diag, int N, int D, int row0, int rows, int* rank_row, int* rank_col, int* tie_row, int* tie_col,
                          void* stream);
/* The k largest Q_i . Db_j over the N database rows for each of the nq queries (ref eval.py:158-184 ranks every row the same way): scores fp32 [nq, k]
   descending, indices int64 [nq, k]; equal scores in ascending database index.  1 <= k <= min(N, 256); finite inputs.  workspace: at least
   oneprot_sim_topk_workspace(nq, N, k) bytes (0 for invalid arguments), 8-byte aligned: [splits, nq, k] partial lists, never O(nq * N). */
size_t oneprot_sim_topk_workspace(int nq, int N, int k);
int oneprot_sim_topk(const float* Q, const float* Db, int nq, int N, int D, int k, float* scores, int64_t* indices, void* workspace, size_t workspace_bytes,
                     void* stream);

/* ---------------- MSA Transformer tower (ref msa_encoder.py:36: `self.transformer(tokens, repr_layers=[12])`, fair-esm's MSATransformer) ----------
 * Forward only (the reference freezes the tower, msa_encoder.py:30-32); eval mode, and the two *_dropout calls at the end for the train-mode
 * forward.  fair-esm is not part of this tree: the call sites below are named by
 * their published functions, and parity with a fair-esm run is UNPINNED (the tests compare against tests/msa_ref.py, an fp64 restatement).
 * Tokens int64 [B, R, L], numbered t = (b * R + r) * L + l, T = B * R * L.  qkv: bf16 [T, 3 * H * 64] = q | k | v of one oneprot_gemm_bf16_nt
 * (ONEPROT_EPI_BF16 + bias) on the stacked projection weights, head h in columns h * 64 .. h * 64 + 63 of each third.  key_bias: fp32 [T] from
 * oneprot_key_padding_bias (0 = token, anything else = padding).  ctx: bf16 [T, H * 64].  hd must be 64 (-1 otherwise).  A masked key is excluded
 * (probability 0) instead of biased by -10000: the two differ only where every key of a query is masked -- padded positions -- which hold 0 here. */
#define ONEPROT_MSA_MAX_LEN 1024      /* longest row L of the tied row attention                       */
#define ONEPROT_MSA_MAX_ROWS 128      /* deepest MSA R of oneprot_msa_col_attn (R = 1: two GEMMs, host) */
/* x fp32 [T, d] = LayerNorm(tok_table[id] + pos_table[pos] + row_table[r]) * (id != pad_id), pos = (non-pad tokens of the row up to and including l) +
   pad_id, pad_id at padding (fair-esm MSATransformer.forward: embed_tokens + LearnedPositionalEmbedding + msa_position_embedding, emb_layer_norm_before,
   `x * (1 - padding_mask)`).  pos_table [n_pos, d] with n_pos >= L + pad_id + 1; row_table [n_rows, d] with n_rows >= R; d <= 2048. */
int oneprot_msa_embed_fwd(const int64_t* tokens, const float* tok_table, const float* pos_table, const float* row_table, const float* gamma,
                          const float* beta, float* x, int B, int R, int L, int d, int vocab, int n_pos, int n_rows, int pad_id, float eps, void* stream);
/* Tied row attention scores (fair-esm RowSelfAttention.compute_attention_weights): S fp32 [B, H, L, L],
   S[b,h,i,j] = scale * sum_{r,c} q[b,r,i,h,c] k[b,r,j,h,c] with q taken as 0 at padded (r, i); scale = hd^-1/2 / sqrt(R).  fp32 accumulation over r = 0 .. R-1
   in that order inside one work-group: no split along K, no atomics, independent of the rest of the batch.  L <= ONEPROT_MSA_MAX_LEN. */
int oneprot_msa_row_scores(const void* qkv, const float* key_bias, float* S, int B, int R, int L, int H, int hd, float scale, void* stream);
/* softmax over j of S with the keys where ROW 0 is padded masked, P rounded to bf16, ctx[b,r,i,h,:] = sum_j P[b,h,i,j] v[b,r,j,h,:] with fp32 accumulation
   (fair-esm RowSelfAttention.compute_attention_update; S is read, not re-derived).  Three launches: the probabilities bf16 [B, H, L, Lp] and V transposed
   bf16 [B, H, R, 64, Lp] (Lp = L rounded up to 32) are formed in `workspace` (16-byte aligned, at least oneprot_msa_row_context_workspace(B, R, L, H)
   bytes, -1 otherwise; the query returns 0 for invalid arguments), then ctx^T = V^T P^T on MFMA tiles. */
size_t oneprot_msa_row_context_workspace(int B, int R, int L, int H);
int oneprot_msa_row_context(const float* S, const void* qkv, const float* key_bias, void* ctx, void* workspace, size_t workspace_bytes, int B, int R, int L,
                            int H, int hd, void* stream);
/* Column attention for 2 <= R <= ONEPROT_MSA_MAX_ROWS (fair-esm ColumnSelfAttention.compute_attention_update): for each (b, l, h) softmax_j(scale * q_i . k_j)
   over the rows j whose token (j, l) is not padding, ctx = P v; scale = hd^-1/2; a query whose keys are all masked gets 0.  A larger R returns -1; R = 1 is
   out_proj(v_proj(x)) on the host, as published. */
int oneprot_msa_col_attn(const void* qkv, const float* key_bias, void* ctx, int B, int R, int L, int H, int hd, float scale, void* stream);
/* Train-mode twins of the two calls above: fair-esm applies nn.Dropout(attention_dropout) to the probabilities between the softmax and the product
   with V, and the reference runs its frozen tower in train mode during training (Lightning's module.train() undoes msa_encoder.py:30).  The mask is the
   per-element hash of oneprot_attn_dropout_keep (same rule, same thr16 / scale, same refusals of p: p < 0, NaN and p >= 1 return -1; p < 2^-17 is no dropout at
   all and equals the undropped call bit for bit); a dropped probability is 0, a kept one bf16(p_ij * 65536 / (65536 - thr16)), scaled in fp32 before its one
   rounding; row maximum and sum are those of the undropped softmax.  Our generator, not torch's: the same distribution as nn.Dropout, another draw.
   oneprot_msa_row_context_dropout (fair-esm RowSelfAttention.compute_attention_update: `attn_probs = self.dropout_module(attn_probs)`): the attention is
   tied, so there is ONE mask element per (b, h, i, j) for all R rows, keep(q = i, k = j, bh = (b_first + b) * H + h) -- in the layout of
   oneprot_attn_dropout_keep(keep, B_total, H, L, ...): keep[b_first + b, h, i, j].  b_first is the place of the call's first MSA in the whole batch, so
   that a batch run in groups of whole MSAs drops what the one call would; b_first < 0 or (b_first + B) * H > 65535 returns -1.
   oneprot_msa_col_attn_dropout (fair-esm ColumnSelfAttention.compute_attention_update, R > 1: `attn_probs = self.dropout_module(attn_probs)`): one mask
   element per (b, h, l, i, j), keep(q = i, k = j, bh = (b * H + h) * L + l) -- oneprot_attn_dropout_keep(keep, B * H * L, 1, R, ...) viewed as
   [B, H, L, R, R]; L <= ONEPROT_MSA_MAX_LEN.  R = 1 returns -1 as in the undropped call: the published shortcut has no attention dropout. */
int oneprot_msa_row_context_dropout(const float* S, const void* qkv, const float* key_bias, void* ctx, void* workspace, size_t workspace_bytes, int B, int R,
                                    int L, int H, int hd, int b_first, float p, uint64_t seed, uint64_t stream_id, void* stream);
int oneprot_msa_col_attn_dropout(const void* qkv, const float* key_bias, void* ctx, int B, int R, int L, int H, int hd, float scale, float p, uint64_t seed,
                                 uint64_t stream_id, void* stream);
/* Ragged batches: a stream of n MSAs, each a dense R_b x L_b block at its own depth and length (host type oneprot_amd.packing.PackedMsa).  Token
   t = cu_tokens[b] + r * L_b + l of a stream of T_pad rows (a multiple of 256), the tail [T_tokens, T_pad) filled with the pad id.  What is cut is an MSA's
   trailing all-pad rows and columns, and the cut is exact: in the published forward such a row has q = 0 and is an excluded key of the column attention,
   such a column is a masked key of the row attention (row 0 is padded there), and positions and the row embedding do not look past a token's own row
   (fair-esm RowSelfAttention.compute_attention_weights, ColumnSelfAttention.compute_attention_update, LearnedPositionalEmbedding).  Each call below
   gives, at every position of a block, the bits its padded twin above gives there on the padded batch.  One number of the padded batch is kept: the
   row scale hd^-1/2 / sqrt(R) of RowSelfAttention.align_scaling uses the PADDED row count, so `scale` is the caller's.
   geo: int64 [n, 8] on the device, 16-byte aligned, one row per MSA of the call in launch order (the host puts the longest first):
     {tok0, R_b, L_b, s0, p0, vt0, b, 0} = first token of the block in the stream; its shape; where its S [H, L_b, L_b] starts (fp32 elements of S), where
     its P [H, L_b, Lp_b] and Vt [H, R_b, 64, Lp_b] start (bf16 elements from the start of the workspace, Lp_b = L_b rounded up to 32); the MSA's index
     (for the dropout streams).  The table lives on the device and is NOT validated: the host type builds it.  max_R / max_L: the largest R_b / L_b of
     the call (the launch grid; a work-group outside its own MSA's extent leaves before any barrier).  n * H <= 65535, max_L <= ONEPROT_MSA_MAX_LEN.
   Every ragged attention call writes the tail rows of ctx as 0, as oneprot_attn_varlen_fwd does. */
/* oneprot_msa_embed_fwd per block: row index and position count run inside the token's own R_b x L_b block (fair-esm MSATransformer.forward,
   LearnedPositionalEmbedding); cu_tokens int32 [n + 1], row_lens int32 [n] = L_b; tail rows of x are written as 0.  max_R <= n_rows,
   max_L + pad_id + 1 <= n_pos. */
int oneprot_msa_embed_ragged_fwd(const int64_t* tokens, const int* cu_tokens, const int* row_lens, const float* tok_table, const float* pos_table,
                                 const float* row_table, const float* gamma, const float* beta, float* x, int n, int T_pad, int max_R, int max_L, int d, int vocab,
                                 int n_pos, int n_rows, int pad_id, float eps, void* stream);
/* oneprot_msa_row_scores per block (fair-esm RowSelfAttention.compute_attention_weights): S = the concatenation of the per-MSA [H, L_b, L_b] maps at
   their s0; rows r = 0 .. R_b - 1 in that order, no split, no atomics. */
int oneprot_msa_row_scores_ragged(const void* qkv, const float* key_bias, float* S, const int64_t* geo, int n, int max_L, int H, int hd, float scale, void* stream);
/* oneprot_msa_row_context per block (fair-esm RowSelfAttention.compute_attention_update).  sum_l_lp = sum of L_b * Lp_b, sum_r_lp = sum of R_b * Lp_b over
   the call's MSAs (both multiples of 32): the workspace holds H * (sum_l_lp + 64 * sum_r_lp) bf16 (the query returns 0 for invalid arguments). */
size_t oneprot_msa_row_context_ragged_workspace(int64_t sum_l_lp, int64_t sum_r_lp, int H);
int oneprot_msa_row_context_ragged(const float* S, const void* qkv, const float* key_bias, void* ctx, void* workspace, size_t workspace_bytes, const int64_t* geo,
                                   int n, int max_R, int max_L, int64_t sum_l_lp, int64_t sum_r_lp, int H, int hd, int T_tokens, int T_pad, void* stream);
/* oneprot_msa_col_attn per block (fair-esm ColumnSelfAttention.compute_attention_update), 1 <= R_b <= ONEPROT_MSA_MAX_ROWS: R_b = 1 has one live key, so
   P = 1 and ctx = v, which is what the padded kernel gives that MSA inside a deeper batch. */
int oneprot_msa_col_attn_ragged(const void* qkv, const float* key_bias, void* ctx, const int64_t* geo, int n, int max_R, int max_L, int H, int hd, float scale,
                                int T_tokens, int T_pad, void* stream);
/* Their train-mode twins (fair-esm `attn_probs = self.dropout_module(attn_probs)` in both attentions): the mask element of the padded batch the stream
   stands for.  Row: keep(q = i, k = j, bh = (b_first + b) * H + h) with b the table's index; column: keep(q = i, k = j, bh = (b * H + h) * l_stride + l)
   with l_stride the padded batch's L (max_L <= l_stride <= ONEPROT_MSA_MAX_LEN).  Refusals of p as above. */
int oneprot_msa_row_context_ragged_dropout(const float* S, const void* qkv, const float* key_bias, void* ctx, void* workspace, size_t workspace_bytes,
                                           const int64_t* geo, int n, int max_R, int max_L, int64_t sum_l_lp, int64_t sum_r_lp, int H, int hd, int T_tokens,
                                           int T_pad, int b_first, float p, uint64_t seed, uint64_t stream_id, void* stream);
int oneprot_msa_col_attn_ragged_dropout(const void* qkv, const float* key_bias, void* ctx, const int64_t* geo, int n, int max_R, int max_L, int H, int hd,
                                        float scale, int T_tokens, int T_pad, int l_stride, float p, uint64_t seed, uint64_t stream_id, void* stream);

/* ---------------- MSA input (ref src/data/datasets/msa_dataset.py:42-58: read_msa, greedy_select, the two tokenizers) ------------------------------
 * A batch of n alignments as one byte stream.  msa_bytes: uint8, 16-byte aligned, n_bytes long; MSA b holds N_b rows of L_b letters (insertions already
 * removed), row j at byte0_b + j * stride_b with stride_b = L_b rounded up to 16 and the bytes [L_b, stride_b) of every row 0: the host pads, so that
 * every 16-byte load is aligned and the padding is no mismatch.  table: int64 [n, 4] = {byte0_b (a multiple of 16), N_b, L_b, k_b} on the device, and
 * table_host the same numbers in host memory: the entry points validate and size their launches from the host copy, the kernels read the device one
 * (oneprot_amd.msa_data builds both from one array).  Refused with -1 before any launch: n outside 1..65535, N_b < 1, L_b outside 1..65535, k_b
 * outside 1..k_max, k_max > 1024, a block outside [0, n_bytes), a workspace that is too small, a pointer that is not aligned. */
/* ref src/data/utils/msa_utils.py:21-40 `greedy_select(msa, num_seqs, mode)` for every MSA of the batch, as an exact integer rule: S_j = the sum over
   the rows chosen so far of the number of positions where that row and row j differ; every step picks the unselected j with the largest (min_mode 1:
   smallest) S_j, the lowest j among equal S_j; the first pick is row 0 and min(k_b, N_b) rows are picked.  (The reference averages in fp64, which
   orders equal sums by rounding noise: DESIGN.md section 7.)  indices int32 [n, k_max]: the picks in ascending order, -1 behind them; order (optional)
   int32 [n, k_max]: the picks in the order made.  max over b of min(k_b, N_b) - 1 step launches and two small ones, all on `stream`, nothing read back.
   workspace: 16-byte aligned, at least oneprot_msa_select_workspace(n, k_max, sum of N_b, largest N_b) bytes (0 for invalid arguments); not cleared. */
size_t oneprot_msa_select_workspace(int n, int k_max, int64_t total_rows, int64_t max_rows);
int oneprot_msa_select(const void* msa_bytes, const int64_t* table, void* workspace, int* indices, int* order, const int64_t* table_host,
                       size_t workspace_bytes, int64_t n_bytes, int n, int k_max, int min_mode, void* stream);
/* ref msa_dataset.py:54-56: fair-esm's MSA batch converter (`get_batch_converter(truncation_seq_length=1022)`, then `msa_input[:, :, :max_length]`) and
   the HF ESM-2 tokenizer (`padding=True, truncation=True`) on row 0.  Row r of MSA b is row indices[b, r] of its block (int32 [n, k_max], the output
   of oneprot_msa_select; min(k_b, N_b) rows are read), written as cls_id followed by byte_map[letter] (int32 [256]) for the first
   Lt_b - 1 = min(L_b, 1022, max_length - 1) letters.  cu_tokens NULL: tokens int64 [n, R_max, Lt_max], pad_id outside the blocks.  cu_tokens int32
   [n + 1] (device; the host derives it from the table): tokens int64 [T_pad], block b dense min(k_b, N_b) x Lt_b at cu_tokens[b] -- the ids of
   oneprot_amd.packing.PackedMsa -- and pad_id from the end of the last block to T_pad.  seq_tokens (optional) int64 [n, Ls_max]: row 0 of the block
   (not of the selection: greedy_select keeps row 0) as cls_id, the first Ls_b - 2 letters, eos_id, then pad_id, Ls_b = min(L_b + 2, max_length).
   R_max / Lt_max / Ls_max below what the table needs, max_length < 2 and T_pad below the token count return -1. */
int oneprot_msa_tokenize(const void* msa_bytes, const int64_t* table, const int* indices, const int* byte_map, int64_t* tokens, const int* cu_tokens,
                         int64_t* seq_tokens, const int64_t* table_host, int64_t n_bytes, int n, int k_max, int R_max, int Lt_max, int Ls_max,
                         int max_length, int64_t T_pad, int cls_id, int pad_id, int eos_id, void* stream);

/* ---------------- text input (ref src/data/datasets/text_dataset.py:25,51: `AutoTokenizer.from_pretrained(text_tokenizer)` and its call with
 * `padding=True, truncation=True`, HF's fast BERT tokenizer) ------------------------------------------------------------------------------------------
 * BertNormalizer + BertPreTokenizer + WordPiece(max_input_chars_per_word = 100) + [CLS] .. [SEP] + truncation of a whole batch in one launch, one
 * work-group per text, integer arithmetic only, no atomics (csrc/wordpiece.hip; the rule is stated once in DESIGN.md section 7 and is
 * oneprot_amd.text_data.BertWordPieceTokenizer.encode_all on the host).  All state lives in LDS, so there is no workspace and no size query.
 * text_bytes: the texts' UTF-8 bytes, concatenated, n_bytes long; offsets int64 [n_texts + 1] on the device (text b is bytes
 * [offsets[b], offsets[b + 1])) and offsets_host the same numbers in host memory, from which the call validates.
 * The normalisation table has two levels: norm_index int32 [0x1100] gives the block of code point c as norm_index[c >> 8], and
 * norm_entries int32 [n_blocks, 256] its entry: bits 23-24 the number of characters it becomes (0: dropped), bits 21-22 the kind of that character
 * (0 part of a word, 1 a word of its own: punctuation and CJK, 2 space) and bits 0-20 its code point when that number is 1, or bits 0-20 an index into
 * norm_pool int32 [n_pool] (code point | kind << 21 per character) when it is 2 or 3.
 * The vocabulary is an open-addressing table: vocab_slots int32 [n_slots, 4] = {key, first character in vocab_chars, length | keyspace << 16, id},
 * 16-byte aligned, n_slots a power of two, id -1 in an empty slot; vocab_chars int32 [n_vocab_chars] the pieces' code points; keyspace 1 holds the
 * "##" pieces without their prefix.  key = fmix32(h ^ length * 0x9e3779b1 ^ (keyspace ? 0x85ebca6b : 0)) with h = h * 0x01000193 + c + 1 (mod 2^32)
 * over the characters and fmix32 MurmurHash3's finaliser; a piece lives at the first free slot from key & (n_slots - 1) upwards.  A hit is verified
 * against the stored characters.  max_piece_chars: the length of the longest piece (1 .. 100), which bounds the greedy search.
 * ids int32 [n_texts, max_length]: cls_id, the first max_length - 2 pieces, sep_id, then pad_id; lengths int32 [n_texts] the ids before the padding.
 * Refused with -1 before any launch: a NULL pointer, n_texts outside 1 .. ONEPROT_WORDPIECE_MAX_TEXTS, max_length outside 2 ..
 * ONEPROT_WORDPIECE_MAX_LENGTH, offsets_host that decrease or leave [0, n_bytes], n_slots no power of two or below 2, n_blocks outside 1 .. 0x1100,
 * n_pool or n_vocab_chars below 1, max_piece_chars outside 1 .. 100, a negative special id, vocab_slots not 16-byte aligned. */
#define ONEPROT_WORDPIECE_MAX_TEXTS 1048576
#define ONEPROT_WORDPIECE_MAX_LENGTH 65535
int oneprot_wordpiece_encode(const void* text_bytes, const int64_t* offsets, const int* norm_index, const int* norm_entries, const int* norm_pool,
                             const int* vocab_slots, const int* vocab_chars, int* ids, int* lengths, const int64_t* offsets_host, int64_t n_bytes,
                             int n_texts, int n_blocks, int n_pool, int n_slots, int n_vocab_chars, int max_piece_chars, int max_length, int cls_id,
                             int sep_id, int unk_id, int pad_id, void* stream);

/* ---------------- graph input (ref src/data/utils/struct_graph_utils.py:31-144: `get_atom_pos`, `compute_diherals`, `calc_side_chain_embs`,
 * `calc_bb_embs`, called once per protein by protein_to_graph) -------------------------------------------------------------------------------------------
 * The atom records of a whole batch of G proteins to the tensors of its GraphBatch, two launches on `stream`, one thread per residue, fp32, no
 * atomics, no workspace, nothing read back (csrc/graph_feats.hip; the rule is stated once in DESIGN.md section 7 and is the four host functions of
 * oneprot_amd/graph_data.py).  A residue's results depend on its own atoms and on the N / CA / C of its two neighbours inside its protein only, so a
 * protein gets the same bits alone and in any batch.
 * atom_pos fp32 [A, 3]; atom_name4 [A]: the first four bytes of every atom name, zero padded, as one 32-bit word (numpy's `names.astype("S4")` viewed
 * as 32-bit words; the 20 names of the nine places have at most 3 bytes, so cutting a longer name can make no match); res_atom_ptr int64 [N + 1]:
 * residue r owns the atoms [res_atom_ptr[r], res_atom_ptr[r + 1]), possibly none; res_type_bytes uint8 [N]; graph_ptr int64 [G + 1]: protein g owns
 * the residues [graph_ptr[g], graph_ptr[g + 1]).  res_atom_ptr_host / graph_ptr_host: the same two tables in host memory, from which the call validates.
 * Out: x int64 [N, 1]; coords_ca / coords_n / coords_c fp32 [N, 3] (for each of N, CA, C, CB, *G, *D, *E, *Z, NH1 the LAST atom of the run whose
 * name is in the place's set, NaN without one; a NaN component of N or C takes CA's); bb_embs fp32 [N, 6] (cos then sin of phi, psi, omega along
 * the protein's N, CA, C chain, differences normalised; phi of a protein's first residue and psi, omega of its last are angle 0); side_chain_embs
 * fp32 [N, 8] (sin then cos of the four torsions over N-CA-CB-G-D-E-Z); batch int64 [N]; ptr int64 [G + 1].  Wherever the host's nan_to_num chain
 * yields angle 0 (a NaN operand, a zero middle vector, atan2(0, 0)) the outputs are exactly (sin, cos) = (0, 1).
 * Refused with -1 before any launch: a NULL pointer, N or G below 1, N above ONEPROT_GRAPH_MAX_NODES, G above N, a table that does not start at 0 or
 * that decreases, a graph_ptr that does not end at N, a res_atom_ptr that does not end at A. */
#define ONEPROT_GRAPH_MAX_NODES 67108864
int oneprot_graph_featurize(const float* atom_pos, const int* atom_name4, const int64_t* res_atom_ptr, const void* res_type_bytes,
                            const int64_t* graph_ptr, int64_t* x, float* coords_ca, float* coords_n, float* coords_c, float* bb_embs,
                            float* side_chain_embs, int64_t* batch, int64_t* ptr, const int64_t* res_atom_ptr_host, const int64_t* graph_ptr_host,
                            int64_t A, int64_t N, int G, void* stream);

/* ---------------- ProNet tower (ref src/models/components/struct_graph_encoder.py:5-42 plugs in dig.threedgraph.method.ProNet; the arithmetic is the
 * published model's, Wang et al. 2023, restated: DESIGN.md section 7, tests/pronet_ref.py is the oracle) ----------------------------------------------
 * N nodes of n_graphs graphs in one batch, a graph's nodes contiguous: graph_ptr int32 [n_graphs + 1], batch int32 [N].  Edges are stored by target in a
 * table ONEPROT_PRONET_SLOTS wide: nbr int32 [N, 32] (sources ascending, -1 behind the first deg[i]), and "slot" i * 32 + e names edge e of target i in
 * every per-edge array.  N <= 2^26.  All of it fp32, no atomics: every sum runs in a fixed order and two runs give the same bits. */
#define ONEPROT_PRONET_SLOTS 32
/* Replaces torch_cluster.radius_graph(pos, r=cutoff, batch, max_num_neighbors) in ProNet.forward: sources j != i of i's graph with |ca_j - ca_i|^2 <=
   cutoff^2 (fp32: products and sums rounded one by one, no FMA), the max_num_neighbors <= 32 LOWEST indices when more are in range (torch_cluster's
   GPU rule).  Any graph size. */
int oneprot_radius_graph(const float* ca, const int* graph_ptr, const int* batch, int* nbr, int* deg, int N, int n_graphs, float cutoff, int max_num_neighbors,
                         void* stream);
/* The same edges grouped by source (what autograd's scatter-add backward of `x_j = x[edge_index[0]]` walks with float atomics): src_off int32 [N + 1],
   src_list int32 [32 N] of slots, for every source its edges with the target ascending.  count_ws int32 [N].  Nothing is read back. */
int oneprot_graph_by_source(const int* graph_ptr, const int* batch, const int* nbr, const int* deg, int* count_ws, int* src_off, int* src_list, int N,
                            int n_graphs, void* stream);
/* Replaces ProNet.forward's per-edge geometry (dist, theta, phi from the CA triplets with neighbours (i -+ 1) mod N over the whole batch; the three Euler
   angles between the backbone frames of i and j) and its three embeddings (emb: dist / theta / phi -> feature0 [4 nr]; the torsion embedding on the
   Euler angles -> feature1 [6 nr]; the sinusoidal j - i embedding -> feature2 [np]), num_spherical = 2, no envelope.  consts fp32 [4 nr + np / 2]:
   the Bessel zeros z_{l,n} (l major), the normalisers sqrt(2) / |j_{l+1}(z_{l,n})|, the np / 2 frequencies.  f0 / f1 / f2 are [32 N, width]; unfilled
   slots are written as 0.  noise != 0: each Euler angle gains clip(sigma * normal, +-clip), the normals being Box-Muller pairs (uniforms ((w >> 9) + 1/2) 2^-23: r = sqrt(-2 ln u1), r cos 2 pi u2 and r sin 2 pi u2) of
   Philox4x32-10(counter = slot, stream_id; key = seed), words (0, 1) -> angles 0 and 1, words (2, 3) -> angle 2.  nr <= 8, np even <= 48. */
int oneprot_pronet_edge_features(const float* ca, const float* cn, const float* cc, const int* nbr, const int* deg, const float* consts, float* f0, float* f1,
                                 float* f2, int N, int num_radial, int num_pos_emb, float cutoff, int noise, float sigma, float clip, uint64_t seed,
                                 uint64_t stream_id, void* stream);
/* Replaces DIG's EdgeGraphConv (propagate with message = edge_weight * x_j, aggr add) together with the TwoLinear that makes edge_weight:
   m[i, :] = sum_e (W2 W1 feat[i * 32 + e, :]) * a[nbr[i, e], :].  WfT fp32 [F, h] is the folded operand (W2 W1)^T; neither w_e nor the messages are
   written.  h a multiple of 64 up to 256, F <= 48. */
int oneprot_edge_conv_fwd(const float* feat, const float* WfT, const float* a, const int* nbr, const int* deg, float* m, int N, int h, int F, void* stream);
/* Its data gradient (autograd's index_add of dm[i] * w_e into source j): da[j, :] = sum over the edges out of j, targets ascending, w_e recomputed. */
int oneprot_edge_conv_bwd_x(const float* feat, const float* WfT, const float* dm, const int* src_off, const int* src_list, float* da, int N, int h, int F,
                            void* stream);
/* The gradient of the folded operand (autograd's two TwoLinear weight gradients over [E, .] operands): dWfT[f, c] = sum_e dm[i, c] a[j, c] feat[slot, f];
   per-work-group partials over fixed target ranges, then one ordered sum.  workspace: oneprot_edge_conv_bwd_w_workspace bytes (0 for a bad shape). */
size_t oneprot_edge_conv_bwd_w_workspace(int N, int h, int F);
int oneprot_edge_conv_bwd_w(const float* feat, const float* a, const float* dm, const int* nbr, const int* deg, float* dWfT, void* workspace,
                            size_t workspace_bytes, int N, int h, int F, void* stream);
/* Replaces ProNet.forward's `self.embedding(torch.cat([F.one_hot(z, 26), bb_embs], dim=1))`: a gathered weight column, a 6-wide product and the bias.
   W fp32 [h, 32], z int64 [N], bb fp32 [N, 6]; feat_out (optional) fp32 [N, 32] is the concatenated input, the operand of the weight-gradient GEMM. */
int oneprot_pronet_embed_fwd(const int64_t* z, const float* bb, const float* W, const float* b, float* x0, float* feat_out, int N, int h, void* stream);
/* The node-side row ops around oneprot_sgemm (torch's `act(lin(x))`, swish = x * sigmoid(x), F.relu): z[M, n] += bias in place (bias optional), then
   y[r * ldy + c] = act(z[r, c]) + resid[r, c] (y, resid optional; ldy >= n writes into a column block of a wider matrix, which is torch.cat).
   act 0 identity, 1 swish, 2 relu.  The backward: dz[r, c] = dy[r * ldy + c] * act'(z[r, c]). */
int oneprot_pronet_bias_act(float* z, const float* bias, const float* resid, float* y, int64_t M, int n, int ldy, int act, void* stream);
int oneprot_pronet_act_bwd(const float* dy, const float* z, float* dz, int64_t M, int n, int ldy, int act, void* stream);
/* out[c] = sum_r x[r, c] of an fp32 [M, n] matrix (autograd's bias gradient `grad.sum(0)` with M = every node of the batch): blocked summation in a
   fixed order, no chain longer than 8, in parallel over row chunks -- oneprot_rowsum_f32 is one serial chain per column, made for a handful of rows.
   workspace: oneprot_colsum_f32_workspace(M, n) bytes (0 for a bad shape). */
size_t oneprot_colsum_f32_workspace(int64_t M, int n);
int oneprot_colsum_f32(const float* x, float* out, void* workspace, size_t workspace_bytes, int64_t M, int n, void* stream);
/* dW[n, k] = sum_r dz[r, n] x[r, k] of fp32 dz [M, n] and x [M, k] (autograd's weight gradient `dz.t() @ x` with M = every node of the batch), blocked like
   the column sum: chains of at most 128 rows (M / 256 beyond 32 768 rows) in parallel, then eight accumulators and a tree over the row blocks -- where
   oneprot_sgemm(transA = 1, b_is_kn = 1) runs one chain of M terms.  M <= 2^26, n and k <= 4096.  workspace: oneprot_wgrad_f32_workspace(M, n, k) bytes
   (0 for a bad shape). */
size_t oneprot_wgrad_f32_workspace(int64_t M, int n, int k);
int oneprot_wgrad_f32(const float* dz, const float* x, float* dW, void* workspace, size_t workspace_bytes, int64_t M, int n, int k, void* stream);
/* Replaces `x + torch.clip(torch.empty_like(x).normal_(0, sigma), -clip, clip)` (ProNet's data_augment_eachlayer): element e takes normal e & 3 of
   Philox4x32-10(counter = e >> 2, stream_id; key = seed), Box-Muller as above.  n a multiple of 4; y may alias x.  Its backward is the identity. */
int oneprot_clipped_normal_add_f32(const float* x, float* y, int64_t n, float sigma, float clip, uint64_t seed, uint64_t stream_id, void* stream);
/* Replaces torch_scatter's `scatter(x, batch, dim=0)` (sum readout) and its backward: y[g] = sum of the rows of graph g in index order; dx[i] = dy[batch[i]]. */
int oneprot_segment_sum_f32(const float* x, const int* graph_ptr, float* y, int n_graphs, int d, void* stream);
int oneprot_segment_sum_bwd_f32(const float* dy, const int* batch, float* dx, int N, int d, void* stream);

/* ---------------- downstream metrics (ref src/utils/downstream.py:12-59 count_f1_max; ref src/saprot_fit_cls.py:41-65 and src/saprot_fit_mlp.py:298-330
 * score with sklearn's roc_auc_score / accuracy_score / f1_score / mean_squared_error / r2_score and scipy's spearmanr) -------------------------------------
 * A stable sort, midranks and ordered scans, and F1-max on top of them.  1 <= n <= 2^31 - 1 everywhere.  No work-group waits on another; a radix pass is
 * three launches (histogram per tile of ONEPROT_SORT_TILE keys, scan of the [256, tiles] table, ranked scatter).  Two runs give the same bits: the order
 * inside a tile comes from wave ballots and prefix counts, and every floating-point sum runs through one fixed tree whose shape depends on n alone.
 * Nothing is read back.  Workspaces are 8-byte aligned; a *_workspace() query returns 0 for invalid arguments. */
#define ONEPROT_SORT_TILE 2048
#define ONEPROT_SCAN_TILE 2048
/* Replaces `pred.flatten().argsort(descending=...)` (ref downstream.py:35; torch's argsort is unstable): perm int32 [n], sorted_keys (optional) fp32 [n].
   LSD radix, four 8-bit passes over the order-preserving bit map of the keys; -0.0 is made +0.0 first, so the zeros are equal keys; +-inf sort as values;
   NaN is outside the contract.  Equal keys keep ASCENDING index in both directions (descending sorts the complemented key). */
size_t oneprot_sort_workspace(int64_t n);
int oneprot_sort_f32(const float* keys, int64_t n, int descending, int* perm, float* sorted_keys, void* workspace, size_t workspace_bytes, void* stream);
/* Stable ascending sort of non-negative int32 keys below 2^key_bits (1 <= key_bits <= 31; ceil(key_bits / 8) passes) with int32 values; values NULL means
   0 .. n-1 (an argsort); keys_out optional.  The outputs must not be the inputs.  workspace: oneprot_sort_workspace(n). */
int oneprot_sort_i32(const int* keys, const int* values, int64_t n, int key_bits, int* keys_out, int* values_out, void* workspace, size_t workspace_bytes,
                     void* stream);
/* Replaces scipy.stats.rankdata(x, "average") inside spearmanr and roc_auc_score's tie handling: rank2[i] = first + last + 2 of the run of equal keys that
   holds x[i] in the ascending order (0-based positions) = twice the average 1-based rank, an exact integer (read it unsigned beyond n = 2^30). */
size_t oneprot_midranks_workspace(int64_t n);
int oneprot_midranks_f32(const float* x, int64_t n, int* rank2, void* workspace, size_t workspace_bytes, void* stream);
/* Replaces `x.cumsum(0)` (ref downstream.py:31-32, 52-57; torch's GPU cumsum fixes no order): y[i] = x[s] + ... + x[i], s the last multiple of seg_len at or
   below i (seg_len 0: s = 0).  is_f64 0: int32 streams, 1: fp64 streams; y may be x. */
size_t oneprot_scan_workspace(int64_t n);
int oneprot_inclusive_scan(const void* x, void* y, int64_t n, int64_t seg_len, int is_f64, void* workspace, size_t workspace_bytes, void* stream);
/* The sums behind accuracy_score / mean_squared_error / r2_score / the Pearson step of spearmanr, in fp64 over two fp32 (is_i32 0) or int32 (1) streams, with
   a' = a - shift_a and b' = b - shift_b formed in fp64: moments_bytes = 8 doubles {n, sum a', sum b', sum a'^2, sum b'^2, sum a'b', sum (a'-b')^2,
   #(a == b)}.  A shift only conditions the sums; the caller undoes it algebraically, so it need not be exact. */
size_t oneprot_moments_workspace(int64_t n);
int oneprot_moments(const void* a, const void* b, int64_t n, int is_i32, float shift_a, float shift_b, void* moments_bytes, void* workspace,
                    size_t workspace_bytes, void* stream);
/* Replaces count_f1_max (ref downstream.py:12-59) for pred fp32 [B, N] and target [B, N] in {0, 1} (int32, or fp32 with target_is_f32 = 1), B * N < 2^31:
   all scores in descending order, equal scores in ascending flat index; after each element k of row i, cnt_i += 1, tp_i += target; P_k = mean over the rows
   with cnt > 0 of tp_i / cnt_i, R_k = mean over all B rows of tp_i / (T_i + 1e-10), F_k = 2 P_k R_k / (P_k + R_k + 1e-10).  f1_bytes = 2 doubles
   {max_k F_k, the score at the first k that reaches it}.  Counts are integers, the quotients and running sums fp64. */
size_t oneprot_f1max_workspace(int B, int N);
int oneprot_f1max(const float* pred, const void* target, int target_is_f32, int B, int N, void* f1_bytes, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------- downstream MLP probe (ref src/saprot_fit_mlp.py: the MLP of :63-115, the losses of :163-169, AdamW of :205-207) ------------------------------
 * "Few rows" fp32 kernels (csrc/probe.hip): a batch is 32 or 64 rows, so a work-group owns every row of a column tile and finishes the layer in its epilogue;
 * a training step of an MLP with H hidden layers is at most 5 H + 8 launches (5 H + 10 with the residual projection) and nothing is read back.  All of it fp32
 * fmaf chains, no float atomics, every sum in a fixed order: two runs give the same bits.  norm: 0 none, 1 BatchNorm1d train mode, 2 BatchNorm1d eval mode;
 * act: 0 identity, 1 ReLU, 2 erf-GELU, 3 LeakyReLU(0.01).  Dropout is the element rule (at oneprot_dropout_bf16) over the flat [M, n] index for (seed,
 * stream_id): the fused epilogues and oneprot_dropout_f32 draw the same mask, and the backward regenerates it.  idx (optional) int32 [M]: row m of the operand is row
 * idx[m] of a resident [N, k] matrix, so a shuffled batch is never materialised. */
#define ONEPROT_PROBE_MAX_BATCH 256      /* rows of a BatchNorm (train mode) batch: one work-group holds a column's whole batch */
/* Replaces nn.Linear -> [nn.BatchNorm1d] -> activation -> [nn.Dropout] (ref saprot_fit_mlp.py:74-92,107-108) and the residual sum (:110-113):
   z[M, n] = gather(x, idx)[M, k] w[n, k]^T + b (written when z is given: the backward needs the pre-norm values), y = dropout(act(norm(z))) (+ resid[M, n], or
   rows resid_idx[m] of resid when resid_idx is given) when y is given.  Any M, n, k >= 1; norm 1 needs 2 <= M <= ONEPROT_PROBE_MAX_BATCH, computes the two-pass mean
   and biased variance (eps 1e-5), writes mean / rstd [n] and updates running_mean / running_var (momentum 0.1, unbiased variance) as nn.BatchNorm1d does;
   norm 2 reads running_mean / running_var. */
int oneprot_probe_linear_fwd(const float* x, const int* idx, const float* w, const float* b, float* z, float* y, const float* resid, const int* resid_idx,
                             const float* gamma, const float* beta, float* mean, float* rstd, float* running_mean, float* running_var, int M, int n, int k,
                             int norm, int act, float p, uint64_t seed, uint64_t stream_id, void* stream);
/* Replaces nn.LayerNorm -> activation -> [nn.Dropout] (ref saprot_fit_mlp.py:79-90 with use_layer_norm): y = dropout(act(LN(z))) (+ resid, rows
   resid_idx[m] when given) over the rows of z[M, n], eps 1e-5; mean / rstd [M] (optional) for the backward. */
int oneprot_probe_rownorm_act_fwd(const float* z, const float* gamma, const float* beta, float* y, const float* resid, const int* resid_idx, float* mean,
                                  float* rstd, int M, int n, int act, float p, uint64_t seed, uint64_t stream_id, void* stream);
/* autograd's backward of the two above: dz[M, n] from dy, with the mask regenerated, act' applied and the norm's backward; dgamma / dbeta [n] (optional) are the
   column sums of u xhat and u, u = dL/d norm(z).  norm_act_bwd: mean / rstd are the forward's [n] for norm 1, running_mean / running_VAR for norm 2. */
int oneprot_probe_norm_act_bwd(const float* dy, const float* z, const float* gamma, const float* beta, const float* mean, const float* rstd, float* dz,
                               float* dgamma, float* dbeta, int M, int n, int norm, int act, float p, uint64_t seed, uint64_t stream_id, void* stream);
int oneprot_probe_rownorm_act_bwd(const float* dy, const float* z, const float* gamma, const float* beta, const float* mean, const float* rstd, float* dz,
                                  float* dgamma, float* dbeta, int M, int n, int act, float p, uint64_t seed, uint64_t stream_id, void* stream);
/* autograd's backward of nn.Linear (ref saprot_fit_mlp.py:75,95,99): dw[n, k] = dz[M, n]^T gather(x, idx)[M, k] and db[n] (optional) = column sums of dz,
   written (not accumulated) wherever dw / db point -- the flat gradient arena; da[M, k] = dz[M, n] w[n, k]. */
int oneprot_probe_linear_bwd_w(const float* dz, const float* x, const int* idx, float* dw, float* db, int M, int n, int k, void* stream);
int oneprot_probe_linear_bwd_x(const float* dz, const float* w, float* da, int M, int n, int k, void* stream);
/* Replaces the loss of ref saprot_fit_mlp.py:163-169,184,197 and its backward.  logits [M, C]; kind 0 F.binary_cross_entropy_with_logits (mean over M C, the
   stable form max(x, 0) - x y + log1p(exp(-|x|))), 1 F.mse_loss (mean), both with target fp32 [., C]; 2 F.cross_entropy with labels int64 [.] (mean over M, row
   log-sum-exp; a label outside [0, C) turns the loss NaN).  Row m's target is row idx[m] when idx is given.  dlogits (optional) carries the mean's scaling.
   loss_bytes: one double, loss_sum += weight x mean loss, summed in fp64 through per-work-group partials and one ordered finish: a validation pass adds its
   slabs up (weight = rows) without a readback.  workspace: oneprot_probe_loss_workspace() bytes. */
size_t oneprot_probe_loss_workspace(void);
int oneprot_probe_loss_fwd_bwd(const float* logits, const float* target, const int64_t* labels, const int* idx, float* dlogits, void* loss_bytes,
                               void* workspace, int M, int C, int kind, float weight, void* stream);
/* torch.optim.AdamW on a flat arena (ref saprot_fit_mlp.py:205-207): p <- p (1 - lr weight_decay), then the Adam update.  Any n; step >= 1.  The betas are
   handed over as 1 - beta (0.1, 0.001), which fp32 holds to 5e-8 where 1 - (float)0.999 is off by 1.3e-5.  (oneprot_adam_step's decay is the L2 form.) */
int oneprot_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float one_minus_beta1, float one_minus_beta2, float eps,
                       float weight_decay, int step, void* stream);

/* ---------------- gradient-boosted tree probes (ref src/saprot_fit_cls.py:32-38 and src/saprot_fit_reg.py:26-32: xgboost.XGBClassifier / XGBRegressor .fit /
 * .predict; ref configs/downstream_model/xgboost_cls.yaml, xgboost_reg.yaml: tree_method gpu_hist) ---------------------------------------------------------
 * The `hist` tree builder on fixed-point histograms (csrc/gbt.hip).  X fp32 [N, F], 1 <= N <= 2^24, 1 <= F <= 65535, 2 <= max_bin <= 256, finite.  Gradients
 * are quantised to integers q = rint(x 2^(20 - e)) before any sum (e = 0, except for the g of reg:squarederror: the smallest e with max |g| < 2^e over the kept
 * rows, at least -100, 0 when every g is 0), histograms are int32 in LDS and int64 in global memory: integer sums, the same bits in every run and for every
 * work decomposition.  No float atomics, no work-group waits on another, nothing is read back.  Trees are heap-numbered (root 0, children 2 n + 1, 2 n + 2)
 * arrays of tree_nodes = 2^(max_depth + 1) - 1 entries per (round, output): tree_feat (-1: leaf), tree_bin (cut index), tree_thr (cut value), tree_leaf
 * ((float)(learning_rate w)).  Byte masks row_keep [N], feat_keep [F] are 0 / 1; bins is uint8 [N, F].  The float parameters are used as doubles. */
/* cuts [F, max_bin - 1] (unused slots +inf) and ncuts [F] from grouped [F, N], every feature's column ascending: the distinct values among
   v[floor(k N / max_bin)], k = 1 .. max_bin - 1, with -0.0 read as +0.0.  bins[i, f] = the number of cuts <= X[i, f], so bin <= j iff x < cut[j]. */
int oneprot_gbt_cuts(const float* grouped, int64_t N, int F, int max_bin, float* cuts, int* ncuts, void* stream);
int oneprot_gbt_bin(const float* X, const float* cuts, const int* ncuts, void* bins, int64_t N, int F, int max_bin, void* stream);
/* One round's masks (xgboost's subsample / colsample_bytree).  The uniform of element e is its 16-bit slice under the element rule (at oneprot_dropout_bf16), over 65536.
   Row i is kept iff uniform(seed, row_stream, i) < subsample (subsample >= 1 keeps all, drawing nothing); the n_keep features with the smallest
   uniform(seed, feat_stream, f) are kept, equal uniforms to the lower index (n_keep = F keeps all, drawing nothing).  feat_uniform: int32 [F] scratch. */
int oneprot_gbt_sample(void* row_keep, void* feat_keep, int* feat_uniform, int64_t N, int F, float subsample, int n_keep, uint64_t seed, uint64_t row_stream,
                       uint64_t feat_stream, void* stream);
/* gq / hq int32 [K, N] and expo int32 [K] from margin fp32 [N, K], in fp32.  objective 0 binary:logistic (target fp32 [N, K]: p = 1 / (1 + exp(-m)), g = p - y,
   h = p (1 - p)), 1 reg:squarederror (K = 1, target fp32 [N]: g = m - y, h = 1), 2 multi:softmax (labels int32 [N]: p the row softmax, g_k = p_k - [y = k],
   h_k = 2 p_k (1 - p_k)).  Rows with row_keep 0 get q = 0.  gmax_bits: one int32 of scratch (the order-free maximum of |g| as float bits). */
int oneprot_gbt_grad(const float* margin, const float* target, const int* labels, const void* row_keep, int* gq, int* hq, int* expo, int* gmax_bits, int64_t N,
                     int K, int objective, void* stream);
/* hist int64 [kc, 2^level, F, max_bin, 2] (g, h), overwritten: the sums of gq / hq [kc, N] over the rows whose pos [kc, N] is node 2^level - 1 + n.
   0 <= level <= 5.  oneprot_gbt_hist_bytes: the bytes of ONE output's histogram at this level (0 for invalid arguments). */
size_t oneprot_gbt_hist_bytes(int F, int max_bin, int level);
int oneprot_gbt_hist(const void* bins, const int* gq, const int* hq, const int* pos, int64_t* hist, int64_t N, int F, int max_bin, int level, int kc, void* stream);
/* Per (output, node of the level): candidates (kept feature f, cut j < ncuts[f]), left = bins <= j; valid iff HL_int > 0, HR_int > 0, HL >= min_child_weight
   and HR >= min_child_weight; T(G) = sign(G) max(|G| - reg_alpha, 0), score = T(G)^2 / (H + reg_lambda), gain = (score(L) + score(R)) - score(node) in fp64;
   best = largest gain, then lowest f, then lowest j; the node splits iff a valid candidate exists and gain > max(gamma, 0).  Writes the node's entries and its
   children's leaf values (0 under a node that does not split) into the tree arrays [kc, tree_nodes]; w = -T(G) / (H + reg_lambda), 0 when H + reg_lambda <= 0.
   gain_bytes (optional): doubles [kc, tree_nodes], the best valid gain of the node, -inf without one.  Two launches: a wave per (output, node, feature) leaves
   the feature's best cut in the workspace (oneprot_gbt_split_workspace bytes, 8-byte aligned), a work-group per (output, node) takes the ordered arg-max. */
size_t oneprot_gbt_split_workspace(int F, int level, int kc);
int oneprot_gbt_split(const int64_t* hist, const float* cuts, const int* ncuts, const void* feat_keep, const int* expo, int* tree_feat, int* tree_bin, float* tree_thr,
                      float* tree_leaf, void* gain_bytes, void* workspace, size_t workspace_bytes, int F, int max_bin, int level, int kc, int tree_nodes,
                      float min_child_weight, float gamma, float reg_alpha, float reg_lambda, float learning_rate, void* stream);
/* Levels 6 .. 8 of a one-output fit (ref saprot_fit_reg.py:26-32 with max_depth 7 .. 9, as configs/saprot_sweep_xgboost_reg.yaml asks): the rows in node
   order, and the level's histograms and split search a group of nodes [node0, node0 + nodes) at a time, so that a level need not fit memory at once.
   oneprot_gbt_node_keys: keys[i] = pos[i] - (2^level - 1) for a row in a node of the level, the sentinel 2^level for every other row.  The caller sorts them
   (oneprot_sort_i32, level + 1 key bits, values NULL) into sorted_keys and order.  oneprot_gbt_node_seg: seg int32 [2^level + 1], seg[n] = the first position
   of sorted_keys that holds a key >= n (seg[2^level]: where the sentinel rows begin). */
int oneprot_gbt_node_keys(const int* pos, int* keys, int64_t N, int level, void* stream);
int oneprot_gbt_node_seg(const int* sorted_keys, int* seg, int64_t N, int level, void* stream);
/* hist int64 [nodes, F, max_bin, 2] (g, h), indexed by the local node n - node0, overwritten: the sums of gq / hq [N] over the rows of node n.  Rows of nodes
   outside the group, sentinel rows, rows with g = h = 0 and bins >= max_bin add nothing.  The launch is a function of the shapes alone: work-group x takes
   2047 consecutive positions of `order`.  tile_features: the features of an LDS tile (a power of two <= 64; the tile holds 64 / tile_features consecutive
   nodes), 0 for the library's choice per level; it cannot change a bit of the result.  oneprot_gbt_hist_nodes_bytes: the bytes of `nodes` nodes. */
size_t oneprot_gbt_hist_nodes_bytes(int F, int max_bin, int nodes);
int oneprot_gbt_hist_nodes(const void* bins, const int* gq, const int* hq, const int* order, const int* sorted_keys, const int* seg, int64_t* hist, int64_t N, int F,
                           int max_bin, int level, int node0, int nodes, int tile_features, void* stream);
/* oneprot_gbt_split for one output and the nodes [node0, node0 + nodes) of a level 0 .. 8, on the same device code: hist and the workspace's records are indexed
   by the local node, the tree arrays [tree_nodes] and gain_bytes by the heap id 2^level - 1 + node0 + n.  With node0 = 0 and nodes = 2^level it writes what
   oneprot_gbt_split writes with kc = 1, bit for bit. */
size_t oneprot_gbt_split_nodes_workspace(int F, int nodes);
int oneprot_gbt_split_nodes(const int64_t* hist, const float* cuts, const int* ncuts, const void* feat_keep, const int* expo, int* tree_feat, int* tree_bin, float* tree_thr,
                            float* tree_leaf, void* gain_bytes, void* workspace, size_t workspace_bytes, int F, int max_bin, int level, int node0, int nodes,
                            int tree_nodes, float min_child_weight, float gamma, float reg_alpha, float reg_lambda, float learning_rate, void* stream);
/* pos [kc, N]: a row in a node of this level (0 .. 8) that split moves to child 2 p + 1 (bin <= tree_bin) or 2 p + 2; every other row stays */
int oneprot_gbt_partition(const void* bins, const int* tree_feat, const int* tree_bin, int* pos, int64_t N, int F, int level, int kc, int tree_nodes, void* stream);
/* margin[i, k0 + kk] += tree_leaf[kk, pos[kk, i]] for the kc outputs of a chunk: every row, kept or dropped (margin fp32 [N, K]) */
int oneprot_gbt_update(float* margin, const int* pos, const float* tree_leaf, int64_t N, int K, int k0, int kc, int tree_nodes, void* stream);
/* Replaces model.predict's margin: margin[i, k] = init_margin + the leaves of trees (t, k), t = 0 .. n_trees - 1 in order, one fp32 chain; raw X against
   tree_thr, x < threshold goes left.  Tree arrays [n_trees, K, tree_nodes]. */
int oneprot_gbt_predict(const float* X, const int* tree_feat, const float* tree_thr, const float* tree_leaf, float* margin, int64_t N, int F, int K, int n_trees,
                        int tree_nodes, float init_margin, void* stream);

#ifdef __cplusplus
}
#endif
#endif
