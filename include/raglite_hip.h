/*
 * raglite_hip.h -- C ABI of libraglite_hip.so: the MI355X (gfx950) retrieval / rerank hot path
 * of RAGLite.  Plain pointers and sizes only; no torch / C++ types cross this boundary.
 *
 * The reference (superlinear-ai/raglite v1.0.0) is pure Python and has no FFI of its own; each
 * entry point below states the reference lines (relative to /root/reference) whose arithmetic
 * it replaces.  INTEGRATION.md shows the ctypes binding a RAGLite maintainer would add.
 *
 * Conventions
 *  - every function returns 0 (RL_OK) or a negative rl_status; rl_last_error() gives the
 *    thread-local message of the last failure on the calling thread.
 *  - `mem` says where the caller's data pointers live: RL_MEM_HOST (the library stages through
 *    its own device scratch, synchronously) or RL_MEM_DEVICE (pointers are HIP device pointers,
 *    work is enqueued on `stream` and NOT synchronised -- the caller owns ordering).
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *  - all matrices are row-major and dense; dim is the embedding dimension.
 *  - thread safety: calls on distinct rl_index handles / distinct streams may run concurrently;
 *    calls on one handle share its device scratch: they serialise on an internal mutex, and a call on
 *    another stream than the handle's previous call first waits for that stream (the reference calls the path from up to
 *    4 worker threads: src/raglite/_insert.py:159,208-237; src/raglite/_rag.py:317-318).
 */
#ifndef RAGLITE_HIP_H
#define RAGLITE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    RL_OK = 0,
    RL_ERR_INVALID = -1,     /* bad argument (maps to Python ValueError) */
    RL_ERR_HIP = -2,         /* HIP runtime failure (RuntimeError) */
    RL_ERR_UNSUPPORTED = -3, /* shape outside what the kernels implement (ValueError) */
    RL_ERR_NOMEM = -4        /* device allocation failed (MemoryError) */
} rl_status;

typedef enum { RL_MEM_HOST = 0, RL_MEM_DEVICE = 1 } rl_mem;
/* A flag or-ed into `mem` of the calls that take `chunk_filter` / `chunk_filters`: that argument ALONE is a device pointer,
 * read in place and not copied (e.g. rl_filter_set_bits' table); every other pointer follows `mem & 1`.  The work is
 * enqueued on `stream` after whatever that stream holds, so a table written on the same stream is complete when it is read. */
#define RL_MEM_FILTERS_DEVICE 2
/* How an index multiplies queries with its corpus in the MFMA streaming kernel (rl_index_set_arithmetic). */
typedef enum {
    RL_ARITH_AUTO = 0,       /* request: RL_ARITH_F16_SPLIT where the corpus allows it, else RL_ARITH_FP32_EXACT */
    RL_ARITH_FP32_EXACT = 1, /* v_mfma_f32_16x16x4_f32: bitwise an ordered fp32 fmaf chain */
    RL_ARITH_F16_SPLIT = 2,  /* in effect only: fp32 operands as fp16 (hi, lo) pairs, see below */
    RL_ARITH_F16_STORED = 3  /* in effect only: an rl_index_create_f16 index */
} rl_arith;
typedef enum { RL_F32 = 0, RL_F16 = 1 } rl_dtype;
/* src/raglite/_config.py:69 `vector_search_distance_metric`; src/raglite/_typing.py:123-134 */
typedef enum { RL_COSINE = 0, RL_DOT = 1, RL_L2 = 2 } rl_metric;
typedef enum { RL_SYNTH_UNIFORM = 0, RL_SYNTH_SMALL_INT = 1 } rl_synth_kind;

typedef struct rl_index rl_index; /* opaque device-resident index (corpus matrix + chunk CSR) */

/* ---- runtime ------------------------------------------------------------------------------ */
int rl_version(void);
const char* rl_last_error(void);
/* Select the HIP device for the calling thread; fails if it is not a gfx950 part. */
int rl_init(int device);
int rl_device_count(int* count);
/* name[<=len], number of CUs, bytes of device memory */
int rl_device_info(int device, char* name, int len, int* compute_units, int64_t* total_mem);

/* Device memory helpers so that a pure-ctypes caller needs no other GPU library. */
int rl_dev_alloc(void** ptr, size_t bytes);
int rl_dev_free(void* ptr);
int rl_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream);
int rl_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream);
int rl_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream);
int rl_stream_sync(void* stream);

/* Counter-based synthetic data, bit-identical to oracle/oracle.py:synth_uniform / synth_small_int:
 * element i (i in [start, start+count)) of stream `seed`.  dst is a DEVICE pointer. */
int rl_synth_fill(float* dst, int64_t start, int64_t count, uint64_t seed, int kind, void* stream);

/* ---- a1 + a2 + a3: late-chunking pool, L2 normalise, fp16 cast ------------------------------
 * Replaces src/raglite/_embed.py:131-140 (per-sentence np.mean over contiguous token rows,
 * rowwise X /= ||X||, astype(float16)) and :154,158-164 (whole-string mean, eps-guarded
 * normalise).  The host computes the row spans (largest-remainder split, :122-129) and passes
 * them in; span s pools token rows [span_begin[s], span_end[s]).
 *   tokens      [T x dim] f32
 *   normalize   0/1            (RAGLiteConfig.embedder_normalize)
 *   eps         0  -> unguarded divide (:139);  >0 -> divide by max(norm, eps) (:160-163)
 *   out_f32     [S x dim] f32 or NULL;  out_f16 [S x dim] IEEE half bits or NULL
 * Accumulation is fp64 (the reference pools float64 arrays), the cast rounds to nearest even.
 * An empty span produces NaN, as np.mean of zero rows does.  Sums start from +0.0, so a column
 * whose rows are all -0.0 pools to +0.0 where np.mean gives -0.0: zeros compare equal, not bitwise. */
int rl_pool_norm(const float* tokens, int64_t n_token_rows, int32_t dim,
                 const int64_t* span_begin, const int64_t* span_end, int64_t n_spans,
                 int32_t normalize, double eps, float* out_f32, uint16_t* out_f16,
                 int mem, void* stream);

/* ---- variable-length attention forward (the packed encoder's attention) --------
 * Non-causal softmax attention over a PACKED batch: the sequences of a call are concatenated along the token axis and every token
 * attends to the tokens of its own sequence only,
 *     out[t, h, :] = softmax_j(scale * q[t,h] . k[j,h]) . v[j,h],   seq_offsets[s] <= t, j < seq_offsets[s + 1].
 *   qkv          [n_tokens x 3 x heads x head_dim] bf16 or fp16: the fused QKV projection, read in place (token row stride
 *                3 * heads * head_dim elements; q, k, v of head h at element offsets h * head_dim, (heads + h) * head_dim,
 *                (2 * heads + h) * head_dim); 16-byte aligned
 *   seq_offsets  int32[n_seqs + 1] on the device: ascending, from 0 to n_tokens; empty sequences are allowed
 *   max_len      at least every sequence length (a host scalar: it sizes the grid, nothing waits for the device); a sequence longer than
 *                max_len gets its first max_len rows (rounded up to the query tile) only
 *   dtype        RL_ATTN_BF16 or RL_ATTN_F16, of qkv and of out
 *   out          [n_tokens x heads x head_dim], 8-byte aligned
 * Scores, the online softmax, the row sums and the output accumulate in f32; `scale` multiplies f32 scores; the probabilities are
 * rounded to `dtype` only as the operand of P.V (in bf16 as two operands, the rounded value and the rounded remainder); the output is rounded to nearest even.  No atomics: the same bits run to run, and a
 * sequence's bits depend neither on the rest of the pack nor on max_len.  Error against exact arithmetic on the rounded inputs: at most
 * (2 u + 2^-12) * sum_j w_j |v_j| per element, u = 2^-9 (bf16) or 2^-11 (fp16), w the exact softmax weights (|scaled score| <= 64).
 * Device offsets are not validated: every token index the kernel forms is clamped into [0, n_tokens), so offsets that break the
 * contract give wrong numbers but never an access outside qkv or out.
 * Device pointers only (mem != RL_MEM_DEVICE: RL_ERR_UNSUPPORTED; bf16 has no host array type in the binding); everything is enqueued on
 * `stream`.  Checked before any HIP call: RL_ERR_INVALID for a null qkv / seq_offsets / out or a misaligned qkv / out with n_tokens > 0,
 * n_seqs < 0, n_tokens < 0 or >= 2^31, max_len < 0, heads < 1 or > 65535, n_seqs > 65535 (the grid's z axis), a non-finite scale, an
 * unknown dtype; RL_ERR_UNSUPPORTED for head_dim outside {32, 64}.  n_tokens == 0 returns RL_OK and writes nothing. */
#define RL_ATTN_BF16 0
#define RL_ATTN_F16 1
int rl_attention_varlen(const void* qkv, const int32_t* seq_offsets, int32_t n_seqs, int64_t n_tokens, int32_t max_len,
                        int32_t heads, int32_t head_dim, int32_t dtype, float scale, void* out, int mem, void* stream);

/* ---- native encoder forward for short packs (text queries) --------------------------------------------------------
 * The forward of a post-LN BERT / XLM-R encoder over a PACKED batch of at most RL_ENCODER_MAX_TOKENS tokens, enqueued by one call:
 *     x = LN(tok[id] + pos[p] + typ[type]);  per layer:  qkv = x Wqkv^T + b;  a = attention_varlen(qkv);
 *     x1 = LN1(x + a Wout^T + b);  x = LN2(x1 + gelu_erf(x1 Wup^T + b) Wdown^T + b)
 * Every sum (embeddings, products, bias, residual, layer norm) is taken in f32 and rounded ONCE to the 16-bit dtype where the next
 * step reads it: after each layer norm, after the QKV bias and after the GELU.  1 + 7 * layers kernel launches, no allocation, no
 * synchronisation, no atomics: the same bits run to run, and a sequence's bits depend neither on its place in the pack nor on
 * what else is in it.
 *
 * rl_encoder_create BORROWS every parameter pointer (device memory, `dtype` elements; the caller keeps the tensors alive and
 * unchanged in place for as long as the handle) and allocates the scratch of RL_ENCODER_MAX_TOKENS rows:
 *   tok [vocab x hidden], pos [max_positions x hidden], typ [type_vocab x hidden], ln_w / ln_b [hidden]
 *   layer_params   HOST array of 12 * layers device pointers, per layer: qkv_w [3 hidden x hidden], qkv_b, out_w [hidden x hidden],
 *                  out_b, ln1_w, ln1_b, up_w [ffn x hidden], up_b, down_w [hidden x ffn], down_b, ln2_w, ln2_b -- the matrices in
 *                  nn.Linear's own row-major [out x in] layout, read in place
 *   every parameter pointer 16-byte aligned
 * Checked before any HIP call: RL_ERR_INVALID for a null argument, a size < 1, hidden % heads != 0, heads > 65535, eps not finite or
 * negative, an unknown dtype, a misaligned parameter; RL_ERR_UNSUPPORTED for a head width outside {32, 64}, hidden or ffn not a multiple of 32,
 * hidden > 8192 or ffn > 32768.
 *
 * rl_encoder_forward: ids, positions, type_ids (NULL: type 0 everywhere) int32[n_tokens], seq_offsets int32[n_seqs + 1] as
 * rl_attention_varlen takes them, all on the device; max_len >= every sequence length; out [n_tokens x hidden] in the handle's dtype,
 * 16-byte aligned.  Ids, positions and type ids are clamped into their tables: a bad id gives a wrong number, never an access
 * outside a table.  Checked before any HIP call, the handle last: mem != RL_MEM_DEVICE (RL_ERR_UNSUPPORTED), a negative size,
 * n_seqs > 65535, n_tokens > RL_ENCODER_MAX_TOKENS (RL_ERR_UNSUPPORTED), null or misaligned pointers with n_tokens > 0, a null handle.
 * n_tokens == 0 returns RL_OK and writes nothing.  Calls on one handle share its scratch (the mutex and stream rule of the header's
 * conventions).
 *
 * rl_encoder_info: max_tokens = RL_ENCODER_MAX_TOKENS; scratch / scratch_bytes: the handle's block; used_bytes: the prefix of it a
 * forward of n_tokens rows writes (nothing behind it is touched); launches = 1 + 7 * layers.  Every output may be NULL. */
#define RL_ENCODER_MAX_TOKENS 256
typedef struct rl_encoder rl_encoder;
int rl_encoder_create(rl_encoder** out, int32_t vocab, int32_t hidden, int32_t layers, int32_t heads, int32_t ffn, int32_t max_positions,
                      int32_t type_vocab, float eps, int32_t dtype, const void* tok, const void* pos, const void* typ, const void* ln_w,
                      const void* ln_b, const void* const* layer_params);
int rl_encoder_forward(rl_encoder* enc, const int32_t* ids, const int32_t* positions, const int32_t* type_ids, const int32_t* seq_offsets,
                       int32_t n_seqs, int64_t n_tokens, int32_t max_len, void* out, int mem, void* stream);
int rl_encoder_info(const rl_encoder* enc, int64_t n_tokens, int32_t* max_tokens, int64_t* scratch_bytes, int64_t* used_bytes,
                    void** scratch, int32_t* launches);
int rl_encoder_destroy(rl_encoder* enc);

/* The three launches of rl_encoder_forward ONE AT A TIME, on the caller's buffers: the same kernels through the same launchers, for
 * callers that hold each to a reference of its own (tests/test_gpu_encoder_kernels.py) or chain them by hand.  Device pointers only
 * (mem must be RL_MEM_DEVICE, else RL_ERR_UNSUPPORTED), no handle, no scratch, nothing allocated; `dtype` (RL_ATTN_BF16 / RL_ATTN_F16) is
 * that of every `void*`.  M, n_tokens in [0, RL_ENCODER_MAX_TOKENS]: 0 returns RL_OK and writes nothing.  K, N and hidden are positive
 * multiples of 32, hidden <= 8192 (RL_ERR_UNSUPPORTED above).  Every argument is checked before the first HIP call: RL_ERR_INVALID for
 * a size outside its range, an unknown dtype or epilogue, an eps that is negative or not finite, a null or misaligned pointer
 * (matrices and `part`: 16 bytes; 16-bit vectors and 16-bit outputs: 8; int32 arrays: 4).
 *
 * rl_encoder_embed: out[t] = LN(tok[ids[t]] + pos[positions[t]] + typ[type_ids ? type_ids[t] : 0]) for t < n_tokens, out
 *   [n_tokens x hidden]; tok [vocab x hidden], pos [max_positions x hidden], typ [type_vocab x hidden]; every index is clamped into its
 *   table; type_ids may be NULL.
 * rl_encoder_linear: x [M x K] . W [N x K]^T (W as nn.Linear keeps it), by `epilogue`:
 *     RL_ENC_EPI_BIAS     out16 [M x N] = the product + bias, rounded once               (the QKV projection)
 *     RL_ENC_EPI_GELU     out16 [M x N] = gelu_erf(the product + bias), rounded once     (the up projection)
 *     RL_ENC_EPI_PARTIAL  part [slices x M x N] f32: the raw sums of the K slices, slices = rl_encoder_linear_slices(N, K); bias is not
 *                         read (the out and down projections: bias, residual and the slices' sum belong to the layer norm)
 *   The output the epilogue does not write, and bias under RL_ENC_EPI_PARTIAL, may be NULL and are not looked at; the one it writes must
 *   be given.  A row's bits depend on (N, K) and its own x row alone, not on M.
 * rl_encoder_layer_norm: out[r] = LN(part[0][r] + .. + part[slices - 1][r] + bias + resid[r]) for r < M, the sum in that order in f32;
 *   part [slices x M x hidden] f32, slices in [1, 8]; bias, ln_w, ln_b [hidden], resid and out [M x hidden].
 * rl_encoder_linear_slices: host only; *slices = the K slices RL_ENC_EPI_PARTIAL uses at (N, K) -- a function of the two alone, in
 *   [1, 8] -- so that a caller can size `part`. */
#define RL_ENC_EPI_BIAS 0
#define RL_ENC_EPI_GELU 1
#define RL_ENC_EPI_PARTIAL 2
int rl_encoder_embed(const int32_t* ids, const int32_t* positions, const int32_t* type_ids, int64_t n_tokens, const void* tok, int32_t vocab,
                     const void* pos, int32_t max_positions, const void* typ, int32_t type_vocab, const void* ln_w, const void* ln_b,
                     int32_t hidden, float eps, int32_t dtype, void* out, int mem, void* stream);
int rl_encoder_linear(const void* x, int64_t M, int32_t K, const void* W, int32_t N, const void* bias, int32_t epilogue, int32_t dtype,
                      void* out16, float* part, int mem, void* stream);
int rl_encoder_layer_norm(const float* part, int32_t slices, int64_t M, int32_t hidden, const void* bias, const void* resid,
                          const void* ln_w, const void* ln_b, float eps, int32_t dtype, void* out, int mem, void* stream);
int rl_encoder_linear_slices(int32_t N, int32_t K, int32_t* slices);

/* ---- the native forward of a pack larger than one token block (all text queries of a batched search) ----------------
 * rl_encoder_forward's cap of RL_ENCODER_MAX_TOKENS rows is what ONE workgroup of the linear kernel keeps in accumulators.  Above it
 * the linear kernel runs one workgroup per TOKEN BLOCK of 256 rows (block z: rows [256 z, min(256 z + 256, M))), each exactly the loop
 * of a 256-row call: the same chunk order, k-step order, wave-order reduction and slice order.  So a row's bits stay a function of
 * (N, K) and its own x row -- NOT of M, of the block it falls in, or of its place in the block -- and a sequence's rows out of a pack
 * of any size are bit for bit the rows rl_encoder_forward gives for that sequence alone, wherever in the pack it lies, block edges
 * included.  That is what lets a batch of queries share one forward and still return what the single calls return.
 *
 * rl_encoder_pack_workspace_bytes: host only; *bytes = the scratch a pack of n_tokens rows needs: the handle's own scratch layout walked
 *   with that many rows (at RL_ENCODER_MAX_TOKENS: rl_encoder_info's scratch_bytes); monotone in n_tokens.  RL_ERR_INVALID for n_tokens
 *   outside [0, RL_ENCODER_MAX_PACK_TOKENS], a null `bytes`, a null handle (looked at last).
 * rl_encoder_forward_pack: rl_encoder_forward's arguments and contract, with n_tokens <= RL_ENCODER_MAX_PACK_TOKENS and the scratch in
 *   `workspace`, device memory the CALLER owns: 16-byte aligned, workspace_bytes >= rl_encoder_pack_workspace_bytes(n_tokens); nothing
 *   behind that many bytes is written.  1 + 7 * layers launches on `stream`, no allocation, no synchronisation.  The handle's own
 *   scratch is not touched, so calls with different workspaces need no ordering among themselves or with rl_encoder_forward; calls
 *   that share a workspace are ordered by the caller (one stream, or events).  At n_tokens <= RL_ENCODER_MAX_TOKENS the launches are
 *   rl_encoder_forward's and so are the bits.  Checked before any HIP call, the handle last: everything rl_encoder_forward checks, in
 *   its order, with n_tokens > RL_ENCODER_MAX_PACK_TOKENS (RL_ERR_UNSUPPORTED) in the place of its cap; then, with n_tokens > 0, a
 *   null or misaligned workspace and (once the handle is known) one that is too small (RL_ERR_INVALID).
 * rl_encoder_linear_pack: rl_encoder_linear with M in [0, RL_ENCODER_MAX_PACK_TOKENS] -- the blocked launch on its own. */
#define RL_ENCODER_MAX_PACK_TOKENS 8192
int rl_encoder_pack_workspace_bytes(const rl_encoder* enc, int64_t n_tokens, int64_t* bytes);
int rl_encoder_forward_pack(rl_encoder* enc, const int32_t* ids, const int32_t* positions, const int32_t* type_ids,
                            const int32_t* seq_offsets, int32_t n_seqs, int64_t n_tokens, int32_t max_len, void* out, void* workspace,
                            int64_t workspace_bytes, int mem, void* stream);
int rl_encoder_linear_pack(const void* x, int64_t M, int32_t K, const void* W, int32_t N, const void* bias, int32_t epilogue, int32_t dtype,
                           void* out16, float* part, int mem, void* stream);

/* ---- the cross-encoder's head on the native forward (reranking) ----------------------------------------------------
 * A BERT sequence classifier is the encoder above plus, on the FIRST token's row x of every sequence,
 *     p = tanh(pooler_w x + pooler_b);   logit = head_w . p + head_b
 * pooler_w [hidden x hidden] as nn.Linear keeps it, pooler_b [hidden], head_w [hidden] (the [1 x hidden] matrix), head_b [1], all in the
 * 16-bit dtype.  Everything after the 16-bit loads is f32 and the logit is stored as f32: nothing is rounded to 16 bits on the way.  One
 * workgroup per sequence, a fixed reduction tree that depends on `hidden` alone, no atomics: a sequence's logit bits depend neither on
 * n_seqs, nor on its index, nor on where its row lies.  The row index seq_offsets[s] is clamped into [0, n_tokens - 1] (a bad offset
 * gives a wrong number, never a read outside x); an empty sequence (seq_offsets[s] == seq_offsets[s + 1]) gives a quiet NaN.
 *
 * rl_encoder_head: the launch on its own, on the caller's buffers (no handle, no scratch, nothing allocated): x [n_tokens x hidden] in
 *   `dtype`, seq_offsets int32[n_seqs + 1], out_logits f32[n_seqs], all on the device.  Checked before any HIP call: mem !=
 *   RL_MEM_DEVICE (RL_ERR_UNSUPPORTED); n_seqs outside [0, 65535], n_tokens outside [0, 2^31), hidden not a positive multiple of 32
 *   (RL_ERR_INVALID); hidden > 8192 (RL_ERR_UNSUPPORTED); an unknown dtype; then, with n_seqs > 0: n_tokens == 0, a null pointer, x or a
 *   parameter not 16-byte aligned, seq_offsets or out_logits not 4-byte aligned (RL_ERR_INVALID).  n_seqs == 0 returns RL_OK and writes
 *   nothing.
 * rl_encoder_set_head: gives the handle its head; the four pointers are BORROWED like rl_encoder_create's, in the handle's dtype, 16-byte
 *   aligned.  All four NULL clears the head.  RL_ERR_INVALID for some but not all NULL, a misaligned pointer, a null handle (looked at
 *   last).  Not to be called while a call on the handle is running.
 * rl_encoder_classify_workspace_bytes: host only; *bytes = the workspace rl_encoder_classify_pack needs for n_tokens rows and n_seqs
 *   sequences: rl_encoder_pack_workspace_bytes(n_tokens) plus the final hidden states [n_tokens x hidden], from one walk of one layout;
 *   monotone in both arguments (the logits are the caller's, so n_seqs adds nothing today).  RL_ERR_INVALID for n_tokens outside
 *   [0, RL_ENCODER_MAX_PACK_TOKENS], n_seqs outside [0, 65535], a null `bytes`, a null handle (looked at last).
 * rl_encoder_classify_pack: rl_encoder_forward_pack's arguments, checks and order, with out_logits f32[n_seqs] (4-byte aligned) in the
 *   place of `out`: the trunk's 1 + 7 * layers launches, exactly rl_encoder_forward_pack's, write the final rows into the workspace, and
 *   one launch of the head reads them: 2 + 7 * layers launches on `stream`, no allocation, no synchronisation; nothing behind
 *   workspace_bytes >= rl_encoder_classify_workspace_bytes(n_tokens, n_seqs) or behind out_logits[n_seqs] is written.  After the
 *   shared checks: a null or misaligned workspace (n_tokens > 0), a null handle, a handle without a head, a workspace that is too small
 *   (RL_ERR_INVALID).  n_tokens == 0 returns RL_OK and writes nothing. */
int rl_encoder_head(const void* x, const int32_t* seq_offsets, int32_t n_seqs, int64_t n_tokens, int32_t hidden, const void* pooler_w,
                    const void* pooler_b, const void* head_w, const void* head_b, int32_t dtype, float* out_logits, int mem, void* stream);
int rl_encoder_set_head(rl_encoder* enc, const void* pooler_w, const void* pooler_b, const void* head_w, const void* head_b);
int rl_encoder_classify_workspace_bytes(const rl_encoder* enc, int64_t n_tokens, int32_t n_seqs, int64_t* bytes);
int rl_encoder_classify_pack(rl_encoder* enc, const int32_t* ids, const int32_t* positions, const int32_t* type_ids,
                             const int32_t* seq_offsets, int32_t n_seqs, int64_t n_tokens, int32_t max_len, float* out_logits,
                             void* workspace, int64_t workspace_bytes, int mem, void* stream);

/* ---- a5: query adapter -----------------------------------------------------------------------
 * Replaces src/raglite/_search.py:62  `(Q @ q).astype(q.dtype)`; out[b] = A @ q[b].
 *   A [dim x dim] f32, queries [B x dim] f32, out_f32 [B x dim] or NULL, out_f16 or NULL. */
int rl_adapter_apply(const float* A, const float* queries, int32_t n_queries, int32_t dim,
                     float* out_f32, uint16_t* out_f16, int mem, void* stream);
/* rl_adapter_apply picks its kernels by n_queries (a scan up to 4 queries, MFMA tiles above), so a query's bits depend on the size of
 * the batch it comes in.  rl_adapter_apply_rows takes the same arguments and gives EVERY row the bits rl_adapter_apply gives it at
 * n_queries = 1 -- the single-query scan's arithmetic, one query per workgroup row of ONE launch -- for callers whose batch must equal
 * the loop of single calls (the text queries of a batched search).  RL_ERR_UNSUPPORTED for dim > 4096, or > 2048 where
 * dim is no multiple of 4. */
int rl_adapter_apply_rows(const float* A, const float* queries, int32_t n_queries, int32_t dim,
                          float* out_f32, uint16_t* out_f16, int mem, void* stream);

/* ---- the dense score GEMMs on the caller's matrices (score_gemm.hip; the row-score mode of maxsim_gemm.hip) --------------------------
 * What a search of 96 and more queries runs, without an index around it (what tests/test_gpu_score_gemm.py holds to float64):
 *     out[q * ld + r] = metric(E[r] . Q[q])        r < n_rows, q < n_queries; nothing else of `out` is written
 *   E [n_rows x dim] f32, Q [n_queries x dim] f32, both 16-byte aligned; dim a multiple of 32 (RL_ERR_UNSUPPORTED otherwise).
 *   metric        RL_SCORE_RAW: the dot; RL_SCORE_COSINE / _DOT / _L2: the index metrics, formed from the dot and the CALLER's
 *                 row_norm [n_rows] = |e| (cosine) or row_sumsq [n_rows] = |e|^2 (l2) exactly as a search forms them from the index' own.
 *   split_scale   0: the exact fp32 MFMA chain; a power of two: RL_ARITH_F16_SPLIT with the rows scaled by it.
 *   kernel        0: as a search over the stored rows chooses (128 x 256 tiles for more than 128 queries in split arithmetic, else
 *                 128 x 128); 1: 128 x 128 tiles; 2: 128 x 256 tiles; 3: the GEMM over the pre-split corpus image, which is built from E
 *                 into a temporary first.  2 and 3 exist in split arithmetic only.
 *   max_workgroups  the most workgroups of the persistent grid; 0: the device's CUs.  Fewer make each walk more tiles; results do not
 *                 depend on it.
 *   out_q_sumsq [n_queries], out_q_scale [n_queries] (both optional; kernels 0 to 2): what the query-side kernels left -- |q|^2 as the
 *                 epilogue reads it, and the power of two each query was scaled by (split arithmetic only).
 * RL_ERR_INVALID for a null argument, a size < 1, ld < n_rows, an unknown metric or kernel, cosine without row_norm, l2 without row_sumsq,
 * kernels 2 and 3 without a split scale, a split scale that is no power of two, out_q_scale without a split scale, a read-back with
 * kernel 3, device pointers E or Q that are not 16-byte aligned.  Every check comes before the first HIP call. */
enum { RL_SCORE_RAW = 0, RL_SCORE_COSINE = 1, RL_SCORE_DOT = 2, RL_SCORE_L2 = 3 };
int rl_score_gemm(const float* E, int64_t n_rows, int32_t dim, const float* Q, int32_t n_queries, int metric, const float* row_norm,
                  const float* row_sumsq, float split_scale, int32_t kernel, int32_t max_workgroups, float* out, int64_t ld,
                  float* out_q_sumsq, float* out_q_scale, int mem, void* stream);

/* ---- index lifecycle -------------------------------------------------------------------------
 * The device-resident equivalent of the `chunk_embedding` table (src/raglite/_database.py:403-430):
 * one row per chunklet vector, rows of a chunk contiguous (a4: src/raglite/_split_chunks.py:116-122,
 * src/raglite/_insert.py:114-123).
 *   embeddings     [n_rows x dim] f32; with mem == RL_MEM_DEVICE the pointer is BORROWED (must
 *                  outlive the index), with RL_MEM_HOST it is copied to the device.
 *   chunk_offsets  [n_chunks + 1] int64 ascending CSR, chunk_offsets[0]==0, [n_chunks]==n_rows
 *                  (always a HOST pointer); NULL -> every row is its own chunk.
 *   metric         rl_metric used by rl_search_rows / rl_search_chunks.
 * Precomputes ||e|| per row (cosine) or ||e||^2 (l2): 4 B/row extra.
 * Widths: 1 <= dim <= 4096.  Up to 2048 any dim and any 4-byte aligned device pointer (a dim that is no multiple of 4, or rows that are
 * not 16-byte aligned, are scanned with scalar loads).  Above 2048 dim must be a multiple of 4 and borrowed device rows 16-byte aligned,
 * whatever the metric: RL_ERR_UNSUPPORTED otherwise.  Device QUERIES of a search over an index wider than 2048 must be 16-byte aligned
 * too (the search reports RL_ERR_UNSUPPORTED; host queries are staged aligned). */
int rl_index_create(rl_index** out, const float* embeddings, int64_t n_rows, int32_t dim,
                    const int64_t* chunk_offsets, int64_t n_chunks, int metric, int mem, void* stream);
/* fp16-STORED index.  The reference stores its embeddings as float16
 * (src/raglite/_embed.py:140, src/raglite/_database.py:279-283), so this storage is lossless for real
 * RAGLite data and halves the bytes of every HBM-bound pass.  embeddings_f16: [n_rows x dim] IEEE
 * binary16 bit patterns; dim must be one of 128, 256, 384, 512, 768, 1024 or (round 6: 1536- / 3072-wide embedders) a multiple of 128 up
 * to 4096.  Queries, scores and every other argument stay fp32; arithmetic is fp32 (VALU) or fp16 x fp16 -> fp32 MFMA (exact products).
 * rl_index_append on such an index takes fp32 rows and rounds them to nearest-even fp16;
 * rl_maxsim_rerank needs nq <= 32 and dim % 16 == 0 on it (dim 128: the cfg 3 kernel); beyond dim 1024 every MaxSim call takes up to 32
 * query vectors. */
int rl_index_create_f16(rl_index** out, const uint16_t* embeddings_f16, int64_t n_rows, int32_t dim,
                        const int64_t* chunk_offsets, int64_t n_chunks, int metric, int mem, void* stream);
int rl_index_destroy(rl_index* index);
int rl_index_info(const rl_index* index, int64_t* n_rows, int32_t* dim, int64_t* n_chunks, int* metric);
/* Device memory of an index, in bytes: out[0] the stored rows (borrowed or owned), out[1] the pre-split corpus image (0: not built),
 * out[2] the image of the hi halves, out[3] the row-major HI plane, out[4] the per-call scratch grown so far, out[5] / out[6] free /
 * total device memory now, out[7] the headroom an image has to leave free to be built.  The three images are optional accelerators
 * (4 + 2 + 2 bytes per element next to the 4 of an fp32 corpus): each is built only while it leaves max(2 GiB, 1/16 of the device) --
 * RL_OPT_IMAGE_HEADROOM_MB overrides -- free for the scratch and the caller; without them the same calls run through the kernels over
 * the stored rows (same results: every image path is bit-identical to, or re-scored exactly against, the rows).
 * Index footprint: all three images make an fp32 index 3 x its corpus.  The headline path -- MaxSim batches -- needs only the HI image:
 * with RL_OPT_KEEP_IMAGE = 0 and RL_OPT_KEEP_HI_PLANE = 0 an fp32 index of dim 256 / 384 / 512 / 768 / 1024 -- or a WIDE one, see below --
 * holds rows + HI image (1.5 x) and rl_maxsim_topk_batch / rl_maxsim_batch_begin run the same pipeline with the same results: approximate
 * pass over the HI image, exact re-scoring over the rows; only the guarded full-precision fallback (list overflow, unusable bound) changes
 * kernel -- the streaming kernels over the rows (a wide index: the exact re-scoring kernel over every chunk) instead of the eight-query
 * pass over the pre-split image.  Row searches on such an index take the kernels over the rows (B <= 16: the full fp32 pass; B >= 96:
 * score_gemm instead of the fused top-k).
 * WIDE indexes (round 6): the half-bytes routes -- HI image / HI plane, bound-filtered MaxSim batches, few-queries and fused row searches --
 * take any dim % 32 == 0 up to 1024 and, beyond, dim % 128 == 0 up to 4096 (1536- / 3072-wide embedders, src/raglite/_embed.py:155-158);
 * on a wide index even one MaxSim query goes through the sixteen-query pass and the few-queries row search takes up to 4 queries (16 at
 * dim <= 1024).  Other widths and k > 512 run on the full-precision routes: same results, 2-3 x slower. */
int rl_index_memory(const rl_index* index, int64_t out[8]);

/* Warm-up for lazy images (RL_OPT_LAZY_IMAGES, the default): build the images in `images` (RL_IMAGE_* bits) NOW, on `stream`, instead of
 * inside the first search whose route reads them -- that first call otherwise allocates device memory (0.5 x / 1 x the corpus per image),
 * makes one pass over the rows and synchronises the stream once (the norm statistics of the error bounds come back to the host), inside
 * an entry point that is asynchronous from then on.  `built` (nullable) receives the bits of the images the index holds afterwards: an
 * image the options / the shape / the free memory do not allow is simply absent (never an error -- the routes over the stored rows
 * answer, same results).  An image skipped for lack of room (it would not have left RL_OPT_IMAGE_HEADROOM_MB free) is asked for again
 * by later searches -- at most one call in 64 retries -- and by every rl_index_prepare.  Which images a workload reads: MaxSim batches
 * RL_IMAGE_HI; row searches of <= 16 queries RL_IMAGE_HI_PLANE, of >= 96 queries RL_IMAGE_PRESPLIT | RL_IMAGE_HI (table above). */
#define RL_IMAGE_PRESPLIT 1u
#define RL_IMAGE_HI 2u
#define RL_IMAGE_HI_PLANE 4u
int rl_index_prepare(rl_index* index, uint32_t images, uint32_t* built, void* stream);

/* ---- index lifecycle beyond create/destroy -----------------------------
 * rl_index_append: the device image of `insert_documents` appending `chunk_embedding` rows
 * (src/raglite/_insert.py:247-272, rows ordered by chunk, src/raglite/_database.py:403-430).
 *   rows             [n_new_rows x dim] f32 (host or device per `mem`)
 *   new_chunk_sizes  HOST int64[n_new_chunks], sum == n_new_rows; NULL -> one chunk per new row.
 * New rows / chunks get the next ordinals; existing ordinals never change.  The index takes
 * ownership of its storage on the first append (a borrowed device matrix is copied once) and grows
 * geometrically afterwards.
 * rl_index_delete_chunks: the device image of `delete_documents` (src/raglite/_delete.py:148-176).
 * The chunks' rows stay in place as tombstones (ordinals stay stable) and never match again in any
 * search of this index; deleting twice is a no-op.  chunk_ordinals is a HOST array.
 * rl_index_live: rows / chunks that are not tombstoned. */
int rl_index_append(rl_index* index, const float* rows, int64_t n_new_rows, const int64_t* new_chunk_sizes,
                    int64_t n_new_chunks, int mem, void* stream);
int rl_index_delete_chunks(rl_index* index, const int64_t* chunk_ordinals, int64_t n, void* stream);
int rl_index_live(rl_index* index, int64_t* live_rows, int64_t* live_chunks, void* stream);
/* rl_index_compact: reclaim the tombstones.  The surviving chunks keep their relative order and get the ordinals
 * 0 .. live_chunks - 1, their rows move together (one gather pass over the matrix, the per-row norms travel with
 * them), every derived structure is rebuilt; afterwards the index equals one created from the surviving rows.
 *   out_remap   HOST int64[old n_chunks] or NULL: new ordinal of every old chunk, -1 for a deleted one
 * A long-lived index under delete_documents traffic (src/raglite/_delete.py:148-176) would otherwise keep streaming
 * its dead rows in every scan.  No-op (identity remap) without tombstones.  Synchronous. */
int rl_index_compact(rl_index* index, int64_t* out_remap, int64_t* new_n_rows, int64_t* new_n_chunks, void* stream);

/* ---- arithmetic of the MFMA streaming kernel over an fp32-stored corpus --------------------------
 * The reference multiplies in fp32 (DuckDB FLOAT[d], src/raglite/_typing.py:99-134) or fp64 (NumPy,
 * src/raglite/_query_adapter.py:174); BASELINE.json asks for scores within 1e-4.  Two ways to get there:
 *   RL_ARITH_FP32_EXACT  fp32 MFMAs, bitwise an ordered fmaf chain; matrix-pipe-bound at 32 query vectors.
 *   RL_ARITH_F16_SPLIT   every fp32 operand x is scaled by a power of two and written as hi + lo with hi, lo
 *                        fp16 (22 significant bits); e.q = eh.qh + (el.qh + eh.ql) on the fp16 matrix pipe,
 *                        whose fp16 x fp16 products are exact and accumulate in fp32.  Measured error against
 *                        float64 is that of the fp32 chain; the kernel becomes
 *                        HBM-bound (10 % faster at 32 x 1M x 1024).
 * Default RL_ARITH_AUTO: F16_SPLIT when every element is finite and the largest elements of all non-zero rows
 * lie within a factor 2^10 of each other (any normalised corpus), FP32_EXACT otherwise;
 * rl_set_default_option(RL_OPT_ARITHMETIC, RL_ARITH_FP32_EXACT) makes FP32_EXACT the start value of every index created
 * afterwards.  The batched GEMM (>= 96 queries) follows the
 * same setting (22 -> 11 ms at 1000 x 1.25 M x 1024) and so does rl_maxsim_rerank's dim-128 MFMA kernel (718 k -> 875 k
 * queries/s at 32 x (256 x 64) x 128); the single-query VALU scan always computes in fp32.
 * rl_index_set_arithmetic: mode = RL_ARITH_AUTO | RL_ARITH_FP32_EXACT.
 * rl_index_arithmetic: what is in effect (FP32_EXACT, F16_SPLIT or F16_STORED). */
int rl_index_set_arithmetic(rl_index* index, int mode);
int rl_index_arithmetic(rl_index* index, int* in_effect);

/* ---- options ---------------------------------------------------------------------------------------------------------------
 * Every search below has ONE result whatever route it takes (exact top-k of exactly computed scores); the routes differ in speed
 * and memory.  The options choose routes: they exist for A/B measurements, for tests that must force a fallback, and for deployments
 * that want a smaller index.  NO environment variable is read by the library: an option is a property of an index, fixed when the
 * index is created from the process-wide defaults (rl_set_default_option: affects indexes created AFTERWARDS) and changed only
 * through rl_index_set_option -- which takes the index' mutex like every call on the handle, so a change never lands in the middle
 * of a search.  Timing-experiment builds of the kernels (instantiations that skip work and return WRONG results) are not in this
 * library at all: they are compiled only with -DRAGLITE_EXPERIMENTS (raglite_amd._build.build(experiments=True) ->
 * libraglite_hip_exp.so, used by scripts/gpu_calls/ only).
 *   key                         values (default)   what it routes
 *   RL_OPT_HI_SEARCH            0 / 1 (1)          B <= 16 row searches rank on the fp16 HI plane + exact re-scoring (else: full pass)
 *   RL_OPT_HI_MAXSIM            0 / 1 (1)          MaxSim batches rank on the HI image + exact re-scoring (else: full-precision passes)
 *   RL_OPT_HI_FEW               0 / 1 (1)          ... and ONE or TWO MaxSim queries (rl_maxsim_topk, batches of < 3) rank from the row-major HI plane
 *                                                  (2 B per element, HBM-bound) and re-score exactly (0: the streaming kernels over the fp32 rows)
 *   RL_OPT_TOPK_BLOCK           0 / 1 / 2 (2)      exact top-k of <= 262 144 scores per query (MaxSim chunk scores, the fused top-k's sample, rl_topk) in
 *                                                  ONE launch, one block per query (0: histogram / filter / final, three launches; same results);
 *                                                  2: the block first cuts the scores to the ~k that reach the k-th largest of its 1024 thread maxima
 *   RL_OPT_HI_PIVOT             0 / 1 (1)          the B <= 16 row search takes its candidate threshold from the k-th largest of ~500 workgroup maxima of the
 *                                                  approximate similarities (two launches, k <= 128) instead of ranking them exactly first (three); same results
 *   RL_OPT_HI_PRODUCTS          1 / 2 (1)          fp16 MFMA products per multiply in that approximate pass
 *   RL_OPT_PP_PASS              0 / 1 (1)          its sixteen-query kernel (maxsim_pp.hip; 0: the eight-query kernel)
 *   RL_OPT_FUSED_TOPK           0 / 1 (1)          B >= 96 row searches keep candidate lists instead of a score matrix
 *   RL_OPT_FUSED_HI             0 / 1 (1)          ... with both GEMM passes over the HI image at one product
 *   RL_OPT_FUSED_PP             0 / 1 (1)          ... and the candidate pass on the sixteen-group tile of maxsim_pp.hip
 *   RL_OPT_FUSED_PP_SAMPLE      0 / 1 (1)          ... and the sample pass before it on the same tile (0: the eight-group kernel of maxsim_gemm.hip)
 *   RL_OPT_LIST_SELECT          0 / 1 (1)          ... whose per-query lists are cut by a radix SELECT of their k-th best score (0: by sorting them)
 *   RL_OPT_FUSED_TWO_ROUNDS     0 / 1 (1)          ... in two rounds: thresholds tightened from the first 3/16 of the rows (0: one round)
 *   RL_OPT_FUSED_TOPK_CAP       0 | 1..8192 (0)    list capacity of the fused top-k (0: built-in; tests force overflows with it)
 *   RL_OPT_FUSED_TOPK_STRIDE    0 | >= 2 (0)       sample stride of the fused top-k (0: built-in rule)
 *   RL_OPT_GEMM_PASS            0 / 1 (1)          MaxSim batches of >= 3 queries share passes over the pre-split image
 *   RL_OPT_QUERY_PAIRS          0 / 1 (1)          two-query passes of the streaming kernel
 *   RL_OPT_PLANES_GEMM          0 / 1 (1)          dense row-score GEMM over the image for B >= 96 (else: score_gemm over the rows)
 *   RL_OPT_KEEP_IMAGE           0 / 1 (1)          keep the pre-split corpus image (4 B per element; 0 releases it -- MaxSim batches of an
 *                                                  fp32 index then run on rows + HI image alone, see "index footprint" below)
 *   RL_OPT_KEEP_HI              0 / 1 (1)          keep the HI plane and the HI image (2 + 2 B per element; 0 releases them)
 *   RL_OPT_KEEP_HI_PLANE        0 / 1 (1)          keep the row-major HI plane (2 B per element; what B <= 16 row searches rank on)
 *   RL_OPT_IMAGE_HEADROOM_MB    -1 | >= 0 (-1)     device memory the images must leave free (-1: max(2 GiB, 1/16 of the device))
 *   RL_OPT_ARITHMETIC           rl_arith (AUTO)    same as rl_index_set_arithmetic
 *   RL_OPT_PAIRS_PACKED         0 / 1 / 2 (2)      exact re-scoring of (query, chunk) pairs packs the candidates' rows into shared 16-row MFMA
 *                                                  tiles (0: every chunk its own tiles; same bits); 2: sixteen waves per workgroup instead of eight
 *                                                  (fp32 rows, dim % 128 == 0)
 *   RL_OPT_EXACT_KTH_THRESHOLD  0 / 1 (1)          MaxSim batches: second, tighter candidate threshold from the EXACT scores of the
 *                                                  approximate top-k (exact k-th - m instead of approximate k-th - 2 m)
 *   RL_OPT_F16_EXACT            0 / 1 (1)          rl_maxsim_topk_batch_f16 over an fp16-stored index returns the one-product pass's own top-k
 *                                                  (exact: fp16 x fp16 products, fp32 sums); 0: the bound-filtered pipeline with exact re-scoring
 *   RL_OPT_LAZY_IMAGES          0 / 1 (1)          an image is built by the FIRST call whose route reads it (allocation + one pass over the rows,
 *                                                  ~2 ms per image at 1 M x 1024, inside that call) instead of with the index: MaxSim batches ask
 *                                                  for the HI image, row searches of <= 16 queries for the HI plane, of >= 96 queries for the
 *                                                  pre-split image + HI image -- a MaxSim-only or a single-query deployment keeps 1.5 x the corpus
 *                                                  (0: every image the KEEP_* options allow is built with the index: 3 x, no first-call cost)
 * KEEP_* and IMAGE_HEADROOM_MB rebuild / release the images at once (synchronous).  Unknown key or a value outside the column above:
 * RL_ERR_INVALID.  rl_index_get_option returns what is set (not whether a route is usable on this index: rl_index_memory and
 * rl_index_filter_stats report that). */
typedef enum {
    RL_OPT_HI_SEARCH = 1, RL_OPT_HI_MAXSIM = 2, RL_OPT_HI_PRODUCTS = 3, RL_OPT_PP_PASS = 4, RL_OPT_FUSED_TOPK = 5, RL_OPT_FUSED_HI = 6,
    RL_OPT_FUSED_PP = 7, RL_OPT_FUSED_TOPK_CAP = 8, RL_OPT_FUSED_TOPK_STRIDE = 9, RL_OPT_GEMM_PASS = 10, RL_OPT_QUERY_PAIRS = 11,
    RL_OPT_PLANES_GEMM = 12, RL_OPT_KEEP_IMAGE = 13, RL_OPT_KEEP_HI = 14, RL_OPT_IMAGE_HEADROOM_MB = 15, RL_OPT_ARITHMETIC = 16,
    RL_OPT_EXACT_KTH_THRESHOLD = 17, RL_OPT_FUSED_TWO_ROUNDS = 18, RL_OPT_KEEP_HI_PLANE = 19, RL_OPT_PAIRS_PACKED = 20,
    RL_OPT_F16_EXACT = 21, RL_OPT_LAZY_IMAGES = 22, RL_OPT_FUSED_PP_SAMPLE = 23,
    RL_OPT_LIST_SELECT = 24, RL_OPT_HI_FEW = 25, RL_OPT_TOPK_BLOCK = 26, RL_OPT_HI_PIVOT = 27, RL_OPT_COUNT_ = 28
} rl_option;
/* Kernel SCHEDULE switches: keys of the same calls, numbered from 64 on (the route options above stay one contiguous range).  They change
 * where and when workgroups run, never what they compute: results are bit-identical under every value.
 *   key                         values (default)   what it schedules
 *   RL_OPT_PP_SCHEDULE          0 / 1 (1)          the sixteen-query MaxSim pass (maxsim_pp.hip): 1 = the passes over one row range run side by
 *                                                  side on one XCD, so one HBM read of the corpus serves all of them; 0 = pass after pass, each
 *                                                  pass streaming the whole HI image (raglite_amd/csrc/pp_schedule.h)
 *   RL_OPT_PP_XCD_PASSES        8 / 4 / 2 / 1 (2)  read only with RL_OPT_PP_SCHEDULE = 1: how many passes of a block of eight share an XCD at a
 *                                                  time.  8 = the co-scheduled order above (a few row ranges x all passes per XCD); 4, 2, 1 =
 *                                                  the XCD-affine order: an XCD serves that many passes for the whole launch, so their query
 *                                                  image stays in its L2, and the XCDs walk the row ranges in step (pp_schedule_affine)
 *   RL_OPT_PP_LOOP              0 / 1 (1)          the same pass at an even number of K slabs (dim % 64 == 0): 0 = the tile loop, every wave
 *                                                  spreads its loads between its own MFMAs; 1 = the alternating loop, a wave's slab is a compute
 *                                                  and a load segment, and the two waves of a SIMD run half a period apart */
enum { RL_OPT_PP_SCHEDULE = 64, RL_OPT_PP_XCD_PASSES = 65, RL_OPT_PP_LOOP = 66 };
int rl_set_default_option(int key, int64_t value);
int rl_get_default_option(int key, int64_t* value);
int rl_index_set_option(rl_index* index, int key, int64_t value);
int rl_index_get_option(rl_index* index, int key, int64_t* value);

/* ---- a6 + a7: similarity + exact row top-k ----------------------------------------------------
 * Replaces the SQL at src/raglite/_search.py:69-79 (`sim = 1 - dist`, ORDER BY dist LIMIT k) with
 * dist per src/raglite/_typing.py:123-134, ranked EXACTLY (the reference's HNSW is approximate).
 *   queries [B x dim] f32;  k <= 2048
 *   out_scores [B x k] f32 (sim, descending), out_rows [B x k] int32 (row ordinals; ties ->
 *   lowest row); when k > n_rows the tail is filled with score -inf / row -1.
 * How the rows are found does not change what is returned: up to 16 queries over a big fp32 corpus
 * rank on an fp16 "HI plane" of the corpus (2 B per element, kept by the index), bound the error
 * rigorously and re-score the candidates with the exact kernels; 96 or more queries rank through a
 * GEMM with fused candidate lists instead of a score matrix.  Both are bit-identical to the plain
 * pass + selection and fall back to it on the device where their bounds do not hold. */
int rl_search_rows(rl_index* index, const float* queries, int32_t n_queries, int32_t k,
                   float* out_scores, int32_t* out_rows, int mem, void* stream);

/* ---- the order-first cut over a corpus SHARDED across several indexes (SURVEY.md section 8e with 8f-1's rank_limit) -----
 * `rank_limit` of rl_search_rows_ranked is the reference's `ORDER BY dist LIMIT 1_000_000` over the WHOLE table
 * (src/raglite/_search.py:120-141); applied per shard it would admit up to world x rank_limit rows.  The cut is a three-level radix
 * select (11 + 11 + 10 bits of the order-preserving score key) whose histograms are additive, so the shards walk to the GLOBAL
 * threshold together when the caller sums each level over them:
 *     rl_rank_cut_begin(index, queries, B)                                  similarities of every live row, kept by the index
 *     for level in 0, 1, 2:
 *         rl_rank_cut_level(index, level, rank_limit, hist)                 hist [B x 2048] uint32: this shard's histogram of the level
 *         <sum hist over the shards: rl_allreduce_sum_u32, or any all-reduce>
 *         rl_rank_cut_level_done(index, level, hist)                        the summed histogram back
 *     rl_rank_cut_ties(index, rank_limit, ties)                             ties [B]: this shard's rows ON the threshold key
 *     <all-gather ties; ties_before[q] = sum of ties[q] over the shards holding LOWER global rows>
 *     rl_rank_cut_finish(index, rank_limit, ties_before, chunk_filter, k, out_scores, out_rows)
 * out_* [B x k]: this shard's top-k among the rows that are inside the global cut (ties on the threshold taken in global row order,
 * as the single-index cut takes them) and pass the filter; merging the shards' lists (rl_allgather_merge_topk) gives bit for bit what
 * ONE index over the whole corpus returns for rl_search_rows_ranked.  rank_limit must be smaller than the total number of rows of all
 * shards (otherwise there is no cut: call rl_search_rows_filtered).  The calls of one search must not be interleaved with other
 * searches on the same index; B x n_rows x 4 bytes of scores must fit one score batch (8 GB). */
int rl_rank_cut_begin(rl_index* index, const float* queries, int32_t n_queries, int mem, void* stream);
int rl_rank_cut_level(rl_index* index, int level, int64_t rank_limit, uint32_t* out_hist, int mem, void* stream);
int rl_rank_cut_level_done(rl_index* index, int level, const uint32_t* hist_sum, int mem, void* stream);
int rl_rank_cut_ties(rl_index* index, int64_t rank_limit, uint32_t* out_ties, int mem, void* stream);
int rl_rank_cut_finish(rl_index* index, int64_t rank_limit, const uint32_t* ties_before, const uint32_t* chunk_filter, int32_t k,
                       float* out_scores, int32_t* out_rows, int mem, void* stream);

/* ---- a6 + a7 + a8: the reference's two-stage semantics ------------------------------------------
 * top-`num_hits` rows -> max(sim) GROUP BY chunk -> top-`k` chunks (src/raglite/_search.py:66-67,
 * 75-79,143-149).  out_counts[b] (<= k) chunks are valid per query; the rest is -inf / -1. */
int rl_search_chunks(rl_index* index, const float* queries, int32_t n_queries, int32_t num_hits,
                     int32_t k, float* out_scores, int32_t* out_chunks, int32_t* out_counts,
                     int mem, void* stream);

/* ---- a9: MaxSim late interaction ----------------------------------------------------------------
 * score[c] = sum_{i<nq} max_{j in chunk c} Q[i].D[j]  -- the multi-query-vector generalisation of
 * src/raglite/_search.py:143-149 / src/raglite/_query_adapter.py:174, offered behind the reranker
 * plugin boundary (src/raglite/_search.py:394-396).  Dot-product similarity (ColBERT convention:
 * rows are pre-normalised), independent of the index metric.
 *
 * rl_maxsim_topk: one query (nq vectors) against EVERY chunk of the index, exact top-k chunks.
 *   out_scores [k] f32 descending, out_chunks [k] int32 (ties -> lowest chunk ordinal).
 * rl_maxsim_scores: the same scores, all chunks, no selection: out_scores [n_chunks]. */
int rl_maxsim_topk(rl_index* index, const float* query_vecs, int32_t nq, int32_t k,
                   float* out_scores, int32_t* out_chunks, int mem, void* stream);
int rl_maxsim_scores(rl_index* index, const float* query_vecs, int32_t nq, float* out_scores,
                     int mem, void* stream);
/* rl_maxsim_topk_batch: `n_queries` independent queries (each nq vectors) against every chunk, then ONE batched
 * selection launch for all of them.  In RL_ARITH_F16_SPLIT arithmetic eight queries (nq <= 32) share one pass over
 * the index' pre-split corpus image (fp16 hi | lo planes written when the index is built: 4 more bytes per element
 * of device memory; RL_OPT_KEEP_IMAGE = 0 releases it), otherwise two queries or one query
 * take a pass over the fp32 / fp16 rows.  On a big fp32 index (>= 64 M elements) the passes of a batch of three or
 * more queries run over an image of the hi halves only (2 more bytes per element; ONE fp16 MFMA product per multiply
 * instead of three -- q_hi . e_hi; RL_OPT_HI_PRODUCTS = 2: two), SIXTEEN queries per pass (maxsim_pp.hip; dim >= 256;
 * RL_OPT_PP_PASS = 0 or smaller dims: eight, maxsim_gemm.hip), every chunk's score error is bounded rigorously from
 * what the hi halves of corpus and queries drop, and the chunks that could be in the top-k are
 * re-scored with exact fp32 products: the same top-k, scores as accurate as before; where the bound does not decide
 * (thousands of near-identical chunks) the full-precision passes run instead, on the device.
 * RL_OPT_HI_MAXSIM = 0 / RL_OPT_KEEP_HI = 0 switch that off.  A big fp16-STORED index (rl_index_create_f16) takes the same
 * pipeline with its stored halves as that image: the approximate pass multiplies q_hi . e (what it drops, q_lo . e, is bounded the same
 * way), the candidates are re-scored over the stored rows, the two-product passes are the guarded fallback.
 *   query_vecs [n_queries x nq x dim] f32; out_scores / out_chunks [n_queries x k]. */
int rl_maxsim_topk_batch(rl_index* index, const float* query_vecs, int32_t n_queries, int32_t nq, int32_t k,
                         float* out_scores, int32_t* out_chunks, int mem, void* stream);
/* rl_maxsim_topk_batch_f16: the same search for queries that ARE IEEE fp16 values -- what the reference's embed_strings returns
 * (src/raglite/_embed.py:140,164: `astype(np.float16)`) and what its query adapter hands on (src/raglite/_search.py:62 casts the adapted
 * query back to the query's dtype).  The queries are widened on the device (exact) and take the route of rl_maxsim_topk_batch -- with one
 * difference over an fp16-STORED index (rl_index_create_f16) or an fp32-stored one whose every element is an fp16 value (measured when its HI
 * image is built: max |e_lo| == 0); batches of >= 3 queries, dim % 32 == 0, dim >= 256, no empty chunk: the product of
 * two fp16 values is exact in fp32, the index stores e itself and an fp16 query has no lo half, so the ONE-product pass of SIXTEEN queries
 * (maxsim_pp.hip) already accumulates q . e in fp32 -- its exact top-k IS the result: no error bound, no candidate list, no re-scoring
 * kernel (RL_OPT_F16_EXACT = 0: the bound-filtered pipeline of rl_maxsim_topk_batch, for A/B and parity tests).  Scores: fp32-accumulated
 * dot products in the pass's summation order (integer-valued data: bit-identical to every other route; float data: within 2^-12 relative
 * of float64, like them).  A query whose elements do not survive the pass's power-of-two scaling (a dynamic range of more than 2^24 inside
 * one query) or an index with fewer than k scorable chunks raises a device flag and the full-precision passes answer the batch (as the
 * bound-filtered pipeline's fallback; rl_index_filter_stats reports kind RL_FILTER_MAXSIM_F16_EXACT, 0 candidates, the flag).
 *   query_vecs_f16 [n_queries x nq x dim] IEEE fp16 bits, 8-byte aligned; outputs as rl_maxsim_topk_batch. */
int rl_maxsim_topk_batch_f16(rl_index* index, const uint16_t* query_vecs_f16, int32_t n_queries, int32_t nq, int32_t k,
                             float* out_scores, int32_t* out_chunks, int mem, void* stream);

/* ---- rl_maxsim_topk_batch over a corpus SHARDED across several indexes, with ONE candidate threshold for all shards -----------------
 * Every shard calling rl_maxsim_topk_batch on its own re-scores the chunks near ITS k-th best approximate score: ~235 candidates per
 * query on each of eight shards of the benchmark corpus where one index re-scores 307 in all, and that work does not shrink with the
 * shard (profiles/r03_ah_shard_step_times.txt).  The threshold only needs the k-th best approximate score over ALL shards -- which lies
 * in the union of the shards' k best -- and the largest of the shards' error bounds:
 *     rl_maxsim_batch_begin(index, queries, B, nq, k, approx)        approximate passes over this shard; approx [B x (k + 1)] f32:
 *                                                                     its k best approximate scores per query (descending), then its bound m
 *     <all-gather approx over the shards: all_approx [world x B x (k + 1)]   (rl_allgather_u32 on the bits, or any all-gather)>
 *     rl_maxsim_batch_finish(index, queries, all_approx, world, rank, out_scores, out_chunks)
 *                                                                     candidates above (global k-th best) - max m - own m, re-scored exactly
 * out_* [B x k]: this shard's chunks of that candidate set, ranked by exact score (fewer than k: padded with -inf / -1); merging the shards'
 * lists (rl_allgather_merge_topk) gives bit for bit what rl_maxsim_topk_batch returns for ONE index over the whole corpus.  A shard whose
 * bound does not decide (list overflow, fewer than k scorable chunks anywhere) answers with its exact local top-k instead, on the device,
 * as the unsharded call does.  `queries` must be the same buffer contents in both calls; no other call on this index in between.
 * RL_ERR_UNSUPPORTED from _begin (no image of the hi halves on this index, fewer than three queries, a batch size with n % 8 in {1, 2},
 * nq > 32, k > 512): call rl_maxsim_topk_batch instead -- the merge accepts either. */
int rl_maxsim_batch_begin(rl_index* index, const float* query_vecs, int32_t n_queries, int32_t nq, int32_t k, float* out_approx, int mem,
                          void* stream);
int rl_maxsim_batch_finish(rl_index* index, const float* query_vecs, const float* all_approx, int32_t world, int32_t rank, float* out_scores,
                           int32_t* out_chunks, int mem, void* stream);

/* rl_maxsim_approx_scores: the FIRST stage of rl_maxsim_topk_batch's bound-filtered pipeline on its own, for tests and for
 * callers that want the bound: the approximate MaxSim score of every (query, chunk) from the hi halves of corpus and queries
 * (one fp16 MFMA product per multiply; `kernel` = 0: the sixteen-queries-per-pass kernel of maxsim_pp.hip, 1: the
 * eight-queries-per-pass kernel of maxsim_gemm.hip -- the same products and the same sums over K; the 32 per-vector maxima of a
 * chunk are added in another order, so float scores agree to the last bits, integer-valued ones exactly), and per query the rigorous bound
 * m with |approximate - exact| <= m for EVERY chunk that rl_maxsim_topk_batch's candidate window (2 m) is built on.
 *   query_vecs [n_queries x nq x dim] f32, nq <= 32;  out_scores [n_queries x n_chunks] f32 (tombstoned chunks included: no mask),
 *   out_bound [n_queries] f32 or NULL.  RL_ERR_UNSUPPORTED when the index keeps no image for the approximate pass (small / exact-fp32
 *   indexes, indexes with empty chunks). */
int rl_maxsim_approx_scores(rl_index* index, const float* query_vecs, int32_t n_queries, int32_t nq, int kernel,
                            float* out_scores, float* out_bound, int mem, void* stream);

/* rl_maxsim_rerank: the rerank shape (SURVEY.md cfg 3).  `n_queries` independent queries in one
 * launch, each with its own nq query vectors and its own list of n_cand candidate chunk ordinals.
 *   query_vecs [n_queries x nq x dim] f32, candidates [n_queries x n_cand] int32
 *   out_scores [n_queries x n_cand] f32 in candidate order (the caller sorts: the reference
 *   reorders by `result.doc_id`, src/raglite/_search.py:396).
 * A candidate of -1 (the padding of rl_search_chunks results), a tombstoned chunk, and -- for RL_MEM_DEVICE
 * callers, whose lists are not validated on the host -- any ordinal outside [0, n_chunks) scores -inf. */
int rl_maxsim_rerank(rl_index* index, const float* query_vecs, int32_t n_queries, int32_t nq,
                     const int32_t* candidates, int32_t n_cand, float* out_scores, int mem, void* stream);

/* rl_maxsim_rerank_ragged: rl_maxsim_rerank where every query carries its own number of vectors, any number >= 1.
 *   query_vecs f32 [qv_off[n_queries] x dim]: query b owns rows qv_off[b] .. qv_off[b + 1] - 1
 *   qv_off     int64 [n_queries + 1] in HOST memory whatever `mem` says: from 0, strictly ascending (no query without vectors)
 *   candidates / out_scores [n_queries x n_cand] as in rl_maxsim_rerank, -1, tombstoned and out-of-range ordinals likewise
 * The contract: every query's scores equal, bit for bit, the fp32 sum in slab order (((s_0 + s_1) + s_2) ...) of what
 * rl_maxsim_rerank returns on this index, with the same options, for each slab of 32 of the query's vectors alone (the last
 * slab with its own shorter nq).  For a query of at most 32 vectors that is rl_maxsim_rerank itself.  No query's bits depend
 * on another query of the call.
 * Routes: dim % 16 == 0, dim <= 1024, dim != 128: one launch for all queries (maxsim_ragged_kernel), over fp32 or fp16-stored
 * rows.  dim 128, 1024 < dim <= 4096 with dim % 128 == 0, and any other dim of an fp32-stored index: a backstop that calls
 * rl_maxsim_rerank's own kernels per (query, slab) and adds the slabs in order -- correct, unhurried.  An fp16-stored index with
 * dim % 16 != 0: RL_ERR_UNSUPPORTED.  The sizes, null pointers and the table are checked before any HIP call (RL_ERR_INVALID);
 * n_queries == 0 returns RL_OK. */
int rl_maxsim_rerank_ragged(rl_index* index, const float* query_vecs, const int64_t* qv_off, int32_t n_queries,
                            const int32_t* candidates, int32_t n_cand, float* out_scores, int mem, void* stream);

/* ---- section 8e: shard merge --------------------------------------------------------------------
 * Merge `n_lists` per-shard top-k lists per query (as produced by an all-gather of each rank's
 * rl_search_rows / rl_maxsim_topk output with GLOBAL ids) into the global top-k by
 * (score desc, id asc).  in_* are [n_lists x n_queries x k_in]; out_* are [n_queries x k].
 * An entry whose id is negative is padding and its score is ignored; slots past the real entries come back as (-inf, -1).
 * n_lists * k_in <= 8192 and k <= 2048, else RL_ERR_UNSUPPORTED; k may exceed n_lists * k_in.
 * The order is rl_topk's (below): one total order on the score's bits, so NaN ranks after -inf (ids ascending, written back as
 * the one quiet NaN 0x7fc00000) and +0.0 ranks BEFORE -0.0 whatever the two ids are; only equal bit patterns tie and fall
 * through to the id. */
int rl_merge_topk(const float* in_scores, const int32_t* in_ids, int32_t n_lists, int32_t n_queries,
                  int32_t k_in, int32_t k, float* out_scores, int32_t* out_ids, int mem, void* stream);

/* The exchange step behind the C ABI: a communicator over RCCL (librccl, loaded on first use) for one process per
 * GPU.  Rank 0 calls rl_comm_unique_id and hands the 128 bytes to every rank by whatever side channel the host
 * program has (a file, an environment variable, MPI, torch.distributed's store); then EVERY rank calls rl_comm_init
 * (collective).  rl_allgather_topk: each rank's local top-k lists (device pointers, [n_queries x k]; ids LOCAL, made
 * global by adding id_offset, -1 stays -1) -> ONE ncclAllGather of (score bits, global id) records on `stream` ->
 * out_* [world x n_queries x k] on every rank.  rl_allgather_merge_topk: the same followed by rl_merge_topk's kernel:
 * out_* [n_queries x k] = the global top-k by (score desc, id asc), identical on every rank and identical to what one
 * GPU holding the whole corpus returns.  Nothing synchronises with the host.  A communicator is used by one
 * thread at a time (calls serialise on an internal mutex).  RL_ERR_UNSUPPORTED when librccl cannot be loaded.
 * A rank whose LOCAL step failed still has to enter the collective (the others are waiting in it): it contributes lists whose
 * ids are RL_ID_SHARD_MISSING (scores ignored).  rl_allgather_topk hands the marker through; rl_allgather_merge_topk answers
 * with every score NaN and every id -1 on EVERY rank -- a merge that lacks a shard never looks like an answer (no host read-back). */
#define RL_COMM_ID_BYTES 128
#define RL_ID_SHARD_MISSING (-2)
typedef struct rl_comm rl_comm;
int rl_comm_unique_id(void* out_id /* RL_COMM_ID_BYTES */);
int rl_comm_init(rl_comm** out, int rank, int world, const void* unique_id);
int rl_comm_info(const rl_comm* comm, int* rank, int* world);
int rl_comm_destroy(rl_comm* comm);
int rl_allgather_topk(rl_comm* comm, const float* local_scores, const int32_t* local_ids, int32_t n_queries, int32_t k,
                      int32_t id_offset, float* out_scores, int32_t* out_ids, void* stream);
int rl_allgather_merge_topk(rl_comm* comm, const float* local_scores, const int32_t* local_ids, int32_t n_queries,
                            int32_t k_in, int32_t id_offset, int32_t k, float* out_scores, int32_t* out_ids, void* stream);
/* The two small collectives the sharded rank cut (rl_rank_cut_*) needs, on DEVICE buffers, asynchronous on `stream`:
 * buf[i] <- sum over the ranks of buf[i] (in place), and out [world x count] <- every rank's local [count]. */
int rl_allreduce_sum_u32(rl_comm* comm, uint32_t* buf, int64_t count, void* stream);
int rl_allgather_u32(rl_comm* comm, const uint32_t* local, int64_t count, uint32_t* out, void* stream);

/* Generic exact top-k over a dense score matrix [n_queries x n] (row stride ld), the selection
 * stage used by every search above; exposed for tests and for callers that score elsewhere.
 * Order: (score desc, index asc) under ONE total order on the score's bits, the 32-bit key every selection kernel, the fused
 * top-k and the shard merge share: +inf > finite > -inf > NaN, and +0.0 > -0.0.  So every +0.0 comes before every -0.0
 * whatever their indices (the two compare equal in C; here they do not tie), every NaN comes last in index order and is
 * written back as the quiet NaN 0x7fc00000 (a payload is not kept), and all other scores come back with their own bits.
 * The host restatements (raglite_amd._sharded.merge_topk_host, oracle.topk_desc) follow the same rule.  No search produces
 * -0.0 (a similarity is 1 - distance); the rerank order (rl_rerank_order) folds -0.0 into +0.0 on purpose and is not this. */
int rl_topk(const float* scores, int32_t n_queries, int64_t n, int64_t ld, int32_t k,
            float* out_scores, int32_t* out_ids, int mem, void* stream);

/* ---- BM25 keyword search (the keyword half of hybrid search) -------------------------------------
 * Replaces src/raglite/_search.py:156-230 (DuckDB FTS `match_bm25` over chunk.body, ORDER BY score DESC LIMIT k,
 * WHERE score IS NOT NULL).  The host analyses the text and computes the statistics (raglite_amd/_keyword.py,
 * DESIGN.md "Keyword search"); a keyword index holds term-major postings over the SAME chunk ordinals as the
 * rl_index it sits beside:
 *   term_off    int64[n_terms + 1], term_off[0] = 0, ascending, term_off[n_terms] = n_postings
 *   post_chunk  int32[n_postings] chunk ordinals in [0, n_chunks), strictly ascending within a term
 *   post_tf     int32[n_postings] >= 1, occurrences of the term in the chunk
 *   post_term   int32[n_postings] the term of each posting (t for every posting of term t)
 *   idf         f32[n_terms], nrm f32[n_chunks]: ln(1 + (N - df + 0.5) / (df + 0.5)) and k1 (1 - b + b len / avgdl),
 *               computed in double and rounded to float (k1 = 1.2, b = 0.75)
 * rl_keyword_index_create checks host postings as stated; device postings are taken as given (kernels skip entries
 * outside the stated ranges).  Each posting's impact idf * ((tf * 2.2f) / (tf + nrm)) is computed once, in float, rounded
 * at every step.  post_tf / post_term / idf / nrm are not kept.
 * rl_keyword_search: query b's term ids are q_terms[q_off[b] .. q_off[b + 1]), ascending and distinct; ids outside
 * [0, n_terms) are ignored.  A chunk's score is the float sum of the impacts of the query terms it contains, in
 * ascending term order; chunks with none of them, and chunks whose chunk_filter bit (as in the *_filtered calls;
 * NULL = none) is clear, are no result.  out_scores / out_chunks [n_queries x k] by (score desc, chunk asc), unfilled
 * slots (-inf, -1); out_counts [n_queries] (may be NULL) the filled slots.  k <= 2048. */
typedef struct rl_keyword_index rl_keyword_index;
int rl_keyword_index_create(rl_keyword_index** out, const int64_t* term_off, int32_t n_terms, const int32_t* post_chunk,
                            const int32_t* post_tf, const int32_t* post_term, int64_t n_postings, const float* idf,
                            const float* nrm, int64_t n_chunks, int mem, void* stream);
int rl_keyword_search(rl_keyword_index* kw, const int64_t* q_off, const int32_t* q_terms, int32_t n_queries, int32_t k,
                      const uint32_t* chunk_filter, float* out_scores, int32_t* out_chunks, int32_t* out_counts, int mem,
                      void* stream);
int rl_keyword_index_info(const rl_keyword_index* kw, int32_t* n_terms, int64_t* n_postings, int64_t* n_chunks);
int rl_keyword_index_destroy(rl_keyword_index* kw);
/* The three arrays the handle keeps, copied out (host or device pointers by `mem`; NULL skips one): term_off [n_terms + 1],
 * post_chunk and post_impact [n_postings]. */
int rl_keyword_index_read(const rl_keyword_index* kw, int64_t* term_off, int32_t* post_chunk, float* post_impact, int mem,
                          void* stream);

/* ---- keyword store: the postings built on the device -------------------------------------------------
 * A keyword store holds, on the device, each chunk's term ids for the chunk ordinals of the rl_index it sits beside:
 *   tok_off   int64[n_chunks + 1]; tok_term int32[n_tokens]: STABLE term ids (they never change once stored), in any order
 *   inside a chunk, a repeated id is a term frequency; and a live flag per chunk.
 * rl_keyword_store_append adds n_new_chunks chunks (offsets [n_new_chunks + 1] starting at 0, ascending; term ids >= 0) with
 * amortised capacity; rl_keyword_store_delete (host ordinals) clears live flags -- a dead chunk again is a no-op -- and the
 * tokens stay.  rl_keyword_store_count builds the term-major postings of the live chunks without the host touching a
 * token: term t of the postings is term_rank[id] (term_rank: a permutation of [0, n_terms), NULL = the ids themselves;
 * checked when it is host memory), by a stable radix sort of (term, chunk) on the term and a run-length encode.  It
 * returns the statistics idf and nrm are made of: out_df [n_terms] (live chunks per term), out_length [n_chunks] (tokens
 * of a live chunk, 0 of a dead one), out_totals = (n_live, total_length, n_postings); any may be NULL.  Every stored id
 * must be < n_terms.  rl_keyword_store_build computes the impacts of the counted postings from idf [n_terms] and
 * nrm [n_chunks] (as rl_keyword_index_create states them: the host computes them, or sums the counts of several shards
 * first) and moves the postings into a fresh rl_keyword_index; it needs a count since the last append, delete or build.
 * The store keeps the scratch of its counts (about 24 B per live token, grown by a quarter beyond need) so that the count after
 * an insert allocates nothing; rl_keyword_store_info reports it in device_bytes, rl_keyword_store_destroy frees it.
 * A store with no chunks or no live tokens counts zeros and builds what rl_keyword_index_create builds from empty arrays.
 * The index is bit for bit the one rl_keyword_index_create makes from the host postings of the same chunks. */
typedef struct rl_keyword_store rl_keyword_store;
int rl_keyword_store_create(rl_keyword_store** out);
int rl_keyword_store_destroy(rl_keyword_store* s);
int rl_keyword_store_info(const rl_keyword_store* s, int64_t* n_chunks, int64_t* n_live, int64_t* n_tokens,
                          int64_t* device_bytes);
int rl_keyword_store_append(rl_keyword_store* s, const int32_t* term_ids, const int64_t* offsets, int64_t n_new_chunks,
                            int mem, void* stream);
int rl_keyword_store_delete(rl_keyword_store* s, const int64_t* chunk_ordinals, int64_t n, void* stream);
int rl_keyword_store_count(rl_keyword_store* s, const int32_t* term_rank, int32_t n_terms, int64_t* out_df,
                           int64_t* out_length, int64_t out_totals[3], int mem, void* stream);
int rl_keyword_store_build(rl_keyword_store* s, const float* idf, const float* nrm, rl_keyword_index** out, int mem,
                           void* stream);

/* ---- keyword analyzer: chunk bodies to stable term ids on the device --------
 * What raglite_amd._keyword.index_stems does per chunk and stems_to_store_ids per token, for many chunk bodies in one call:
 * fold (NFKD, drop combining marks, lowercase), split on DuckDB's `(\\.|[^a-z])+`, drop stopwords, Porter-stem, and number
 * the stems.  The library embeds neither Unicode data nor a word list: rl_keyword_analyzer_create takes
 *   fold_table  uint32[n_table] (host; n_table <= 2^21, 0x110000 covers Unicode): the image of each code point under the
 *               fold, up to six symbols in fields of 5 bits from bit 0, field = symbol + 1, 0 = no further symbol; symbols
 *               0 .. 25 = a .. z, 26 = a separator (a run of them may be given as one), 27 = a backslash, 28 = a newline.
 *               An empty image is no symbol at all.  A code point >= n_table is a separator.
 *   stopwords   the words' bytes back to back, stop_off int64[n_stop + 1] into them (host); words with a byte outside a-z
 *               can equal no token and are dropped
 *   hash_bits   0 = the full 64-bit hash of a stem; b > 0 = only its b low bits (for tests: forces stems to collide)
 * rl_keyword_analyze_begin takes codepoints uint32[n] (UTF-32) and text_off int64[n_texts + 1] (a CSR over them; starts at
 * 0, ascends, ends at n: checked when it is host memory), host or device pointers by `mem`.  Nothing carries from one text
 * to the next: neither a token nor an escape crosses a text boundary.  It leaves the call's distinct stems on the device,
 * numbered by first appearance (text order, then token order, stopwords not counted), and returns
 *   out_counts = (n_tokens: the non-stopword tokens, n_distinct, stem_bytes: the letters of all distinct stems, n_symbols:
 *   the length of the folded stream, n_all_tokens: stopwords included).
 * rl_keyword_analyze_stems copies them out (NULL skips one): stem_bytes [stem_bytes] ASCII letters, stem_off [n_distinct + 1],
 * first_pos [n_distinct] the index among the call's n_tokens of each stem's first token (ascending).  A stem may be empty
 * (the token `s`, unless it is a stopword).  The caller owns the vocabulary: rl_keyword_analyze_finish takes
 * ids int32[n_distinct] >= 0, one per distinct stem in that order, and writes, in device memory the analyzer owns until its
 * next begin or its destruction,
 *   term_ids int32[n_tokens]: the id of every kept token in text order;  offsets int64[n_texts + 1]: text c holds
 *   term_ids[offsets[c] .. offsets[c + 1]) -- what rl_keyword_store_append takes with RL_MEM_DEVICE.
 * rl_keyword_analyze_result copies both out.  Stems are made distinct by an open-addressing table of token numbers
 * (64-bit integer compare-and-swap and min, bytes compared on every hit: exact under hash collisions); nothing in the
 * outputs depends on the order in which lanes arrive, so they are the same bytes run to run.  Positions are 64-bit; one
 * call takes fewer than 2^40 code points.  The calls on one analyzer are serialised; each returns synchronised. */
typedef struct rl_keyword_analyzer rl_keyword_analyzer;
int rl_keyword_analyzer_create(rl_keyword_analyzer** out, const uint32_t* fold_table, int64_t n_table, const char* stopwords,
                               const int64_t* stop_off, int32_t n_stop, int32_t hash_bits);
int rl_keyword_analyzer_destroy(rl_keyword_analyzer* a);
int rl_keyword_analyze_begin(rl_keyword_analyzer* a, const uint32_t* codepoints, const int64_t* text_off, int64_t n,
                             int64_t n_texts, int64_t out_counts[5], int mem, void* stream);
int rl_keyword_analyze_stems(rl_keyword_analyzer* a, uint8_t* stem_bytes, int64_t* stem_off, int64_t* first_pos, int mem,
                             void* stream);
int rl_keyword_analyze_finish(rl_keyword_analyzer* a, const int32_t* ids, int mem, const int32_t** term_ids,
                              const int64_t** offsets, void* stream);
int rl_keyword_analyze_result(rl_keyword_analyzer* a, int32_t* term_ids, int64_t* offsets, int mem, void* stream);

/* ---- weighted Reciprocal Rank Fusion and batched hybrid search ---------------------------------------
 * rl_rrf_fuse replaces src/raglite/_search.py:233-252 (`reciprocal_rank_fusion`) for a batch of queries, bit for bit:
 *   lists       int32 [n_lists x n_queries x len], 1 <= n_lists <= 4, n_lists * len <= 4096: list r of query b is
 *               lists[(r * n_queries + b) * len ..]; an entry < 0 is padding (anywhere in the list) and takes no rank
 *   weights     double[n_lists], ALWAYS host memory (checked before any HIP call): finite, |w| <= 2^1000
 *   rrf_k       1 .. 2^30 (the reference's `k`, 60 in hybrid_search)
 * An ordinal's score is the float64 sum of w_r / (rrf_k + i) over its occurrences (i = its 0-based rank among the
 * results of list r), added from +0.0 in the order the reference's loop meets them -- list 0 first, each list in rank
 * order, a repeat within a list adding again -- every division and addition rounded to nearest, no contraction.
 * out_scores double / out_ids int32 [n_queries x k], 1 <= k <= n_lists * len: by score descending, equal scores by first
 * occurrence in list 0 || list 1 || ... (the reference's stable sort over its dict's insertion order); unfilled slots
 * (-inf, -1); out_counts [n_queries] (may be NULL) the filled slots.  Host or device pointers per `mem`, like rl_merge_topk.
 *
 * rl_hybrid_search replaces src/raglite/_search.py:255-279 (`hybrid_search`: vector search and keyword search, each for
 * n_each = oversample * num_results results, fused by RRF with weights (vector, keyword)) for n_queries queries at once,
 * on one stream, with no host copy of the intermediate lists:
 *   the vector half   rl_search_chunks_ranked(index, queries [n_queries x dim], num_hits, n_each, chunk_filter, rank_limit)
 *   the keyword half  rl_keyword_search(kw, q_off [n_queries + 1], q_terms, n_each, chunk_filter); kw == NULL: no keyword
 *                     half, only the vector list is fused (weights[0]); otherwise kw must cover the index' n_chunks
 *   the fusion        rl_rrf_fuse of (vector list, keyword list) with weights double[1 or 2] (host) and rrf_k -> out_scores
 *                     double / out_chunks int32 [n_queries x k], out_counts [n_queries], k <= (kw ? 2 : 1) * n_each
 * Both lists live in scratch the index owns.  Host synchronisation: none of its own beyond the RL_MEM_HOST staging;
 * the two searches keep theirs -- a call on another stream than the handle's (index or kw) previous one first waits for
 * that stream, and the first search whose route reads an image the index has not built yet builds it (synchronises). */
int rl_rrf_fuse(const int32_t* lists, int32_t n_lists, int32_t n_queries, int32_t len, const double* weights, int32_t rrf_k,
                int32_t k, double* out_scores, int32_t* out_ids, int32_t* out_counts, int mem, void* stream);
int rl_hybrid_search(rl_index* index, rl_keyword_index* kw, const float* queries, int32_t n_queries, int32_t num_hits,
                     int32_t n_each, const int64_t* q_off, const int32_t* q_terms, const uint32_t* chunk_filter,
                     int64_t rank_limit, const double* weights, int32_t rrf_k, int32_t k, double* out_scores,
                     int32_t* out_chunks, int32_t* out_counts, int mem, void* stream);

/* rl_shard_hybrid_fuse: everything after the ONE all-gather of a sharded hybrid batch (raglite_amd/_sharded.py
 * ShardedIndex.hybrid_search), one workgroup per query, LDS only.  `gathered` int32 [world x n_queries x W] is what the
 * all-gather returns: rank r's records for query b at ((r * n_queries + b) * W), W = 3 num_hits + (n_lists == 2 ? 2 n_each : 0):
 *   num_hits row records   (score f32 bits, GLOBAL row, GLOBAL chunk): that rank's rl_search_rows_ranked output
 *   n_each keyword records (score f32 bits, GLOBAL chunk): that rank's rl_keyword_search output (n_lists == 2 only)
 * An id < 0 is padding, anywhere.  Per query:
 *   1. the rows merged by (score desc, row asc; NaN after -inf), the first num_hits real ones: the global top rows;
 *   2. the first hit of each chunk among them, in that order, up to n_each: the vector list (rl_search_chunks_ranked's);
 *   3. the keyword records merged by (score desc, chunk asc), the first n_each: the keyword list;
 *   4. rl_rrf_fuse of (vector list[, keyword list]) with weights double[n_lists] (host) and rrf_k, the same arithmetic and ties.
 * out_scores double / out_chunks int32 [n_queries x k], out_counts [n_queries] (may be NULL) as rl_hybrid_search returns them:
 * the same bits as rl_hybrid_search on one index holding the whole corpus.  n_lists == 1: the vector list alone (kw == NULL there).
 * If any record of a query carries RL_ID_SHARD_MISSING, that query's outputs are poisoned: every score NaN, every id -1, count 0.
 * Limits: the rl_rrf_fuse ones on (n_lists, n_each, k, weights, rrf_k), checked before any HIP call; world * num_hits <= 4096 and
 * (n_lists == 2) world * n_each <= 4096, else RL_ERR_UNSUPPORTED (the caller composes rl_merge_topk-style merges + rl_rrf_fuse).
 * Host or device pointers per `mem`. */
int rl_shard_hybrid_fuse(const int32_t* gathered, int32_t world, int32_t n_queries, int32_t num_hits, int32_t n_each, int32_t n_lists,
                         const double* weights, int32_t rrf_k, int32_t k, double* out_scores, int32_t* out_chunks, int32_t* out_counts,
                         int mem, void* stream);

/* ---- metadata filter pushed down ---------------------------------------
 * The filter-first branch of the reference's vector search (src/raglite/_search.py:96-119): only
 * rows of chunks that match the metadata filter are ranked.  The caller evaluates the filter on its
 * metadata (host) and passes the result as a bitset over chunk ordinals:
 *   chunk_filter  uint32[(n_chunks + 31) / 32], bit (c % 32) of word (c / 32) set <=> chunk c may
 *                 match (host or device per `mem`); NULL = no filter.
 * Semantics otherwise identical to the unfiltered calls; slots that cannot be filled are reported
 * as (-inf, -1) and excluded from out_counts.  Tombstoned chunks never match, filter or not. */
int rl_search_rows_filtered(rl_index* index, const float* queries, int32_t n_queries, int32_t k,
                            const uint32_t* chunk_filter, float* out_scores, int32_t* out_rows, int mem,
                            void* stream);
int rl_search_chunks_filtered(rl_index* index, const float* queries, int32_t n_queries, int32_t num_hits,
                              int32_t k, const uint32_t* chunk_filter, float* out_scores, int32_t* out_chunks,
                              int32_t* out_counts, int mem, void* stream);
int rl_maxsim_topk_filtered(rl_index* index, const float* query_vecs, int32_t nq, int32_t k,
                            const uint32_t* chunk_filter, float* out_scores, int32_t* out_chunks, int mem,
                            void* stream);

/* The order-first-then-filter branch of the reference (src/raglite/_search.py:120-141, taken when the
 * metadata filter matches more than 100 000 embedding rows): `ORDER BY dist LIMIT 1_000_000` over the
 * UNFILTERED table, then the filter, then `ORDER BY dist LIMIT num_hits`.
 *   rank_limit  > 0: per query only its rank_limit nearest live rows -- order (similarity descending,
 *               row ascending), ties on the boundary resolved to the lowest rows (SQL leaves them
 *               unspecified) -- are eligible; chunk_filter (may be NULL) is applied to those.
 *               rank_limit >= live rows, or 0, gives exactly the *_filtered result.
 * The cut is exact (three-level radix select over the score keys), not an ANN artefact. */
int rl_search_rows_ranked(rl_index* index, const float* queries, int32_t n_queries, int32_t k,
                          const uint32_t* chunk_filter, int64_t rank_limit, float* out_scores, int32_t* out_rows,
                          int mem, void* stream);
int rl_search_chunks_ranked(rl_index* index, const float* queries, int32_t n_queries, int32_t num_hits,
                            int32_t k, const uint32_t* chunk_filter, int64_t rank_limit, float* out_scores,
                            int32_t* out_chunks, int32_t* out_counts, int mem, void* stream);

/* ---- per-query metadata filters and rank limits in one batch ------------------------------------------
 * The *_per_query calls are rl_search_chunks_ranked, rl_keyword_search and rl_hybrid_search with a filter SET in place of
 * chunk_filter and one rank limit per query: query b of the batch gets bit for bit what the single-query call returns for
 * it alone, with its own filter and limit (the same ids, score bits and count).  The single-filter calls run the same
 * device path (one filter, every query mapped to it, one limit for all).
 *   chunk_filters  uint32 [n_filters x (n_chunks + 31) / 32], each row a bitset as in the *_filtered calls; host or
 *                  device memory per `mem` (device memory whatever the rest is with RL_MEM_FILTERS_DEVICE or-ed into
 *                  `mem`).  NULL only when n_filters == 0.
 *   query_filter   int32 [n_queries], ALWAYS host memory: -1 = the query has no filter, else a row of chunk_filters.
 *                  NULL: no query has a filter.
 *   rank_limits    int64 [n_queries], ALWAYS host memory (not in the keyword call): each >= 0, as rank_limit of
 *                  rl_search_rows_ranked -- 0 or a limit at or above the live rows: no cut.  NULL: no cut for any query.
 * Tombstoned chunks never match, whether or not a query has a filter.  These arguments are checked before the index is
 * looked at and before any HIP call (RL_ERR_INVALID, naming the argument).  The host plans each sub-batch of queries:
 * its distinct filters are expanded to row bitsets (index-owned scratch, counted in rl_index_memory out[4]) in one launch,
 * and a sub-batch with a cut takes the score-matrix route with the cut, as rank_limit does; where every query of a
 * sub-batch has no filter and no cut, it runs exactly as the unfiltered call. */
int rl_search_chunks_per_query(rl_index* index, const float* queries, int32_t n_queries, int32_t num_hits, int32_t k,
                               const uint32_t* chunk_filters, int32_t n_filters, const int32_t* query_filter,
                               const int64_t* rank_limits, float* out_scores, int32_t* out_chunks, int32_t* out_counts,
                               int mem, void* stream);
int rl_keyword_search_per_query(rl_keyword_index* kw, const int64_t* q_off, const int32_t* q_terms, int32_t n_queries,
                                int32_t k, const uint32_t* chunk_filters, int32_t n_filters, const int32_t* query_filter,
                                float* out_scores, int32_t* out_chunks, int32_t* out_counts, int mem, void* stream);
int rl_hybrid_search_per_query(rl_index* index, rl_keyword_index* kw, const float* queries, int32_t n_queries,
                               int32_t num_hits, int32_t n_each, const int64_t* q_off, const int32_t* q_terms,
                               const uint32_t* chunk_filters, int32_t n_filters, const int32_t* query_filter,
                               const int64_t* rank_limits, const double* weights, int32_t rrf_k, int32_t k,
                               double* out_scores, int32_t* out_chunks, int32_t* out_counts, int mem, void* stream);

/* ---- batched search-and-rerank (src/raglite/_search.py:364-414, `search_and_rerank_chunks` with a MaxSim reranker) ----------
 * rl_rerank_order orders each query's reranked candidates as raglite_amd's MaxSimRanker.rank does on the host
 * (np.lexsort((arange, -key)), key = where(isnan(s), -inf, s)):
 *   scores      f32   [n_queries x n_cand], e.g. rl_maxsim_rerank's output
 *   candidates  int32 [n_queries x n_cand]; an entry < 0 is padding (anywhere in the list): it comes after every real
 *               candidate and is not counted.  1 <= k <= n_cand <= 4096 (one workgroup's LDS, as rl_rrf_fuse's limit).
 * The real candidates rank by score descending, NaN as -inf, -0.0 equal to +0.0, equal keys by position (stable).
 * out_scores f32 / out_chunks int32 / out_pos int32 [n_queries x k]: the input score's own bits (a NaN stays that NaN,
 * -0.0 stays -0.0), the candidate, and its position in the input list (what the reference reads as `result.doc_id`);
 * unfilled slots (-inf, -1, -1); out_counts [n_queries] the real candidates among the first k.  Sizes and `mem` are
 * checked before any HIP call (RL_ERR_INVALID); n_queries == 0 returns RL_OK.  Host or device pointers per `mem`.
 *
 * rl_search_rerank_per_query is the whole pipeline for n_queries queries on one stream, nothing read back in between:
 *   1. rl_hybrid_search_per_query (the same arguments, checks, locks and routes) with k = n_cand <= (kw ? 2 : 1) * n_each:
 *      the fused candidates [n_queries x n_cand] stay in scratch the index owns.  kw == NULL: the vector list alone,
 *      which for distinct chunks is rl_search_chunks_per_query's list;
 *   2. rl_maxsim_rerank of those candidates against query_vecs f32 [n_queries x nq x dim] (its shapes: on an fp16-stored
 *      index nq <= 32 and dim % 16 == 0, else RL_ERR_UNSUPPORTED); padding, tombstoned and out-of-range candidates
 *      score -inf;
 *   3. rl_rerank_order, the first k <= n_cand: out_scores f32 (the MaxSim scores) / out_chunks int32 [n_queries x k],
 *      best first, out_counts [n_queries].
 * nq >= 1 and 1 <= k <= n_cand <= 4096 are checked before the index is looked at.
 *
 * rl_search_rerank_ragged is that pipeline with (query_vecs f32 [qv_off[n_queries] x dim], qv_off int64 [n_queries + 1] in HOST
 * memory) in place of (query_vecs, nq): step 2 is rl_maxsim_rerank_ragged, its table, contract and routes; a query may have more
 * than 32 vectors on either storage.  The sizes, the filters and the table are checked before any HIP call. */
int rl_rerank_order(const float* scores, const int32_t* candidates, int32_t n_queries, int32_t n_cand, int32_t k,
                    float* out_scores, int32_t* out_chunks, int32_t* out_pos, int32_t* out_counts, int mem, void* stream);
int rl_search_rerank_per_query(rl_index* index, rl_keyword_index* kw, const float* queries, int32_t n_queries,
                               int32_t num_hits, int32_t n_each, const int64_t* q_off, const int32_t* q_terms,
                               const uint32_t* chunk_filters, int32_t n_filters, const int32_t* query_filter,
                               const int64_t* rank_limits, const double* weights, int32_t rrf_k, int32_t n_cand,
                               const float* query_vecs, int32_t nq, int32_t k, float* out_scores, int32_t* out_chunks,
                               int32_t* out_counts, int mem, void* stream);
int rl_search_rerank_ragged(rl_index* index, rl_keyword_index* kw, const float* queries, int32_t n_queries,
                            int32_t num_hits, int32_t n_each, const int64_t* q_off, const int32_t* q_terms,
                            const uint32_t* chunk_filters, int32_t n_filters, const int32_t* query_filter,
                            const int64_t* rank_limits, const double* weights, int32_t rrf_k, int32_t n_cand,
                            const float* query_vecs, const int64_t* qv_off, int32_t k, float* out_scores, int32_t* out_chunks,
                            int32_t* out_counts, int mem, void* stream);

/* ---- chunk spans (src/raglite/_search.py:302-361, `retrieve_chunk_spans`; :417-433, `search_and_rerank_chunk_spans`) ---------
 * A span table sits beside an rl_index as a keyword index does: it covers the SAME chunk ordinals, is immutable, and is built
 * again from the live chunks after every change of the index.
 *   doc   int32[n_chunks] (host) the dense number of the chunk's document: the place of its `Chunk.document_id` among the
 *         distinct ids in ascending string order (what the reference's sort key compares); < 0: the chunk has no position
 *         (a tombstoned chunk), it is never kept and never a neighbour
 *   pos   int32[n_chunks] (host) `Chunk.index`, >= 0 where doc >= 0; two chunks with the same (doc, pos): RL_ERR_INVALID
 * rl_span_table_create sorts the chunks that have a position by (doc, pos) on the host and uploads ordinal -> rank,
 * rank -> (doc, pos) as one 64-bit key, and rank -> ordinal.  rl_span_table_info: the chunks covered, those with a position, and
 * the device bytes held (each pointer may be NULL).
 *
 * rl_chunk_spans replaces `_search.py:323-361` for n_queries lists of chunk ordinals:
 *   chunks   int32 [n_queries x n_in], each query's chunks best first.  An entry < 0, >= the table's n_chunks or without a
 *            position is skipped and takes no rank (what `retrieve_chunks` does to unknown ids before `:324` enumerates); kept
 *            entry number i (from 0) scores 1.0 / (i + 1) in double; of a chunk that appears twice the LAST score stands (`:324`)
 *   offsets  int32 [n_off] in HOST memory whatever `mem` says; may be empty, hold 0 and repeat values.  Every kept entry adds the
 *            chunk at (doc, pos + offset) where the table holds one (`:328-340`); pos + offset is taken in 64 bits
 *   E = n_in * (1 + n_off) <= 4096, n_in >= 1, 0 <= n_off <= 64: checked with `mem` and the table before any HIP call
 *   (RL_ERR_INVALID); n_queries == 0 returns RL_OK.
 * The distinct chunks are ordered by (doc, pos) (`:342`); a chunk continues the span of the one before it iff it has the same doc
 * and the next pos (`:345-353`).  A span's score is the IEEE double sum of its members' scores, a neighbour that is no entry
 * counting 0.0, added left to right in ascending pos from 0.0 (`:356-358`; Python's sum() before 3.12).  Spans are ordered by score
 * descending, equal scores by the (doc, pos) of their first chunk (`:355-360`, a stable sort).
 *   out_chunks      int32 [n_queries x E] the distinct chunks, span after span in that order, ascending pos within a span; then -1
 *   out_span_len    int32 [n_queries x E] the chunks of each span; 0 beyond the last span
 *   out_span_scores f64   [n_queries x E] the spans' scores; 0.0 beyond the last span
 *   out_n_spans / out_n_chunks int32 [n_queries]
 *
 * rl_search_rerank_spans_per_query replaces `_search.py:417-433` with a MaxSim reranker: rl_search_rerank_per_query (its
 * arguments, checks, locks and routes) into scratch the index owns, then rl_chunk_spans of each query's reranked first k on the
 * same stream, nothing read back in between.  k * (1 + n_off) <= 4096 and the table are checked first.  out_top_chunks
 * int32 [n_queries x k] / out_top_counts [n_queries] are rl_search_rerank_per_query's out_chunks / out_counts; the span outputs
 * are rl_chunk_spans' with n_in = k.  rl_search_rerank_spans_ragged: the same over rl_search_rerank_ragged. */
typedef struct rl_span_table rl_span_table;
int rl_span_table_create(rl_span_table** out, const int32_t* doc, const int32_t* pos, int64_t n_chunks);
int rl_span_table_info(const rl_span_table* table, int64_t* n_chunks, int64_t* n_live, int64_t* device_bytes);
int rl_span_table_destroy(rl_span_table* table);
int rl_chunk_spans(const rl_span_table* table, const int32_t* chunks, int32_t n_queries, int32_t n_in, const int32_t* offsets,
                   int32_t n_off, int32_t* out_chunks, int32_t* out_span_len, double* out_span_scores, int32_t* out_n_spans,
                   int32_t* out_n_chunks, int mem, void* stream);
int rl_search_rerank_spans_per_query(rl_index* index, rl_keyword_index* kw, const float* queries, int32_t n_queries,
                                     int32_t num_hits, int32_t n_each, const int64_t* q_off, const int32_t* q_terms,
                                     const uint32_t* chunk_filters, int32_t n_filters, const int32_t* query_filter,
                                     const int64_t* rank_limits, const double* weights, int32_t rrf_k, int32_t n_cand,
                                     const float* query_vecs, int32_t nq, int32_t k, const rl_span_table* table,
                                     const int32_t* offsets, int32_t n_off, int32_t* out_top_chunks, int32_t* out_top_counts,
                                     int32_t* out_chunks, int32_t* out_span_len, double* out_span_scores, int32_t* out_n_spans,
                                     int32_t* out_n_chunks, int mem, void* stream);
int rl_search_rerank_spans_ragged(rl_index* index, rl_keyword_index* kw, const float* queries, int32_t n_queries,
                                  int32_t num_hits, int32_t n_each, const int64_t* q_off, const int32_t* q_terms,
                                  const uint32_t* chunk_filters, int32_t n_filters, const int32_t* query_filter,
                                  const int64_t* rank_limits, const double* weights, int32_t rrf_k, int32_t n_cand,
                                  const float* query_vecs, const int64_t* qv_off, int32_t k, const rl_span_table* table,
                                  const int32_t* offsets, int32_t n_off, int32_t* out_top_chunks, int32_t* out_top_counts,
                                  int32_t* out_chunks, int32_t* out_span_len, double* out_span_scores, int32_t* out_n_spans,
                                  int32_t* out_n_chunks, int mem, void* stream);

/* ---- metadata filters on the device ---------------------------------------------------------------------------------------
 * The reference's metadata filter is JSON containment (src/raglite/_search.py:82-94): a chunk matches when, for every key of
 * the filter, every wanted value occurs among the chunk's values.  The host numbers the (key, value) pairs ("tags",
 * raglite_amd/_metadata.py); an rl_metadata_store holds every chunk's tags beside the rl_index whose chunk ordinals it follows,
 * as a CSR: tag_off int64 [n_chunks + 1] from 0, ascending, and tags int32 [tag_off[n_chunks]], each chunk's list ASCENDING
 * and free of duplicates (fewer than 2^31 tags in all).  rl_metadata_store_append adds n_new chunks at the end (tag_off
 * [n_new + 1] from 0) with amortised capacity.  Deleting chunks needs no call: tombstoned chunks are evaluated like any other
 * (the searches and-in the live rows); after rl_index_compact the store is made anew.  rl_metadata_store_memory: out[0] the
 * bytes the two arrays use, out[1] the bytes reserved.  The arrays are host or device memory per `mem`; create and append
 * synchronise the stream.
 *
 * rl_metadata_filters evaluates n_filters filters in one launch.  Filter j is the tags f_tags[f_off[j] .. f_off[j + 1])
 * (f_off int64 [n_filters + 1] from 0, ascending; any order; host or device per `mem`) and matches the chunks whose list
 * holds every one of them: a filter without tags matches every chunk, a tag that no chunk carries -- INT32_MAX is never a
 * chunk's tag -- matches none.  The results stay on the device in *inout_set (NULL: a new set; else reused, grown if too small,
 * so a warm call allocates nothing): rl_filter_set_bits gives the table uint32 [n_filters x (n_chunks + 31) / 32] in the layout
 * of `chunk_filters`, the bits past n_chunks zero, which the *_per_query calls read in place under RL_MEM_FILTERS_DEVICE.
 * out_chunks[j] is the number of matching chunks and out_rows[j] the sum of their embedding rows (the index's chunk offsets):
 * what decides filter first or order first.  Both count tombstoned chunks, as the bits do, and are exact (integer atomics).
 * store->n_chunks != index->n_chunks is RL_ERR_INVALID.  Arguments that need no handle are checked first.  With RL_MEM_HOST the
 * call returns after the counts have arrived; with RL_MEM_DEVICE everything is enqueued on `stream`. */
typedef struct rl_metadata_store rl_metadata_store;
typedef struct rl_filter_set rl_filter_set;
int rl_metadata_store_create(rl_metadata_store** out, const int64_t* tag_off, const int32_t* tags, int64_t n_chunks, int mem,
                             void* stream);
int rl_metadata_store_append(rl_metadata_store* store, const int64_t* tag_off, const int32_t* tags, int64_t n_new, int mem,
                             void* stream);
int rl_metadata_store_memory(const rl_metadata_store* store, int64_t out[2]);
int rl_metadata_store_destroy(rl_metadata_store* store);
int rl_metadata_filters(rl_metadata_store* store, rl_index* index, const int64_t* f_off, const int32_t* f_tags, int32_t n_filters,
                        rl_filter_set** inout_set, int64_t* out_chunks, int64_t* out_rows, int mem, void* stream);
int rl_filter_set_bits(const rl_filter_set* set, const uint32_t** out_device_bits, int32_t* out_n_filters, int64_t* out_words);
int rl_filter_set_read(const rl_filter_set* set, uint32_t* out, int mem, void* stream); /* a copy of the table (tests, tools) */
int rl_filter_set_destroy(rl_filter_set* set);

/* ---- device half of update_query_adapter ----------------------------------
 * src/raglite/_query_adapter.py:153-205 fits the query adapter from evals: per eval a vector search
 * (rl_search_chunks, batched over all evals), then for every retrieved chunk the row
 * np.argmax(chunk.embedding_matrix @ q) (:174,180) as positive / negative example, then NNLS +
 * Procrustes on the host.
 *   rl_chunk_best_rows: queries [B x dim] f32, candidates [B x n_cand] int32 chunk ordinals (-1 =
 *     none) -> out_rows [B x n_cand] int32 row ordinals (first maximum on ties; -1 for no chunk or an
 *     empty chunk).
 *   rl_gather_rows: out[i] = embedding row rows[i] as f32 (NaN row for an out-of-range ordinal). */
int rl_chunk_best_rows(rl_index* index, const float* queries, int32_t n_queries, const int32_t* candidates,
                       int32_t n_cand, int32_t* out_rows, int mem, void* stream);
int rl_gather_rows(rl_index* index, const int32_t* rows, int64_t n, float* out, int mem, void* stream);

/* ---- the target vectors of update_query_adapter (src/raglite/_query_adapter.py:20-38) ---------------
 * Per eval the reference solves t* = argmin |q + D^T mu|^2 over mu >= 0 with D = P_i - (1 + gap) N_j over
 * the eval's positive rows P and negative rows N (an NNLS on the host).  t* is the projection of the
 * origin onto q + cone(D): unique, and an active-set iteration on the Gram matrix of the eval's example
 * rows finds it exactly.  rl_query_targets does that for every eval in one call; the rows are read in
 * place from the index by ordinal (no rl_gather_rows).
 *   queries    [B x dim] f32
 *   rows       [B x n_examples] int32 row ordinals (rl_chunk_best_rows' output), -1 = no example in
 *              this slot (anywhere in the list)
 *   relevant   [B x n_examples] uint8, nonzero = the slot's row is a positive example
 *   n_examples 2 .. RL_QT_MAX_EXAMPLES;  gap >= 0 (optimize_gap, :48)
 *   targets    [B x dim] f64: t = q + sum_i a_i P_i - (1 + gap) sum_j b_j N_j   (NaN for status 1, 2)
 *   weights    [B x n_examples] f64 by slot: the non-negative marginals a_i = sum_j mu_ij of a positive,
 *              b_j = sum_i mu_ij of a negative; 0 for an empty slot
 *   objective  [B] f64: |t|^2 (NaN for status 1, 2)
 *   status     [B]: 0 ok; 1 no positive or no negative example (the eval does not qualify, :169);
 *              2 a non-finite query / example row, or a row ordinal outside the index (never read);
 *              3 zero target, |t| <= 1e-9 |q| (the constraints cannot be met; the reference would divide
 *              by |t| = 0); 4 the cap of 4 (p + n) entering steps was reached without status 3
 *   iterations [B]: entering steps taken
 * An eval's status never affects its neighbours.  Same bits run to run and for host and device pointers. */
#define RL_QT_MAX_EXAMPLES 64
int rl_query_targets(rl_index* index, const float* queries, int32_t n_queries, const int32_t* rows, const uint8_t* relevant,
                     int32_t n_examples, double gap, double* targets, double* weights, double* objective, int32_t* status,
                     int32_t* iterations, int mem, void* stream);

/* ---- semantic-chunking similarities ---------------------------------------
 * src/raglite/_split_chunks.py:54-72, the consumer of the pooled chunklet embeddings and the cost
 * vector of the chunk partition, batched over documents.  The partition itself no longer has to
 * stay on the host: rl_partition_chunks below solves the reference's integer programme exactly on
 * the device, and rl_split_chunks chains the two without a repack.
 *   X            [n x dim] f32 chunklet embeddings of all documents, concatenated (nonzero rows)
 *   doc_offsets  int64[n_docs + 1] CSR over those rows (same side as X; starts at 0, ascends, ends at n:
 *                RL_ERR_INVALID for RL_MEM_HOST offsets that do not); NULL = one document
 *   nonoutlying  uint8[n], nonzero = chunklet size within the document's 15 %..85 % quantiles
 *                (:57-58, computed on the host from string lengths); NULL = no discourse removal
 *   out          f32[n]: out[i] = max((x_i . x_{i+1} + 1) / 2, sqrt(eps)) on the normalised,
 *                discourse-free rows (:59-72); 0 for the last row of a document.
 * A document with exactly ONE nonoutlying row keeps its plain similarities (no discourse removal):
 * its discourse vector IS that row, so the row's residual is zero in exact arithmetic, which is the
 * reference's own "would zero a row" case (:62-65).  The reference decides it by fp32 rounding (a
 * residual norm of 0 .. 2.5e-7 against eps = 1.19e-7); before this rule the device did too, and 25 /
 * 23 / 20 / 9 of 200 such documents at dim 64 / 128 / 256 / 1024 got arbitrary similarities. */
int rl_partition_similarity(const float* X, int64_t n, int32_t dim, const int64_t* doc_offsets, int64_t n_docs,
                            const uint8_t* nonoutlying, float* out, int mem, void* stream);

/* ---- chunk partition on the device --------------------------------------
 * src/raglite/_split_chunks.py:87-113 minimises cost . x over binary x (x[j] = split after chunklet j)
 * such that every window of chunklets that overflows max_size holds a split.  The windows' ends
 * ascend with their starts, so the optimum is a shortest path over split positions: exact, float64,
 * one document per wave, no limit on a document's length.  Ties: no predecessor before an equal
 * predecessor, then the smallest position (raglite_amd._chunking.partition_dp states the same
 * recurrence on the host; the two agree bit for bit).
 *   cost         f32[n], the layout rl_partition_similarity writes: cost[i] = price of a split after
 *                chunklet i; the entry at every document's last chunklet is ignored
 *   sizes        int64[n] chunklet string lengths (>= 0)
 *   doc_offsets  int64[n_docs + 1] CSR over the chunklets (starts at 0, ascends, ends at n)
 *   cut          uint8[n]: 1 = a split after chunklet i (never at a document's last chunklet)
 *   objective    f64[n_docs] (nullable): the cost of the chosen cuts; 0 without cuts; NaN with status != 0
 *   status       int32[n_docs]: 0 = ok; 1 = a chunklet larger than max_size (the reference's "Chunklet
 *                larger than chunk max_size detected."); 2 = a non-finite cost -- or, from
 *                rl_split_chunks, an embedding row of zero or NaN norm (the reference's "Chunklet
 *                embeddings with zero norm detected.").  Such a document gets no cuts.
 * RL_ERR_INVALID before any HIP call: n < 0, max_size < 1, n > 0 with n_docs < 1 or a null pointer,
 * and for RL_MEM_HOST offsets that do not start at 0 / ascend / end at n, or a negative size.  n == 0
 * returns RL_OK and writes nothing.
 *
 * rl_split_chunks = rl_partition_similarity (X, nonoutlying as there) -> the Markdown-heading
 * adjustments of :73-86 (is_heading uint8[n], nonzero = the chunklet is a heading; NULL = none) ->
 * rl_partition_chunks, on one stream, nothing through the host, one read-back for host callers.
 * cost_out f32[n] (nullable): the adjusted costs.  dim > 4096: RL_ERR_UNSUPPORTED. */
int rl_partition_chunks(const float* cost, const int64_t* sizes, const int64_t* doc_offsets, int64_t n, int64_t n_docs,
                        int64_t max_size, uint8_t* cut, double* objective, int32_t* status, int mem, void* stream);
int rl_split_chunks(const float* X, int64_t n, int32_t dim, const int64_t* doc_offsets, int64_t n_docs,
                    const uint8_t* nonoutlying, const uint8_t* is_heading, const int64_t* sizes, int64_t max_size,
                    uint8_t* cut, float* cost_out, double* objective, int32_t* status, int mem, void* stream);

/* ---- chunklet partition on the device -----------------------------------
 * src/raglite/_split_chunklets.py:136-178 cuts a document's sentences into chunklets by an exact
 * shortest path over split positions in float64:
 *   dp[i] = min over j in [lo(i), i) of dp[j] + cost(j, i),   lo(i) = smallest j with chars(j..i) <= max_size
 *   cost(j, i) = ((1.0 - p[j]) + (pb[i] - pb[j+1])) + (s - 3.0)^2 / sqrt(max(s, 1e-6)) / 2.0,  s = ps[i] - ps[j]
 * (pb, ps: prefix sums of boundary and statements, summed strictly left to right per document).  One
 * document per wave, no limit on a document's length, no atomics, same bits run to run and for host
 * and device pointers.  Ties: the smallest j; +inf takes part in ties and NaN never wins, so behind a
 * sentence longer than max_size the partition is still the reference's.  The square is x * x, where
 * the reference's NumPy scalar `** 2` calls libm pow (a last-bit difference for about one value in a
 * thousand): raglite_amd._chunklets.chunklet_dp states the same recurrence on the host and the two
 * agree bit for bit; against the reference the partitions agree.
 *   boundary     f64[n] Markdown boundary probability of every sentence (markdown_chunklet_boundaries)
 *   statements   f64[n] statement count of every sentence (compute_num_statements)
 *   lengths      int64[n] sentence string lengths (>= 0)
 *   doc_offsets  int64[n_docs + 1] CSR over the sentences (starts at 0, ascends, ends at n)
 *   cut          uint8[n]: 1 = a chunklet ends after sentence i (never at a document's last sentence)
 *   objective    f64[n_docs] (nullable): dp[n_d]; 0 for an empty document; may be +inf (status 1);
 *                NaN with status 2
 *   status       int32[n_docs]: 0 = ok; 1 = a sentence longer than max_size (the reference does not
 *                raise there, the cuts are its cuts); 2 = a non-finite boundary or statements value
 *                (no cuts; it wins over 1)
 * RL_ERR_INVALID before any HIP call: n < 0, max_size < 1, n > 0 with n_docs < 1 or a null pointer,
 * and for RL_MEM_HOST offsets that do not start at 0 / ascend / end at n, or a negative length.  n == 0
 * returns RL_OK and writes nothing. */
int rl_partition_chunklets(const double* boundary, const double* statements, const int64_t* lengths,
                           const int64_t* doc_offsets, int64_t n, int64_t n_docs, int64_t max_size,
                           uint8_t* cut, double* objective, int32_t* status, int mem, void* stream);

/* ---- sentence partition on the device -----------------------------------
 * src/raglite/_split_sentences.py:183-218: what the reference does with its model's boundary
 * probability per character.  Known boundaries override the prediction; white space is made to trail
 * a sentence (per run of white space behind a character: the minimum up to the penultimate position,
 * the maximum at the last); a dynamic programme in float64 picks the boundaries that maximise the sum
 * of (probability - 0.25) with no sentence shorter than min_len (phase 1: the earliest of equal
 * predecessors wins); every resulting sentence longer than max_len is solved again under max_len
 * (phase 2: the latest of equal predecessors in the window wins).  One document per wave, no atomics,
 * same bits run to run and for host and device pointers; raglite_amd._sentences.sentence_partition
 * states the same computation on the host and the two agree bit for bit.
 *   codepoints   uint32[n] the characters (UTF-32); the white-space class is Python's str.isspace
 *   probas       f32[n] (probas_f64 == 0) or f64[n]: the subtraction of 0.25 is done in that type
 *   known        f64[n] or NULL: a finite value replaces the prediction (cast to the type of probas)
 *   doc_offsets  int64[n_docs + 1] CSR over the characters (starts at 0, ascends, ends at n)
 *   min_len      >= 1;  max_len  0 = none
 *   cut          uint8[n]: 1 = character i is the last of a sentence (never a document's last one)
 *   objective    f64[n_docs] (nullable): the phase-1 best score; 0.0 with no boundary; NaN with status 2
 *   status       int32[n_docs]: 0 = ok; 1 = some sentence is longer than max_len (one longer than
 *                max_len but shorter than 2 * min_len comes back unsplit, as in the reference; the
 *                cuts are its cuts); 2 = a non-finite probability after the override (no cuts);
 *                3 = no valid split under max_len (no cuts; the reference raises).  2 wins over 3,
 *                3 over 1.
 * RL_ERR_INVALID before any HIP call: n < 0, min_len < 1, max_len < 0, n > 0 with n_docs < 1 or a
 * null codepoints / probas / doc_offsets / cut / status, a document of 2^31 characters or more, and
 * for RL_MEM_HOST offsets that do not start at 0 / ascend / end at n.  n == 0 returns RL_OK and
 * writes nothing. */
int rl_partition_sentences(const uint32_t* codepoints, const void* probas, int probas_f64, const double* known,
                           const int64_t* doc_offsets, int64_t n, int64_t n_docs, int64_t min_len, int64_t max_len,
                           uint8_t* cut, double* objective, int32_t* status, int mem, void* stream);

/* ---- Markdown block structure on the device ------------------------------
 * What the two splitters read from markdown-it-py's `MarkdownIt().parse` (its `commonmark` block
 * phase: code, fence, blockquote, hr, list, heading, lheading, paragraph), for many documents in one
 * call, as two arrays per line.  Lines end at \n, \r\n or a lone \r.  The contract is exact or
 * undecided: a document with status 0 has the library's tokens, token for token; a document with
 * status 1 was given up and its rows are unspecified (parse it on the host).  A document is given up
 * only where the parse meets: '<' as the first character of a line where block rules are tried (the
 * html_block rule); '[' where a paragraph would start (the reference rule); a tab in a line's leading
 * white space or behind a container marker; one of the other str.splitlines separators (U+000B,
 * U+000C, U+001C-U+001E, U+0085, U+2028, U+2029); a block at nesting level 16 or deeper.  One
 * document per wave, no atomics, the same bytes run to run and for host and device pointers.
 *   codepoints   uint32[n] the characters (UTF-32)
 *   doc_offsets  int64[n_docs + 1] CSR over the characters (starts at 0, ascends, ends at n)
 *   first_open   uint8[n + n_docs], rows line_offsets[d] .. of document d: the first of these block
 *                tokens that starts on the line: 0 none, 1 heading_open, 2 blockquote_open,
 *                3 paragraph_open, 4 bullet_list_open, 5 ordered_list_open
 *   heading_end  int32[n + n_docs]: map[1] of the heading that starts on the line, else 0
 *   line_start   int64[n + n_docs] (nullable): the line's first character, an index into codepoints
 *   line_offsets int64[n_docs + 1] CSR over the lines (str.splitlines lines; at most n + n_docs)
 *   status       int32[n_docs]: 0 = decided, 1 = undecided
 * RL_ERR_INVALID before any HIP call: n < 0, n > 0 with n_docs < 1 or a null codepoints /
 * doc_offsets / first_open / heading_end / line_offsets / status, a document of 2^31 - 64 characters
 * or more, and for RL_MEM_HOST offsets that do not start at 0 / ascend / end at n.  n == 0 returns
 * RL_OK and writes nothing. */
int rl_markdown_blocks(const uint32_t* codepoints, const int64_t* doc_offsets, int64_t n, int64_t n_docs,
                       uint8_t* first_open, int32_t* heading_end, int64_t* line_start, int64_t* line_offsets,
                       int32_t* status, int mem, void* stream);

/* The known sentence boundaries of raglite_amd._sentences.markdown_sentence_boundaries, same bits,
 * from rl_markdown_blocks' arrays (n_lines rows each, at least line_offsets[n_docs]): known f64[n] is
 * NaN by default, 0 on a heading's lines, 1 on the character before a heading and on the first
 * character behind it; where two headings write one character the later heading wins.  The
 * characters of an undecided document are NaN.  What rl_partition_sentences takes as `known`.
 * n == 0 returns RL_OK and writes nothing. */
int rl_markdown_sentence_known(const int32_t* heading_end, const int64_t* line_start, const int64_t* line_offsets,
                               const int32_t* status, const int64_t* doc_offsets, int64_t n, int64_t n_docs,
                               int64_t n_lines, double* known, int mem, void* stream);

/* The boundary probabilities of raglite_amd._chunklets.markdown_chunklet_boundaries, same bits, for
 * documents that are the concatenation of their sentences: sentence i holds the characters
 * [sentence_offsets[i], sentence_offsets[i + 1]) of codepoints (int64[n_sentences + 1]); doc_offsets
 * int64[n_docs + 1] is the CSR over the sentences.  A sentence takes the first line that starts in it
 * and bears a token: 1.0 heading, 0.75 blockquote, 0.5 paragraph, 0.25 either list, else 0; of a run
 * of consecutive non-zero sentences only the first largest keeps its value.  The sentences of an
 * undecided document get 0.  What rl_partition_chunklets takes as `boundary`.  n_sentences == 0
 * returns RL_OK and writes nothing. */
int rl_markdown_chunklet_boundary(const uint8_t* first_open, const int64_t* line_start, const int64_t* line_offsets,
                                  const int32_t* status, const int64_t* sentence_offsets, const int64_t* doc_offsets,
                                  int64_t n_sentences, int64_t n_docs, int64_t n_lines, double* boundary, int mem,
                                  void* stream);

/* ---- WordPiece on the device: the cross-encoder's tokenizer --------------
 * What the `tokenizers` library's BERT pipeline (BertNormalizer, BertPreTokenizer, WordPiece) does for
 * many texts, on their UTF-32 code points: token ids equal to tok.encode(text, add_special_tokens =
 * False).ids of the tokenizer the tables were probed from.  The library embeds neither Unicode data
 * nor a vocabulary: rl_wordpiece_create takes (all HOST pointers, copied)
 *   image        uint64[n_table]: the normalised image of a code point, three 21-bit fields from bit 0,
 *                field = code point + 1, 0 = no further one; a code point >= n_table has the empty image
 *   cls          uint8[n_table]: bits 0-1 the class of a code point where it occurs in an image (0 word
 *                character, 1 white space, 2 punctuation -- a word of its own); bit 2 the context flag of
 *                an input code point: its image may depend on its neighbours, so a text that holds one
 *                gets status 1 and its ids are NOT the contract's (the caller tokenizes it elsewhere)
 *   piece_cp     uint32: the vocabulary's pieces as UTF-32 back to back, the continuation prefix stripped
 *   piece_off    int64[n_pieces + 1] into piece_cp;  piece_flags uint8[n_pieces]: bit 0 = a continuation;
 *   piece_ids    int32[n_pieces] the token ids (>= 0).  Empty pieces and pieces longer than
 *                max_word_chars can match nothing and are left out; of equal pieces the first stays
 *   unk_id, max_word_chars (the model's max_input_chars_per_word; RL_ERR_UNSUPPORTED above 200)
 *   hash_bits    0 or 64 = all; otherwise only that many low bits of the piece hash are used (tests
 *                force collisions with it; results never depend on it: every hit compares code points)
 * rl_wordpiece_encode takes codepoints uint32[n] (UTF-32) and text_off int64[n_texts + 1] (a CSR over
 * them), host or device by `mem`; nothing carries across a text boundary.  Per text: expand through
 * image; words are maximal runs of word characters and single punctuation symbols, white space is
 * dropped; a word of more than max_word_chars normalised symbols is one unk_id; otherwise greedy
 * longest match from the left, as a continuation behind the word's first piece, and one position
 * without a match makes the whole word one unk_id.  It leaves ids int32[n_tokens], offsets
 * int64[n_texts + 1] and status uint8[n_texts] in device memory the handle owns until its next encode
 * (rl_wordpiece_device returns the pointers, rl_wordpiece_result copies them out; NULL skips one) and
 * fills out_counts (HOST) = (n_tokens, n_words, unk words, texts with status 1, normalised symbols).
 * Synchronises `stream`.  Each phase is its own launch; the only atomics are integer adds of the two
 * counters; same bytes run to run and for host and device pointers.  Calls on one handle are
 * serialised.  rl_wordpiece_info: out = (pieces kept, longest piece, table slots, device bytes held).
 * RL_ERR_INVALID before any HIP call: a null handle or pointer, n_table outside [1, 0x110000], a
 * malformed image or cls entry, piece_off that does not start at 0 or ascend, a negative id or size,
 * hash_bits outside 0 .. 64, code points without a text, and for RL_MEM_HOST text_off that does not
 * start at 0 / ascend / end at n.  RL_ERR_UNSUPPORTED: n >= 2^28 code points in one call.
 *
 * rl_wordpiece_pairs is a free function over ANY token lists (ids int32, tok_off int64[n_texts + 1]):
 * for pair p with query text a = query_text[p] and doc text b = doc_text[p] (int32 indices),
 *   (nq, nd) = the `longest_first` truncation of (tokens of a, tokens of b) to max_length - 3: one token
 *              at a time from the longer list, from the doc on a tie
 *   row p    = cls_id, a's first nq ids, sep_id, b's first nd ids, sep_id
 *   type ids = 0 for the first nq + 2 tokens, then 1;  positions = position_offset + 0, 1, ...
 *   out_seq_offsets int32[n_pairs + 1], *out_total (HOST) = the rows' tokens
 * -- the four arrays rl_encoder_classify_pack takes.  With out_ids, out_positions and out_type_ids all
 * NULL only the offsets and the total are computed (what a caller sizes the three by).  Synchronises
 * `stream`.  RL_ERR_INVALID before any HIP call: bad mem, a negative size, max_length < 3, a null
 * tok_off / out_seq_offsets / out_total / index list, one or two of the three outputs, and for
 * RL_MEM_HOST tok_off that does not start at 0 or ascend, or an index outside [0, n_texts) (device
 * callers: such a text counts as empty).  RL_ERR_UNSUPPORTED: 2^31 tokens or more in one call. */
typedef struct rl_wordpiece rl_wordpiece;
int rl_wordpiece_create(rl_wordpiece** out, const uint64_t* image, const uint8_t* cls, int64_t n_table, const uint32_t* piece_cp,
                        const int64_t* piece_off, const uint8_t* piece_flags, const int32_t* piece_ids, int64_t n_pieces,
                        int32_t unk_id, int32_t max_word_chars, int32_t hash_bits);
int rl_wordpiece_destroy(rl_wordpiece* tok);
int rl_wordpiece_info(rl_wordpiece* tok, int64_t out[4]);
int rl_wordpiece_encode(rl_wordpiece* tok, const uint32_t* codepoints, const int64_t* text_off, int64_t n, int64_t n_texts,
                        int64_t out_counts[5], int mem, void* stream);
int rl_wordpiece_result(rl_wordpiece* tok, int32_t* ids, int64_t* offsets, uint8_t* status, int mem, void* stream);
int rl_wordpiece_device(rl_wordpiece* tok, const int32_t** ids, const int64_t** offsets, const uint8_t** status);
int rl_wordpiece_pairs(const int32_t* ids, const int64_t* tok_off, int64_t n_texts, const int32_t* query_text, const int32_t* doc_text,
                       int64_t n_pairs, int32_t max_length, int32_t cls_id, int32_t sep_id, int32_t position_offset, int32_t* out_ids,
                       int32_t* out_positions, int32_t* out_type_ids, int32_t* out_seq_offsets, int64_t* out_total, int mem,
                       void* stream);

/* ---- SentencePiece Unigram on the device: the embedder's tokenizer --------
 * What a SentencePieceProcessor over a UNIGRAM model (normaliser with a precompiled character map,
 * add_dummy_prefix, remove_extra_whitespaces, escape_whitespaces; no byte fallback, no user-defined
 * pieces) does for many texts, on their UTF-32 code points: ids equal to sp.encode(text) of the model the
 * tables were read from.  The library embeds neither Unicode data nor a vocabulary: rl_sentencepiece_create
 * takes (all HOST pointers, copied)
 *   image_off    int32[n_table]: where the normalised image of a code point begins in image_pool; < 0 = the
 *                code point is its own image (as is every code point >= n_table)
 *   image_len    uint8[n_table]: bits 0-6 the image's length in code points (0: it vanishes); bit 7 the
 *                trailing-set flag of an input code point: the normaliser may consume it together with its
 *                predecessor, so a text that holds one gets status 1 and its ids are NOT the contract's
 *                (the caller tokenizes it elsewhere)
 *   image_pool   uint32[n_pool]: the images' code points back to back
 *   piece_cp     uint32: the matchable (NORMAL) pieces as UTF-32 back to back;  piece_off int64[n_pieces + 1]
 *   piece_ids    int32[n_pieces] SentencePiece ids (>= 0);  piece_scores float[n_pieces] as stored (finite)
 *                Empty pieces match nothing and are left out; of equal pieces the first stays; a piece of
 *                more than 64 code points is RL_ERR_UNSUPPORTED (one lane of a wave per start)
 *   unk_id       the SentencePiece id of the unknown piece;  unk_score = float(min score) - 10.f
 *   hash_bits    0 or 64 = all; otherwise only that many low bits of the piece hash are used (tests
 *                force collisions with it; results never depend on it: every hit compares code points)
 * rl_sentencepiece_encode takes codepoints uint32[n] (UTF-32) and text_off int64[n_texts + 1] (a CSR over
 * them), host or device by `mem`; nothing carries across a text boundary.  Per text: expand through the
 * images; U+0020 of the expanded stream is white space: leading and trailing runs go, inner runs become one
 * U+2581, one U+2581 stands in front of a text that is not empty then.  Over these symbols s[0..n) the best
 * path: best[0] = 0; for every start i ascending and every length l ascending up to the longest piece, a
 * piece s[i:i+l] offers score + best[i] (ONE float32 addition) to position i + l, taken if the position has
 * no predecessor or the sum is strictly greater; where no piece of length 1 matched at i, the unknown piece
 * offers unk_score + best[i] to i + 1 after the pieces.  The sum is carried across the WHOLE text.
 * Backtracked from n, a run of consecutive unknowns is one id.  raw_ids = 1: SentencePiece ids, the unknown
 * piece unk_id; raw_ids = 0: the XLM-RoBERTa layout, every id + 1 and the unknown piece 3.  It leaves ids
 * int32[n_tokens], offsets int64[n_texts + 1], status uint8[n_texts], the normalised symbols uint32[n_symbols]
 * and their per-text offsets int64[n_texts + 1] in device memory the handle owns until its next encode
 * (rl_sentencepiece_device returns the pointers, NULL skips one; rl_sentencepiece_result copies the first
 * three out, NULL skips one) and fills out_counts (HOST) = (n_tokens, n_symbols, unknown ids, texts with
 * status 1, the longest text in symbols).  Synchronises `stream`.  Each phase is its own launch; one text
 * per wave in the search; no float atomics, the only atomics are integer adds and one integer maximum of
 * the counters; same bytes run to run and for host and device pointers.  Calls on one handle are
 * serialised.  rl_sentencepiece_info: out = (pieces kept, longest piece, table slots, device bytes held).
 * RL_ERR_INVALID before any HIP call: a null handle or pointer, n_table outside [1, 0x110000], an image
 * outside the pool, a pool entry that is no code point, piece_off that does not start at 0 or ascend, a
 * negative id or size, a score that is not finite, hash_bits outside 0 .. 64, raw_ids outside {0, 1}, code
 * points without a text, and for RL_MEM_HOST text_off that does not start at 0 / ascend / end at n.
 * RL_ERR_UNSUPPORTED: n >= 2^25 code points or 2^31 symbols in one call.
 *
 * rl_sentencepiece_rows is a free function over ANY token lists (ids int32, tok_off int64[n_texts + 1]):
 *   row t     = bos_id, the first min(tokens of t, max_len - 2) ids of text t, eos_id
 *   positions = position_offset + 0, 1, ...
 *   out_seq_offsets int32[n_texts + 1], *out_total (HOST) = the rows' tokens
 * -- the arrays rl_encoder_forward / rl_encoder_forward_pack take.  With out_ids and out_positions both NULL
 * only the offsets and the total are computed (what a caller sizes the two by).  Synchronises `stream`.
 * RL_ERR_INVALID before any HIP call: bad mem, a negative size, max_len < 2, a null tok_off /
 * out_seq_offsets / out_total, one of the two outputs without the other, null ids with outputs, and for
 * RL_MEM_HOST tok_off that does not start at 0 or ascend.  RL_ERR_UNSUPPORTED: 2^31 tokens or more. */
typedef struct rl_sentencepiece rl_sentencepiece;
int rl_sentencepiece_create(rl_sentencepiece** out, const int32_t* image_off, const uint8_t* image_len, int64_t n_table,
                            const uint32_t* image_pool, int64_t n_pool, const uint32_t* piece_cp, const int64_t* piece_off,
                            const int32_t* piece_ids, const float* piece_scores, int64_t n_pieces, int32_t unk_id, float unk_score,
                            int32_t hash_bits);
int rl_sentencepiece_destroy(rl_sentencepiece* tok);
int rl_sentencepiece_info(rl_sentencepiece* tok, int64_t out[4]);
int rl_sentencepiece_encode(rl_sentencepiece* tok, const uint32_t* codepoints, const int64_t* text_off, int64_t n, int64_t n_texts,
                            int32_t raw_ids, int64_t out_counts[5], int mem, void* stream);
int rl_sentencepiece_result(rl_sentencepiece* tok, int32_t* ids, int64_t* offsets, uint8_t* status, int mem, void* stream);
int rl_sentencepiece_device(rl_sentencepiece* tok, const int32_t** ids, const int64_t** offsets, const uint8_t** status,
                            const uint32_t** symbols, const int64_t** symbol_offsets);
int rl_sentencepiece_rows(const int32_t* ids, const int64_t* tok_off, int64_t n_texts, int32_t max_len, int32_t bos_id, int32_t eos_id,
                          int32_t position_offset, int32_t* out_ids, int32_t* out_positions, int32_t* out_seq_offsets,
                          int64_t* out_total, int mem, void* stream);

/* What the last bound-filtered search on this index did (diagnostic; bench.py reports it next to every timed number that depends
 * on it).  The searches that rank on approximate scores and re-score what a rigorous bound cannot rule out -- rl_maxsim_topk_batch
 * over the HI image, rl_search_rows for B <= 16 over the HI plane, the fused top-k of B >= 96 -- keep per-query candidate lists of a
 * fixed capacity and a device flag on which their full-precision fallback runs.  Synchronises `stream`, then fills
 *   out[0] = kind (rl_filter_kind; 0 = no such search ran since the index was created)   out[1] = queries of that call
 *   out[2] = sum of the candidate counts   out[3] = largest count   out[4] = list capacity   out[5] = 1 when the fallback ran.
 * How the data decides both numbers is the reason this exists: they are not constants of the algorithm. */
enum rl_filter_kind { RL_FILTER_NONE = 0, RL_FILTER_MAXSIM_BATCH = 1, RL_FILTER_ROWS_HI = 2, RL_FILTER_ROWS_FUSED = 3, RL_FILTER_ROWS_FUSED_HI = 4,
                      RL_FILTER_MAXSIM_F16_EXACT = 5 };
int rl_index_filter_stats(rl_index* index, int64_t out[6], void* stream);

/* Timing hook for bench.py: run `fn`-independent -- records the elapsed milliseconds between two
 * events on `stream` bracketing `iters` back-to-back launches of the named kernel path with the
 * given index / query.  kind: 0 = rl_maxsim_scores kernel only, 1 = rl_search_rows scan kernel
 * only (no selection), 2 = the two-queries-per-pass MaxSim kernel of rl_maxsim_topk_batch (query_vecs_dev
 * then holds two queries of nq / 2 vectors each; RL_ERR_UNSUPPORTED where that kernel does not apply), 3 = the
 * eight-queries-per-pass kernel over the pre-split corpus image (eight queries of nq / 8 vectors each), 4 = the
 * ranking pass of the half-bytes search of rl_search_rows (nq <= 16 queries over the fp16 HI plane;
 * RL_ERR_UNSUPPORTED when the index has none), 5 = the approximate eight-query MaxSim pass over the HI image
 * (as kind 3) with two MFMA products per multiply, 6 = the same pass with one,
 * 7 = the SIXTEEN-queries-per-pass kernel over the HI image, one product (maxsim_pp.hip: what rl_maxsim_topk_batch runs by default;
 * sixteen queries of nq / 16 vectors each; nq > 512: nq / 32 queries of 32 vectors, all their passes in ONE launch -- grid row = pass --
 * as the batch pipeline launches them), 8 = the candidate pass of the LAST rl_search_rows call of >= 96 queries on this index that
 * went through the fused top-k over the HI image, replayed with that call's queries and thresholds (query_vecs_dev / nq are not read;
 * RL_ERR_UNSUPPORTED when no such call ran or any other search used the index since), 9 = the matrix pipe alone: the sixteen-query
 * kernel's MFMA stream (8 waves per CU, 128 accumulators each) on register-resident pseudo-random fp16 operands -- no loads, no LDS, no
 * epilogue; one launch = compute units x 8 waves x 32 000 v_mfma_f32_16x16x32_f16 (x 16 384 flop): the SUSTAINED fp16 rate of this
 * device at the clock it settles at, which bench.py prints next to the nominal peak (query_vecs_dev / nq are not read),
 * 10 = the approximate pass of the few-queries MaxSim route (rl_maxsim_topk, batches of < 3; RL_OPT_HI_FEW): ONE query of nq <= 32 vectors,
 * MaxSim over the row-major fp16 HI plane (RL_ERR_UNSUPPORTED when the index has none).
 * Used so that roofline.achieved is measured with HIP
 * events on the stream the kernel runs on. */
int rl_time_kernel(rl_index* index, int kind, const float* query_vecs_dev, int32_t nq, int32_t iters,
                   float* out_ms_total, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RAGLITE_HIP_H */
