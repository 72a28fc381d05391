// The ingestion entry points of the C ABI: pooling and normalising token embeddings, the packed encoder's attention, the native
// encoder forward for short packs and for packs of several token blocks (rl_encoder), the document-batched splitters and the WordPiece
// tokenizer that feeds the cross-encoder (rl_wordpiece) (include/raglite_hip.h for the contract of each).
#include <cmath>
#include <string>

#include "handles.h"
#include "staging.h"
#include "wordpiece_table.h"

using namespace rl;

extern "C" {

// ---- a1 + a2 + a3 ----------------------------------------------------------------------------------
int rl_pool_norm(const float* tokens, int64_t n_token_rows, int32_t dim, const int64_t* span_begin,
                 const int64_t* span_end, int64_t n_spans, int32_t normalize, double eps, float* out_f32,
                 uint16_t* out_f16, int mem, void* stream) {
    if (dim <= 0 || n_token_rows < 0 || n_spans < 0) return fail(RL_ERR_INVALID, "rl_pool_norm: negative size");
    if (n_spans > 0 && (!span_begin || !span_end)) return fail(RL_ERR_INVALID, "rl_pool_norm: null spans");
    if (!out_f32 && !out_f16) return fail(RL_ERR_INVALID, "rl_pool_norm: no output requested");
    if (!(eps >= 0.0)) return fail(RL_ERR_INVALID, "rl_pool_norm: eps must be >= 0");
    if (n_spans == 0) return RL_OK;
    hipStream_t s = as_stream(stream);
    if (mem == RL_MEM_HOST) {  // validate the spans the host handed over (device callers own their spans)
        for (int64_t i = 0; i < n_spans; ++i)
            if (span_begin[i] < 0 || span_end[i] < span_begin[i] || span_end[i] > n_token_rows)
                return fail(RL_ERR_INVALID, "rl_pool_norm: span outside the token matrix");
    }
    Staging st(mem, s);
    const float* d_tok; const int64_t* d_b; const int64_t* d_e;
    RL_TRY(st.in(tokens, (size_t)n_token_rows * dim, &d_tok));
    RL_TRY(st.in(span_begin, (size_t)n_spans, &d_b));
    RL_TRY(st.in(span_end, (size_t)n_spans, &d_e));
    float* d_o32; uint16_t* d_o16;
    RL_TRY(st.out(out_f32, (size_t)n_spans * dim, &d_o32));
    RL_TRY(st.out(out_f16, (size_t)n_spans * dim, &d_o16));
    RL_TRY(launch_pool_norm(d_tok, dim, d_b, d_e, n_spans, normalize, eps, d_o32, d_o16, s));
    return st.finish();
}

// ---- the packed encoder's attention (attention_varlen.hip) -------------------------------------------------------------------------
int rl_attention_varlen(const void* qkv, const int32_t* seq_offsets, int32_t n_seqs, int64_t n_tokens, int32_t max_len, int32_t heads,
                        int32_t head_dim, int32_t dtype, float scale, void* out, int mem, void* stream) {
    if (n_seqs < 0 || n_tokens < 0 || max_len < 0) return fail(RL_ERR_INVALID, "rl_attention_varlen: negative size");
    if (heads < 1) return fail(RL_ERR_INVALID, "rl_attention_varlen: heads must be >= 1");
    if (!(scale - scale == 0.0f)) return fail(RL_ERR_INVALID, "rl_attention_varlen: scale must be finite");
    if (dtype != RL_ATTN_BF16 && dtype != RL_ATTN_F16) return fail(RL_ERR_INVALID, "rl_attention_varlen: unknown dtype");
    if (n_seqs > 65535) return fail(RL_ERR_INVALID, "rl_attention_varlen: n_seqs must be <= 65535 (the grid's z axis)");
    if (heads > 65535) return fail(RL_ERR_INVALID, "rl_attention_varlen: heads must be <= 65535 (the grid's y axis)");
    if (n_tokens >= ((int64_t)1 << 31)) return fail(RL_ERR_INVALID, "rl_attention_varlen: n_tokens must be < 2^31 (offsets are int32)");
    if (head_dim != 32 && head_dim != 64) return fail(RL_ERR_UNSUPPORTED, "rl_attention_varlen: head_dim must be 32 or 64");
    if (mem != RL_MEM_DEVICE) return fail(RL_ERR_UNSUPPORTED, "rl_attention_varlen: device pointers only (mem must be RL_MEM_DEVICE)");
    if (n_tokens == 0) return RL_OK;
    if (!qkv || !seq_offsets || !out) return fail(RL_ERR_INVALID, "rl_attention_varlen: null argument");
    if ((reinterpret_cast<uintptr_t>(qkv) & 15) || (reinterpret_cast<uintptr_t>(out) & 7))
        return fail(RL_ERR_INVALID, "rl_attention_varlen: qkv must be 16-byte and out 8-byte aligned");
    return launch_attention_varlen(qkv, seq_offsets, n_seqs, n_tokens, max_len, heads, head_dim, dtype, scale, out, as_stream(stream));
}

// ---- the native encoder forward for short packs (encoder.hip) -------------------------------------------------------
static bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

int rl_encoder_create(rl_encoder** out, int32_t vocab, int32_t hidden, int32_t layers, int32_t heads, int32_t ffn, int32_t max_positions,
                      int32_t type_vocab, float eps, int32_t dtype, const void* tok, const void* pos, const void* typ, const void* ln_w,
                      const void* ln_b, const void* const* layer_params) {
    if (!out) return fail(RL_ERR_INVALID, "rl_encoder_create: out is null");
    *out = nullptr;
    if (vocab < 1 || hidden < 1 || layers < 1 || heads < 1 || ffn < 1 || max_positions < 1 || type_vocab < 1)
        return fail(RL_ERR_INVALID, "rl_encoder_create: every size must be >= 1");
    if (hidden % heads) return fail(RL_ERR_INVALID, "rl_encoder_create: hidden must be a multiple of heads");
    if (!(eps - eps == 0.0f) || eps < 0.0f) return fail(RL_ERR_INVALID, "rl_encoder_create: eps must be finite and >= 0");
    if (dtype != RL_ATTN_BF16 && dtype != RL_ATTN_F16) return fail(RL_ERR_INVALID, "rl_encoder_create: unknown dtype");
    if (heads > 65535) return fail(RL_ERR_INVALID, "rl_encoder_create: heads must be <= 65535 (the attention grid's y axis)");
    if (hidden / heads != 32 && hidden / heads != 64) return fail(RL_ERR_UNSUPPORTED, "rl_encoder_create: head width must be 32 or 64");
    if (hidden % 32 || ffn % 32) return fail(RL_ERR_UNSUPPORTED, "rl_encoder_create: hidden and ffn must be multiples of 32");
    if (hidden > ENC_HIDDEN_MAX || ffn > 4 * ENC_HIDDEN_MAX) return fail(RL_ERR_UNSUPPORTED, "rl_encoder_create: hidden must be <= 8192 and ffn <= 32768");
    if (!tok || !pos || !typ || !ln_w || !ln_b || !layer_params) return fail(RL_ERR_INVALID, "rl_encoder_create: null argument");
    if (misaligned(tok, 16) || misaligned(pos, 16) || misaligned(typ, 16) || misaligned(ln_w, 16) || misaligned(ln_b, 16))
        return fail(RL_ERR_INVALID, "rl_encoder_create: the embedding tables and their layer norm must be 16-byte aligned");
    for (int64_t i = 0; i < (int64_t)12 * layers; ++i) {
        if (!layer_params[i]) return fail(RL_ERR_INVALID, "rl_encoder_create: null layer parameter");
        if (misaligned(layer_params[i], 16)) return fail(RL_ERR_INVALID, "rl_encoder_create: every layer parameter must be 16-byte aligned");
    }
    std::unique_ptr<rl_encoder> e(new rl_encoder);
    e->vocab = vocab; e->hidden = hidden; e->layers = layers; e->heads = heads; e->ffn = ffn;
    e->max_positions = max_positions; e->type_vocab = type_vocab; e->dtype = dtype; e->eps = eps;
    e->tok = tok; e->pos = pos; e->typ = typ; e->ln_w = ln_w; e->ln_b = ln_b;
    e->layer.resize((size_t)layers);
    for (int32_t l = 0; l < layers; ++l) {
        const void* const* p = layer_params + (size_t)12 * l;
        e->layer[(size_t)l] = {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11]};
    }
    e->ksplit = std::max(encoder_ksplit(hidden, hidden), encoder_ksplit(hidden, ffn));
    EncoderScratch all;
    RL_TRY(carve(e->scratch, all, (size_t)RL_ENCODER_MAX_TOKENS, (size_t)hidden, (size_t)ffn, (size_t)e->ksplit));
    *out = e.release();
    return RL_OK;
}

int rl_encoder_destroy(rl_encoder* enc) {
    delete enc;
    return RL_OK;
}

int rl_encoder_info(const rl_encoder* enc, int64_t n_tokens, int32_t* max_tokens, int64_t* scratch_bytes, int64_t* used_bytes,
                    void** scratch, int32_t* launches) {
    if (n_tokens < 0 || n_tokens > RL_ENCODER_MAX_TOKENS) return fail(RL_ERR_INVALID, "rl_encoder_info: n_tokens must be in [0, RL_ENCODER_MAX_TOKENS]");
    if (!enc) return fail(RL_ERR_INVALID, "rl_encoder_info: null handle");
    if (max_tokens) *max_tokens = RL_ENCODER_MAX_TOKENS;
    if (scratch_bytes) *scratch_bytes = (int64_t)enc->scratch.cap;
    if (used_bytes) *used_bytes = (int64_t)EncoderScratch().lay(Carver(), (size_t)n_tokens, (size_t)enc->hidden, (size_t)enc->ffn, (size_t)enc->ksplit);
    if (scratch) *scratch = enc->scratch.p;
    if (launches) *launches = 1 + 7 * enc->layers;
    return RL_OK;
}

// The checks rl_encoder_forward and rl_encoder_forward_pack share, in the header's order; `cap` / `cap_name`: the most tokens of `who`.
// The handle comes after them, in the callers.
static int check_forward_args(const char* who, int64_t cap, const char* cap_name, const int32_t* ids, const int32_t* positions,
                              const int32_t* type_ids, const int32_t* seq_offsets, int32_t n_seqs, int64_t n_tokens, int32_t max_len,
                              const void* out, int mem, uintptr_t out_align = 16) {
    const std::string w(who);
    if (mem != RL_MEM_DEVICE) return fail(RL_ERR_UNSUPPORTED, w + ": device pointers only (mem must be RL_MEM_DEVICE)");
    if (n_seqs < 0 || n_tokens < 0 || max_len < 0) return fail(RL_ERR_INVALID, w + ": negative size");
    if (n_seqs > 65535) return fail(RL_ERR_INVALID, w + ": n_seqs must be <= 65535 (the attention grid's z axis)");
    if (n_tokens > cap) return fail(RL_ERR_UNSUPPORTED, w + ": n_tokens must be <= " + cap_name + " (" + std::to_string(cap) + ")");
    if (n_tokens > 0) {
        if (!ids || !positions || !seq_offsets || !out) return fail(RL_ERR_INVALID, w + ": null argument");
        if (misaligned(ids, 4) || misaligned(positions, 4) || misaligned(type_ids, 4) || misaligned(seq_offsets, 4) || misaligned(out, out_align))
            return fail(RL_ERR_INVALID, w + ": the int32 arrays must be 4-byte and out " + std::to_string(out_align) + "-byte aligned");
    }
    return RL_OK;
}

// The 1 + 7 * layers launches of a forward of M > 0 rows, with `block` as its scratch: at least EncoderScratch's walk over M rows.
static int encoder_launches(const rl_encoder* enc, const int32_t* ids, const int32_t* positions, const int32_t* type_ids,
                            const int32_t* seq_offsets, int32_t n_seqs, int32_t M, int32_t max_len, void* out, void* block, hipStream_t s) {
    const int32_t H = enc->hidden, F = enc->ffn, dt = enc->dtype;
    EncoderScratch b;  // this call's rows: a prefix of the block
    b.lay(Carver(block), (size_t)M, (size_t)H, (size_t)F, (size_t)enc->ksplit);
    const int32_t ks_out = encoder_ksplit(H, H), ks_down = encoder_ksplit(H, F);
    const float scale = 1.0f / sqrtf((float)(H / enc->heads));
    RL_TRY(launch_encoder_embed(ids, positions, type_ids, M, enc->tok, enc->vocab, enc->pos, enc->max_positions, enc->typ, enc->type_vocab,
                                enc->ln_w, enc->ln_b, H, enc->eps, dt, enc->layers ? (void*)b.x : out, s));
    for (int32_t l = 0; l < enc->layers; ++l) {
        const rl_encoder::Layer& p = enc->layer[(size_t)l];
        void* x_next = l + 1 < enc->layers ? (void*)b.x : out;  // the last layer writes the caller's rows
        RL_TRY(launch_encoder_linear(b.x, M, H, p.qkv_w, 3 * H, p.qkv_b, ENC_EPI_BIAS, dt, b.qkv, nullptr, s));
        RL_TRY(launch_attention_varlen(b.qkv, seq_offsets, n_seqs, M, max_len, enc->heads, H / enc->heads, dt, scale, b.attn, s));
        RL_TRY(launch_encoder_linear(b.attn, M, H, p.out_w, H, nullptr, ENC_EPI_PARTIAL, dt, nullptr, b.part, s));
        RL_TRY(launch_encoder_ln(b.part, ks_out, M, H, p.out_b, b.x, p.ln1_w, p.ln1_b, enc->eps, dt, b.x1, s));
        RL_TRY(launch_encoder_linear(b.x1, M, H, p.up_w, F, p.up_b, ENC_EPI_GELU, dt, b.mid, nullptr, s));
        RL_TRY(launch_encoder_linear(b.mid, M, F, p.down_w, H, nullptr, ENC_EPI_PARTIAL, dt, nullptr, b.part, s));
        RL_TRY(launch_encoder_ln(b.part, ks_down, M, H, p.down_b, b.x1, p.ln2_w, p.ln2_b, enc->eps, dt, x_next, s));
    }
    return RL_OK;
}

int rl_encoder_forward(rl_encoder* enc, const int32_t* ids, const int32_t* positions, const int32_t* type_ids, const int32_t* seq_offsets,
                       int32_t n_seqs, int64_t n_tokens, int32_t max_len, void* out, int mem, void* stream) {
    RL_TRY(check_forward_args("rl_encoder_forward", RL_ENCODER_MAX_TOKENS, "RL_ENCODER_MAX_TOKENS", ids, positions, type_ids, seq_offsets,
                              n_seqs, n_tokens, max_len, out, mem));
    if (!enc) return fail(RL_ERR_INVALID, "rl_encoder_forward: null handle");
    if (n_tokens == 0) return RL_OK;
    hipStream_t s = as_stream(stream);
    std::lock_guard<std::mutex> lock(enc->mu);
    RL_TRY(enc->last_stream.use(s));
    return encoder_launches(enc, ids, positions, type_ids, seq_offsets, n_seqs, (int32_t)n_tokens, max_len, out, enc->scratch.p, s);
}

// ---- a pack of several token blocks, on the caller's workspace -----------------------------------------------------
static size_t pack_workspace_bytes(const rl_encoder* enc, int64_t n_tokens) {  // the handle's layout, walked with the pack's rows
    return EncoderScratch().lay(Carver(), (size_t)n_tokens, (size_t)enc->hidden, (size_t)enc->ffn, (size_t)enc->ksplit);
}

int rl_encoder_pack_workspace_bytes(const rl_encoder* enc, int64_t n_tokens, int64_t* bytes) {
    if (n_tokens < 0 || n_tokens > RL_ENCODER_MAX_PACK_TOKENS)
        return fail(RL_ERR_INVALID, "rl_encoder_pack_workspace_bytes: n_tokens must be in [0, RL_ENCODER_MAX_PACK_TOKENS]");
    if (!bytes) return fail(RL_ERR_INVALID, "rl_encoder_pack_workspace_bytes: bytes is null");
    if (!enc) return fail(RL_ERR_INVALID, "rl_encoder_pack_workspace_bytes: null handle");
    *bytes = (int64_t)pack_workspace_bytes(enc, n_tokens);
    return RL_OK;
}

int rl_encoder_forward_pack(rl_encoder* enc, const int32_t* ids, const int32_t* positions, const int32_t* type_ids,
                            const int32_t* seq_offsets, int32_t n_seqs, int64_t n_tokens, int32_t max_len, void* out, void* workspace,
                            int64_t workspace_bytes, int mem, void* stream) {
    RL_TRY(check_forward_args("rl_encoder_forward_pack", RL_ENCODER_MAX_PACK_TOKENS, "RL_ENCODER_MAX_PACK_TOKENS", ids, positions, type_ids,
                              seq_offsets, n_seqs, n_tokens, max_len, out, mem));
    if (n_tokens > 0) {
        if (!workspace) return fail(RL_ERR_INVALID, "rl_encoder_forward_pack: workspace is null");
        if (misaligned(workspace, 16)) return fail(RL_ERR_INVALID, "rl_encoder_forward_pack: workspace must be 16-byte aligned");
    }
    if (!enc) return fail(RL_ERR_INVALID, "rl_encoder_forward_pack: null handle");
    if (n_tokens == 0) return RL_OK;
    if (workspace_bytes < 0 || (uint64_t)workspace_bytes < (uint64_t)pack_workspace_bytes(enc, n_tokens))
        return fail(RL_ERR_INVALID, "rl_encoder_forward_pack: workspace_bytes is less than rl_encoder_pack_workspace_bytes(n_tokens)");
    // (the handle's own scratch, its mutex and its stream record are not involved: the workspace is the caller's)
    return encoder_launches(enc, ids, positions, type_ids, seq_offsets, n_seqs, (int32_t)n_tokens, max_len, out, workspace, as_stream(stream));
}

// The forward's three launches one at a time (what tests/test_gpu_encoder_kernels.py holds to float64): every argument checked here, the
// launchers as rl_encoder_forward calls them.
static_assert(RL_ENC_EPI_BIAS == ENC_EPI_BIAS && RL_ENC_EPI_GELU == ENC_EPI_GELU && RL_ENC_EPI_PARTIAL == ENC_EPI_PARTIAL,
              "the header's epilogue names are the launcher's");

static bool bad_width(int32_t n) { return n < 32 || n % 32 != 0; }
static bool bad_eps(float eps) { return !(eps - eps == 0.0f) || eps < 0.0f; }

int rl_encoder_embed(const int32_t* ids, const int32_t* positions, const int32_t* type_ids, int64_t n_tokens, const void* tok, int32_t vocab,
                     const void* pos, int32_t max_positions, const void* typ, int32_t type_vocab, const void* ln_w, const void* ln_b,
                     int32_t hidden, float eps, int32_t dtype, void* out, int mem, void* stream) {
    if (mem != RL_MEM_DEVICE) return fail(RL_ERR_UNSUPPORTED, "rl_encoder_embed: device pointers only (mem must be RL_MEM_DEVICE)");
    if (n_tokens < 0 || n_tokens > RL_ENCODER_MAX_TOKENS) return fail(RL_ERR_INVALID, "rl_encoder_embed: n_tokens must be in [0, RL_ENCODER_MAX_TOKENS]");
    if (vocab < 1 || max_positions < 1 || type_vocab < 1) return fail(RL_ERR_INVALID, "rl_encoder_embed: every table must have at least one row");
    if (bad_width(hidden)) return fail(RL_ERR_INVALID, "rl_encoder_embed: hidden must be a positive multiple of 32");
    if (hidden > ENC_HIDDEN_MAX) return fail(RL_ERR_UNSUPPORTED, "rl_encoder_embed: hidden must be <= 8192");
    if (bad_eps(eps)) return fail(RL_ERR_INVALID, "rl_encoder_embed: eps must be finite and >= 0");
    if (dtype != RL_ATTN_BF16 && dtype != RL_ATTN_F16) return fail(RL_ERR_INVALID, "rl_encoder_embed: unknown dtype");
    if (n_tokens == 0) return RL_OK;
    if (!ids || !positions || !tok || !pos || !typ || !ln_w || !ln_b || !out) return fail(RL_ERR_INVALID, "rl_encoder_embed: null argument");
    if (misaligned(ids, 4) || misaligned(positions, 4) || misaligned(type_ids, 4))
        return fail(RL_ERR_INVALID, "rl_encoder_embed: the int32 arrays must be 4-byte aligned");
    if (misaligned(tok, 16) || misaligned(pos, 16) || misaligned(typ, 16))
        return fail(RL_ERR_INVALID, "rl_encoder_embed: the embedding tables must be 16-byte aligned");
    if (misaligned(ln_w, 8) || misaligned(ln_b, 8) || misaligned(out, 8))
        return fail(RL_ERR_INVALID, "rl_encoder_embed: ln_w, ln_b and out must be 8-byte aligned");
    return launch_encoder_embed(ids, positions, type_ids, (int32_t)n_tokens, tok, vocab, pos, max_positions, typ, type_vocab, ln_w, ln_b, hidden,
                                eps, dtype, out, as_stream(stream));
}

int rl_encoder_linear_slices(int32_t N, int32_t K, int32_t* slices) {
    if (bad_width(N) || bad_width(K)) return fail(RL_ERR_INVALID, "rl_encoder_linear_slices: N and K must be positive multiples of 32");
    if (!slices) return fail(RL_ERR_INVALID, "rl_encoder_linear_slices: slices is null");
    *slices = encoder_ksplit(N, K);
    return RL_OK;
}

// rl_encoder_linear and rl_encoder_linear_pack: the same checks and the same launcher; `cap_name` names the most rows of `who`.
static int linear_entry(const char* who, int64_t cap, const char* cap_name, const void* x, int64_t M, int32_t K, const void* W, int32_t N,
                        const void* bias, int32_t epilogue, int32_t dtype, void* out16, float* part, int mem, void* stream) {
    const std::string w(who);
    if (mem != RL_MEM_DEVICE) return fail(RL_ERR_UNSUPPORTED, w + ": device pointers only (mem must be RL_MEM_DEVICE)");
    if (M < 0 || M > cap) return fail(RL_ERR_INVALID, w + ": M must be in [0, " + cap_name + "]");
    if (bad_width(K) || bad_width(N)) return fail(RL_ERR_INVALID, w + ": K and N must be positive multiples of 32");
    if (dtype != RL_ATTN_BF16 && dtype != RL_ATTN_F16) return fail(RL_ERR_INVALID, w + ": unknown dtype");
    if (epilogue != RL_ENC_EPI_BIAS && epilogue != RL_ENC_EPI_GELU && epilogue != RL_ENC_EPI_PARTIAL)
        return fail(RL_ERR_INVALID, w + ": unknown epilogue");
    if (M == 0) return RL_OK;
    const bool partial = epilogue == RL_ENC_EPI_PARTIAL;
    if (!x || !W) return fail(RL_ERR_INVALID, w + ": null argument");
    if (partial && !part) return fail(RL_ERR_INVALID, w + ": the partial epilogue writes part, which is null");
    if (!partial && !out16) return fail(RL_ERR_INVALID, w + ": the bias and GELU epilogues write out16, which is null");
    if (!partial && !bias) return fail(RL_ERR_INVALID, w + ": the bias and GELU epilogues read bias, which is null");
    if (misaligned(x, 16) || misaligned(W, 16) || (partial && misaligned(part, 16)))
        return fail(RL_ERR_INVALID, w + ": x, W and part must be 16-byte aligned");
    if (!partial && (misaligned(bias, 8) || misaligned(out16, 8)))
        return fail(RL_ERR_INVALID, w + ": bias and out16 must be 8-byte aligned");
    return launch_encoder_linear(x, (int32_t)M, K, W, N, partial ? nullptr : bias, epilogue, dtype, partial ? nullptr : out16,
                                 partial ? part : nullptr, as_stream(stream));
}

int rl_encoder_linear(const void* x, int64_t M, int32_t K, const void* W, int32_t N, const void* bias, int32_t epilogue, int32_t dtype,
                      void* out16, float* part, int mem, void* stream) {
    return linear_entry("rl_encoder_linear", RL_ENCODER_MAX_TOKENS, "RL_ENCODER_MAX_TOKENS", x, M, K, W, N, bias, epilogue, dtype, out16, part,
                        mem, stream);
}

int rl_encoder_linear_pack(const void* x, int64_t M, int32_t K, const void* W, int32_t N, const void* bias, int32_t epilogue, int32_t dtype,
                           void* out16, float* part, int mem, void* stream) {
    return linear_entry("rl_encoder_linear_pack", RL_ENCODER_MAX_PACK_TOKENS, "RL_ENCODER_MAX_PACK_TOKENS", x, M, K, W, N, bias, epilogue,
                        dtype, out16, part, mem, stream);
}

int rl_encoder_layer_norm(const float* part, int32_t slices, int64_t M, int32_t hidden, const void* bias, const void* resid, const void* ln_w,
                          const void* ln_b, float eps, int32_t dtype, void* out, int mem, void* stream) {
    if (mem != RL_MEM_DEVICE) return fail(RL_ERR_UNSUPPORTED, "rl_encoder_layer_norm: device pointers only (mem must be RL_MEM_DEVICE)");
    if (M < 0 || M > RL_ENCODER_MAX_TOKENS) return fail(RL_ERR_INVALID, "rl_encoder_layer_norm: M must be in [0, RL_ENCODER_MAX_TOKENS]");
    if (slices < 1 || slices > ENC_KSPLIT_MAX) return fail(RL_ERR_INVALID, "rl_encoder_layer_norm: slices must be in [1, 8]");
    if (bad_width(hidden)) return fail(RL_ERR_INVALID, "rl_encoder_layer_norm: hidden must be a positive multiple of 32");
    if (hidden > ENC_HIDDEN_MAX) return fail(RL_ERR_UNSUPPORTED, "rl_encoder_layer_norm: hidden must be <= 8192");
    if (bad_eps(eps)) return fail(RL_ERR_INVALID, "rl_encoder_layer_norm: eps must be finite and >= 0");
    if (dtype != RL_ATTN_BF16 && dtype != RL_ATTN_F16) return fail(RL_ERR_INVALID, "rl_encoder_layer_norm: unknown dtype");
    if (M == 0) return RL_OK;
    if (!part || !bias || !resid || !ln_w || !ln_b || !out) return fail(RL_ERR_INVALID, "rl_encoder_layer_norm: null argument");
    if (misaligned(part, 16)) return fail(RL_ERR_INVALID, "rl_encoder_layer_norm: part must be 16-byte aligned");
    if (misaligned(bias, 8) || misaligned(resid, 8) || misaligned(ln_w, 8) || misaligned(ln_b, 8) || misaligned(out, 8))
        return fail(RL_ERR_INVALID, "rl_encoder_layer_norm: bias, resid, ln_w, ln_b and out must be 8-byte aligned");
    return launch_encoder_ln(part, slices, (int32_t)M, hidden, bias, resid, ln_w, ln_b, eps, dtype, out, as_stream(stream));
}

// ---- the cross-encoder's head on the native forward (encoder_head.hip) ------------------------------------------------
int rl_encoder_head(const void* x, const int32_t* seq_offsets, int32_t n_seqs, int64_t n_tokens, int32_t hidden, const void* pooler_w,
                    const void* pooler_b, const void* head_w, const void* head_b, int32_t dtype, float* out_logits, int mem, void* stream) {
    if (mem != RL_MEM_DEVICE) return fail(RL_ERR_UNSUPPORTED, "rl_encoder_head: device pointers only (mem must be RL_MEM_DEVICE)");
    if (n_seqs < 0 || n_seqs > 65535) return fail(RL_ERR_INVALID, "rl_encoder_head: n_seqs must be in [0, 65535]");
    if (n_tokens < 0 || n_tokens >= ((int64_t)1 << 31)) return fail(RL_ERR_INVALID, "rl_encoder_head: n_tokens must be in [0, 2^31)");
    if (bad_width(hidden)) return fail(RL_ERR_INVALID, "rl_encoder_head: hidden must be a positive multiple of 32");
    if (hidden > ENC_HIDDEN_MAX) return fail(RL_ERR_UNSUPPORTED, "rl_encoder_head: hidden must be <= 8192");
    if (dtype != RL_ATTN_BF16 && dtype != RL_ATTN_F16) return fail(RL_ERR_INVALID, "rl_encoder_head: unknown dtype");
    if (n_seqs == 0) return RL_OK;
    if (n_tokens == 0) return fail(RL_ERR_INVALID, "rl_encoder_head: n_tokens must be >= 1 when there are sequences");
    if (!x || !seq_offsets || !pooler_w || !pooler_b || !head_w || !head_b || !out_logits) return fail(RL_ERR_INVALID, "rl_encoder_head: null argument");
    if (misaligned(x, 16) || misaligned(pooler_w, 16) || misaligned(pooler_b, 16) || misaligned(head_w, 16) || misaligned(head_b, 16))
        return fail(RL_ERR_INVALID, "rl_encoder_head: x and the four parameters must be 16-byte aligned");
    if (misaligned(seq_offsets, 4) || misaligned(out_logits, 4)) return fail(RL_ERR_INVALID, "rl_encoder_head: seq_offsets and out_logits must be 4-byte aligned");
    return launch_encoder_head(x, seq_offsets, n_seqs, (int32_t)n_tokens, hidden, pooler_w, pooler_b, head_w, head_b, dtype, out_logits,
                               as_stream(stream));
}

int rl_encoder_set_head(rl_encoder* enc, const void* pooler_w, const void* pooler_b, const void* head_w, const void* head_b) {
    const int given = (pooler_w != nullptr) + (pooler_b != nullptr) + (head_w != nullptr) + (head_b != nullptr);
    if (given != 0 && given != 4) return fail(RL_ERR_INVALID, "rl_encoder_set_head: give all four pointers, or none to clear the head");
    if (misaligned(pooler_w, 16) || misaligned(pooler_b, 16) || misaligned(head_w, 16) || misaligned(head_b, 16))
        return fail(RL_ERR_INVALID, "rl_encoder_set_head: every parameter must be 16-byte aligned");
    if (!enc) return fail(RL_ERR_INVALID, "rl_encoder_set_head: null handle");
    std::lock_guard<std::mutex> lock(enc->mu);
    enc->pooler_w = pooler_w; enc->pooler_b = pooler_b; enc->head_w = head_w; enc->head_b = head_b;
    return RL_OK;
}

static size_t classify_workspace_bytes(const rl_encoder* enc, int64_t n_tokens) {  // the one walk: rl_encoder_classify_pack takes its pointers from it
    return EncoderClassifyScratch().lay(Carver(), (size_t)n_tokens, (size_t)enc->hidden, (size_t)enc->ffn, (size_t)enc->ksplit);
}

int rl_encoder_classify_workspace_bytes(const rl_encoder* enc, int64_t n_tokens, int32_t n_seqs, int64_t* bytes) {
    if (n_tokens < 0 || n_tokens > RL_ENCODER_MAX_PACK_TOKENS)
        return fail(RL_ERR_INVALID, "rl_encoder_classify_workspace_bytes: n_tokens must be in [0, RL_ENCODER_MAX_PACK_TOKENS]");
    if (n_seqs < 0 || n_seqs > 65535) return fail(RL_ERR_INVALID, "rl_encoder_classify_workspace_bytes: n_seqs must be in [0, 65535]");
    if (!bytes) return fail(RL_ERR_INVALID, "rl_encoder_classify_workspace_bytes: bytes is null");
    if (!enc) return fail(RL_ERR_INVALID, "rl_encoder_classify_workspace_bytes: null handle");
    *bytes = (int64_t)classify_workspace_bytes(enc, n_tokens);
    return RL_OK;
}

int rl_encoder_classify_pack(rl_encoder* enc, const int32_t* ids, const int32_t* positions, const int32_t* type_ids,
                             const int32_t* seq_offsets, int32_t n_seqs, int64_t n_tokens, int32_t max_len, float* out_logits,
                             void* workspace, int64_t workspace_bytes, int mem, void* stream) {
    RL_TRY(check_forward_args("rl_encoder_classify_pack", RL_ENCODER_MAX_PACK_TOKENS, "RL_ENCODER_MAX_PACK_TOKENS", ids, positions, type_ids,
                              seq_offsets, n_seqs, n_tokens, max_len, out_logits, mem, 4));
    if (n_tokens > 0) {
        if (!workspace) return fail(RL_ERR_INVALID, "rl_encoder_classify_pack: workspace is null");
        if (misaligned(workspace, 16)) return fail(RL_ERR_INVALID, "rl_encoder_classify_pack: workspace must be 16-byte aligned");
    }
    if (!enc) return fail(RL_ERR_INVALID, "rl_encoder_classify_pack: null handle");
    const void *pw, *pb, *hw, *hb;
    {
        std::lock_guard<std::mutex> lock(enc->mu);
        pw = enc->pooler_w; pb = enc->pooler_b; hw = enc->head_w; hb = enc->head_b;
    }
    if (!pw) return fail(RL_ERR_INVALID, "rl_encoder_classify_pack: the handle has no head (rl_encoder_set_head)");
    if (n_tokens == 0) return RL_OK;
    if (workspace_bytes < 0 || (uint64_t)workspace_bytes < (uint64_t)classify_workspace_bytes(enc, n_tokens))
        return fail(RL_ERR_INVALID, "rl_encoder_classify_pack: workspace_bytes is less than rl_encoder_classify_workspace_bytes(n_tokens, n_seqs)");
    EncoderClassifyScratch w;  // the trunk's scratch lies at the workspace's start: its launches get the block rl_encoder_forward_pack gives them
    w.lay(Carver(workspace), (size_t)n_tokens, (size_t)enc->hidden, (size_t)enc->ffn, (size_t)enc->ksplit);
    hipStream_t s = as_stream(stream);
    RL_TRY(encoder_launches(enc, ids, positions, type_ids, seq_offsets, n_seqs, (int32_t)n_tokens, max_len, w.final_rows, workspace, s));
    return launch_encoder_head(w.final_rows, seq_offsets, n_seqs, (int32_t)n_tokens, enc->hidden, pw, pb, hw, hb, enc->dtype, out_logits, s);
}

// ---- document-batched ingestion: similarities, chunk / chunklet / sentence partitions (kernels in partition_sim.hip, partition_dp.hip,
// ---- chunklet_dp.hip, sentence_dp.hip; the offset conventions in doc_batch.h) ---------------------------------------------------------
// Host offsets are checked here, before the first HIP call; device offsets are clamped by the kernels (doc_batch.h).  doc_max > 0:
// every document must be shorter than that many rows; its one caller is rl_partition_sentences with 2^31, which the text names.
static int check_doc_offsets(const char* who, const int64_t* off, int64_t n, int64_t n_docs, int mem, int64_t doc_max) {
    if (mem != RL_MEM_HOST) return RL_OK;
    const std::string w(who);
    if (off[0] != 0) return fail(RL_ERR_INVALID, w + ": doc_offsets must start at 0");
    for (int64_t d = 0; d < n_docs; ++d) {
        if (off[d + 1] < off[d]) return fail(RL_ERR_INVALID, w + ": doc_offsets must be ascending");
        if (doc_max > 0 && off[d + 1] - off[d] >= doc_max) return fail(RL_ERR_INVALID, w + ": a document must be shorter than 2^31 characters");
    }
    if (off[n_docs] != n) return fail(RL_ERR_INVALID, w + ": doc_offsets must end at n");
    return RL_OK;
}

int rl_partition_similarity(const float* X, int64_t n, int32_t dim, const int64_t* doc_offsets, int64_t n_docs,
                            const uint8_t* nonoutlying, float* out, int mem, void* stream) {
    if (n < 0 || dim <= 0) return fail(RL_ERR_INVALID, "rl_partition_similarity: bad shape");
    if (n == 0) return RL_OK;
    if (!X || !out) return fail(RL_ERR_INVALID, "rl_partition_similarity: null argument");
    if (dim > 4096) return fail(RL_ERR_UNSUPPORTED, "rl_partition_similarity: dim must be <= 4096");
    if (!doc_offsets) n_docs = 1;
    if (n_docs < 1) return fail(RL_ERR_INVALID, "rl_partition_similarity: need at least one document");
    if (doc_offsets) RL_TRY(check_doc_offsets("rl_partition_similarity", doc_offsets, n, n_docs, mem, 0));
    hipStream_t s = as_stream(stream);
    Staging st(mem, s);
    const float* d_x; const int64_t* d_off; const uint8_t* d_sel = nullptr; float* d_out;
    RL_TRY(st.in(X, (size_t)n * dim, &d_x));
    const int64_t one[2] = {0, n};  // one document: offsets made here (outlives the copy: the call ends synchronised)
    if (doc_offsets) RL_TRY(st.in(doc_offsets, (size_t)n_docs + 1, &d_off));
    else RL_TRY(st.in(one, 2, &d_off, RL_MEM_HOST));
    if (nonoutlying) RL_TRY(st.in(nonoutlying, (size_t)n, &d_sel));
    RL_TRY(st.out(out, (size_t)n, &d_out));
    void* d_scr;
    RL_TRY(st.temp(partition_sim_scratch_bytes(n, n_docs, dim), &d_scr));
    RL_TRY(launch_partition_similarity(d_x, n, dim, d_off, n_docs, d_sel, d_out, d_scr, s));
    return st.finish();
}

// Argument checks shared by rl_partition_chunks, rl_split_chunks and rl_partition_chunklets; all of them return before the first HIP call.
static int partition_args(const char* who, const int64_t* sizes, const int64_t* doc_offsets, int64_t n, int64_t n_docs, const uint8_t* cut,
                          const int32_t* status, int mem) {
    const std::string w(who);
    if (n_docs < 1) return fail(RL_ERR_INVALID, w + ": n_docs must be >= 1");
    if (!sizes) return fail(RL_ERR_INVALID, w + ": sizes is null");
    if (!doc_offsets) return fail(RL_ERR_INVALID, w + ": doc_offsets is null");
    if (!cut) return fail(RL_ERR_INVALID, w + ": cut is null");
    if (!status) return fail(RL_ERR_INVALID, w + ": status is null");
    RL_TRY(check_doc_offsets(who, doc_offsets, n, n_docs, mem, 0));
    if (mem == RL_MEM_HOST) {
        for (int64_t i = 0; i < n; ++i)
            if (sizes[i] < 0) return fail(RL_ERR_INVALID, w + ": sizes must be >= 0");
    }
    return RL_OK;
}

int rl_partition_chunks(const float* cost, const int64_t* sizes, const int64_t* doc_offsets, int64_t n, int64_t n_docs, int64_t max_size,
                        uint8_t* cut, double* objective, int32_t* status, int mem, void* stream) {
    if (n < 0) return fail(RL_ERR_INVALID, "rl_partition_chunks: n must be >= 0");
    if (max_size < 1) return fail(RL_ERR_INVALID, "rl_partition_chunks: max_size must be >= 1");
    RL_TRY(check_mem(mem, "rl_partition_chunks"));
    if (n == 0) return RL_OK;
    if (!cost) return fail(RL_ERR_INVALID, "rl_partition_chunks: cost is null");
    RL_TRY(partition_args("rl_partition_chunks", sizes, doc_offsets, n, n_docs, cut, status, mem));
    hipStream_t s = as_stream(stream);
    Staging st(mem, s);
    const float* d_c; const int64_t* d_sz; const int64_t* d_off;
    RL_TRY(st.in(cost, (size_t)n, &d_c));
    RL_TRY(st.in(sizes, (size_t)n, &d_sz));
    RL_TRY(st.in(doc_offsets, (size_t)n_docs + 1, &d_off));
    uint8_t* d_cut; double* d_obj; int32_t* d_status;
    RL_TRY(st.out(cut, (size_t)n, &d_cut));
    RL_TRY(st.out(objective, (size_t)n_docs, &d_obj));  // (optional)
    RL_TRY(st.out(status, (size_t)n_docs, &d_status));
    void* d_scr;
    RL_TRY(st.temp(partition_dp_scratch_bytes(n), &d_scr));
    RL_TRY(launch_partition_dp(d_c, d_sz, nullptr, d_off, n, n_docs, max_size, d_cut, d_obj, d_status, d_scr, s));
    return st.finish();
}

int rl_split_chunks(const float* X, int64_t n, int32_t dim, const int64_t* doc_offsets, int64_t n_docs, const uint8_t* nonoutlying,
                    const uint8_t* is_heading, const int64_t* sizes, int64_t max_size, uint8_t* cut, float* cost_out, double* objective,
                    int32_t* status, int mem, void* stream) {
    if (n < 0 || dim <= 0) return fail(RL_ERR_INVALID, "rl_split_chunks: bad shape (n, dim)");
    if (max_size < 1) return fail(RL_ERR_INVALID, "rl_split_chunks: max_size must be >= 1");
    RL_TRY(check_mem(mem, "rl_split_chunks"));
    if (n == 0) return RL_OK;
    if (!X) return fail(RL_ERR_INVALID, "rl_split_chunks: X is null");
    RL_TRY(partition_args("rl_split_chunks", sizes, doc_offsets, n, n_docs, cut, status, mem));
    if (dim > 4096) return fail(RL_ERR_UNSUPPORTED, "rl_split_chunks: dim must be <= 4096");
    hipStream_t s = as_stream(stream);
    Staging st(mem, s);
    const float* d_x; const int64_t* d_sz; const int64_t* d_off; const uint8_t* d_sel = nullptr; const uint8_t* d_head = nullptr;
    float* d_cost;
    RL_TRY(st.in(X, (size_t)n * dim, &d_x));
    RL_TRY(st.in(sizes, (size_t)n, &d_sz));
    RL_TRY(st.in(doc_offsets, (size_t)n_docs + 1, &d_off));
    if (nonoutlying) RL_TRY(st.in(nonoutlying, (size_t)n, &d_sel));
    if (is_heading) RL_TRY(st.in(is_heading, (size_t)n, &d_head));
    uint8_t* d_cut; double* d_obj; int32_t* d_status;
    RL_TRY(st.out(cut, (size_t)n, &d_cut));
    RL_TRY(st.out(objective, (size_t)n_docs, &d_obj));  // (optional)
    RL_TRY(st.out(status, (size_t)n_docs, &d_status));
    RL_TRY(st.out_or_temp(cost_out, (size_t)n, &d_cost));
    void* d_scr;
    RL_TRY(st.temp(partition_sim_scratch_bytes(n, n_docs, dim), &d_scr));
    void* d_dp;
    RL_TRY(st.temp(partition_dp_scratch_bytes(n), &d_dp));
    RL_TRY(launch_partition_similarity(d_x, n, dim, d_off, n_docs, d_sel, d_cost, d_scr, s));
    if (d_head) RL_TRY(launch_partition_headings(d_cost, d_head, d_off, n_docs, n, s));  // in place: entry i reads sim[i] alone
    RL_TRY(launch_partition_dp(d_cost, d_sz, static_cast<float*>(d_scr) /* 1 / |x_i| */, d_off, n, n_docs, max_size, d_cut, d_obj, d_status,
                               d_dp, s));
    return st.finish();
}

int rl_partition_chunklets(const double* boundary, const double* statements, const int64_t* lengths, const int64_t* doc_offsets, int64_t n,
                           int64_t n_docs, int64_t max_size, uint8_t* cut, double* objective, int32_t* status, int mem, void* stream) {
    if (n < 0) return fail(RL_ERR_INVALID, "rl_partition_chunklets: n must be >= 0");
    if (max_size < 1) return fail(RL_ERR_INVALID, "rl_partition_chunklets: max_size must be >= 1");
    RL_TRY(check_mem(mem, "rl_partition_chunklets"));
    if (n == 0) return RL_OK;
    if (!boundary) return fail(RL_ERR_INVALID, "rl_partition_chunklets: boundary is null");
    if (!statements) return fail(RL_ERR_INVALID, "rl_partition_chunklets: statements is null");
    RL_TRY(partition_args("rl_partition_chunklets", lengths, doc_offsets, n, n_docs, cut, status, mem));
    hipStream_t s = as_stream(stream);
    Staging st(mem, s);
    const double* d_b; const double* d_s; const int64_t* d_len; const int64_t* d_off;
    RL_TRY(st.in(boundary, (size_t)n, &d_b));
    RL_TRY(st.in(statements, (size_t)n, &d_s));
    RL_TRY(st.in(lengths, (size_t)n, &d_len));
    RL_TRY(st.in(doc_offsets, (size_t)n_docs + 1, &d_off));
    uint8_t* d_cut; double* d_obj; int32_t* d_status;
    RL_TRY(st.out(cut, (size_t)n, &d_cut));
    RL_TRY(st.out(objective, (size_t)n_docs, &d_obj));  // (optional)
    RL_TRY(st.out(status, (size_t)n_docs, &d_status));
    void* d_scr;
    RL_TRY(st.temp(chunklet_dp_scratch_bytes(n, n_docs), &d_scr));
    RL_TRY(launch_chunklet_dp(d_b, d_s, d_len, d_off, n, n_docs, max_size, d_cut, d_obj, d_status, d_scr, s));
    return st.finish();
}

int rl_partition_sentences(const uint32_t* codepoints, const void* probas, int probas_f64, const double* known, const int64_t* doc_offsets,
                           int64_t n, int64_t n_docs, int64_t min_len, int64_t max_len, uint8_t* cut, double* objective, int32_t* status,
                           int mem, void* stream) {
    if (n < 0) return fail(RL_ERR_INVALID, "rl_partition_sentences: n must be >= 0");
    if (min_len < 1) return fail(RL_ERR_INVALID, "rl_partition_sentences: min_len must be >= 1");
    if (max_len < 0) return fail(RL_ERR_INVALID, "rl_partition_sentences: max_len must be >= 0 (0: none)");
    RL_TRY(check_mem(mem, "rl_partition_sentences"));
    if (n == 0) return RL_OK;
    if (n_docs < 1) return fail(RL_ERR_INVALID, "rl_partition_sentences: n_docs must be >= 1");
    if (!codepoints) return fail(RL_ERR_INVALID, "rl_partition_sentences: codepoints is null");
    if (!probas) return fail(RL_ERR_INVALID, "rl_partition_sentences: probas is null");
    if (!doc_offsets) return fail(RL_ERR_INVALID, "rl_partition_sentences: doc_offsets is null");
    if (!cut) return fail(RL_ERR_INVALID, "rl_partition_sentences: cut is null");
    if (!status) return fail(RL_ERR_INVALID, "rl_partition_sentences: status is null");
    const int64_t doc_max = (int64_t)1 << 31;  // back-pointers are int32
    if (n_docs == 1 && n >= doc_max) return fail(RL_ERR_INVALID, "rl_partition_sentences: a document must be shorter than 2^31 characters");
    RL_TRY(check_doc_offsets("rl_partition_sentences", doc_offsets, n, n_docs, mem, doc_max));
    hipStream_t s = as_stream(stream);
    Staging st(mem, s);
    const uint32_t* d_cp; const uint8_t* d_p; const double* d_k = nullptr; const int64_t* d_off;
    RL_TRY(st.in(codepoints, (size_t)n, &d_cp));
    RL_TRY(st.in(static_cast<const uint8_t*>(probas), (size_t)n * (probas_f64 ? 8 : 4), &d_p));
    if (known) RL_TRY(st.in(known, (size_t)n, &d_k));
    RL_TRY(st.in(doc_offsets, (size_t)n_docs + 1, &d_off));
    uint8_t* d_cut; double* d_obj; int32_t* d_status;
    RL_TRY(st.out(cut, (size_t)n, &d_cut));
    RL_TRY(st.out(objective, (size_t)n_docs, &d_obj));  // (optional)
    RL_TRY(st.out(status, (size_t)n_docs, &d_status));
    void* d_scr;
    RL_TRY(st.temp(sentence_dp_scratch_bytes(n, n_docs), &d_scr));
    RL_TRY(launch_sentence_dp(d_cp, d_p, probas_f64, d_k, d_off, n, n_docs, min_len, max_len, d_cut, d_obj, d_status, d_scr, s));
    return st.finish();
}

// ---- Markdown block structure for the splitters (markdown.hip, markdown_blocks.h) --------------------------------------
// The line offsets a host caller hands to the two derived entries: ascending from 0 and inside the per-line arrays.
static int check_line_offsets(const char* who, const int64_t* off, int64_t n_docs, int64_t n_lines, int mem) {
    if (mem != RL_MEM_HOST) return RL_OK;
    const std::string w(who);
    if (off[0] != 0) return fail(RL_ERR_INVALID, w + ": line_offsets must start at 0");
    for (int64_t d = 0; d < n_docs; ++d)
        if (off[d + 1] < off[d]) return fail(RL_ERR_INVALID, w + ": line_offsets must be ascending");
    if (off[n_docs] > n_lines) return fail(RL_ERR_INVALID, w + ": line_offsets must end at or before n_lines");
    return RL_OK;
}

int rl_markdown_blocks(const uint32_t* codepoints, const int64_t* doc_offsets, int64_t n, int64_t n_docs, uint8_t* first_open,
                       int32_t* heading_end, int64_t* line_start, int64_t* line_offsets, int32_t* status, int mem, void* stream) {
    if (n < 0) return fail(RL_ERR_INVALID, "rl_markdown_blocks: n must be >= 0");
    RL_TRY(check_mem(mem, "rl_markdown_blocks"));
    if (n == 0) return RL_OK;
    if (n_docs < 1) return fail(RL_ERR_INVALID, "rl_markdown_blocks: n_docs must be >= 1");
    if (!codepoints) return fail(RL_ERR_INVALID, "rl_markdown_blocks: codepoints is null");
    if (!doc_offsets) return fail(RL_ERR_INVALID, "rl_markdown_blocks: doc_offsets is null");
    if (!first_open || !heading_end) return fail(RL_ERR_INVALID, "rl_markdown_blocks: first_open or heading_end is null");
    if (!line_offsets) return fail(RL_ERR_INVALID, "rl_markdown_blocks: line_offsets is null");
    if (!status) return fail(RL_ERR_INVALID, "rl_markdown_blocks: status is null");
    const int64_t doc_max = ((int64_t)1 << 31) - 64;  // positions are int32 (markdown.hip: MB_DOC_MAX)
    if (n_docs == 1 && n >= doc_max) return fail(RL_ERR_INVALID, "rl_markdown_blocks: a document must be shorter than 2^31 characters");
    RL_TRY(check_doc_offsets("rl_markdown_blocks", doc_offsets, n, n_docs, mem, doc_max));
    hipStream_t s = as_stream(stream);
    Staging st(mem, s);
    const size_t rows = (size_t)n + (size_t)n_docs;
    const uint32_t* d_cp; const int64_t* d_off;
    RL_TRY(st.in(codepoints, (size_t)n, &d_cp));
    RL_TRY(st.in(doc_offsets, (size_t)n_docs + 1, &d_off));
    uint8_t* d_first; int32_t* d_end; int64_t* d_start; int64_t* d_loff; int32_t* d_status;
    RL_TRY(st.out(first_open, rows, &d_first));
    RL_TRY(st.out(heading_end, rows, &d_end));
    RL_TRY(st.out(line_start, rows, &d_start));  // (optional)
    RL_TRY(st.out(line_offsets, (size_t)n_docs + 1, &d_loff));
    RL_TRY(st.out(status, (size_t)n_docs, &d_status));
    void* d_scr;
    RL_TRY(st.temp(markdown_blocks_scratch_bytes(n, n_docs), &d_scr));
    RL_TRY(launch_markdown_blocks(d_cp, d_off, n, n_docs, d_first, d_end, d_start, d_loff, d_status, d_scr, s));
    return st.finish();
}

int rl_markdown_sentence_known(const int32_t* heading_end, const int64_t* line_start, const int64_t* line_offsets, const int32_t* status,
                               const int64_t* doc_offsets, int64_t n, int64_t n_docs, int64_t n_lines, double* known, int mem,
                               void* stream) {
    if (n < 0 || n_lines < 0) return fail(RL_ERR_INVALID, "rl_markdown_sentence_known: n and n_lines must be >= 0");
    RL_TRY(check_mem(mem, "rl_markdown_sentence_known"));
    if (n == 0) return RL_OK;
    if (n_docs < 1) return fail(RL_ERR_INVALID, "rl_markdown_sentence_known: n_docs must be >= 1");
    if (!heading_end || !line_start || !line_offsets || !status || !doc_offsets || !known)
        return fail(RL_ERR_INVALID, "rl_markdown_sentence_known: null argument");
    RL_TRY(check_doc_offsets("rl_markdown_sentence_known", doc_offsets, n, n_docs, mem, 0));
    RL_TRY(check_line_offsets("rl_markdown_sentence_known", line_offsets, n_docs, n_lines, mem));
    hipStream_t s = as_stream(stream);
    Staging st(mem, s);
    const int32_t* d_end; const int64_t* d_start; const int64_t* d_loff; const int32_t* d_status; const int64_t* d_off; double* d_known;
    RL_TRY(st.in(heading_end, (size_t)n_lines, &d_end));
    RL_TRY(st.in(line_start, (size_t)n_lines, &d_start));
    RL_TRY(st.in(line_offsets, (size_t)n_docs + 1, &d_loff));
    RL_TRY(st.in(status, (size_t)n_docs, &d_status));
    RL_TRY(st.in(doc_offsets, (size_t)n_docs + 1, &d_off));
    RL_TRY(st.out(known, (size_t)n, &d_known));
    void* d_scr;
    RL_TRY(st.temp(markdown_known_scratch_bytes(n_lines), &d_scr));
    RL_TRY(launch_markdown_sentence_known(d_end, d_start, d_loff, d_status, d_off, n, n_docs, n_lines, d_known, d_scr, s));
    return st.finish();
}

int rl_markdown_chunklet_boundary(const uint8_t* first_open, const int64_t* line_start, const int64_t* line_offsets, const int32_t* status,
                                  const int64_t* sentence_offsets, const int64_t* doc_offsets, int64_t n_sentences, int64_t n_docs,
                                  int64_t n_lines, double* boundary, int mem, void* stream) {
    if (n_sentences < 0 || n_lines < 0) return fail(RL_ERR_INVALID, "rl_markdown_chunklet_boundary: n_sentences and n_lines must be >= 0");
    RL_TRY(check_mem(mem, "rl_markdown_chunklet_boundary"));
    if (n_sentences == 0) return RL_OK;
    if (n_docs < 1) return fail(RL_ERR_INVALID, "rl_markdown_chunklet_boundary: n_docs must be >= 1");
    if (!first_open || !line_start || !line_offsets || !status || !sentence_offsets || !doc_offsets || !boundary)
        return fail(RL_ERR_INVALID, "rl_markdown_chunklet_boundary: null argument");
    RL_TRY(check_doc_offsets("rl_markdown_chunklet_boundary", doc_offsets, n_sentences, n_docs, mem, 0));
    RL_TRY(check_line_offsets("rl_markdown_chunklet_boundary", line_offsets, n_docs, n_lines, mem));
    if (mem == RL_MEM_HOST) {
        if (sentence_offsets[0] < 0) return fail(RL_ERR_INVALID, "rl_markdown_chunklet_boundary: sentence_offsets must be >= 0");
        for (int64_t i = 0; i < n_sentences; ++i)
            if (sentence_offsets[i + 1] < sentence_offsets[i])
                return fail(RL_ERR_INVALID, "rl_markdown_chunklet_boundary: sentence_offsets must be ascending");
    }
    hipStream_t s = as_stream(stream);
    Staging st(mem, s);
    const uint8_t* d_first; const int64_t* d_start; const int64_t* d_loff; const int32_t* d_status; const int64_t* d_soff; const int64_t* d_off;
    double* d_out;
    RL_TRY(st.in(first_open, (size_t)n_lines, &d_first));
    RL_TRY(st.in(line_start, (size_t)n_lines, &d_start));
    RL_TRY(st.in(line_offsets, (size_t)n_docs + 1, &d_loff));
    RL_TRY(st.in(status, (size_t)n_docs, &d_status));
    RL_TRY(st.in(sentence_offsets, (size_t)n_sentences + 1, &d_soff));
    RL_TRY(st.in(doc_offsets, (size_t)n_docs + 1, &d_off));
    RL_TRY(st.out(boundary, (size_t)n_sentences, &d_out));
    void* d_scr;
    RL_TRY(st.temp(markdown_boundary_scratch_bytes(n_sentences), &d_scr));
    RL_TRY(launch_markdown_chunklet_boundary(d_first, d_start, d_loff, d_status, d_soff, d_off, n_sentences, n_docs, n_lines, d_out, d_scr, s));
    return st.finish();
}

}  // extern "C"

// ---- WordPiece on the device: texts -> token ids -> [CLS] q [SEP] d [SEP] rows (kernels in wordpiece.hip) ---------------
struct rl_wordpiece {
    std::mutex mu;
    int hash_bits = 0;
    int64_t n_table = 0, n_pieces = 0, n_slots = 0, table_bytes = 0;
    int32_t max_piece = 0, unk_id = 0, max_word_chars = 0;
    rl::DevArray<uint64_t> image;      // [n_table]
    rl::DevArray<uint8_t> cls;         // [n_table]
    rl::DevArray<uint32_t> piece_cp;   // the kept pieces' code points, back to back
    rl::DevArray<int32_t> piece_off;   // [n_pieces + 1]
    rl::DevArray<uint8_t> piece_flags; // [n_pieces]
    rl::DevArray<int32_t> piece_ids;   // [n_pieces]
    rl::DevArray<int32_t> slots;       // [n_slots]
    // what the last rl_wordpiece_encode left (nothing until then)
    bool encoded = false;
    int64_t n_texts = 0, n_tokens = 0;
    // device arrays of a call, kept between calls with amortised capacity
    rl::Pool count, scan_scratch, sym, kind, start, head, ftext_off, word_pos, tmp, tok_count, ids, offsets, status, counters;
    rl::LastStream last_stream;
    rl::WpTable table() const { return {piece_cp, piece_off, piece_flags, slots, n_slots, hash_bits}; }
};

namespace {

constexpr int64_t WP_MAX_CODEPOINTS = int64_t(1) << 28;  // per call: the expansion's scan keeps two fields in one int64 (wordpiece.hip)

// the exclusive scan of data [n] in place and its total, copied to *total_host (valid after the next synchronisation of `s`)
int wp_scan(rl::Pool& scratch, int64_t* data, int64_t n, int64_t* total_host, hipStream_t s, const char* who) {
    RL_TRY(reserve_amortised(scratch, kb_scan_scratch_items(n) * sizeof(int64_t), who));
    const int64_t* total = nullptr;
    RL_TRY(launch_kb_exclusive_scan(data, n, scratch.as<int64_t>(), &total, s));
    RL_TRY(hip_status(hipMemcpyAsync(total_host, total, sizeof(int64_t), hipMemcpyDeviceToHost, s), who));
    return RL_OK;
}

int check_text_off(const std::string& who, const char* name, const int64_t* off, int64_t n_texts, int64_t n, bool ends_at_n) {
    if (off[0] != 0) return fail(RL_ERR_INVALID, who + ": " + name + " must start at 0");
    for (int64_t t = 0; t < n_texts; ++t)
        if (off[t + 1] < off[t]) return fail(RL_ERR_INVALID, who + ": " + name + " must be ascending");
    if (ends_at_n && off[n_texts] != n) return fail(RL_ERR_INVALID, who + ": " + name + " must end at n");
    return RL_OK;
}

template <class T>
int wp_upload(rl::DevArray<T>& dst, const T* src, size_t count, const char* who) {
    RL_TRY(dst.alloc(std::max<size_t>(count * sizeof(T), 16), who));
    if (count) RL_TRY(hip_status(hipMemcpy(dst.p, src, count * sizeof(T), hipMemcpyHostToDevice), who));
    return RL_OK;
}

}  // namespace

extern "C" {

int rl_wordpiece_create(rl_wordpiece** out, const uint64_t* image, const uint8_t* cls, int64_t n_table, const uint32_t* piece_cp,
                        const int64_t* piece_off, const uint8_t* piece_flags, const int32_t* piece_ids, int64_t n_pieces, int32_t unk_id,
                        int32_t max_word_chars, int32_t hash_bits) {
    const std::string who = "rl_wordpiece_create";
    if (!out) return fail(RL_ERR_INVALID, who + ": out is null");
    *out = nullptr;
    if (!image) return fail(RL_ERR_INVALID, who + ": image is null");
    if (!cls) return fail(RL_ERR_INVALID, who + ": cls is null");
    if (n_table < 1 || n_table > 0x110000) return fail(RL_ERR_INVALID, who + ": n_table must be in [1, 0x110000]");
    if (n_pieces < 0 || n_pieces >= (int64_t(1) << 31)) return fail(RL_ERR_INVALID, who + ": n_pieces must be in [0, 2^31)");
    if (!piece_off) return fail(RL_ERR_INVALID, who + ": piece_off is null");
    if (n_pieces > 0 && (!piece_cp || !piece_flags || !piece_ids)) return fail(RL_ERR_INVALID, who + ": piece_cp, piece_flags or piece_ids is null");
    if (unk_id < 0) return fail(RL_ERR_INVALID, who + ": unk_id must be >= 0");
    if (max_word_chars < 1) return fail(RL_ERR_INVALID, who + ": max_word_chars must be >= 1");
    if (max_word_chars > WP_MAX_WORD_CHARS) return fail(RL_ERR_UNSUPPORTED, who + ": max_word_chars must be <= 200");
    if (hash_bits < 0 || hash_bits > 64) return fail(RL_ERR_INVALID, who + ": hash_bits must be 0 .. 64");
    if (piece_off[0] != 0) return fail(RL_ERR_INVALID, who + ": piece_off must start at 0");
    for (int64_t i = 0; i < n_pieces; ++i) {
        if (piece_off[i + 1] < piece_off[i]) return fail(RL_ERR_INVALID, who + ": piece_off must be ascending");
        if (piece_ids[i] < 0) return fail(RL_ERR_INVALID, who + ": piece_ids must be >= 0");
    }
    if (piece_off[n_pieces] >= (int64_t(1) << 31)) return fail(RL_ERR_UNSUPPORTED, who + ": the pieces must hold fewer than 2^31 code points");
    for (int64_t i = 0; i < n_table; ++i) {  // every field a code point + 1, no symbol behind an empty field, nothing above the fields
        uint64_t e = image[i];
        bool ended = false;
        for (int j = 0; j < WP_IMAGE_MAX; ++j, e >>= 21) {
            const uint64_t f = e & 0x1FFFFFull;
            if (f > 0x110000ull || (ended && f)) return fail(RL_ERR_INVALID, who + ": malformed image entry");
            ended |= f == 0;
        }
        if (e) return fail(RL_ERR_INVALID, who + ": malformed image entry");
        if ((cls[i] & ~7u) || (cls[i] & 3u) == 3u) return fail(RL_ERR_INVALID, who + ": malformed cls entry");
    }
    // the pieces a word can match: 1 .. max_word_chars code points (a longer word is unk_id before any lookup)
    std::vector<uint32_t> h_cp;
    std::vector<int32_t> h_off{0}, h_ids;
    std::vector<uint8_t> h_flags;
    int32_t longest = 0;
    for (int64_t i = 0; i < n_pieces; ++i) {
        const int64_t b = piece_off[i], len = piece_off[i + 1] - b;
        if (len < 1 || len > max_word_chars) continue;
        h_cp.insert(h_cp.end(), piece_cp + b, piece_cp + b + len);
        h_off.push_back((int32_t)h_cp.size());
        h_ids.push_back(piece_ids[i]);
        h_flags.push_back(piece_flags[i] & 1u);
        longest = std::max(longest, (int32_t)len);
    }
    const int64_t kept = (int64_t)h_ids.size(), n_slots = wp_table_slots(kept);
    std::vector<int32_t> h_slots((size_t)n_slots, WP_EMPTY);
    const WpTable host{h_cp.data(), h_off.data(), h_flags.data(), h_slots.data(), n_slots, hash_bits == 64 ? 0 : hash_bits};
    for (int64_t i = 0; i < kept; ++i) (void)wp_table_insert(host, h_slots.data(), (int32_t)i);  // (of equal pieces the first stays)
    std::unique_ptr<rl_wordpiece> t(new rl_wordpiece());
    t->hash_bits = host.hash_bits;
    t->n_table = n_table; t->n_pieces = kept; t->n_slots = n_slots;
    t->max_piece = longest; t->unk_id = unk_id; t->max_word_chars = max_word_chars;
    const char* w = "rl_wordpiece_create";
    RL_TRY(wp_upload(t->image, image, (size_t)n_table, w));
    RL_TRY(wp_upload(t->cls, cls, (size_t)n_table, w));
    RL_TRY(wp_upload(t->piece_cp, const_cast<const uint32_t*>(h_cp.data()), h_cp.size(), w));
    RL_TRY(wp_upload(t->piece_off, const_cast<const int32_t*>(h_off.data()), h_off.size(), w));
    RL_TRY(wp_upload(t->piece_flags, const_cast<const uint8_t*>(h_flags.data()), h_flags.size(), w));
    RL_TRY(wp_upload(t->piece_ids, const_cast<const int32_t*>(h_ids.data()), h_ids.size(), w));
    RL_TRY(wp_upload(t->slots, const_cast<const int32_t*>(h_slots.data()), h_slots.size(), w));
    t->table_bytes = (int64_t)(t->image.cap + t->cls.cap + t->piece_cp.cap + t->piece_off.cap + t->piece_flags.cap + t->piece_ids.cap + t->slots.cap);
    *out = t.release();
    return RL_OK;
}

int rl_wordpiece_destroy(rl_wordpiece* tok) {
    delete tok;
    return RL_OK;
}

int rl_wordpiece_info(rl_wordpiece* tok, int64_t out[4]) {
    if (!tok) return fail(RL_ERR_INVALID, "rl_wordpiece_info: null handle");
    if (!out) return fail(RL_ERR_INVALID, "rl_wordpiece_info: out is null");
    std::lock_guard<std::mutex> lock(tok->mu);
    int64_t bytes = tok->table_bytes;
    for (const rl::Pool* p : {&tok->count, &tok->scan_scratch, &tok->sym, &tok->kind, &tok->start, &tok->head, &tok->ftext_off, &tok->word_pos, &tok->tmp,
                              &tok->tok_count, &tok->ids, &tok->offsets, &tok->status, &tok->counters})
        bytes += (int64_t)p->cap;
    out[0] = tok->n_pieces;
    out[1] = tok->max_piece;
    out[2] = tok->n_slots;
    out[3] = bytes;
    return RL_OK;
}

int rl_wordpiece_encode(rl_wordpiece* tok, const uint32_t* codepoints, const int64_t* text_off, int64_t n, int64_t n_texts, int64_t out_counts[5],
                        int mem, void* stream) {
    const char* who = "rl_wordpiece_encode";
    const std::string w(who);
    if (!tok) return fail(RL_ERR_INVALID, w + ": null handle");
    if (n < 0 || n_texts < 0) return fail(RL_ERR_INVALID, w + ": negative size");
    RL_TRY(check_mem(mem, who));
    if (!text_off) return fail(RL_ERR_INVALID, w + ": text_off is null");
    if (!out_counts) return fail(RL_ERR_INVALID, w + ": out_counts is null");
    if (n > 0 && !codepoints) return fail(RL_ERR_INVALID, w + ": codepoints is null");
    if (n > 0 && n_texts < 1) return fail(RL_ERR_INVALID, w + ": code points without a text");
    if (n >= WP_MAX_CODEPOINTS) return fail(RL_ERR_UNSUPPORTED, w + ": n must be < 2^28 code points in one call");
    if (mem == RL_MEM_HOST) RL_TRY(check_text_off(w, "text_off", text_off, n_texts, n, true));
    hipStream_t s = as_stream(stream);
    std::lock_guard<std::mutex> lock(tok->mu);
    RL_TRY(tok->last_stream.use(s));
    tok->encoded = false;
    Staging st(mem, s);
    const uint32_t* d_cp;
    const int64_t* d_off;
    RL_TRY(st.in(codepoints, (size_t)n, &d_cp));
    RL_TRY(st.in(text_off, (size_t)n_texts + 1, &d_off));
    // 1. expand
    RL_TRY(reserve_amortised(tok->count, (size_t)(n + 1) * sizeof(int64_t), who));
    RL_TRY(reserve_amortised(tok->counters, 2 * sizeof(unsigned long long), who));
    unsigned long long* counters = tok->counters.as<unsigned long long>();
    RL_TRY(hip_status(hipMemsetAsync(counters, 0, 2 * sizeof(unsigned long long), s), who));
    int64_t* scan = tok->count.as<int64_t>();
    RL_TRY(launch_wp_expand_count(d_cp, n, tok->image, tok->cls, tok->n_table, scan, s));
    int64_t packed = 0, n_words = 0, n_tokens = 0;
    RL_TRY(wp_scan(tok->scan_scratch, scan, n + 1, &packed, s, who));
    RL_TRY(hip_status(hipStreamSynchronize(s), who));
    const int64_t m = packed & ((int64_t(1) << 32) - 1);
    const size_t m_items = std::max<size_t>((size_t)m, 16);
    RL_TRY(reserve_amortised(tok->sym, m_items * sizeof(uint32_t), who));
    RL_TRY(reserve_amortised(tok->kind, m_items, who));
    RL_TRY(reserve_amortised(tok->start, m_items, who));
    RL_TRY(reserve_amortised(tok->tmp, m_items * sizeof(int32_t), who));
    RL_TRY(reserve_amortised(tok->ids, m_items * sizeof(int32_t), who));  // (a word has at most as many pieces as symbols)
    RL_TRY(reserve_amortised(tok->head, (size_t)(m + 1) * sizeof(int64_t), who));
    RL_TRY(reserve_amortised(tok->ftext_off, (size_t)(n_texts + 1) * sizeof(int64_t), who));
    RL_TRY(reserve_amortised(tok->offsets, (size_t)(n_texts + 1) * sizeof(int64_t), who));
    RL_TRY(reserve_amortised(tok->status, std::max<size_t>((size_t)n_texts, 16), who));
    RL_TRY(hip_status(hipMemsetAsync(tok->start.p, 0, m_items, s), who));
    RL_TRY(launch_wp_expand_write(d_cp, n, tok->image, tok->cls, tok->n_table, scan, m, tok->sym.as<uint32_t>(), tok->kind.as<uint8_t>(), s));
    RL_TRY(launch_wp_texts(d_off, n_texts, n, scan, m, tok->ftext_off.as<int64_t>(), tok->start.as<uint8_t>(), tok->status.as<uint8_t>(), counters, s));
    // 2. words
    RL_TRY(launch_wp_heads(tok->kind.as<uint8_t>(), tok->start.as<uint8_t>(), m, tok->head.as<int64_t>(), s));
    RL_TRY(wp_scan(tok->scan_scratch, tok->head.as<int64_t>(), m + 1, &n_words, s, who));
    RL_TRY(hip_status(hipStreamSynchronize(s), who));
    // 3. match, 4. emit
    RL_TRY(reserve_amortised(tok->word_pos, std::max<size_t>((size_t)n_words, 2) * sizeof(int64_t), who));
    RL_TRY(reserve_amortised(tok->tok_count, (size_t)(n_words + 1) * sizeof(int64_t), who));
    RL_TRY(launch_wp_match(tok->sym.as<uint32_t>(), tok->kind.as<uint8_t>(), tok->start.as<uint8_t>(), tok->head.as<int64_t>(), m, n_words, tok->table(),
                           tok->piece_ids, tok->max_piece, tok->unk_id, tok->max_word_chars, tok->word_pos.as<int64_t>(), tok->tmp.as<int32_t>(),
                           tok->tok_count.as<int64_t>(), counters, s));
    RL_TRY(wp_scan(tok->scan_scratch, tok->tok_count.as<int64_t>(), n_words + 1, &n_tokens, s, who));
    RL_TRY(launch_wp_emit(tok->word_pos.as<int64_t>(), tok->tok_count.as<int64_t>(), n_words, tok->tmp.as<int32_t>(), m, m, tok->ids.as<int32_t>(), s));
    RL_TRY(launch_wp_offsets(tok->ftext_off.as<int64_t>(), n_texts, tok->head.as<int64_t>(), m, tok->tok_count.as<int64_t>(), n_words,
                             tok->offsets.as<int64_t>(), s));
    unsigned long long h_counters[2] = {0, 0};
    RL_TRY(hip_status(hipMemcpyAsync(h_counters, counters, sizeof(h_counters), hipMemcpyDeviceToHost, s), who));
    RL_TRY(hip_status(hipStreamSynchronize(s), who));
    st.drain();  // (the stream has been synchronised above)
    tok->n_texts = n_texts;
    tok->n_tokens = n_tokens;
    tok->encoded = true;
    out_counts[0] = n_tokens;
    out_counts[1] = n_words;
    out_counts[2] = (int64_t)h_counters[WP_COUNT_UNK];
    out_counts[3] = (int64_t)h_counters[WP_COUNT_FLAGGED];
    out_counts[4] = m;
    return RL_OK;
}

int rl_wordpiece_result(rl_wordpiece* tok, int32_t* ids, int64_t* offsets, uint8_t* status, int mem, void* stream) {
    const char* who = "rl_wordpiece_result";
    if (!tok) return fail(RL_ERR_INVALID, std::string(who) + ": null handle");
    RL_TRY(check_mem(mem, who));
    hipStream_t s = as_stream(stream);
    std::lock_guard<std::mutex> lock(tok->mu);
    if (!tok->encoded) return fail(RL_ERR_INVALID, std::string(who) + ": no rl_wordpiece_encode before it");
    RL_TRY(tok->last_stream.use(s));
    const hipMemcpyKind kind = mem == RL_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (ids && tok->n_tokens) RL_TRY(hip_status(hipMemcpyAsync(ids, tok->ids.p, (size_t)tok->n_tokens * sizeof(int32_t), kind, s), who));
    if (offsets) RL_TRY(hip_status(hipMemcpyAsync(offsets, tok->offsets.p, (size_t)(tok->n_texts + 1) * sizeof(int64_t), kind, s), who));
    if (status && tok->n_texts) RL_TRY(hip_status(hipMemcpyAsync(status, tok->status.p, (size_t)tok->n_texts, kind, s), who));
    RL_TRY(hip_status(hipStreamSynchronize(s), who));
    return RL_OK;
}

int rl_wordpiece_device(rl_wordpiece* tok, const int32_t** ids, const int64_t** offsets, const uint8_t** status) {
    const char* who = "rl_wordpiece_device";
    if (!tok) return fail(RL_ERR_INVALID, std::string(who) + ": null handle");
    std::lock_guard<std::mutex> lock(tok->mu);
    if (!tok->encoded) return fail(RL_ERR_INVALID, std::string(who) + ": no rl_wordpiece_encode before it");
    if (ids) *ids = tok->ids.as<int32_t>();
    if (offsets) *offsets = tok->offsets.as<int64_t>();
    if (status) *status = tok->status.as<uint8_t>();
    return RL_OK;
}

int rl_wordpiece_pairs(const int32_t* ids, const int64_t* tok_off, int64_t n_texts, const int32_t* query_text, const int32_t* doc_text, int64_t n_pairs,
                       int32_t max_length, int32_t cls_id, int32_t sep_id, int32_t position_offset, int32_t* out_ids, int32_t* out_positions,
                       int32_t* out_type_ids, int32_t* out_seq_offsets, int64_t* out_total, int mem, void* stream) {
    const char* who = "rl_wordpiece_pairs";
    const std::string w(who);
    RL_TRY(check_mem(mem, who));
    if (n_texts < 0 || n_pairs < 0) return fail(RL_ERR_INVALID, w + ": negative size");
    if (n_pairs >= (int64_t(1) << 31) / 3) return fail(RL_ERR_UNSUPPORTED, w + ": one call takes fewer than 2^31 tokens");
    if (max_length < 3) return fail(RL_ERR_INVALID, w + ": max_length must be >= 3");
    if (!tok_off) return fail(RL_ERR_INVALID, w + ": tok_off is null");
    if (!out_seq_offsets) return fail(RL_ERR_INVALID, w + ": out_seq_offsets is null");
    if (!out_total) return fail(RL_ERR_INVALID, w + ": out_total is null");
    if (n_pairs > 0 && !query_text) return fail(RL_ERR_INVALID, w + ": query_text is null");
    if (n_pairs > 0 && !doc_text) return fail(RL_ERR_INVALID, w + ": doc_text is null");
    const int given = (out_ids != nullptr) + (out_positions != nullptr) + (out_type_ids != nullptr);
    if (given != 0 && given != 3) return fail(RL_ERR_INVALID, w + ": give out_ids, out_positions and out_type_ids, or none of them for the sizes alone");
    if (given && n_pairs > 0 && !ids) return fail(RL_ERR_INVALID, w + ": ids is null");
    int64_t n_tokens = 0;
    if (mem == RL_MEM_HOST) {
        RL_TRY(check_text_off(w, "tok_off", tok_off, n_texts, 0, false));
        n_tokens = tok_off[n_texts];
        for (int64_t p = 0; p < n_pairs; ++p) {
            if (query_text[p] < 0 || query_text[p] >= n_texts) return fail(RL_ERR_INVALID, w + ": query_text holds an index outside [0, n_texts)");
            if (doc_text[p] < 0 || doc_text[p] >= n_texts) return fail(RL_ERR_INVALID, w + ": doc_text holds an index outside [0, n_texts)");
        }
    }
    hipStream_t s = as_stream(stream);
    Staging st(mem, s);
    const int64_t* d_off; const int32_t* d_q; const int32_t* d_d; const int32_t* d_ids = ids;
    RL_TRY(st.in(tok_off, (size_t)n_texts + 1, &d_off));
    RL_TRY(st.in(query_text, (size_t)n_pairs, &d_q));
    RL_TRY(st.in(doc_text, (size_t)n_pairs, &d_d));
    if (given && n_pairs > 0) RL_TRY(st.in(ids, (size_t)n_tokens, &d_ids));
    int64_t* d_len; int64_t* d_scr;
    RL_TRY(st.temp((size_t)(n_pairs + 1) * sizeof(int64_t), &d_len));
    RL_TRY(st.temp(kb_scan_scratch_items(n_pairs + 1) * sizeof(int64_t), &d_scr));
    RL_TRY(launch_wp_pair_lengths(d_off, n_texts, d_q, d_d, n_pairs, max_length, d_len, s));
    const int64_t* d_total = nullptr;
    RL_TRY(launch_kb_exclusive_scan(d_len, n_pairs + 1, d_scr, &d_total, s));
    int64_t total = 0;
    RL_TRY(hip_status(hipMemcpyAsync(&total, d_total, sizeof(int64_t), hipMemcpyDeviceToHost, s), who));
    RL_TRY(hip_status(hipStreamSynchronize(s), who));
    if (total >= (int64_t(1) << 31)) return fail(RL_ERR_UNSUPPORTED, w + ": one call takes fewer than 2^31 tokens");
    *out_total = total;
    int32_t* d_so;
    RL_TRY(st.out(out_seq_offsets, (size_t)n_pairs + 1, &d_so));
    RL_TRY(launch_wp_pair_offsets(d_len, n_pairs, d_so, s));
    if (given) {
        int32_t *d_oi, *d_op, *d_ot;
        RL_TRY(st.out(out_ids, (size_t)total, &d_oi));
        RL_TRY(st.out(out_positions, (size_t)total, &d_op));
        RL_TRY(st.out(out_type_ids, (size_t)total, &d_ot));
        RL_TRY(launch_wp_pair_write(d_ids, d_off, n_texts, d_q, d_d, n_pairs, max_length, cls_id, sep_id, position_offset, d_len, total, d_oi, d_op, d_ot, s));
    }
    return st.finish();
}

}  // extern "C"

// ---- SentencePiece Unigram on the device: texts -> token ids -> bos ids eos rows (kernels in sentencepiece.hip) ----------
namespace {

constexpr int64_t SP_MAX_SYMBOLS = int64_t(1) << 31;     // per call: back-pointers and row offsets are int32
constexpr int64_t SP_MAX_CODEPOINTS = int64_t(1) << 25;  // per call: times SP_MAX_IMAGE symbols each, the expansion's scan keeps its low field
static_assert(SP_MAX_CODEPOINTS * rl::SP_MAX_IMAGE < (int64_t(1) << 32), "the symbol count of a call fits the scan's low field");

const rl::Pool* const* sp_pools(const rl_sentencepiece* t, size_t* n) {
    static thread_local const rl::Pool* pools[16];
    const rl::Pool* all[] = {&t->count, &t->scan_scratch, &t->raw, &t->start, &t->rtext_off, &t->keep, &t->sym, &t->sym_off,
                             &t->bp_start, &t->bp_id, &t->tmp, &t->tok_count, &t->ids, &t->offsets, &t->status, &t->counters};
    *n = sizeof(all) / sizeof(all[0]);
    for (size_t i = 0; i < *n; ++i) pools[i] = all[i];
    return pools;
}

}  // namespace

extern "C" {

int rl_sentencepiece_create(rl_sentencepiece** out, const int32_t* image_off, const uint8_t* image_len, int64_t n_table, const uint32_t* image_pool,
                            int64_t n_pool, const uint32_t* piece_cp, const int64_t* piece_off, const int32_t* piece_ids, const float* piece_scores,
                            int64_t n_pieces, int32_t unk_id, float unk_score, int32_t hash_bits) {
    const std::string who = "rl_sentencepiece_create";
    if (!out) return fail(RL_ERR_INVALID, who + ": out is null");
    *out = nullptr;
    if (!image_off) return fail(RL_ERR_INVALID, who + ": image_off is null");
    if (!image_len) return fail(RL_ERR_INVALID, who + ": image_len is null");
    if (n_table < 1 || n_table > 0x110000) return fail(RL_ERR_INVALID, who + ": n_table must be in [1, 0x110000]");
    if (n_pool < 0 || n_pool >= (int64_t(1) << 31)) return fail(RL_ERR_INVALID, who + ": n_pool must be in [0, 2^31)");
    if (n_pool > 0 && !image_pool) return fail(RL_ERR_INVALID, who + ": image_pool is null");
    if (n_pieces < 0 || n_pieces >= (int64_t(1) << 31)) return fail(RL_ERR_INVALID, who + ": n_pieces must be in [0, 2^31)");
    if (!piece_off) return fail(RL_ERR_INVALID, who + ": piece_off is null");
    if (n_pieces > 0 && (!piece_cp || !piece_ids || !piece_scores)) return fail(RL_ERR_INVALID, who + ": piece_cp, piece_ids or piece_scores is null");
    if (unk_id < 0) return fail(RL_ERR_INVALID, who + ": unk_id must be >= 0");
    if (!std::isfinite(unk_score)) return fail(RL_ERR_INVALID, who + ": unk_score must be finite");
    if (hash_bits < 0 || hash_bits > 64) return fail(RL_ERR_INVALID, who + ": hash_bits must be 0 .. 64");
    if (piece_off[0] != 0) return fail(RL_ERR_INVALID, who + ": piece_off must start at 0");
    for (int64_t i = 0; i < n_pieces; ++i) {
        if (piece_off[i + 1] < piece_off[i]) return fail(RL_ERR_INVALID, who + ": piece_off must be ascending");
        if (piece_off[i + 1] - piece_off[i] > SP_MAX_PIECE) return fail(RL_ERR_UNSUPPORTED, who + ": a piece must have at most 64 code points");
        if (piece_ids[i] < 0) return fail(RL_ERR_INVALID, who + ": piece_ids must be >= 0");
        if (!std::isfinite(piece_scores[i])) return fail(RL_ERR_INVALID, who + ": piece_scores must be finite");
    }
    if (piece_off[n_pieces] >= (int64_t(1) << 31)) return fail(RL_ERR_UNSUPPORTED, who + ": the pieces must hold fewer than 2^31 code points");
    for (int64_t i = 0; i < n_table; ++i) {  // an image lies inside the pool and holds code points
        if (image_off[i] < 0) continue;
        const int64_t len = image_len[i] & 0x7F;
        if ((int64_t)image_off[i] + len > n_pool) return fail(RL_ERR_INVALID, who + ": malformed image entry");
    }
    for (int64_t i = 0; i < n_pool; ++i)
        if (image_pool[i] >= 0x110000u) return fail(RL_ERR_INVALID, who + ": malformed image_pool entry");
    // the pieces a span can match: at least one code point
    std::vector<uint32_t> h_cp;
    std::vector<int32_t> h_off{0}, h_ids;
    std::vector<float> h_scores;
    int32_t longest = 0;
    for (int64_t i = 0; i < n_pieces; ++i) {
        const int64_t b = piece_off[i], len = piece_off[i + 1] - b;
        if (len < 1) continue;
        h_cp.insert(h_cp.end(), piece_cp + b, piece_cp + b + len);
        h_off.push_back((int32_t)h_cp.size());
        h_ids.push_back(piece_ids[i]);
        h_scores.push_back(piece_scores[i]);
        longest = std::max(longest, (int32_t)len);
    }
    const int64_t kept = (int64_t)h_ids.size(), n_slots = wp_table_slots(kept);
    std::vector<uint8_t> h_flags((size_t)kept, 0);
    std::vector<int32_t> h_slots((size_t)n_slots, WP_EMPTY);
    const WpTable host{h_cp.data(), h_off.data(), h_flags.data(), h_slots.data(), n_slots, hash_bits == 64 ? 0 : hash_bits};
    for (int64_t i = 0; i < kept; ++i) (void)wp_table_insert(host, h_slots.data(), (int32_t)i);  // (of equal pieces the first stays)
    std::unique_ptr<rl_sentencepiece> t(new rl_sentencepiece());
    t->hash_bits = host.hash_bits;
    t->n_table = n_table; t->n_pool = n_pool; t->n_pieces = kept; t->n_slots = n_slots;
    t->longest = std::max(longest, 1); t->unk_id = unk_id; t->unk_score = unk_score;
    const char* w = "rl_sentencepiece_create";
    RL_TRY(wp_upload(t->image_off, image_off, (size_t)n_table, w));
    RL_TRY(wp_upload(t->image_len, image_len, (size_t)n_table, w));
    RL_TRY(wp_upload(t->image_pool, image_pool, (size_t)n_pool, w));
    RL_TRY(wp_upload(t->piece_cp, const_cast<const uint32_t*>(h_cp.data()), h_cp.size(), w));
    RL_TRY(wp_upload(t->piece_off, const_cast<const int32_t*>(h_off.data()), h_off.size(), w));
    RL_TRY(wp_upload(t->piece_flags, const_cast<const uint8_t*>(h_flags.data()), h_flags.size(), w));
    RL_TRY(wp_upload(t->piece_ids, const_cast<const int32_t*>(h_ids.data()), h_ids.size(), w));
    RL_TRY(wp_upload(t->piece_scores, const_cast<const float*>(h_scores.data()), h_scores.size(), w));
    RL_TRY(wp_upload(t->slots, const_cast<const int32_t*>(h_slots.data()), h_slots.size(), w));
    t->table_bytes = (int64_t)(t->image_off.cap + t->image_len.cap + t->image_pool.cap + t->piece_cp.cap + t->piece_off.cap + t->piece_flags.cap +
                               t->piece_ids.cap + t->piece_scores.cap + t->slots.cap);
    *out = t.release();
    return RL_OK;
}

int rl_sentencepiece_destroy(rl_sentencepiece* tok) {
    delete tok;
    return RL_OK;
}

int rl_sentencepiece_info(rl_sentencepiece* tok, int64_t out[4]) {
    if (!tok) return fail(RL_ERR_INVALID, "rl_sentencepiece_info: null handle");
    if (!out) return fail(RL_ERR_INVALID, "rl_sentencepiece_info: out is null");
    std::lock_guard<std::mutex> lock(tok->mu);
    int64_t bytes = tok->table_bytes;
    size_t n_pools = 0;
    const rl::Pool* const* pools = sp_pools(tok, &n_pools);
    for (size_t i = 0; i < n_pools; ++i) bytes += (int64_t)pools[i]->cap;
    out[0] = tok->n_pieces;
    out[1] = tok->longest;
    out[2] = tok->n_slots;
    out[3] = bytes;
    return RL_OK;
}

int rl_sentencepiece_encode(rl_sentencepiece* tok, const uint32_t* codepoints, const int64_t* text_off, int64_t n, int64_t n_texts, int32_t raw_ids,
                            int64_t out_counts[5], int mem, void* stream) {
    const char* who = "rl_sentencepiece_encode";
    const std::string w(who);
    if (!tok) return fail(RL_ERR_INVALID, w + ": null handle");
    if (n < 0 || n_texts < 0) return fail(RL_ERR_INVALID, w + ": negative size");
    RL_TRY(check_mem(mem, who));
    if (raw_ids != 0 && raw_ids != 1) return fail(RL_ERR_INVALID, w + ": raw_ids must be 0 or 1");
    if (!text_off) return fail(RL_ERR_INVALID, w + ": text_off is null");
    if (!out_counts) return fail(RL_ERR_INVALID, w + ": out_counts is null");
    if (n > 0 && !codepoints) return fail(RL_ERR_INVALID, w + ": codepoints is null");
    if (n > 0 && n_texts < 1) return fail(RL_ERR_INVALID, w + ": code points without a text");
    if (n >= SP_MAX_CODEPOINTS) return fail(RL_ERR_UNSUPPORTED, w + ": n must be < 2^25 code points in one call");
    if (n_texts >= (int64_t(1) << 31) - 1) return fail(RL_ERR_UNSUPPORTED, w + ": n_texts must be < 2^31 - 1 in one call");
    if (mem == RL_MEM_HOST) RL_TRY(check_text_off(w, "text_off", text_off, n_texts, n, true));
    hipStream_t s = as_stream(stream);
    std::lock_guard<std::mutex> lock(tok->mu);
    RL_TRY(tok->last_stream.use(s));
    tok->encoded = false;
    Staging st(mem, s);
    const uint32_t* d_cp;
    const int64_t* d_off;
    RL_TRY(st.in(codepoints, (size_t)n, &d_cp));
    RL_TRY(st.in(text_off, (size_t)n_texts + 1, &d_off));
    const rl::SpImage image = tok->image();
    // 1. expand
    RL_TRY(reserve_amortised(tok->count, (size_t)(n + 1) * sizeof(int64_t), who));
    RL_TRY(reserve_amortised(tok->counters, SP_COUNTERS * sizeof(unsigned long long), who));
    unsigned long long* counters = tok->counters.as<unsigned long long>();
    RL_TRY(hip_status(hipMemsetAsync(counters, 0, SP_COUNTERS * sizeof(unsigned long long), s), who));
    int64_t* scan = tok->count.as<int64_t>();
    RL_TRY(launch_sp_expand_count(d_cp, n, image, scan, s));
    int64_t packed = 0, m = 0, n_tokens = 0;
    RL_TRY(wp_scan(tok->scan_scratch, scan, n + 1, &packed, s, who));
    RL_TRY(hip_status(hipStreamSynchronize(s), who));
    const int64_t m0 = packed & ((int64_t(1) << 32) - 1);  // (n < 2^25 code points of at most 127 symbols: the field cannot overflow)
    if (m0 >= SP_MAX_SYMBOLS) return fail(RL_ERR_UNSUPPORTED, w + ": one call takes fewer than 2^31 symbols");
    const size_t m0_items = std::max<size_t>((size_t)m0, 16);
    RL_TRY(reserve_amortised(tok->raw, m0_items * sizeof(uint32_t), who));
    RL_TRY(reserve_amortised(tok->start, m0_items + 1, who));
    RL_TRY(reserve_amortised(tok->keep, (size_t)(m0 + 1) * sizeof(int64_t), who));
    RL_TRY(reserve_amortised(tok->rtext_off, (size_t)(n_texts + 1) * sizeof(int64_t), who));
    RL_TRY(reserve_amortised(tok->sym_off, (size_t)(n_texts + 1) * sizeof(int64_t), who));
    RL_TRY(reserve_amortised(tok->tok_count, (size_t)(n_texts + 1) * sizeof(int64_t), who));
    RL_TRY(reserve_amortised(tok->offsets, (size_t)(n_texts + 1) * sizeof(int64_t), who));
    RL_TRY(reserve_amortised(tok->status, std::max<size_t>((size_t)n_texts, 16), who));
    RL_TRY(hip_status(hipMemsetAsync(tok->start.p, 0, m0_items + 1, s), who));
    RL_TRY(launch_sp_expand_write(d_cp, n, image, scan, m0, tok->raw.as<uint32_t>(), s));
    RL_TRY(launch_sp_texts(d_off, n_texts, n, scan, m0, tok->rtext_off.as<int64_t>(), tok->start.as<uint8_t>(), tok->status.as<uint8_t>(), counters, s));
    // 2. the white-space rule
    RL_TRY(launch_sp_keep_count(tok->raw.as<uint32_t>(), tok->start.as<uint8_t>(), m0, tok->keep.as<int64_t>(), s));
    RL_TRY(wp_scan(tok->scan_scratch, tok->keep.as<int64_t>(), m0 + 1, &m, s, who));
    RL_TRY(hip_status(hipStreamSynchronize(s), who));
    if (m >= SP_MAX_SYMBOLS) return fail(RL_ERR_UNSUPPORTED, w + ": one call takes fewer than 2^31 symbols");
    const size_t m_items = std::max<size_t>((size_t)m, 16);
    RL_TRY(reserve_amortised(tok->sym, m_items * sizeof(uint32_t), who));
    RL_TRY(reserve_amortised(tok->bp_start, m_items * sizeof(int32_t), who));
    RL_TRY(reserve_amortised(tok->bp_id, m_items * sizeof(int32_t), who));
    RL_TRY(reserve_amortised(tok->tmp, m_items * sizeof(int32_t), who));
    RL_TRY(reserve_amortised(tok->ids, m_items * sizeof(int32_t), who));  // (a text has at most as many ids as symbols)
    RL_TRY(launch_sp_keep_write(tok->raw.as<uint32_t>(), tok->start.as<uint8_t>(), m0, tok->keep.as<int64_t>(), m, tok->rtext_off.as<int64_t>(), n_texts,
                                tok->sym.as<uint32_t>(), tok->sym_off.as<int64_t>(), counters, s));
    // 3. search, 4. emit
    RL_TRY(launch_sp_viterbi(tok->sym.as<uint32_t>(), tok->sym_off.as<int64_t>(), n_texts, m, tok->table(), tok->longest, tok->unk_score,
                             tok->bp_start.as<int32_t>(), tok->bp_id.as<int32_t>(), tok->tmp.as<int32_t>(), tok->tok_count.as<int64_t>(), counters, s));
    RL_TRY(wp_scan(tok->scan_scratch, tok->tok_count.as<int64_t>(), n_texts + 1, &n_tokens, s, who));
    RL_TRY(launch_sp_emit(tok->tmp.as<int32_t>(), tok->sym_off.as<int64_t>(), tok->tok_count.as<int64_t>(), n_texts, m, m, raw_ids ? 0 : 1,
                          raw_ids ? tok->unk_id : 3, tok->ids.as<int32_t>(), tok->offsets.as<int64_t>(), s));
    unsigned long long h_counters[SP_COUNTERS] = {0, 0, 0};
    RL_TRY(hip_status(hipMemcpyAsync(h_counters, counters, sizeof(h_counters), hipMemcpyDeviceToHost, s), who));
    RL_TRY(hip_status(hipStreamSynchronize(s), who));
    st.drain();  // (the stream has been synchronised above)
    tok->n_texts = n_texts;
    tok->n_tokens = n_tokens;
    tok->encoded = true;
    out_counts[0] = n_tokens;
    out_counts[1] = m;
    out_counts[2] = (int64_t)h_counters[SP_COUNT_UNK];
    out_counts[3] = (int64_t)h_counters[SP_COUNT_FLAGGED];
    out_counts[4] = (int64_t)h_counters[SP_COUNT_LONGEST];
    return RL_OK;
}

int rl_sentencepiece_result(rl_sentencepiece* tok, int32_t* ids, int64_t* offsets, uint8_t* status, int mem, void* stream) {
    const char* who = "rl_sentencepiece_result";
    if (!tok) return fail(RL_ERR_INVALID, std::string(who) + ": null handle");
    RL_TRY(check_mem(mem, who));
    hipStream_t s = as_stream(stream);
    std::lock_guard<std::mutex> lock(tok->mu);
    if (!tok->encoded) return fail(RL_ERR_INVALID, std::string(who) + ": no rl_sentencepiece_encode before it");
    RL_TRY(tok->last_stream.use(s));
    const hipMemcpyKind kind = mem == RL_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (ids && tok->n_tokens) RL_TRY(hip_status(hipMemcpyAsync(ids, tok->ids.p, (size_t)tok->n_tokens * sizeof(int32_t), kind, s), who));
    if (offsets) RL_TRY(hip_status(hipMemcpyAsync(offsets, tok->offsets.p, (size_t)(tok->n_texts + 1) * sizeof(int64_t), kind, s), who));
    if (status && tok->n_texts) RL_TRY(hip_status(hipMemcpyAsync(status, tok->status.p, (size_t)tok->n_texts, kind, s), who));
    RL_TRY(hip_status(hipStreamSynchronize(s), who));
    return RL_OK;
}

int rl_sentencepiece_device(rl_sentencepiece* tok, const int32_t** ids, const int64_t** offsets, const uint8_t** status, const uint32_t** symbols,
                            const int64_t** symbol_offsets) {
    const char* who = "rl_sentencepiece_device";
    if (!tok) return fail(RL_ERR_INVALID, std::string(who) + ": null handle");
    std::lock_guard<std::mutex> lock(tok->mu);
    if (!tok->encoded) return fail(RL_ERR_INVALID, std::string(who) + ": no rl_sentencepiece_encode before it");
    if (ids) *ids = tok->ids.as<int32_t>();
    if (offsets) *offsets = tok->offsets.as<int64_t>();
    if (status) *status = tok->status.as<uint8_t>();
    if (symbols) *symbols = tok->sym.as<uint32_t>();
    if (symbol_offsets) *symbol_offsets = tok->sym_off.as<int64_t>();
    return RL_OK;
}

int rl_sentencepiece_rows(const int32_t* ids, const int64_t* tok_off, int64_t n_texts, int32_t max_len, int32_t bos_id, int32_t eos_id,
                          int32_t position_offset, int32_t* out_ids, int32_t* out_positions, int32_t* out_seq_offsets, int64_t* out_total, int mem,
                          void* stream) {
    const char* who = "rl_sentencepiece_rows";
    const std::string w(who);
    RL_TRY(check_mem(mem, who));
    if (n_texts < 0) return fail(RL_ERR_INVALID, w + ": negative size");
    if (n_texts >= (int64_t(1) << 31) / 2) return fail(RL_ERR_UNSUPPORTED, w + ": one call takes fewer than 2^31 tokens");
    if (max_len < 2) return fail(RL_ERR_INVALID, w + ": max_len must be >= 2");
    if (!tok_off) return fail(RL_ERR_INVALID, w + ": tok_off is null");
    if (!out_seq_offsets) return fail(RL_ERR_INVALID, w + ": out_seq_offsets is null");
    if (!out_total) return fail(RL_ERR_INVALID, w + ": out_total is null");
    const int given = (out_ids != nullptr) + (out_positions != nullptr);
    if (given == 1) return fail(RL_ERR_INVALID, w + ": give out_ids and out_positions, or neither for the sizes alone");
    if (given && n_texts > 0 && !ids) return fail(RL_ERR_INVALID, w + ": ids is null");
    int64_t n_tokens = 0;
    if (mem == RL_MEM_HOST) {
        RL_TRY(check_text_off(w, "tok_off", tok_off, n_texts, 0, false));
        n_tokens = tok_off[n_texts];
    }
    hipStream_t s = as_stream(stream);
    Staging st(mem, s);
    const int64_t* d_off; const int32_t* d_ids = ids;
    RL_TRY(st.in(tok_off, (size_t)n_texts + 1, &d_off));
    if (given && n_texts > 0) RL_TRY(st.in(ids, (size_t)n_tokens, &d_ids));
    int64_t* d_len; int64_t* d_scr;
    RL_TRY(st.temp((size_t)(n_texts + 1) * sizeof(int64_t), &d_len));
    RL_TRY(st.temp(kb_scan_scratch_items(n_texts + 1) * sizeof(int64_t), &d_scr));
    RL_TRY(launch_sp_row_lengths(d_off, n_texts, max_len, d_len, s));
    const int64_t* d_total = nullptr;
    RL_TRY(launch_kb_exclusive_scan(d_len, n_texts + 1, d_scr, &d_total, s));
    int64_t total = 0;
    RL_TRY(hip_status(hipMemcpyAsync(&total, d_total, sizeof(int64_t), hipMemcpyDeviceToHost, s), who));
    RL_TRY(hip_status(hipStreamSynchronize(s), who));
    if (total >= (int64_t(1) << 31)) return fail(RL_ERR_UNSUPPORTED, w + ": one call takes fewer than 2^31 tokens");
    *out_total = total;
    int32_t* d_so;
    RL_TRY(st.out(out_seq_offsets, (size_t)n_texts + 1, &d_so));
    RL_TRY(launch_sp_row_offsets(d_len, n_texts, d_so, s));
    if (given) {
        int32_t *d_oi, *d_op;
        RL_TRY(st.out(out_ids, (size_t)total, &d_oi));
        RL_TRY(st.out(out_positions, (size_t)total, &d_op));
        RL_TRY(launch_sp_row_write(d_ids, d_off, n_texts, max_len, bos_id, eos_id, position_offset, d_len, total, d_oi, d_op, s));
    }
    return st.finish();
}

}  // extern "C"
