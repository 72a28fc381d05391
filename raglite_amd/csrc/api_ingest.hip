// The ingestion entry points of the C ABI, which take no handle: pooling and normalising token embeddings, the packed
// encoder's attention, and the document-batched splitters (include/raglite_hip.h for the contract of each).
#include <string>

#include "staging.h"

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

}  // extern "C"
