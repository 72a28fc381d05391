// The retrieval entry points of the C ABI that combine handles: rank fusion, hybrid search, search-and-rerank, chunk spans and the
// metadata filters (include/raglite_hip.h for the contract of each).  They drive rl_index and rl_keyword_index through the functions
// handles.h declares, under the lock orders stated there.
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "handles.h"

using namespace rl;

// ---- weighted Reciprocal Rank Fusion and batched hybrid search (include/raglite_hip.h; the kernel is in fuse.hip) ------------------
namespace {
// rl_rrf_fuse's limits (weights: host memory)
int check_fuse_args(int32_t n_lists, int32_t n_queries, int32_t len, const double* weights, int32_t rrf_k, int32_t k, const char* who) {
    if (n_lists < 1 || n_lists > RRF_MAX_LISTS) return fail(RL_ERR_INVALID, std::string(who) + ": n_lists must be in [1, 4]");
    if (n_queries < 0 || len < 1) return fail(RL_ERR_INVALID, std::string(who) + ": n_queries must be >= 0 and len >= 1");
    if ((int64_t)n_lists * len > RRF_MAX_ENTRIES) return fail(RL_ERR_INVALID, std::string(who) + ": n_lists * len must be <= 4096");
    if (k < 1 || k > n_lists * len) return fail(RL_ERR_INVALID, std::string(who) + ": k must be in [1, n_lists * len]");
    if (rrf_k < 1 || rrf_k > RRF_MAX_K) return fail(RL_ERR_INVALID, std::string(who) + ": rrf_k must be in [1, 2^30]");
    if (!weights) return fail(RL_ERR_INVALID, std::string(who) + ": null weights");
    for (int32_t r = 0; r < n_lists; ++r)
        if (!(std::fabs(weights[r]) <= RRF_MAX_WEIGHT))
            return fail(RL_ERR_INVALID, std::string(who) + ": weights must be finite, of magnitude <= 2^1000");
    return RL_OK;
}
}  // namespace

extern "C" {

int rl_rrf_fuse(const int32_t* lists, int32_t n_lists, int32_t n_queries, int32_t len, const double* weights, int32_t rrf_k, int32_t k,
                double* out_scores, int32_t* out_ids, int32_t* out_counts, int mem, void* stream) {
    RL_TRY(check_fuse_args(n_lists, n_queries, len, weights, rrf_k, k, "rl_rrf_fuse"));
    RL_TRY(check_mem(mem, "rl_rrf_fuse"));
    if (n_queries == 0) return RL_OK;
    if (!lists || !out_scores || !out_ids) return fail(RL_ERR_INVALID, "rl_rrf_fuse: null argument");
    hipStream_t s = as_stream(stream);
    const size_t n_in = (size_t)n_lists * n_queries * len, n_out = (size_t)n_queries * k;
    Staging st(mem, s);
    const int32_t* d_l;
    double* d_s;
    int32_t *d_i, *d_n = nullptr;
    RL_TRY(st.in(lists, n_in, &d_l));
    RL_TRY(st.out(out_scores, n_out, &d_s));
    RL_TRY(st.out(out_ids, n_out, &d_i));
    RL_TRY(st.out(out_counts, (size_t)n_queries, &d_n));  // (optional)
    RL_TRY(launch_rrf_fuse(d_l, n_lists, n_queries, len, weights, rrf_k, k, d_s, d_i, d_n, s));
    return st.finish();
}

int rl_shard_hybrid_fuse(const int32_t* gathered, int32_t world, int32_t n_queries, int32_t num_hits, int32_t n_each, int32_t n_lists,
                         const double* weights, int32_t rrf_k, int32_t k, double* out_scores, int32_t* out_chunks, int32_t* out_counts, int mem,
                         void* stream) {
    const char* who = "rl_shard_hybrid_fuse";
    if (world < 1) return fail(RL_ERR_INVALID, "rl_shard_hybrid_fuse: world must be >= 1");
    if (n_lists != 1 && n_lists != 2) return fail(RL_ERR_INVALID, "rl_shard_hybrid_fuse: n_lists must be 1 or 2");
    if (num_hits < 1) return fail(RL_ERR_INVALID, "rl_shard_hybrid_fuse: num_hits must be >= 1");
    RL_TRY(check_fuse_args(n_lists, n_queries, n_each, weights, rrf_k, k, who));
    RL_TRY(check_mem(mem, "rl_shard_hybrid_fuse"));
    if ((int64_t)world * num_hits > SHARD_FUSE_MAX_ENTRIES || (n_lists == 2 && (int64_t)world * n_each > SHARD_FUSE_MAX_ENTRIES))
        return fail(RL_ERR_UNSUPPORTED, "rl_shard_hybrid_fuse: world * num_hits and world * n_each must be <= 4096");
    if (n_queries == 0) return RL_OK;
    if (!gathered || !out_scores || !out_chunks) return fail(RL_ERR_INVALID, "rl_shard_hybrid_fuse: null argument");
    hipStream_t s = as_stream(stream);
    const size_t W = (size_t)3 * num_hits + (n_lists == 2 ? (size_t)2 * n_each : 0);
    const size_t n_in = (size_t)world * n_queries * W, n_out = (size_t)n_queries * k;
    Staging st(mem, s);
    const int32_t* d_g;
    double* d_s;
    int32_t *d_c, *d_n = nullptr;
    RL_TRY(st.in(gathered, n_in, &d_g));
    RL_TRY(st.out(out_scores, n_out, &d_s));
    RL_TRY(st.out(out_chunks, n_out, &d_c));
    RL_TRY(st.out(out_counts, (size_t)n_queries, &d_n));  // (optional)
    RL_TRY(launch_shard_hybrid_fuse(d_g, world, n_queries, num_hits, n_each, n_lists, weights, rrf_k, k, d_s, d_c, d_n, s));
    return st.finish();
}

}  // extern "C"

namespace {
// What every hybrid call needs before its device work: the arguments checked, both handles locked on the stream, the inputs staged.
struct HybridCall {
    std::unique_lock<std::mutex> idx_lock, kw_lock;  // (taken in this order: handles.h, struct rl_index)
    Staging st;                                      // (after the locks: its buffers are released while they are held)
    const float* d_q = nullptr;
    const int64_t* d_off = nullptr;
    const int32_t* d_terms = nullptr;
    BatchFilters f;
    int32_t n_filters = 0;
    const int32_t* query_filter = nullptr;
    bool empty = false;  // n_queries == 0: nothing to do
    HybridCall(int mem, hipStream_t s) : st(args_mem(mem), s) {}  // (`mem` as the caller of the entry point gave it)
};

// The checks of rl_hybrid_search (k: the fusion's), the locks and the staging-in
int hybrid_search_begin(rl_index* idx, rl_keyword_index* kw, const float* queries, int32_t B, int32_t num_hits, int32_t n_each,
                        const int64_t* q_off, const int32_t* q_terms, const uint32_t* chunk_filters, int32_t n_filters,
                        const int32_t* query_filter, const int64_t* rank_limits, int64_t rank_limit, const double* weights, int32_t rrf_k,
                        int32_t k, bool outputs, int mem, hipStream_t s, const char* who, HybridCall* c) {
    const int fmem = filters_mem(mem);  // (`mem` as the caller of the entry point gave it; the callers go on with args_mem(mem))
    mem = args_mem(mem);
    const int32_t R = kw ? 2 : 1;
    RL_TRY(check_search_args(idx, queries, B, n_each, who));
    if (rank_limit < 0) return fail(RL_ERR_INVALID, std::string(who) + ": rank_limit must be >= 0 (0 = no cut)");
    if (num_hits < 1 || num_hits > K_MAX) return fail(RL_ERR_INVALID, std::string(who) + ": num_hits must be in [1, 2048]");
    RL_TRY(check_fuse_args(R, B, n_each, weights, rrf_k, k, who));
    RL_TRY(check_mem(mem, who));
    if (kw && kw->n_chunks != idx->n_chunks) return fail(RL_ERR_INVALID, std::string(who) + ": the keyword index covers another number of chunks");
    if (B == 0) { c->empty = true; return RL_OK; }
    if (!outputs) return fail(RL_ERR_INVALID, std::string(who) + ": null output");
    int64_t n_q_terms = 0;
    if (kw) {
        if (!q_off) return fail(RL_ERR_INVALID, std::string(who) + ": null q_off");
        if (mem == RL_MEM_HOST) {
            RL_TRY(check_host_q_off(q_off, q_terms, B, who));
            n_q_terms = q_off[B];
        } else if (!q_terms) {
            return fail(RL_ERR_INVALID, std::string(who) + ": null q_terms");
        }
    }
    c->idx_lock = std::unique_lock<std::mutex>(idx->mu);  // (then kw->mu)
    RL_TRY(use_scratch(idx, s));
    if (kw) {
        c->kw_lock = std::unique_lock<std::mutex>(kw->mu);
        RL_TRY(keyword_use_stream(kw, s));
    }
    c->d_terms = q_terms;
    c->n_filters = n_filters;
    c->query_filter = query_filter;
    c->f.n = n_filters;
    c->f.qf = query_filter;
    c->f.lim = rank_limits;
    c->f.limit = rank_limit;
    RL_TRY(c->st.in(queries, (size_t)B * idx->dim, &c->d_q));
    if (n_filters) RL_TRY(c->st.in(chunk_filters, (size_t)n_filters * ((idx->n_chunks + 31) / 32), &c->f.chunk_bits, fmem));
    if (kw) {
        RL_TRY(c->st.in(q_off, (size_t)B + 1, &c->d_off));
        if (mem == RL_MEM_HOST) RL_TRY(c->st.in(q_terms, (size_t)n_q_terms, &c->d_terms));
    }
    return RL_OK;
}

// The two searches and the fusion on device pointers (after hybrid_search_begin): d_s / d_c [B x k], d_n [B]
int hybrid_search_device(rl_index* idx, rl_keyword_index* kw, const HybridCall& c, int32_t B, int32_t num_hits, int32_t n_each,
                         const double* weights, int32_t rrf_k, int32_t k, double* d_s, int32_t* d_c, int32_t* d_n, hipStream_t s) {
    const int32_t R = kw ? 2 : 1;
    const size_t n_list = (size_t)B * n_each;
    // index-owned scratch: lists [R x B x n_each] int32 (what the fusion reads), the two searches' scores [R x B x n_each] f32 and
    // counts [R x B] int32 (written, not read)
    HybridLists L;
    RL_TRY(carve(idx->hybrid, L, R, B, n_each));
    int32_t *const lists = L.lists, *const list_counts = L.counts;
    float* const list_scores = L.scores;
    RL_TRY(search_chunks_device(idx, c.d_q, B, num_hits, n_each, c.f, list_scores, lists, list_counts, s));
    if (kw) {
        QueryMask mask;
        RL_TRY(keyword_mask(kw, c.f.chunk_bits, c.n_filters, c.query_filter, B, s, &mask));
        RL_TRY(keyword_search_device(kw, c.d_off, c.d_terms, B, n_each, mask, list_scores + n_list, lists + n_list, list_counts + B, s));
    }
    return launch_rrf_fuse(lists, R, B, n_each, weights, rrf_k, k, d_s, d_c, d_n, s);
}

// rl_hybrid_search and rl_hybrid_search_per_query: one device path
int hybrid_search_call(rl_index* idx, rl_keyword_index* kw, const float* queries, int32_t n_queries, int32_t num_hits, int32_t n_each,
                       const int64_t* q_off, const int32_t* q_terms, const uint32_t* chunk_filters, int32_t n_filters, const int32_t* query_filter,
                       const int64_t* rank_limits, int64_t rank_limit, const double* weights, int32_t rrf_k, int32_t k, double* out_scores,
                       int32_t* out_chunks, int32_t* out_counts, int mem, void* stream, const char* who) {
    const int32_t B = n_queries;
    hipStream_t s = as_stream(stream);
    HybridCall c(mem, s);
    RL_TRY(hybrid_search_begin(idx, kw, queries, B, num_hits, n_each, q_off, q_terms, chunk_filters, n_filters, query_filter, rank_limits,
                               rank_limit, weights, rrf_k, k, out_scores && out_chunks && out_counts, mem, s, who, &c));
    if (c.empty) return RL_OK;
    Staging& st = c.st;
    const size_t n_out = (size_t)B * k;
    double* d_s;
    int32_t *d_c, *d_n;
    RL_TRY(st.out(out_scores, n_out, &d_s));
    RL_TRY(st.out(out_chunks, n_out, &d_c));
    RL_TRY(st.out(out_counts, (size_t)B, &d_n));
    RL_TRY(hybrid_search_device(idx, kw, c, B, num_hits, n_each, weights, rrf_k, k, d_s, d_c, d_n, s));
    return st.finish();
}
}  // namespace

extern "C" {

int rl_hybrid_search(rl_index* idx, rl_keyword_index* kw, const float* queries, int32_t n_queries, int32_t num_hits, int32_t n_each,
                     const int64_t* q_off, const int32_t* q_terms, const uint32_t* chunk_filter, int64_t rank_limit, const double* weights,
                     int32_t rrf_k, int32_t k, double* out_scores, int32_t* out_chunks, int32_t* out_counts, int mem, void* stream) {
    return hybrid_search_call(idx, kw, queries, n_queries, num_hits, n_each, q_off, q_terms, chunk_filter, chunk_filter ? 1 : 0, nullptr, nullptr,
                              rank_limit, weights, rrf_k, k, out_scores, out_chunks, out_counts, mem, stream, "rl_hybrid_search");
}

int rl_hybrid_search_per_query(rl_index* idx, rl_keyword_index* kw, const float* queries, int32_t n_queries, int32_t num_hits, int32_t n_each,
                               const int64_t* q_off, const int32_t* q_terms, const uint32_t* chunk_filters, int32_t n_filters,
                               const int32_t* query_filter, const int64_t* rank_limits, const double* weights, int32_t rrf_k, int32_t k,
                               double* out_scores, int32_t* out_chunks, int32_t* out_counts, int mem, void* stream) {
    const char* who = "rl_hybrid_search_per_query";
    RL_TRY(check_query_filters(n_queries, chunk_filters, n_filters, query_filter, rank_limits, who));
    return hybrid_search_call(idx, kw, queries, n_queries, num_hits, n_each, q_off, q_terms, chunk_filters, query_filter ? n_filters : 0,
                              query_filter, rank_limits, 0, weights, rrf_k, k, out_scores, out_chunks, out_counts, mem, stream, who);
}

// ---- batched search-and-rerank (include/raglite_hip.h; the ordering kernel is in rerank.hip) -----------------------------------------
int rl_rerank_order(const float* scores, const int32_t* candidates, int32_t n_queries, int32_t n_cand, int32_t k, float* out_scores,
                    int32_t* out_chunks, int32_t* out_pos, int32_t* out_counts, int mem, void* stream) {
    if (n_queries < 0) return fail(RL_ERR_INVALID, "rl_rerank_order: n_queries must be >= 0");
    if (n_cand < 1 || n_cand > RERANK_MAX_ENTRIES) return fail(RL_ERR_INVALID, "rl_rerank_order: n_cand must be in [1, 4096]");
    if (k < 1 || k > n_cand) return fail(RL_ERR_INVALID, "rl_rerank_order: k must be in [1, n_cand]");
    RL_TRY(check_mem(mem, "rl_rerank_order"));
    if (n_queries == 0) return RL_OK;
    if (!scores || !candidates || !out_scores || !out_chunks || !out_pos || !out_counts)
        return fail(RL_ERR_INVALID, "rl_rerank_order: null argument");
    hipStream_t s = as_stream(stream);
    const size_t n_in = (size_t)n_queries * n_cand, n_out = (size_t)n_queries * k;
    Staging st(mem, s);
    const float* d_sc;
    const int32_t* d_ca;
    float* d_s;
    int32_t *d_c, *d_p, *d_n;
    RL_TRY(st.in(scores, n_in, &d_sc));
    RL_TRY(st.in(candidates, n_in, &d_ca));
    RL_TRY(st.out(out_scores, n_out, &d_s));
    RL_TRY(st.out(out_chunks, n_out, &d_c));
    RL_TRY(st.out(out_pos, n_out, &d_p));
    RL_TRY(st.out(out_counts, (size_t)n_queries, &d_n));
    RL_TRY(launch_rerank_order(d_sc, d_ca, n_queries, n_cand, k, d_s, d_c, d_p, d_n, s));
    return st.finish();
}

}  // extern "C"

// ---- chunk spans (include/raglite_hip.h; the kernel is in spans.hip) -------------------------------------------------------------------
// Immutable after rl_span_table_create: calls on any stream may share it without a lock.
struct rl_span_table {
    int64_t n_chunks = 0;
    int64_t n_live = 0;                 // chunks with a position
    rl::DevArray<int32_t> rank_of;      // [n_chunks] the chunk's rank in (doc, pos) order, -1: no position
    rl::DevArray<uint64_t> tab_key;     // [n_live] doc << 32 | pos, ascending
    rl::DevArray<int32_t> tab_ord;      // [n_live] the chunk ordinal at that rank
};

namespace {
// What rl_search_rerank_per_query and rl_search_rerank_spans_per_query need before their device work: hybrid_search_begin's, and the
// query token vectors staged.
struct RerankCall {
    HybridCall c;
    const float* d_v = nullptr;
    const int64_t *qv_off = nullptr, *d_qv_off = nullptr;  // the ragged entries: each query's vectors, on the host and staged
    RerankCall(int mem, hipStream_t s) : c(mem, s) {}
};

// ... of the ragged entries (qv_off [B + 1], host memory, in place of nq): the same checks with the table's in front of the first HIP
// call, no limit on a query's vectors, the table staged behind the vectors
int search_rerank_ragged_begin(rl_index* idx, rl_keyword_index* kw, const float* queries, int32_t B, int32_t num_hits, int32_t n_each,
                               const int64_t* q_off, const int32_t* q_terms, const uint32_t* chunk_filters, int32_t n_filters,
                               const int32_t* query_filter, const int64_t* rank_limits, const double* weights, int32_t rrf_k, int32_t n_cand,
                               const float* query_vecs, const int64_t* qv_off, int32_t k, bool outputs, int mem, hipStream_t s, const char* who,
                               RerankCall* rc) {
    if (B < 0) return fail(RL_ERR_INVALID, std::string(who) + ": n_queries must be >= 0");
    if (n_cand < 1 || n_cand > RERANK_MAX_ENTRIES) return fail(RL_ERR_INVALID, std::string(who) + ": n_cand must be in [1, 4096]");
    if (k < 1 || k > n_cand) return fail(RL_ERR_INVALID, std::string(who) + ": k must be in [1, n_cand]");
    RL_TRY(check_query_filters(B, chunk_filters, n_filters, query_filter, rank_limits, who));
    RL_TRY(check_mem(args_mem(mem), who));
    if (B == 0) { rc->c.empty = true; return RL_OK; }
    if (!qv_off) return fail(RL_ERR_INVALID, std::string(who) + ": null qv_off");
    RL_TRY(check_qv_off(qv_off, B, who));
    if (idx && idx->E16 && idx->dim % 16)
        return fail(RL_ERR_UNSUPPORTED, std::string(who) + ": MaxSim reranking on an fp16-stored index needs dim % 16 == 0");
    RL_TRY(hybrid_search_begin(idx, kw, queries, B, num_hits, n_each, q_off, q_terms, chunk_filters, query_filter ? n_filters : 0, query_filter,
                               rank_limits, 0, weights, rrf_k, n_cand, query_vecs && outputs, mem, s, who, &rc->c));
    rc->qv_off = qv_off;
    RL_TRY(rc->c.st.in(query_vecs, (size_t)qv_off[B] * idx->dim, &rc->d_v));
    return rc->c.st.in(qv_off, (size_t)B + 1, &rc->d_qv_off, RL_MEM_HOST);
}

// The checks of rl_search_rerank_per_query, the locks and the staging-in
int search_rerank_begin(rl_index* idx, rl_keyword_index* kw, const float* queries, int32_t B, int32_t num_hits, int32_t n_each,
                        const int64_t* q_off, const int32_t* q_terms, const uint32_t* chunk_filters, int32_t n_filters,
                        const int32_t* query_filter, const int64_t* rank_limits, const double* weights, int32_t rrf_k, int32_t n_cand,
                        const float* query_vecs, int32_t nq, int32_t k, bool outputs, int mem, hipStream_t s, const char* who, RerankCall* rc) {
    if (nq < 1) return fail(RL_ERR_INVALID, std::string(who) + ": nq must be >= 1");
    if (n_cand < 1 || n_cand > RERANK_MAX_ENTRIES) return fail(RL_ERR_INVALID, std::string(who) + ": n_cand must be in [1, 4096]");
    if (k < 1 || k > n_cand) return fail(RL_ERR_INVALID, std::string(who) + ": k must be in [1, n_cand]");
    RL_TRY(check_query_filters(B, chunk_filters, n_filters, query_filter, rank_limits, who));
    if (idx && idx->E16 && (nq > 32 || idx->dim % 16))
        return fail(RL_ERR_UNSUPPORTED, std::string(who) + ": MaxSim reranking on an fp16-stored index needs nq <= 32 and dim % 16 == 0");
    RL_TRY(hybrid_search_begin(idx, kw, queries, B, num_hits, n_each, q_off, q_terms, chunk_filters, query_filter ? n_filters : 0, query_filter,
                               rank_limits, 0, weights, rrf_k, n_cand, query_vecs && outputs, mem, s, who, &rc->c));
    if (rc->c.empty) return RL_OK;
    return rc->c.st.in(query_vecs, (size_t)B * nq * idx->dim, &rc->d_v);
}

// The searches, the fusion, the MaxSim rerank and the ordering on device pointers (after search_rerank_begin): d_c [B x k], d_n [B];
// d_s [B x k], or nullptr: the scores stay in the index's scratch
int search_rerank_device(rl_index* idx, rl_keyword_index* kw, const RerankCall& rc, int32_t B, int32_t num_hits, int32_t n_each,
                         const double* weights, int32_t rrf_k, int32_t n_cand, int32_t nq, int32_t k, float* d_s, int32_t* d_c, int32_t* d_n,
                         hipStream_t s, const char* who = "" /* the ragged entries: their name, for the rerank's errors */) {
    // index-owned scratch: the fused scores [B x n_cand] f64 (written, not read), the fused candidates [B x n_cand] int32, their
    // MaxSim scores [B x n_cand] f32, the fusion's counts [B] and the positions of the first k [B x k] int32 (written, not read);
    // without d_s the scores of the first k [B x k] f32 (written, not read)
    RerankScratch L;
    RL_TRY(carve(idx->rerank, L, B, n_cand, k, !d_s));
    if (!d_s) d_s = L.own_scores;
    RL_TRY(hybrid_search_device(idx, kw, rc.c, B, num_hits, n_each, weights, rrf_k, n_cand, L.fused_scores, L.fused, L.fused_counts, s));
    if (rc.qv_off) RL_TRY(maxsim_rerank_ragged_device(idx, rc.d_v, rc.qv_off, rc.d_qv_off, B, L.fused, n_cand, L.maxsim, s, who));
    else RL_TRY(maxsim_rerank_device(idx, rc.d_v, B, nq, L.fused, n_cand, L.maxsim, s));
    return launch_rerank_order(L.maxsim, L.fused, B, n_cand, k, d_s, d_c, L.pos, d_n, s);
}

// rl_chunk_spans' limits
int check_span_args(const rl_span_table* table, int32_t n_queries, int32_t n_in, const int32_t* offsets, int32_t n_off, int mem,
                    const char* who) {
    if (!table) return fail(RL_ERR_INVALID, std::string(who) + ": null span table");
    if (n_queries < 0) return fail(RL_ERR_INVALID, std::string(who) + ": n_queries must be >= 0");
    if (n_off < 0 || n_off > SPANS_MAX_OFFSETS) return fail(RL_ERR_INVALID, std::string(who) + ": n_off must be in [0, 64]");
    if (n_in < 1 || (int64_t)n_in * (1 + n_off) > SPANS_MAX_ENTRIES)
        return fail(RL_ERR_INVALID, std::string(who) + ": need n_in >= 1 and n_in * (1 + n_off) <= 4096");
    if (n_off > 0 && !offsets) return fail(RL_ERR_INVALID, std::string(who) + ": null offsets");
    RL_TRY(check_mem(mem, who));
    return RL_OK;
}

// The five outputs of the span kernel for a batch, as the kernel takes them ...
struct SpanPtrs {
    int32_t *d_c = nullptr, *d_l = nullptr, *d_ns = nullptr, *d_nc = nullptr;
    double* d_s = nullptr;
};
// ... registered on a call's frame: [n] chunks, span lengths and span scores, [B] span and chunk counts
int span_outputs(Staging& st, int32_t* out_chunks, int32_t* out_span_len, double* out_span_scores, int32_t* out_n_spans, int32_t* out_n_chunks,
                 size_t n, size_t B, SpanPtrs* o) {
    RL_TRY(st.out(out_chunks, n, &o->d_c));
    RL_TRY(st.out(out_span_len, n, &o->d_l));
    RL_TRY(st.out(out_span_scores, n, &o->d_s));
    RL_TRY(st.out(out_n_spans, B, &o->d_ns));
    return st.out(out_n_chunks, B, &o->d_nc);
}

int spans_device(const rl_span_table* t, const int32_t* d_in, int32_t B, int32_t n_in, const int32_t* offsets, int32_t n_off,
                 const SpanPtrs& o, hipStream_t s) {
    return launch_chunk_spans(t->rank_of, t->tab_key, t->tab_ord, (int32_t)t->n_chunks, (int32_t)t->n_live, d_in, B, n_in, offsets, n_off,
                              o.d_c, o.d_l, o.d_s, o.d_ns, o.d_nc, s);
}
}  // namespace

extern "C" {

int rl_search_rerank_per_query(rl_index* idx, rl_keyword_index* kw, const float* queries, int32_t n_queries, int32_t num_hits, int32_t n_each,
                               const int64_t* q_off, const int32_t* q_terms, const uint32_t* chunk_filters, int32_t n_filters,
                               const int32_t* query_filter, const int64_t* rank_limits, const double* weights, int32_t rrf_k, int32_t n_cand,
                               const float* query_vecs, int32_t nq, int32_t k, float* out_scores, int32_t* out_chunks, int32_t* out_counts,
                               int mem, void* stream) {
    const char* who = "rl_search_rerank_per_query";
    const int32_t B = n_queries;
    hipStream_t s = as_stream(stream);
    RerankCall rc(mem, s);
    RL_TRY(search_rerank_begin(idx, kw, queries, B, num_hits, n_each, q_off, q_terms, chunk_filters, n_filters, query_filter, rank_limits, weights,
                               rrf_k, n_cand, query_vecs, nq, k, out_scores && out_chunks && out_counts, mem, s, who, &rc));
    if (rc.c.empty) return RL_OK;
    Staging& st = rc.c.st;
    const size_t n_out = (size_t)B * k;
    float* d_s;
    int32_t *d_c, *d_n;
    RL_TRY(st.out(out_scores, n_out, &d_s));
    RL_TRY(st.out(out_chunks, n_out, &d_c));
    RL_TRY(st.out(out_counts, (size_t)B, &d_n));
    RL_TRY(search_rerank_device(idx, kw, rc, B, num_hits, n_each, weights, rrf_k, n_cand, nq, k, d_s, d_c, d_n, s));
    return st.finish();
}

int rl_search_rerank_ragged(rl_index* idx, rl_keyword_index* kw, const float* queries, int32_t n_queries, int32_t num_hits, int32_t n_each,
                            const int64_t* q_off, const int32_t* q_terms, const uint32_t* chunk_filters, int32_t n_filters,
                            const int32_t* query_filter, const int64_t* rank_limits, const double* weights, int32_t rrf_k, int32_t n_cand,
                            const float* query_vecs, const int64_t* qv_off, int32_t k, float* out_scores, int32_t* out_chunks,
                            int32_t* out_counts, int mem, void* stream) {
    const char* who = "rl_search_rerank_ragged";
    const int32_t B = n_queries;
    hipStream_t s = as_stream(stream);
    RerankCall rc(mem, s);
    RL_TRY(search_rerank_ragged_begin(idx, kw, queries, B, num_hits, n_each, q_off, q_terms, chunk_filters, n_filters, query_filter, rank_limits,
                                      weights, rrf_k, n_cand, query_vecs, qv_off, k, out_scores && out_chunks && out_counts, mem, s, who, &rc));
    if (rc.c.empty) return RL_OK;
    Staging& st = rc.c.st;
    const size_t n_out = (size_t)B * k;
    float* d_s;
    int32_t *d_c, *d_n;
    RL_TRY(st.out(out_scores, n_out, &d_s));
    RL_TRY(st.out(out_chunks, n_out, &d_c));
    RL_TRY(st.out(out_counts, (size_t)B, &d_n));
    RL_TRY(search_rerank_device(idx, kw, rc, B, num_hits, n_each, weights, rrf_k, n_cand, 0, k, d_s, d_c, d_n, s, who));
    return st.finish();
}

int rl_span_table_create(rl_span_table** out, const int32_t* doc, const int32_t* pos, int64_t n_chunks) {
    const char* who = "rl_span_table_create";
    if (!out) return fail(RL_ERR_INVALID, std::string(who) + ": null output handle");
    *out = nullptr;
    if (n_chunks < 0) return fail(RL_ERR_INVALID, std::string(who) + ": negative size");
    if (n_chunks >= (int64_t)0x7fffffff - 1) return fail(RL_ERR_UNSUPPORTED, std::string(who) + ": more than 2^31-2 chunks");
    if (n_chunks > 0 && (!doc || !pos)) return fail(RL_ERR_INVALID, std::string(who) + ": null argument");
    std::vector<std::pair<uint64_t, int32_t>> live;  // (doc << 32 | pos, ordinal)
    for (int64_t c = 0; c < n_chunks; ++c) {
        if (doc[c] < 0) continue;
        if (pos[c] < 0) return fail(RL_ERR_INVALID, std::string(who) + ": pos must be >= 0");
        live.emplace_back(((uint64_t)(uint32_t)doc[c] << 32) | (uint32_t)pos[c], (int32_t)c);
    }
    std::sort(live.begin(), live.end());
    for (size_t r = 1; r < live.size(); ++r)
        if (live[r].first == live[r - 1].first) return fail(RL_ERR_INVALID, std::string(who) + ": two chunks share a (doc, pos)");
    std::vector<int32_t> rank_of((size_t)n_chunks, -1), tab_ord(live.size());
    std::vector<uint64_t> tab_key(live.size());
    for (size_t r = 0; r < live.size(); ++r) {
        tab_key[r] = live[r].first;
        tab_ord[r] = live[r].second;
        rank_of[(size_t)live[r].second] = (int32_t)r;
    }
    std::unique_ptr<rl_span_table> t(new rl_span_table());
    t->n_chunks = n_chunks;
    t->n_live = (int64_t)live.size();
    RL_TRY(t->rank_of.alloc(std::max<size_t>(rank_of.size() * sizeof(int32_t), 16), who));
    RL_TRY(t->tab_key.alloc(std::max<size_t>(tab_key.size() * sizeof(uint64_t), 16), who));
    RL_TRY(t->tab_ord.alloc(std::max<size_t>(tab_ord.size() * sizeof(int32_t), 16), who));
    if (n_chunks) RL_HIP(hipMemcpy(t->rank_of, rank_of.data(), rank_of.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if (!live.empty()) {
        RL_HIP(hipMemcpy(t->tab_key, tab_key.data(), tab_key.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
        RL_HIP(hipMemcpy(t->tab_ord, tab_ord.data(), tab_ord.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    *out = t.release();
    return RL_OK;
}

int rl_span_table_destroy(rl_span_table* table) {
    if (!table) return RL_OK;
    delete table;
    return RL_OK;
}

int rl_span_table_info(const rl_span_table* table, int64_t* n_chunks, int64_t* n_live, int64_t* device_bytes) {
    if (!table) return fail(RL_ERR_INVALID, "rl_span_table_info: null span table");
    if (n_chunks) *n_chunks = table->n_chunks;
    if (n_live) *n_live = table->n_live;
    if (device_bytes) *device_bytes = (int64_t)(table->rank_of.cap + table->tab_key.cap + table->tab_ord.cap);
    return RL_OK;
}

int rl_chunk_spans(const rl_span_table* table, const int32_t* chunks, int32_t n_queries, int32_t n_in, const int32_t* offsets, int32_t n_off,
                   int32_t* out_chunks, int32_t* out_span_len, double* out_span_scores, int32_t* out_n_spans, int32_t* out_n_chunks, int mem,
                   void* stream) {
    const char* who = "rl_chunk_spans";
    RL_TRY(check_span_args(table, n_queries, n_in, offsets, n_off, mem, who));
    if (n_queries == 0) return RL_OK;
    if (!chunks || !out_chunks || !out_span_len || !out_span_scores || !out_n_spans || !out_n_chunks)
        return fail(RL_ERR_INVALID, std::string(who) + ": null argument");
    hipStream_t s = as_stream(stream);
    const size_t B = (size_t)n_queries, n_out = B * n_in * (1 + n_off);
    Staging st(mem, s);
    const int32_t* d_in;
    SpanPtrs o;
    RL_TRY(st.in(chunks, B * n_in, &d_in));
    RL_TRY(span_outputs(st, out_chunks, out_span_len, out_span_scores, out_n_spans, out_n_chunks, n_out, B, &o));
    RL_TRY(spans_device(table, d_in, n_queries, n_in, offsets, n_off, o, s));
    return st.finish();
}

int rl_search_rerank_spans_per_query(rl_index* idx, rl_keyword_index* kw, const float* queries, int32_t n_queries, int32_t num_hits,
                                     int32_t n_each, const int64_t* q_off, const int32_t* q_terms, const uint32_t* chunk_filters,
                                     int32_t n_filters, const int32_t* query_filter, const int64_t* rank_limits, const double* weights,
                                     int32_t rrf_k, int32_t n_cand, const float* query_vecs, int32_t nq, int32_t k, const rl_span_table* table,
                                     const int32_t* offsets, int32_t n_off, int32_t* out_top_chunks, int32_t* out_top_counts,
                                     int32_t* out_chunks, int32_t* out_span_len, double* out_span_scores, int32_t* out_n_spans,
                                     int32_t* out_n_chunks, int mem, void* stream) {
    const char* who = "rl_search_rerank_spans_per_query";
    const int32_t B = n_queries;
    RL_TRY(check_span_args(table, B, k, offsets, n_off, args_mem(mem), who));  // (k * (1 + n_off) <= 4096)
    if (idx && table->n_chunks != idx->n_chunks) return fail(RL_ERR_INVALID, std::string(who) + ": the span table covers another number of chunks");
    hipStream_t s = as_stream(stream);
    RerankCall rc(mem, s);
    RL_TRY(search_rerank_begin(idx, kw, queries, B, num_hits, n_each, q_off, q_terms, chunk_filters, n_filters, query_filter, rank_limits, weights,
                               rrf_k, n_cand, query_vecs, nq, k,
                               out_top_chunks && out_top_counts && out_chunks && out_span_len && out_span_scores && out_n_spans && out_n_chunks,
                               mem, s, who, &rc));
    if (rc.c.empty) return RL_OK;
    Staging& st = rc.c.st;
    const size_t n_top = (size_t)B * k, n_out = n_top * (1 + n_off);
    int32_t *d_c, *d_n;
    SpanPtrs o;
    RL_TRY(st.out(out_top_chunks, n_top, &d_c));
    RL_TRY(st.out(out_top_counts, (size_t)B, &d_n));
    RL_TRY(span_outputs(st, out_chunks, out_span_len, out_span_scores, out_n_spans, out_n_chunks, n_out, (size_t)B, &o));
    RL_TRY(search_rerank_device(idx, kw, rc, B, num_hits, n_each, weights, rrf_k, n_cand, nq, k, nullptr, d_c, d_n, s));
    RL_TRY(spans_device(table, d_c, B, k, offsets, n_off, o, s));
    return st.finish();
}

int rl_search_rerank_spans_ragged(rl_index* idx, rl_keyword_index* kw, const float* queries, int32_t n_queries, int32_t num_hits,
                                  int32_t n_each, const int64_t* q_off, const int32_t* q_terms, const uint32_t* chunk_filters,
                                  int32_t n_filters, const int32_t* query_filter, const int64_t* rank_limits, const double* weights,
                                  int32_t rrf_k, int32_t n_cand, const float* query_vecs, const int64_t* qv_off, int32_t k,
                                  const rl_span_table* table, const int32_t* offsets, int32_t n_off, int32_t* out_top_chunks,
                                  int32_t* out_top_counts, int32_t* out_chunks, int32_t* out_span_len, double* out_span_scores,
                                  int32_t* out_n_spans, int32_t* out_n_chunks, int mem, void* stream) {
    const char* who = "rl_search_rerank_spans_ragged";
    const int32_t B = n_queries;
    RL_TRY(check_span_args(table, B, k, offsets, n_off, args_mem(mem), who));  // (k * (1 + n_off) <= 4096)
    if (idx && table->n_chunks != idx->n_chunks) return fail(RL_ERR_INVALID, std::string(who) + ": the span table covers another number of chunks");
    hipStream_t s = as_stream(stream);
    RerankCall rc(mem, s);
    RL_TRY(search_rerank_ragged_begin(idx, kw, queries, B, num_hits, n_each, q_off, q_terms, chunk_filters, n_filters, query_filter, rank_limits,
                                      weights, rrf_k, n_cand, query_vecs, qv_off, k,
                                      out_top_chunks && out_top_counts && out_chunks && out_span_len && out_span_scores && out_n_spans && out_n_chunks,
                                      mem, s, who, &rc));
    if (rc.c.empty) return RL_OK;
    Staging& st = rc.c.st;
    const size_t n_top = (size_t)B * k, n_out = n_top * (1 + n_off);
    int32_t *d_c, *d_n;
    SpanPtrs o;
    RL_TRY(st.out(out_top_chunks, n_top, &d_c));
    RL_TRY(st.out(out_top_counts, (size_t)B, &d_n));
    RL_TRY(span_outputs(st, out_chunks, out_span_len, out_span_scores, out_n_spans, out_n_chunks, n_out, (size_t)B, &o));
    RL_TRY(search_rerank_device(idx, kw, rc, B, num_hits, n_each, weights, rrf_k, n_cand, 0, k, nullptr, d_c, d_n, s, who));
    RL_TRY(spans_device(table, d_c, B, k, offsets, n_off, o, s));
    return st.finish();
}

}  // extern "C"

// ---- metadata filters on the device (include/raglite_hip.h; the kernel is in metadata.hip) --------------------------------------------
struct rl_metadata_store {
    int64_t n_chunks = 0, n_tags = 0;
    int64_t cap_off = 0, cap_tags = 0;  // items the two arrays can hold
    rl::DevArray<int64_t> tag_off;      // [n_chunks + 1]
    rl::DevArray<int32_t> tags;         // [n_tags]
    std::mutex mu;
};

// What rl_metadata_filters leaves on the device: the bitsets [n_filters x words] and the counts [2 x n_filters].  Grown, never shrunk.
struct rl_filter_set {
    rl::Pool bits, counts, f_off, f_tags;  // (the last two: the filters' own CSR, staged for host callers)
    int32_t n_filters = 0;
    int64_t words = 0;
};

namespace {

// A CSR handed in by the caller, read on the host: from 0, ascending; returns its last entry in *total
int check_csr(const int64_t* off, int64_t n, int mem, hipStream_t s, const char* who, const char* name, std::vector<int64_t>* h_off,
              int64_t* total) {
    h_off->resize((size_t)n + 1);
    if (mem == RL_MEM_HOST) std::memcpy(h_off->data(), off, h_off->size() * sizeof(int64_t));
    else {
        RL_TRY(hip_status(hipMemcpyAsync(h_off->data(), off, h_off->size() * sizeof(int64_t), hipMemcpyDeviceToHost, s), who));
        RL_TRY(hip_status(hipStreamSynchronize(s), who));
    }
    if ((*h_off)[0] != 0) return fail(RL_ERR_INVALID, std::string(who) + ": " + name + " must start at 0");
    for (int64_t i = 0; i < n; ++i)
        if ((*h_off)[(size_t)i + 1] < (*h_off)[(size_t)i]) return fail(RL_ERR_INVALID, std::string(who) + ": " + name + " must be ascending");
    *total = (*h_off)[(size_t)n];
    return RL_OK;
}

// rl_metadata_store_append, and the one append of rl_metadata_store_create
int metadata_append(rl_metadata_store* st, const int64_t* tag_off, const int32_t* tags, int64_t n_new, int mem, void* stream, const char* who) {
    if (n_new < 0) return fail(RL_ERR_INVALID, std::string(who) + ": negative size");
    RL_TRY(check_mem(mem, who));
    if (n_new > 0 && !tag_off) return fail(RL_ERR_INVALID, std::string(who) + ": null tag_off");
    if (!st) return fail(RL_ERR_INVALID, std::string(who) + ": null store");
    if (n_new == 0) return RL_OK;
    hipStream_t s = as_stream(stream);
    std::vector<int64_t> h_off;
    int64_t n_add = 0;
    RL_TRY(check_csr(tag_off, n_new, mem, s, who, "tag_off", &h_off, &n_add));
    if (n_add > 0 && !tags) return fail(RL_ERR_INVALID, std::string(who) + ": null tags");
    std::lock_guard<std::mutex> lock(st->mu);
    if (st->n_chunks + n_new >= (int64_t)0x7fffffff - 1) return fail(RL_ERR_UNSUPPORTED, std::string(who) + ": more than 2^31-2 chunks");
    if (st->n_tags + n_add >= (int64_t)0x7fffffff) return fail(RL_ERR_UNSUPPORTED, std::string(who) + ": 2^31 tags or more");
    RL_TRY(store_grow(st->tag_off, &st->cap_off, st->n_chunks ? st->n_chunks + 1 : 0, st->n_chunks + n_new + 1, s, who));
    RL_TRY(store_grow(st->tags, &st->cap_tags, st->n_tags, st->n_tags + n_add, s, who));
    for (int64_t& o : h_off) o += st->n_tags;  // (h_off[0] is what tag_off[n_chunks] holds already, or the first 0)
    RL_TRY(hip_status(hipMemcpyAsync(st->tag_off + st->n_chunks, h_off.data(), h_off.size() * sizeof(int64_t), hipMemcpyHostToDevice, s), who));
    if (n_add > 0)
        RL_TRY(hip_status(hipMemcpyAsync(st->tags + st->n_tags, tags, (size_t)n_add * sizeof(int32_t),
                                         mem == RL_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s), who));
    RL_TRY(hip_status(hipStreamSynchronize(s), who));  // the caller's arrays and h_off may go away after return
    st->n_chunks += n_new;
    st->n_tags += n_add;
    return RL_OK;
}

}  // namespace

extern "C" {

int rl_metadata_store_append(rl_metadata_store* st, const int64_t* tag_off, const int32_t* tags, int64_t n_new, int mem, void* stream) {
    return metadata_append(st, tag_off, tags, n_new, mem, stream, "rl_metadata_store_append");
}

int rl_metadata_store_create(rl_metadata_store** out, const int64_t* tag_off, const int32_t* tags, int64_t n_chunks, int mem, void* stream) {
    const char* who = "rl_metadata_store_create";
    if (!out) return fail(RL_ERR_INVALID, std::string(who) + ": null output handle");
    *out = nullptr;
    if (n_chunks < 0) return fail(RL_ERR_INVALID, std::string(who) + ": negative size");
    RL_TRY(check_mem(mem, who));
    if (n_chunks > 0 && !tag_off) return fail(RL_ERR_INVALID, std::string(who) + ": null tag_off");
    std::unique_ptr<rl_metadata_store> st(new rl_metadata_store());
    RL_TRY(metadata_append(st.get(), tag_off, tags, n_chunks, mem, stream, who));
    *out = st.release();
    return RL_OK;
}

int rl_metadata_store_memory(const rl_metadata_store* st, int64_t out[2]) {
    if (!st || !out) return fail(RL_ERR_INVALID, "rl_metadata_store_memory: null argument");
    std::lock_guard<std::mutex> lock(const_cast<rl_metadata_store*>(st)->mu);
    out[0] = (st->n_chunks ? (st->n_chunks + 1) * (int64_t)sizeof(int64_t) : 0) + st->n_tags * (int64_t)sizeof(int32_t);
    out[1] = (int64_t)(st->tag_off.cap + st->tags.cap);
    return RL_OK;
}

int rl_metadata_store_destroy(rl_metadata_store* st) {
    delete st;
    return RL_OK;
}

int rl_metadata_filters(rl_metadata_store* st, rl_index* idx, const int64_t* f_off, const int32_t* f_tags, int32_t n_filters,
                        rl_filter_set** inout_set, int64_t* out_chunks, int64_t* out_rows, int mem, void* stream) {
    const char* who = "rl_metadata_filters";
    if (n_filters < 0) return fail(RL_ERR_INVALID, std::string(who) + ": n_filters must be >= 0");
    if (n_filters > MF_GROUP * 65535) return fail(RL_ERR_UNSUPPORTED, std::string(who) + ": more than 64 * 65535 filters");
    RL_TRY(check_mem(mem, who));
    if (!inout_set) return fail(RL_ERR_INVALID, std::string(who) + ": null inout_set");
    if (n_filters > 0 && (!f_off || !out_chunks || !out_rows)) return fail(RL_ERR_INVALID, std::string(who) + ": null f_off or output");
    if (!st) return fail(RL_ERR_INVALID, std::string(who) + ": null store");
    if (!idx) return fail(RL_ERR_INVALID, std::string(who) + ": null index");
    hipStream_t s = as_stream(stream);
    std::vector<int64_t> h_off;
    int64_t n_ftags = 0;
    if (n_filters > 0) RL_TRY(check_csr(f_off, n_filters, mem, s, who, "f_off", &h_off, &n_ftags));
    if (n_ftags >= (int64_t)0x7fffffff) return fail(RL_ERR_UNSUPPORTED, std::string(who) + ": 2^31 filter tags or more");
    if (n_ftags > 0 && !f_tags) return fail(RL_ERR_INVALID, std::string(who) + ": null f_tags");
    std::lock_guard<std::mutex> idx_lock(idx->mu);  // (then the store's: handles.h, struct rl_index)
    std::lock_guard<std::mutex> lock(st->mu);
    if (st->n_chunks != idx->n_chunks) return fail(RL_ERR_INVALID, std::string(who) + ": the metadata store covers another number of chunks");
    std::unique_ptr<rl_filter_set> fresh;
    rl_filter_set* set = *inout_set;
    if (!set) {
        fresh.reset(new rl_filter_set());
        set = fresh.get();
    }
    const int64_t n = st->n_chunks, words = (n + 31) / 32;
    set->n_filters = 0;  // (until the launch is enqueued)
    RL_TRY(set->bits.reserve(std::max<size_t>((size_t)n_filters * (size_t)words * sizeof(uint32_t), 16)));  // (never null: an empty index)
    RL_TRY(set->counts.reserve((size_t)2 * n_filters * sizeof(unsigned long long)));
    const int64_t* d_off = f_off;
    const int32_t* d_tags = f_tags;
    if (mem == RL_MEM_HOST && n_filters > 0) {
        RL_TRY(set->f_off.reserve(h_off.size() * sizeof(int64_t)));
        RL_TRY(set->f_tags.reserve((size_t)std::max<int64_t>(n_ftags, 1) * sizeof(int32_t)));
        RL_HIP(hipMemcpyAsync(set->f_off.p, h_off.data(), h_off.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
        if (n_ftags) RL_HIP(hipMemcpyAsync(set->f_tags.p, f_tags, (size_t)n_ftags * sizeof(int32_t), hipMemcpyHostToDevice, s));
        d_off = set->f_off.as<int64_t>();
        d_tags = set->f_tags.as<int32_t>();
    }
    unsigned long long* counts = set->counts.as<unsigned long long>();
    RL_TRY(launch_metadata_filters(st->tag_off, st->tags, n, idx->offsets, d_off, d_tags, n_filters, set->bits.as<uint32_t>(), counts, s));
    if (n_filters > 0) {
        const hipMemcpyKind kind = mem == RL_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        RL_HIP(hipMemcpyAsync(out_chunks, counts, (size_t)n_filters * sizeof(int64_t), kind, s));
        RL_HIP(hipMemcpyAsync(out_rows, counts + n_filters, (size_t)n_filters * sizeof(int64_t), kind, s));
    }
    if (mem == RL_MEM_HOST) RL_HIP(hipStreamSynchronize(s));
    set->n_filters = n_filters;
    set->words = words;
    if (fresh) *inout_set = fresh.release();
    return RL_OK;
}

int rl_filter_set_bits(const rl_filter_set* set, const uint32_t** out_device_bits, int32_t* out_n_filters, int64_t* out_words) {
    if (!set) return fail(RL_ERR_INVALID, "rl_filter_set_bits: null filter set");
    if (out_device_bits) *out_device_bits = set->bits.as<uint32_t>();
    if (out_n_filters) *out_n_filters = set->n_filters;
    if (out_words) *out_words = set->words;
    return RL_OK;
}

int rl_filter_set_read(const rl_filter_set* set, uint32_t* out, int mem, void* stream) {
    const char* who = "rl_filter_set_read";
    RL_TRY(check_mem(mem, who));
    if (!set) return fail(RL_ERR_INVALID, std::string(who) + ": null filter set");
    const size_t bytes = (size_t)set->n_filters * (size_t)set->words * sizeof(uint32_t);
    if (bytes == 0) return RL_OK;
    if (!out) return fail(RL_ERR_INVALID, std::string(who) + ": null output");
    hipStream_t s = as_stream(stream);
    RL_HIP(hipMemcpyAsync(out, set->bits.p, bytes, mem == RL_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
    if (mem == RL_MEM_HOST) RL_HIP(hipStreamSynchronize(s));
    return RL_OK;
}

int rl_filter_set_destroy(rl_filter_set* set) {
    delete set;
    return RL_OK;
}

}  // extern "C"
