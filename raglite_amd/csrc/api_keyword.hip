// The BM25 keyword entry points of the C ABI: rl_keyword_index (the struct is in handles.h: the hybrid calls read it), rl_keyword_store
// and rl_keyword_analyzer (include/raglite_hip.h for the contract of each).
#include <cstring>
#include <limits>
#include <memory>
#include <mutex>
#include <vector>

#include "handles.h"

using namespace rl;

// ---- BM25 keyword search (include/raglite_hip.h; kernels in keyword.hip; struct rl_keyword_index in handles.h) -----------------
namespace rl {
namespace {

// The host postings as the header states them; device postings are taken as given (the kernels skip what lies outside them).
int check_host_postings(const int64_t* term_off, int32_t n_terms, const int32_t* post_chunk, const int32_t* post_tf, const int32_t* post_term,
                        int64_t n_postings, int64_t n_chunks) {
    const char* who = "rl_keyword_index_create";
    if (term_off[0] != 0 || term_off[n_terms] != n_postings)
        return fail(RL_ERR_INVALID, std::string(who) + ": term_off must start at 0 and end at n_postings");
    for (int32_t t = 0; t < n_terms; ++t) {
        if (term_off[t + 1] < term_off[t]) return fail(RL_ERR_INVALID, std::string(who) + ": term_off must be ascending");
        for (int64_t p = term_off[t]; p < term_off[t + 1]; ++p) {
            if (post_chunk[p] < 0 || post_chunk[p] >= n_chunks) return fail(RL_ERR_INVALID, std::string(who) + ": chunk ordinal out of range");
            if (p > term_off[t] && post_chunk[p] <= post_chunk[p - 1])
                return fail(RL_ERR_INVALID, std::string(who) + ": the chunks of a term must be strictly ascending");
            if (post_tf[p] < 1) return fail(RL_ERR_INVALID, std::string(who) + ": term frequencies must be >= 1");
            if (post_term[p] != t) return fail(RL_ERR_INVALID, std::string(who) + ": post_term disagrees with term_off");
        }
    }
    return RL_OK;
}

}  // namespace

// A call on another stream than the handle's previous one first waits for that stream (the handle's scratch is shared).
int keyword_use_stream(rl_keyword_index* kw, hipStream_t s) {
    return kw->last_stream.use(s);
}

// The device half of rl_keyword_search on device pointers (under kw->mu, after keyword_use_stream): d_s / d_c [B x k], d_n [B]
int keyword_search_device(rl_keyword_index* kw, const int64_t* d_off, const int32_t* d_terms, int32_t n_queries, int32_t k, const QueryMask& d_f,
                          float* d_s, int32_t* d_c, int32_t* d_n, hipStream_t s) {
    const int64_t n = kw->n_chunks;
    const size_t n_out = (size_t)n_queries * k;
    if (n == 0) {  // no chunks: every slot is padding
        RL_TRY(launch_fill_f32(d_s, -std::numeric_limits<float>::infinity(), (int64_t)n_out, s));
        RL_HIP(hipMemsetAsync(d_c, 0xff, n_out * sizeof(int32_t), s));
    } else {
        const int64_t ld = (n + 3) & ~int64_t(3);
        // (a sub-batch is one grid row per query: at most 65535 of them)
        const int32_t batch = (int32_t)std::max<int64_t>(1, std::min<int64_t>({(int64_t)n_queries, int64_t(65535),
                                                                                (int64_t)(SCORE_BATCH_BYTES / ((size_t)ld * 4))}));
        RL_TRY(kw->scores.reserve((size_t)batch * ld * sizeof(float)));
        for (int32_t b0 = 0; b0 < n_queries; b0 += batch) {
            const int32_t nb = std::min<int32_t>(batch, n_queries - b0);
            RL_TRY(launch_bm25_score(kw->term_off, kw->post_chunk, kw->post_impact, kw->n_terms, n, d_off + b0, d_terms, nb, d_f.from(b0),
                                     bm25_tile(n, nb, kw->n_cu), kw->scores.as<float>(), ld, s));
            RL_TRY(launch_topk(kw->scores.as<float>(), nb, n, ld, k, kw->ws, d_s + (int64_t)b0 * k, d_c + (int64_t)b0 * k, s));
        }
        RL_TRY(launch_fix_masked(d_s, d_c, (int64_t)n_out, s));  // chunks without a query term are "no hit": (-inf, -1)
    }
    return launch_bm25_count(d_s, n_queries, k, d_n, s);
}

// The chunk bitset each query of a keyword search reads (d_filters [n_filters x (n_chunks + 31) / 32] on the device; query_filter: host,
// nullptr: every query reads bitset 0 when n_filters > 0).  Where every query reads the same bitset, no map goes to the device.
int keyword_mask(rl_keyword_index* kw, const uint32_t* d_filters, int32_t n_filters, const int32_t* query_filter, int32_t B, hipStream_t s,
                 QueryMask* out) {
    *out = QueryMask();
    if (n_filters == 0 || B == 0) return RL_OK;
    if (!query_filter) { *out = QueryMask(d_filters); return RL_OK; }
    const int64_t cw = (kw->n_chunks + 31) / 32;
    if (std::all_of(query_filter, query_filter + B, [&](int32_t f) { return f == query_filter[0]; })) {
        if (query_filter[0] >= 0) *out = QueryMask(d_filters + (int64_t)query_filter[0] * cw);
        return RL_OK;
    }
    RL_TRY(kw->qmap.reserve((size_t)B * sizeof(int32_t)));
    RL_HIP(hipMemcpyAsync(kw->qmap.p, query_filter, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s));  // (pageable: consumed on return)
    *out = QueryMask(d_filters, cw, kw->qmap.as<int32_t>(), nullptr);
    return RL_OK;
}

// q_off as rl_keyword_search states it (host pointers only)
int check_host_q_off(const int64_t* q_off, const int32_t* q_terms, int32_t n_queries, const char* who) {
    if (q_off[0] != 0) return fail(RL_ERR_INVALID, std::string(who) + ": q_off must start at 0");
    for (int32_t b = 0; b < n_queries; ++b)
        if (q_off[b + 1] < q_off[b]) return fail(RL_ERR_INVALID, std::string(who) + ": q_off must be ascending");
    if (q_off[n_queries] > 0 && !q_terms) return fail(RL_ERR_INVALID, std::string(who) + ": null q_terms");
    return RL_OK;
}

namespace {

// A fresh handle with its sizes, the default top-k route and the device's CU count; the arrays are the caller's to fill.
int new_keyword_index(int32_t n_terms, int64_t n_postings, int64_t n_chunks, std::unique_ptr<rl_keyword_index>* out) {
    std::unique_ptr<rl_keyword_index> kw(new rl_keyword_index());
    kw->n_terms = n_terms;
    kw->n_postings = n_postings;
    kw->n_chunks = n_chunks;
    kw->ws.block_route = (int)default_option(RL_OPT_TOPK_BLOCK);
    RL_TRY(device_cu_count(&kw->n_cu));
    *out = std::move(kw);
    return RL_OK;
}

}  // namespace
}  // namespace rl

extern "C" {

int rl_keyword_index_create(rl_keyword_index** out, const int64_t* term_off, int32_t n_terms, const int32_t* post_chunk, const int32_t* post_tf,
                            const int32_t* post_term, int64_t n_postings, const float* idf, const float* nrm, int64_t n_chunks, int mem,
                            void* stream) {
    const char* who = "rl_keyword_index_create";
    if (!out) return fail(RL_ERR_INVALID, "rl_keyword_index_create: null output handle");
    *out = nullptr;
    if (n_terms < 0 || n_postings < 0 || n_chunks < 0) return fail(RL_ERR_INVALID, "rl_keyword_index_create: negative size");
    if (n_chunks >= (int64_t)0x7fffffff - 1) return fail(RL_ERR_UNSUPPORTED, "rl_keyword_index_create: more than 2^31-2 chunks");
    if (!term_off || (n_postings > 0 && (!post_chunk || !post_tf || !post_term)) || (n_terms > 0 && !idf) || (n_chunks > 0 && !nrm))
        return fail(RL_ERR_INVALID, "rl_keyword_index_create: null argument");
    RL_TRY(check_mem(mem, "rl_keyword_index_create"));
    if (mem == RL_MEM_HOST) RL_TRY(check_host_postings(term_off, n_terms, post_chunk, post_tf, post_term, n_postings, n_chunks));
    hipStream_t s = as_stream(stream);
    std::unique_ptr<rl_keyword_index> kw;
    RL_TRY(new_keyword_index(n_terms, n_postings, n_chunks, &kw));
    const size_t np = (size_t)n_postings;
    RL_TRY(kw->term_off.alloc((size_t)(n_terms + 1) * sizeof(int64_t), who));
    RL_TRY(kw->post_chunk.alloc(std::max<size_t>(np * sizeof(int32_t), 16), who));
    RL_TRY(kw->post_impact.alloc(std::max<size_t>(np * sizeof(float), 16), who));
    RL_HIP(hipMemcpyAsync(kw->term_off, term_off, (size_t)(n_terms + 1) * sizeof(int64_t),
                          mem == RL_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
    if (np) RL_HIP(hipMemcpyAsync(kw->post_chunk, post_chunk, np * sizeof(int32_t), mem == RL_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
    Staging st(mem, s);
    const int32_t *d_tf, *d_term;
    const float *d_idf, *d_nrm;
    RL_TRY(st.in(post_tf, np, &d_tf));
    RL_TRY(st.in(post_term, np, &d_term));
    RL_TRY(st.in(idf, (size_t)n_terms, &d_idf));
    RL_TRY(st.in(nrm, (size_t)n_chunks, &d_nrm));
    RL_TRY(launch_bm25_impact(kw->post_chunk, d_tf, d_term, d_idf, d_nrm, n_postings, n_terms, n_chunks, kw->post_impact, s));
    RL_TRY(st.sync());  // the staging buffers and the caller's arrays may go away after return
    *out = kw.release();
    return RL_OK;
}

int rl_keyword_index_destroy(rl_keyword_index* kw) {
    if (!kw) return RL_OK;
    delete kw;
    return RL_OK;
}

int rl_keyword_index_info(const rl_keyword_index* kw, int32_t* n_terms, int64_t* n_postings, int64_t* n_chunks) {
    if (!kw) return fail(RL_ERR_INVALID, "rl_keyword_index_info: null index");
    if (n_terms) *n_terms = kw->n_terms;
    if (n_postings) *n_postings = kw->n_postings;
    if (n_chunks) *n_chunks = kw->n_chunks;
    return RL_OK;
}

int rl_keyword_index_read(const rl_keyword_index* kw, int64_t* term_off, int32_t* post_chunk, float* post_impact, int mem, void* stream) {
    if (!kw) return fail(RL_ERR_INVALID, "rl_keyword_index_read: null index");
    RL_TRY(check_mem(mem, "rl_keyword_index_read"));
    hipStream_t s = as_stream(stream);
    const hipMemcpyKind kind = mem == RL_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    const size_t np = (size_t)kw->n_postings;
    if (term_off) RL_HIP(hipMemcpyAsync(term_off, kw->term_off, (size_t)(kw->n_terms + 1) * sizeof(int64_t), kind, s));
    if (post_chunk && np) RL_HIP(hipMemcpyAsync(post_chunk, kw->post_chunk, np * sizeof(int32_t), kind, s));
    if (post_impact && np) RL_HIP(hipMemcpyAsync(post_impact, kw->post_impact, np * sizeof(float), kind, s));
    if (mem == RL_MEM_HOST) RL_HIP(hipStreamSynchronize(s));
    return RL_OK;
}

}  // extern "C"

// ---- keyword store: the chunks' term ids on the device, and the postings built from them (kernels in keyword_build.hip) -------------
struct rl_keyword_store {
    int64_t n_chunks = 0, n_tokens = 0, n_live = 0;
    int64_t cap_off = 0, cap_live = 0, cap_tokens = 0;  // items the three arrays can hold
    int32_t max_id = -1;                  // the largest term id ever stored
    rl::DevArray<int64_t> tok_off;        // [n_chunks + 1]
    rl::DevArray<int32_t> tok_term;       // [n_tokens]
    rl::DevArray<uint8_t> live;           // [n_chunks]: 1 = live
    std::vector<uint8_t> h_live;          // host copy of `live`
    std::mutex mu;
    // what rl_keyword_store_count left for rl_keyword_store_build (dropped by an append or a delete)
    bool counted = false;
    int32_t c_terms = 0;
    int64_t c_postings = 0, c_chunks = 0;
    rl::DevArray<int64_t> term_off;       // fresh per count: these two become the index' own
    rl::DevArray<int32_t> post_chunk;
    rl::DevArray<int32_t> post_term, post_tf;  // [c_postings], kept with the scratch below
    // Scratch of count, kept between calls with amortised capacity (an insert changes every size a little, and allocating ~24 B per
    // token afresh costs more than the kernels: DESIGN.md 4.12): lengths, their scan, the scan levels, the (key, value) planes of the
    // sort, its (digit, block) table, the head counts and positions, df
    rl::Pool lens, offs, scan_scratch, sortbuf, table, heads, head_pos, df;
    void drop_count() {
        counted = false;
        term_off.release();
        post_chunk.release();
    }
    size_t device_bytes() const {
        return tok_off.cap + tok_term.cap + live.cap + term_off.cap + post_term.cap + post_chunk.cap + post_tf.cap + lens.cap + offs.cap +
               scan_scratch.cap + sortbuf.cap + table.cap + heads.cap + head_pos.cap + df.cap;
    }
};

extern "C" {

int rl_keyword_store_create(rl_keyword_store** out) {
    if (!out) return fail(RL_ERR_INVALID, "rl_keyword_store_create: null output handle");
    *out = new rl_keyword_store();
    return RL_OK;
}

int rl_keyword_store_destroy(rl_keyword_store* st) {
    if (!st) return RL_OK;
    delete st;
    return RL_OK;
}

int rl_keyword_store_info(const rl_keyword_store* st, int64_t* n_chunks, int64_t* n_live, int64_t* n_tokens, int64_t* device_bytes) {
    if (!st) return fail(RL_ERR_INVALID, "rl_keyword_store_info: null store");
    std::lock_guard<std::mutex> lock(const_cast<rl_keyword_store*>(st)->mu);
    if (n_chunks) *n_chunks = st->n_chunks;
    if (n_live) *n_live = st->n_live;
    if (n_tokens) *n_tokens = st->n_tokens;
    if (device_bytes) *device_bytes = (int64_t)st->device_bytes();
    return RL_OK;
}

int rl_keyword_store_append(rl_keyword_store* st, const int32_t* term_ids, const int64_t* offsets, int64_t n_new_chunks, int mem, void* stream) {
    const char* who = "rl_keyword_store_append";
    if (!st) return fail(RL_ERR_INVALID, std::string(who) + ": null store");
    if (n_new_chunks < 0) return fail(RL_ERR_INVALID, std::string(who) + ": negative size");
    RL_TRY(check_mem(mem, who));
    if (n_new_chunks == 0) return RL_OK;
    if (!offsets) return fail(RL_ERR_INVALID, std::string(who) + ": null offsets");
    hipStream_t s = as_stream(stream);
    const hipMemcpyKind in_kind = mem == RL_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    std::vector<int64_t> h_off((size_t)n_new_chunks + 1);
    if (mem == RL_MEM_HOST) std::memcpy(h_off.data(), offsets, h_off.size() * sizeof(int64_t));
    else {
        RL_TRY(hip_status(hipMemcpyAsync(h_off.data(), offsets, h_off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s), who));
        RL_TRY(hip_status(hipStreamSynchronize(s), who));
    }
    if (h_off[0] != 0) return fail(RL_ERR_INVALID, std::string(who) + ": offsets must start at 0");
    for (int64_t c = 0; c < n_new_chunks; ++c)
        if (h_off[c + 1] < h_off[c]) return fail(RL_ERR_INVALID, std::string(who) + ": offsets must be ascending");
    const int64_t n_add = h_off[n_new_chunks];
    if (n_add > 0 && !term_ids) return fail(RL_ERR_INVALID, std::string(who) + ": null term_ids");
    int32_t range[2] = {std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min()};  // min, max of the new ids
    if (mem == RL_MEM_HOST) {
        for (int64_t i = 0; i < n_add; ++i) {
            range[0] = std::min(range[0], term_ids[i]);
            range[1] = std::max(range[1], term_ids[i]);
        }
    } else if (n_add > 0) {
        Staging up(RL_MEM_HOST, s);
        const int32_t* d_range;
        RL_TRY(up.in(range, 2, &d_range));
        RL_TRY(launch_kb_minmax(term_ids, n_add, const_cast<int32_t*>(d_range), s));  // (folds the ids into the staged copy, which is this call's own)
        RL_TRY(hip_status(hipMemcpyAsync(range, d_range, sizeof(range), hipMemcpyDeviceToHost, s), who));
        RL_TRY(hip_status(hipStreamSynchronize(s), who));
        up.drain();
    }
    if (n_add > 0 && range[0] < 0) return fail(RL_ERR_INVALID, std::string(who) + ": negative term id");
    std::lock_guard<std::mutex> lock(st->mu);
    if (st->n_chunks + n_new_chunks >= (int64_t)0x7fffffff - 1) return fail(RL_ERR_UNSUPPORTED, std::string(who) + ": more than 2^31-2 chunks");
    RL_TRY(store_grow(st->tok_off, &st->cap_off, st->n_chunks ? st->n_chunks + 1 : 0, st->n_chunks + n_new_chunks + 1, s, who));
    RL_TRY(store_grow(st->live, &st->cap_live, st->n_chunks, st->n_chunks + n_new_chunks, s, who));
    RL_TRY(store_grow(st->tok_term, &st->cap_tokens, st->n_tokens, st->n_tokens + n_add, s, who));
    for (int64_t& o : h_off) o += st->n_tokens;  // (h_off[0] is what tok_off[n_chunks] holds already, or the first 0)
    RL_TRY(hip_status(hipMemcpyAsync(st->tok_off + st->n_chunks, h_off.data(), h_off.size() * sizeof(int64_t), hipMemcpyHostToDevice, s), who));
    if (n_add > 0) RL_TRY(hip_status(hipMemcpyAsync(st->tok_term + st->n_tokens, term_ids, (size_t)n_add * sizeof(int32_t), in_kind, s), who));
    RL_TRY(hip_status(hipMemsetAsync(st->live + st->n_chunks, 1, (size_t)n_new_chunks, s), who));
    RL_TRY(hip_status(hipStreamSynchronize(s), who));  // the caller's arrays and h_off may go away after return
    st->h_live.resize((size_t)(st->n_chunks + n_new_chunks), 1);
    st->n_chunks += n_new_chunks;
    st->n_live += n_new_chunks;
    st->n_tokens += n_add;
    if (n_add > 0) st->max_id = std::max(st->max_id, range[1]);
    st->drop_count();
    return RL_OK;
}

int rl_keyword_store_delete(rl_keyword_store* st, const int64_t* chunk_ordinals, int64_t n, void* stream) {
    const char* who = "rl_keyword_store_delete";
    if (!st) return fail(RL_ERR_INVALID, std::string(who) + ": null store");
    if (n < 0 || (n > 0 && !chunk_ordinals)) return fail(RL_ERR_INVALID, std::string(who) + ": bad ordinals");
    hipStream_t s = as_stream(stream);
    std::lock_guard<std::mutex> lock(st->mu);
    for (int64_t i = 0; i < n; ++i)
        if (chunk_ordinals[i] < 0 || chunk_ordinals[i] >= st->n_chunks) return fail(RL_ERR_INVALID, std::string(who) + ": chunk ordinal out of range");
    if (n == 0) return RL_OK;
    st->drop_count();  // (any delete, even of dead chunks alone, asks for a new count)
    // the touched range of the live bytes goes up before the host copy changes: a failure leaves the store as it was
    int64_t lo = st->n_chunks, hi = -1, gone = 0;
    for (int64_t i = 0; i < n; ++i) {  // (deleting a dead chunk is a no-op, as in rl_index_delete_chunks)
        if (!st->h_live[(size_t)chunk_ordinals[i]]) continue;
        lo = std::min(lo, chunk_ordinals[i]);
        hi = std::max(hi, chunk_ordinals[i]);
    }
    if (hi < 0) return RL_OK;
    std::vector<uint8_t> range(st->h_live.begin() + lo, st->h_live.begin() + hi + 1);
    for (int64_t i = 0; i < n; ++i) {
        if (chunk_ordinals[i] < lo || chunk_ordinals[i] > hi) continue;  // (dead already: every live one lies in [lo, hi])
        uint8_t& flag = range[(size_t)(chunk_ordinals[i] - lo)];
        gone += flag;
        flag = 0;
    }
    RL_TRY(hip_status(hipMemcpyAsync(st->live + lo, range.data(), range.size(), hipMemcpyHostToDevice, s), who));
    RL_TRY(hip_status(hipStreamSynchronize(s), who));
    std::copy(range.begin(), range.end(), st->h_live.begin() + lo);
    st->n_live -= gone;
    return RL_OK;
}

int rl_keyword_store_count(rl_keyword_store* st, const int32_t* term_rank, int32_t n_terms, int64_t* out_df, int64_t* out_length,
                           int64_t out_totals[3], int mem, void* stream) {
    const char* who = "rl_keyword_store_count";
    if (!st) return fail(RL_ERR_INVALID, std::string(who) + ": null store");
    if (n_terms < 0) return fail(RL_ERR_INVALID, std::string(who) + ": negative size");
    RL_TRY(check_mem(mem, who));
    hipStream_t s = as_stream(stream);
    std::lock_guard<std::mutex> lock(st->mu);
    if ((int64_t)st->max_id >= (int64_t)n_terms) return fail(RL_ERR_INVALID, std::string(who) + ": the store holds a term id >= n_terms");
    if (term_rank && mem == RL_MEM_HOST) {
        std::vector<bool> seen((size_t)n_terms, false);
        for (int32_t t = 0; t < n_terms; ++t) {
            if (term_rank[t] < 0 || term_rank[t] >= n_terms || seen[(size_t)term_rank[t]])
                return fail(RL_ERR_INVALID, std::string(who) + ": term_rank must be a permutation of [0, n_terms)");
            seen[(size_t)term_rank[t]] = true;
        }
    }
    st->drop_count();
    const hipMemcpyKind out_kind = mem == RL_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    const int64_t n = st->n_chunks;
    int64_t m = 0, np = 0;  // live tokens, postings
    Pool &lens = st->lens, &offs = st->offs, &scan_scratch = st->scan_scratch;  // (kept by the store: see its declaration)
    if (n > 0) {
        RL_TRY(reserve_amortised(lens, (size_t)n * sizeof(int64_t), who));
        RL_TRY(reserve_amortised(offs, (size_t)n * sizeof(int64_t), who));
        RL_TRY(reserve_amortised(scan_scratch, kb_scan_scratch_items(n) * sizeof(int64_t), who));
        RL_TRY(launch_kb_lengths(st->tok_off, st->live, n, lens.as<int64_t>(), s));
        RL_HIP(hipMemcpyAsync(offs.p, lens.p, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
        const int64_t* d_total;
        RL_TRY(launch_kb_exclusive_scan(offs.as<int64_t>(), n, scan_scratch.as<int64_t>(), &d_total, s));
        RL_HIP(hipMemcpyAsync(&m, d_total, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        RL_HIP(hipStreamSynchronize(s));
        if (m < 0 || m > st->n_tokens) return fail(RL_ERR_HIP, std::string(who) + ": inconsistent token count");
    }
    DevArray<int64_t> term_off;
    DevArray<int32_t> post_chunk;
    DevArray<int32_t>&post_term = st->post_term, &post_tf = st->post_tf;
    Pool& df = st->df;
    RL_TRY(term_off.alloc((size_t)(n_terms + 1) * sizeof(int64_t), who));
    RL_TRY(reserve_amortised(df, std::max<size_t>((size_t)n_terms * sizeof(int64_t), 16), who));
    if (m > 0) {
        Pool &sortbuf = st->sortbuf, &table = st->table, &heads = st->heads, &head_pos = st->head_pos;
        Staging up(mem, s);
        const int32_t* d_rank = nullptr;
        if (term_rank) RL_TRY(up.in(term_rank, (size_t)n_terms, &d_rank));
        const size_t plane = ((size_t)m * 4 + 255) & ~size_t(255);
        RL_TRY(reserve_amortised(sortbuf, 4 * plane, who));  // keys and values, twice: the passes go back and forth
        uint32_t* keys[2] = {reinterpret_cast<uint32_t*>(sortbuf.as<char>()), reinterpret_cast<uint32_t*>(sortbuf.as<char>() + 2 * plane)};
        int32_t* vals[2] = {reinterpret_cast<int32_t*>(sortbuf.as<char>() + plane), reinterpret_cast<int32_t*>(sortbuf.as<char>() + 3 * plane)};
        const int64_t table_items = 256 * kb_sort_blocks(m);
        RL_TRY(reserve_amortised(table, (size_t)table_items * sizeof(int64_t), who));
        RL_TRY(reserve_amortised(scan_scratch, std::max(kb_scan_scratch_items(table_items), kb_scan_scratch_items(kb_rle_blocks(m))) * sizeof(int64_t), who));
        RL_TRY(launch_kb_emit(st->tok_off, st->tok_term, st->live, offs.as<int64_t>(), d_rank, n_terms, n, st->n_tokens, m, keys[0], vals[0], s));
        int at = 0;
        for (int pass = 0; pass < kb_sort_passes(n_terms); ++pass, at ^= 1)
            RL_TRY(launch_kb_sort_pass(keys[at], vals[at], m, pass, table.as<int64_t>(), scan_scratch.as<int64_t>(), keys[at ^ 1], vals[at ^ 1], s));
        RL_TRY(reserve_amortised(heads, (size_t)kb_rle_blocks(m) * sizeof(int64_t), who));
        RL_TRY(launch_kb_rle_count(keys[at], vals[at], m, heads.as<int64_t>(), s));
        const int64_t* d_total;
        RL_TRY(launch_kb_exclusive_scan(heads.as<int64_t>(), kb_rle_blocks(m), scan_scratch.as<int64_t>(), &d_total, s));
        RL_HIP(hipMemcpyAsync(&np, d_total, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        RL_HIP(hipStreamSynchronize(s));
        if (np < 1 || np > m) return fail(RL_ERR_HIP, std::string(who) + ": inconsistent posting count");
        RL_TRY(reserve_amortised(post_term, (size_t)np * sizeof(int32_t), who));
        RL_TRY(post_chunk.alloc((size_t)np * sizeof(int32_t), who));
        RL_TRY(reserve_amortised(post_tf, (size_t)np * sizeof(int32_t), who));
        RL_TRY(reserve_amortised(head_pos, (size_t)np * sizeof(int64_t), who));
        RL_TRY(launch_kb_rle_write(keys[at], vals[at], m, heads.as<int64_t>(), np, post_term, post_chunk, post_tf, head_pos.as<int64_t>(), s));
        RL_TRY(launch_kb_term_off(post_term, np, n_terms, term_off, df.as<int64_t>(), s));
        RL_TRY(up.sync());  // the staged term_rank goes with this scope
    } else {  // no chunks, or no live tokens: what rl_keyword_index_create holds for empty arrays
        RL_TRY(reserve_amortised(post_term, 16, who));
        RL_TRY(post_chunk.alloc(16, who));
        RL_TRY(reserve_amortised(post_tf, 16, who));
        RL_HIP(hipMemsetAsync(term_off.p, 0, (size_t)(n_terms + 1) * sizeof(int64_t), s));
        RL_HIP(hipMemsetAsync(df.p, 0, std::max<size_t>((size_t)n_terms * sizeof(int64_t), 16), s));
    }
    if (out_df && n_terms > 0) RL_HIP(hipMemcpyAsync(out_df, df.p, (size_t)n_terms * sizeof(int64_t), out_kind, s));
    if (out_length && n > 0) RL_HIP(hipMemcpyAsync(out_length, lens.p, (size_t)n * sizeof(int64_t), out_kind, s));
    const int64_t totals[3] = {st->n_live, m, np};
    if (out_totals) {
        if (mem == RL_MEM_HOST) std::memcpy(out_totals, totals, sizeof(totals));
        else RL_HIP(hipMemcpyAsync(out_totals, totals, sizeof(totals), hipMemcpyHostToDevice, s));
    }
    RL_HIP(hipStreamSynchronize(s));  // `totals` goes with this frame
    st->term_off = std::move(term_off);
    st->post_chunk = std::move(post_chunk);
    st->c_terms = n_terms;
    st->c_postings = np;
    st->c_chunks = n;
    st->counted = true;
    return RL_OK;
}

int rl_keyword_store_build(rl_keyword_store* st, const float* idf, const float* nrm, rl_keyword_index** out, int mem, void* stream) {
    const char* who = "rl_keyword_store_build";
    if (!out) return fail(RL_ERR_INVALID, std::string(who) + ": null output handle");
    *out = nullptr;
    if (!st) return fail(RL_ERR_INVALID, std::string(who) + ": null store");
    RL_TRY(check_mem(mem, who));
    hipStream_t s = as_stream(stream);
    std::lock_guard<std::mutex> lock(st->mu);
    if (!st->counted)
        return fail(RL_ERR_INVALID, std::string(who) + ": no rl_keyword_store_count since the store was created, appended to, deleted from or built");
    if ((st->c_terms > 0 && !idf) || (st->c_chunks > 0 && !nrm)) return fail(RL_ERR_INVALID, std::string(who) + ": null argument");
    std::unique_ptr<rl_keyword_index> kw;
    RL_TRY(new_keyword_index(st->c_terms, st->c_postings, st->c_chunks, &kw));
    RL_TRY(kw->post_impact.alloc(std::max<size_t>((size_t)st->c_postings * sizeof(float), 16), who));
    Staging up(mem, s);
    const float *d_idf, *d_nrm;
    RL_TRY(up.in(idf, (size_t)st->c_terms, &d_idf));
    RL_TRY(up.in(nrm, (size_t)st->c_chunks, &d_nrm));
    RL_TRY(launch_bm25_impact(st->post_chunk, st->post_tf, st->post_term, d_idf, d_nrm, st->c_postings, st->c_terms, st->c_chunks, kw->post_impact, s));
    RL_TRY(up.sync());  // the staging buffers and the caller's arrays may go away after return
    kw->term_off = std::move(st->term_off);  // the counted postings become the index: no copy
    kw->post_chunk = std::move(st->post_chunk);
    st->drop_count();
    *out = kw.release();
    return RL_OK;
}

}  // extern "C"

// ---- keyword analyzer: chunk bodies -> stable term ids on the device (kernels in keyword_analyze.hip) ----------------------------------
struct rl_keyword_analyzer {
    std::mutex mu;
    int hash_bits = 0;
    int64_t n_table = 0;
    int32_t n_stop = 0, stop_max_len = 0;
    rl::DevArray<uint32_t> table;      // [n_table] the fold table
    rl::DevArray<uint8_t> stop_bytes;  // the stopwords, sorted, as symbols 0 .. 25
    rl::DevArray<int32_t> stop_off;    // [n_stop + 1]
    // what the last rl_keyword_analyze_begin left (sizes 0 until then)
    bool begun = false, finished = false;
    int64_t n_texts = 0, m = 0, n_tok = 0, n_kept = 0, n_distinct = 0, n_bytes = 0, cap = 0;
    // device arrays of a call, kept between calls with amortised capacity
    rl::Pool count, scan_scratch, sym, start, letter, stem, head, ftext_off, tok_pos, tok_len, tok_hash, tok_slot, slots, kept, first, dist_tok,
        dist_first, dist_len, dist_bytes, term_ids, offsets;
};

namespace rl {
namespace {

// the exclusive scan of data [n] in place and its total, copied to *total_host (valid after the next synchronisation of `s`)
int ka_scan(rl_keyword_analyzer* a, int64_t* data, int64_t n, int64_t* total_host, hipStream_t s, const char* who) {
    RL_TRY(reserve_amortised(a->scan_scratch, kb_scan_scratch_items(n) * sizeof(int64_t), who));
    const int64_t* total = nullptr;
    RL_TRY(launch_kb_exclusive_scan(data, n, a->scan_scratch.as<int64_t>(), &total, s));
    RL_TRY(hip_status(hipMemcpyAsync(total_host, total, sizeof(int64_t), hipMemcpyDeviceToHost, s), who));
    return RL_OK;
}

}  // namespace
}  // namespace rl

extern "C" {

int rl_keyword_analyzer_create(rl_keyword_analyzer** out, const uint32_t* fold_table, int64_t n_table, const char* stopwords,
                               const int64_t* stop_off, int32_t n_stop, int32_t hash_bits) {
    const char* who = "rl_keyword_analyzer_create";
    if (!out) return fail(RL_ERR_INVALID, std::string(who) + ": null output handle");
    *out = nullptr;
    if (!fold_table || n_table < 1 || n_table > (int64_t(1) << 21)) return fail(RL_ERR_INVALID, std::string(who) + ": bad fold table");
    if (n_stop < 0 || (n_stop > 0 && (!stopwords || !stop_off))) return fail(RL_ERR_INVALID, std::string(who) + ": bad stopword list");
    if (hash_bits < 0 || hash_bits > 64) return fail(RL_ERR_INVALID, std::string(who) + ": hash_bits must be 0 .. 64");
    for (int64_t i = 0; i < n_table; ++i) {  // every field a symbol + 1 (<= 29), no symbol behind an empty field, nothing above the fields
        uint32_t e = fold_table[i];
        bool ended = false;
        for (int j = 0; j < KA_IMAGE_MAX; ++j, e >>= 5) {
            const uint32_t f = e & 31u;
            if (f > 29u || (ended && f)) return fail(RL_ERR_INVALID, std::string(who) + ": malformed fold table entry");
            ended |= f == 0;
        }
        if (e) return fail(RL_ERR_INVALID, std::string(who) + ": malformed fold table entry");
    }
    // the words that a token can equal (a-z only, non-empty), sorted and distinct, as symbols
    std::vector<std::string> words;
    for (int32_t i = 0; i < n_stop; ++i) {
        if (stop_off[i] < 0 || stop_off[i + 1] < stop_off[i]) return fail(RL_ERR_INVALID, std::string(who) + ": stopword offsets must ascend from 0");
        std::string w(stopwords + stop_off[i], (size_t)(stop_off[i + 1] - stop_off[i]));
        bool ok = !w.empty();
        for (char& c : w) {
            ok = ok && c >= 'a' && c <= 'z';
            c = (char)(c - 'a');
        }
        if (ok) words.push_back(std::move(w));
    }
    std::sort(words.begin(), words.end());
    words.erase(std::unique(words.begin(), words.end()), words.end());
    std::vector<int32_t> h_off(words.size() + 1, 0);
    std::string h_bytes;
    size_t longest = 0;
    for (size_t i = 0; i < words.size(); ++i) {
        h_bytes += words[i];
        h_off[i + 1] = (int32_t)h_bytes.size();
        longest = std::max(longest, words[i].size());
    }
    std::unique_ptr<rl_keyword_analyzer> a(new rl_keyword_analyzer());
    a->hash_bits = hash_bits == 64 ? 0 : hash_bits;
    a->n_table = n_table;
    a->n_stop = (int32_t)words.size();
    a->stop_max_len = (int32_t)longest;
    RL_TRY(a->table.alloc((size_t)n_table * sizeof(uint32_t), who));
    RL_TRY(a->stop_bytes.alloc(std::max<size_t>(h_bytes.size(), 16), who));
    RL_TRY(a->stop_off.alloc(h_off.size() * sizeof(int32_t), who));
    RL_TRY(hip_status(hipMemcpy(a->table.p, fold_table, (size_t)n_table * sizeof(uint32_t), hipMemcpyHostToDevice), who));
    if (!h_bytes.empty()) RL_TRY(hip_status(hipMemcpy(a->stop_bytes.p, h_bytes.data(), h_bytes.size(), hipMemcpyHostToDevice), who));
    RL_TRY(hip_status(hipMemcpy(a->stop_off.p, h_off.data(), h_off.size() * sizeof(int32_t), hipMemcpyHostToDevice), who));
    *out = a.release();
    return RL_OK;
}

int rl_keyword_analyzer_destroy(rl_keyword_analyzer* a) {
    if (!a) return RL_OK;
    delete a;
    return RL_OK;
}

int rl_keyword_analyze_begin(rl_keyword_analyzer* a, const uint32_t* codepoints, const int64_t* text_off, int64_t n, int64_t n_texts,
                             int64_t out_counts[5], int mem, void* stream) {
    const char* who = "rl_keyword_analyze_begin";
    if (!a) return fail(RL_ERR_INVALID, std::string(who) + ": null analyzer");
    if (n < 0 || n_texts < 0) return fail(RL_ERR_INVALID, std::string(who) + ": negative size");
    RL_TRY(check_mem(mem, who));
    if (!text_off) return fail(RL_ERR_INVALID, std::string(who) + ": null text_off");
    if (n > 0 && !codepoints) return fail(RL_ERR_INVALID, std::string(who) + ": null codepoints");
    if (n > 0 && n_texts < 1) return fail(RL_ERR_INVALID, std::string(who) + ": code points without a text");
    if (n >= (int64_t(1) << 40)) return fail(RL_ERR_UNSUPPORTED, std::string(who) + ": more than 2^40 code points in one call");
    if (mem == RL_MEM_HOST) {
        if (text_off[0] != 0) return fail(RL_ERR_INVALID, std::string(who) + ": text_off must start at 0");
        for (int64_t t = 0; t < n_texts; ++t)
            if (text_off[t + 1] < text_off[t]) return fail(RL_ERR_INVALID, std::string(who) + ": text_off must be ascending");
        if (text_off[n_texts] != n) return fail(RL_ERR_INVALID, std::string(who) + ": text_off must end at n");
    }
    hipStream_t s = as_stream(stream);
    std::lock_guard<std::mutex> lock(a->mu);
    a->begun = a->finished = false;
    a->n_texts = n_texts;
    a->m = a->n_tok = a->n_kept = a->n_distinct = a->n_bytes = a->cap = 0;
    Staging st(mem, s);
    const uint32_t* d_cp;
    const int64_t* d_off;
    RL_TRY(st.in(codepoints, (size_t)n, &d_cp));
    RL_TRY(st.in(text_off, (size_t)n_texts + 1, &d_off));
    // 1. fold
    RL_TRY(reserve_amortised(a->count, (size_t)(n + 1) * sizeof(int64_t), who));
    RL_TRY(launch_ka_fold_count(d_cp, n, a->table, a->n_table, a->count.as<int64_t>(), s));
    int64_t m = 0, n_tok = 0, n_kept = 0, n_distinct = 0, n_bytes = 0;
    RL_TRY(ka_scan(a, a->count.as<int64_t>(), n + 1, &m, s, who));
    RL_TRY(hip_status(hipStreamSynchronize(s), who));
    const int64_t* sym_off = a->count.as<int64_t>();
    const size_t m_bytes = std::max<size_t>((size_t)m, 16);
    RL_TRY(reserve_amortised(a->sym, m_bytes, who));
    RL_TRY(reserve_amortised(a->start, m_bytes, who));
    RL_TRY(reserve_amortised(a->letter, m_bytes, who));
    RL_TRY(reserve_amortised(a->stem, m_bytes, who));
    RL_TRY(reserve_amortised(a->head, (size_t)(m + 1) * sizeof(int64_t), who));
    RL_TRY(reserve_amortised(a->ftext_off, (size_t)(n_texts + 1) * sizeof(int64_t), who));
    RL_TRY(hip_status(hipMemsetAsync(a->start.p, 0, m_bytes, s), who));
    RL_TRY(launch_ka_fold_write(d_cp, n, a->table, a->n_table, sym_off, m, a->sym.as<uint8_t>(), s));
    RL_TRY(launch_ka_text_starts(d_off, n_texts, n, sym_off, m, a->ftext_off.as<int64_t>(), a->start.as<uint8_t>(), s));
    // 2. tokenize
    RL_TRY(launch_ka_heads(a->sym.as<uint8_t>(), a->start.as<uint8_t>(), m, a->letter.as<uint8_t>(), a->head.as<int64_t>(), s));
    RL_TRY(ka_scan(a, a->head.as<int64_t>(), m + 1, &n_tok, s, who));
    RL_TRY(hip_status(hipStreamSynchronize(s), who));
    if (n_tok > 0) {
        // 3. stem
        const int64_t cap = ka_table_slots(n_tok);
        RL_TRY(reserve_amortised(a->tok_pos, (size_t)n_tok * sizeof(int64_t), who));
        RL_TRY(reserve_amortised(a->tok_len, (size_t)n_tok * sizeof(int64_t), who));
        RL_TRY(reserve_amortised(a->tok_hash, (size_t)n_tok * sizeof(uint64_t), who));
        RL_TRY(reserve_amortised(a->tok_slot, (size_t)n_tok * sizeof(int64_t), who));
        RL_TRY(reserve_amortised(a->kept, (size_t)(n_tok + 1) * sizeof(int64_t), who));
        RL_TRY(reserve_amortised(a->first, (size_t)(n_tok + 1) * sizeof(int64_t), who));
        RL_TRY(reserve_amortised(a->slots, (size_t)cap * sizeof(uint64_t), who));
        RL_TRY(launch_ka_stem(a->sym.as<uint8_t>(), a->letter.as<uint8_t>(), a->start.as<uint8_t>(), a->head.as<int64_t>(), m, n_tok, a->stop_bytes,
                              a->stop_off, a->n_stop, a->stop_max_len, a->hash_bits, a->tok_pos.as<int64_t>(), a->stem.as<uint8_t>(),
                              a->tok_len.as<int64_t>(), a->tok_hash.as<uint64_t>(), s));
        // 4. distinct
        RL_TRY(launch_ka_distinct(a->stem.as<uint8_t>(), a->tok_pos.as<int64_t>(), a->tok_len.as<int64_t>(), a->tok_hash.as<uint64_t>(), n_tok,
                                  a->slots.as<uint64_t>(), cap, a->tok_slot.as<int64_t>(), a->kept.as<int64_t>(), a->first.as<int64_t>(), s));
        RL_TRY(ka_scan(a, a->kept.as<int64_t>(), n_tok + 1, &n_kept, s, who));
        RL_TRY(ka_scan(a, a->first.as<int64_t>(), n_tok + 1, &n_distinct, s, who));
        RL_TRY(hip_status(hipStreamSynchronize(s), who));
        RL_TRY(reserve_amortised(a->dist_tok, std::max<size_t>((size_t)n_distinct * sizeof(int64_t), 16), who));
        RL_TRY(reserve_amortised(a->dist_first, std::max<size_t>((size_t)n_distinct * sizeof(int64_t), 16), who));
        RL_TRY(reserve_amortised(a->dist_len, (size_t)(n_distinct + 1) * sizeof(int64_t), who));
        RL_TRY(launch_ka_distinct_out(a->tok_len.as<int64_t>(), a->tok_slot.as<int64_t>(), a->slots.as<uint64_t>(), cap, n_tok, a->kept.as<int64_t>(),
                                      a->first.as<int64_t>(), n_distinct, a->dist_tok.as<int64_t>(), a->dist_first.as<int64_t>(),
                                      a->dist_len.as<int64_t>(), s));
        RL_TRY(ka_scan(a, a->dist_len.as<int64_t>(), n_distinct + 1, &n_bytes, s, who));
        RL_TRY(hip_status(hipStreamSynchronize(s), who));
        RL_TRY(reserve_amortised(a->dist_bytes, std::max<size_t>((size_t)n_bytes, 16), who));
        RL_TRY(launch_ka_distinct_bytes(a->stem.as<uint8_t>(), a->tok_pos.as<int64_t>(), a->tok_len.as<int64_t>(), a->dist_tok.as<int64_t>(),
                                        a->dist_len.as<int64_t>(), n_distinct, n_bytes, a->dist_bytes.as<uint8_t>(), s));
        RL_TRY(hip_status(hipStreamSynchronize(s), who));
        a->cap = cap;
    }
    st.drain();  // (the stream has been synchronised above)
    a->m = m;
    a->n_tok = n_tok;
    a->n_kept = n_kept;
    a->n_distinct = n_distinct;
    a->n_bytes = n_bytes;
    a->begun = true;
    if (out_counts) {
        out_counts[0] = n_kept;
        out_counts[1] = n_distinct;
        out_counts[2] = n_bytes;
        out_counts[3] = m;
        out_counts[4] = n_tok;
    }
    return RL_OK;
}

int rl_keyword_analyze_stems(rl_keyword_analyzer* a, uint8_t* stem_bytes, int64_t* stem_off, int64_t* first_pos, int mem, void* stream) {
    const char* who = "rl_keyword_analyze_stems";
    if (!a) return fail(RL_ERR_INVALID, std::string(who) + ": null analyzer");
    RL_TRY(check_mem(mem, who));
    hipStream_t s = as_stream(stream);
    std::lock_guard<std::mutex> lock(a->mu);
    if (!a->begun) return fail(RL_ERR_INVALID, std::string(who) + ": no rl_keyword_analyze_begin before it");
    const hipMemcpyKind kind = mem == RL_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    const size_t nd = (size_t)a->n_distinct;
    if (a->n_tok == 0) {  // (no token: the device arrays were not written)
        if (stem_off && mem == RL_MEM_HOST) stem_off[0] = 0;
        else if (stem_off) RL_TRY(hip_status(hipMemsetAsync(stem_off, 0, sizeof(int64_t), s), who));
    } else {
        if (stem_bytes && a->n_bytes) RL_TRY(hip_status(hipMemcpyAsync(stem_bytes, a->dist_bytes.p, (size_t)a->n_bytes, kind, s), who));
        if (stem_off) RL_TRY(hip_status(hipMemcpyAsync(stem_off, a->dist_len.p, (nd + 1) * sizeof(int64_t), kind, s), who));
        if (first_pos && nd) RL_TRY(hip_status(hipMemcpyAsync(first_pos, a->dist_first.p, nd * sizeof(int64_t), kind, s), who));
    }
    RL_TRY(hip_status(hipStreamSynchronize(s), who));
    return RL_OK;
}

int rl_keyword_analyze_finish(rl_keyword_analyzer* a, const int32_t* ids, int mem, const int32_t** term_ids, const int64_t** offsets, void* stream) {
    const char* who = "rl_keyword_analyze_finish";
    if (!a) return fail(RL_ERR_INVALID, std::string(who) + ": null analyzer");
    RL_TRY(check_mem(mem, who));
    hipStream_t s = as_stream(stream);
    std::lock_guard<std::mutex> lock(a->mu);
    if (!a->begun) return fail(RL_ERR_INVALID, std::string(who) + ": no rl_keyword_analyze_begin before it");
    if (a->n_distinct > 0 && !ids) return fail(RL_ERR_INVALID, std::string(who) + ": null ids");
    if (mem == RL_MEM_HOST)
        for (int64_t d = 0; d < a->n_distinct; ++d)
            if (ids[d] < 0) return fail(RL_ERR_INVALID, std::string(who) + ": negative term id");
    a->finished = false;
    RL_TRY(reserve_amortised(a->term_ids, std::max<size_t>((size_t)a->n_kept * sizeof(int32_t), 16), who));
    RL_TRY(reserve_amortised(a->offsets, (size_t)(a->n_texts + 1) * sizeof(int64_t), who));
    Staging st(mem, s);
    const int32_t* d_ids;
    RL_TRY(st.in(ids, (size_t)a->n_distinct, &d_ids));
    if (a->n_tok > 0) {
        // 5. emit
        RL_TRY(launch_ka_emit(a->tok_len.as<int64_t>(), a->tok_slot.as<int64_t>(), a->slots.as<uint64_t>(), a->cap, a->n_tok, a->kept.as<int64_t>(),
                              a->first.as<int64_t>(), d_ids, a->n_distinct, a->n_kept, a->term_ids.as<int32_t>(), s));
        RL_TRY(launch_ka_offsets(a->ftext_off.as<int64_t>(), a->n_texts, a->head.as<int64_t>(), a->m, a->kept.as<int64_t>(), a->n_tok,
                                 a->offsets.as<int64_t>(), s));
    } else {
        RL_TRY(hip_status(hipMemsetAsync(a->offsets.p, 0, (size_t)(a->n_texts + 1) * sizeof(int64_t), s), who));
    }
    RL_TRY(hip_status(hipStreamSynchronize(s), who));  // the staging buffer and the caller's ids may go away after return
    st.drain();
    a->finished = true;
    if (term_ids) *term_ids = a->term_ids.as<int32_t>();
    if (offsets) *offsets = a->offsets.as<int64_t>();
    return RL_OK;
}

int rl_keyword_analyze_result(rl_keyword_analyzer* a, int32_t* term_ids, int64_t* offsets, int mem, void* stream) {
    const char* who = "rl_keyword_analyze_result";
    if (!a) return fail(RL_ERR_INVALID, std::string(who) + ": null analyzer");
    RL_TRY(check_mem(mem, who));
    hipStream_t s = as_stream(stream);
    std::lock_guard<std::mutex> lock(a->mu);
    if (!a->finished) return fail(RL_ERR_INVALID, std::string(who) + ": no rl_keyword_analyze_finish before it");
    const hipMemcpyKind kind = mem == RL_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (term_ids && a->n_kept) RL_TRY(hip_status(hipMemcpyAsync(term_ids, a->term_ids.p, (size_t)a->n_kept * sizeof(int32_t), kind, s), who));
    if (offsets) RL_TRY(hip_status(hipMemcpyAsync(offsets, a->offsets.p, (size_t)(a->n_texts + 1) * sizeof(int64_t), kind, s), who));
    RL_TRY(hip_status(hipStreamSynchronize(s), who));
    return RL_OK;
}

}  // extern "C"

namespace {
// rl_keyword_search and rl_keyword_search_per_query: one device path
int keyword_search_call(rl_keyword_index* kw, const int64_t* q_off, const int32_t* q_terms, int32_t n_queries, int32_t k,
                        const uint32_t* chunk_filters, int32_t n_filters, const int32_t* query_filter, float* out_scores, int32_t* out_chunks,
                        int32_t* out_counts, int mem, void* stream, const char* who) {
    if (!kw) return fail(RL_ERR_INVALID, std::string(who) + ": null index");
    if (n_queries < 0 || k < 1) return fail(RL_ERR_INVALID, std::string(who) + ": n_queries must be >= 0 and k >= 1");
    if (k > K_MAX) return fail(RL_ERR_UNSUPPORTED, std::string(who) + ": k must be <= 2048");
    if (n_queries == 0) return RL_OK;
    if (!q_off) return fail(RL_ERR_INVALID, std::string(who) + ": null q_off");
    if (!out_scores || !out_chunks) return fail(RL_ERR_INVALID, std::string(who) + ": null output");
    const int fmem = filters_mem(mem);
    mem = args_mem(mem);
    int64_t n_q_terms = 0;
    if (mem == RL_MEM_HOST) {
        RL_TRY(check_host_q_off(q_off, q_terms, n_queries, who));
        n_q_terms = q_off[n_queries];
    } else if (!q_terms) {
        return fail(RL_ERR_INVALID, std::string(who) + ": null q_terms");
    }
    hipStream_t s = as_stream(stream);
    std::lock_guard<std::mutex> lock(kw->mu);
    RL_TRY(keyword_use_stream(kw, s));
    const int64_t n = kw->n_chunks;
    const size_t n_out = (size_t)n_queries * k;
    Staging st(mem, s);
    const int64_t* d_off;
    const int32_t* d_terms;
    const uint32_t* d_f = nullptr;
    float* d_s;
    int32_t *d_c, *d_n;
    RL_TRY(st.in(q_off, (size_t)n_queries + 1, &d_off));
    if (mem == RL_MEM_HOST) RL_TRY(st.in(q_terms, (size_t)n_q_terms, &d_terms));
    else d_terms = q_terms;
    if (n_filters) RL_TRY(st.in(chunk_filters, (size_t)n_filters * ((n + 31) / 32), &d_f, fmem));
    QueryMask mask;
    RL_TRY(keyword_mask(kw, d_f, n_filters, query_filter, n_queries, s, &mask));
    RL_TRY(st.out(out_scores, n_out, &d_s));
    RL_TRY(st.out(out_chunks, n_out, &d_c));
    RL_TRY(st.out_or_temp(out_counts, (size_t)n_queries, &d_n));
    RL_TRY(keyword_search_device(kw, d_off, d_terms, n_queries, k, mask, d_s, d_c, d_n, s));
    return st.finish();
}
}  // namespace

extern "C" {

int rl_keyword_search(rl_keyword_index* kw, const int64_t* q_off, const int32_t* q_terms, int32_t n_queries, int32_t k,
                      const uint32_t* chunk_filter, float* out_scores, int32_t* out_chunks, int32_t* out_counts, int mem, void* stream) {
    return keyword_search_call(kw, q_off, q_terms, n_queries, k, chunk_filter, chunk_filter ? 1 : 0, nullptr, out_scores, out_chunks,
                               out_counts, mem, stream, "rl_keyword_search");
}

int rl_keyword_search_per_query(rl_keyword_index* kw, const int64_t* q_off, const int32_t* q_terms, int32_t n_queries, int32_t k,
                                const uint32_t* chunk_filters, int32_t n_filters, const int32_t* query_filter, float* out_scores,
                                int32_t* out_chunks, int32_t* out_counts, int mem, void* stream) {
    const char* who = "rl_keyword_search_per_query";
    RL_TRY(check_query_filters(n_queries, chunk_filters, n_filters, query_filter, nullptr, who));
    return keyword_search_call(kw, q_off, q_terms, n_queries, k, chunk_filters, query_filter ? n_filters : 0, query_filter, out_scores,
                               out_chunks, out_counts, mem, stream, who);
}

}  // extern "C"
