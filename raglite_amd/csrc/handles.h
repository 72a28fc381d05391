// What the api*.hip files share: the two handle types that more than one of them reads, what those are made of, and
// the prototypes of the functions that cross a file boundary.  Every other handle type is private to the file of its entry points.
// Through device_mem.h also: memory ownership (Pool, DevArray) and how the routes cut a scratch pool into sub-buffers (scratch_layout.h).
#pragma once
#include <limits>
#include <memory>
#include <mutex>
#include <vector>

#include "device_mem.h"
#include "sentencepiece_table.h"

namespace rl {

// RL_MEM_FILTERS_DEVICE or-ed into `mem`: the filter table alone is a device pointer, read in place; every other pointer follows the
// rest of `mem`.  Each entry that takes filters splits `mem` once, into where its filters live and where everything else does.
inline int filters_mem(int mem) { return (mem & RL_MEM_FILTERS_DEVICE) ? RL_MEM_DEVICE : mem; }
inline int args_mem(int mem) { return mem & ~RL_MEM_FILTERS_DEVICE; }

constexpr size_t SCORE_BATCH_BYTES = size_t(8) << 30;  // cap of the [B x N] score scratch per sub-batch

// Route options (raglite_hip.h "options"): per index, copied from the process-wide defaults when the index is created.  The library
// reads no environment variable.
struct Options {
    int64_t v[RL_OPT_PP_LOOP + 1];  // (keys 1 .. RL_OPT_COUNT_ - 1, and the schedule switches from 64 on)
    Options() {
        for (auto& x : v) x = 0;
        v[RL_OPT_HI_SEARCH] = v[RL_OPT_HI_MAXSIM] = v[RL_OPT_HI_PRODUCTS] = v[RL_OPT_PP_PASS] = v[RL_OPT_FUSED_TOPK] = v[RL_OPT_FUSED_HI] = 1;
        v[RL_OPT_FUSED_PP] = v[RL_OPT_GEMM_PASS] = v[RL_OPT_QUERY_PAIRS] = v[RL_OPT_PLANES_GEMM] = v[RL_OPT_KEEP_IMAGE] = v[RL_OPT_KEEP_HI] = 1;
        v[RL_OPT_EXACT_KTH_THRESHOLD] = v[RL_OPT_FUSED_TWO_ROUNDS] = v[RL_OPT_KEEP_HI_PLANE] = v[RL_OPT_F16_EXACT] = v[RL_OPT_LAZY_IMAGES] = v[RL_OPT_FUSED_PP_SAMPLE] = v[RL_OPT_LIST_SELECT] = v[RL_OPT_HI_FEW] = 1;
        v[RL_OPT_TOPK_BLOCK] = v[RL_OPT_PAIRS_PACKED] = 2;
        v[RL_OPT_HI_PIVOT] = 1;
        v[RL_OPT_PP_SCHEDULE] = 1;
        v[RL_OPT_PP_XCD_PASSES] = 2;  // (measured: DESIGN.md 4.1)
        v[RL_OPT_PP_LOOP] = 1;        // (measured: DESIGN.md 4.1)
        v[RL_OPT_IMAGE_HEADROOM_MB] = -1;
        v[RL_OPT_ARITHMETIC] = RL_ARITH_AUTO;
    }
    bool on(int key) const { return v[key] != 0; }
};

// The three derived images of the rows (IMG_* bits): a block, the scale it was built with (0 = no image) and the rows it covers.
struct Image {
    Pool buf;
    float scale = 0.f;
    int64_t rows = 0;
    void drop() {
        buf.release();
        scale = 0.f;
        rows = 0;
    }
    bool covers(float at, int64_t n_rows) const { return scale > 0.f && scale == at && rows == n_rows && n_rows > 0; }
};
// max |e|, max |e_lo|, max |e_lo| / |e|, min |e| over the rows (e_lo: what the HI halves drop), the split scale they were computed at and
// the rows folded in so far: what the error bounds of the half-bytes routes are made of.  min |e| is never raised by deletions (conservative).
struct NormStats {
    float max_row_norm = 0.f, max_lo_norm = 0.f, max_lo_ratio = 0.f;
    float min_row_norm = std::numeric_limits<float>::infinity();
    float max_row_norm_scale = 0.f;
    int64_t max_row_norm_rows = 0;
    void reset() { *this = NormStats(); }
    bool measured(int64_t n_rows) const { return max_row_norm_rows == n_rows && max_row_norm > 0.f; }
};

// The last stream a handle's shared scratch was used on.  Device-mode calls are asynchronous, so a call arriving on a DIFFERENT stream
// than the previous one first waits for that stream (host-side; the rare case).
struct LastStream {
    hipStream_t stream = nullptr;
    bool set = false;
    int use(hipStream_t s) {
        if (set && stream != s) RL_HIP(hipStreamSynchronize(stream));
        stream = s;
        set = true;
        return RL_OK;
    }
};

// The CU count of the current device: what a handle sizes its grids by.
inline int device_cu_count(int* n_cu) {
    int dev = 0;
    RL_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    RL_HIP(hipGetDeviceProperties(&prop, dev));
    *n_cu = prop.multiProcessorCount;
    return RL_OK;
}

// The metadata filters and rank limits of a batch as the host describes them (the chunk bitsets are on the device): query b reads chunk
// bitset filter_of(b) (-1: none) and cuts at limit_of(b) (n_rows: no cut).  The single-filter entry points give n <= 1 and no arrays.
struct BatchFilters {
    const uint32_t* chunk_bits = nullptr;  // device [n x (n_chunks + 31) / 32]
    int32_t n = 0;
    const int32_t* qf = nullptr;   // host [B]: each query's bitset (-1: none); nullptr: every query reads bitset 0 (when n > 0)
    const int64_t* lim = nullptr;  // host [B]: each query's rank limit (0: no cut); nullptr: every query `limit`
    int64_t limit = 0;
    int32_t filter_of(int32_t b) const { return n == 0 ? -1 : qf ? qf[b] : 0; }
    int64_t limit_of(int32_t b, int64_t n_rows) const {
        const int64_t L = lim ? lim[b] : limit;
        return L > 0 && L < n_rows ? L : n_rows;
    }
};

}  // namespace rl

struct rl_index {
    const float* E = nullptr;       // fp32 storage ...
    const uint16_t* E16 = nullptr;  // ... or IEEE fp16 storage (rl_index_create_f16); exactly one is set: the caller's rows or `owned_rows`
    rl::Pool owned_rows;            // the rows when the index owns them (copied from the host, appended to, compacted)
    bool owns_E() const { return owned_rows.p != nullptr; }
    int64_t n_rows = 0;
    int32_t dim = 0;
    int64_t n_chunks = 0;
    int metric = RL_COSINE;
    bool has_empty_chunk = false;
    rl::DevArray<int64_t> offsets;       // device [n_chunks + 1]
    rl::DevArray<int32_t> row_to_chunk;  // device [n_rows + 65]
    rl::DevArray<float> norm;            // device [n_rows]  (cosine)
    rl::DevArray<float> sumsq;           // device [n_rows]  (l2)
    int n_cu = 256;
    // Lock orders, for the calls that hold two handles: idx->mu, then kw->mu (the hybrid and rerank calls); idx->mu, then the metadata
    // store's (rl_metadata_filters: the chunk offsets must not move under the launch).  Never the other way round.
    std::mutex mu;
    rl::SelectWorkspace ws;
    rl::Pool scores;                  // [B x ld] similarity scratch / chunk scores
    rl::Pool hits;                    // search_chunks: [B x num_hits] (score, row)
    rl::Pool misc;
    // lifecycle (append / delete / filter)
    int64_t cap_rows = 0;                 // rows the owned buffers (E, norm, sumsq, row_to_chunk) can hold
    int64_t cap_chunks = 0;               // chunks the device CSR can hold
    std::vector<int64_t> h_offsets;       // host copy of the CSR
    std::vector<uint32_t> h_live;         // host bitset over chunks: 1 = live (empty until the first delete)
    rl::DevArray<uint32_t> live_chunk_bits;  // device copy of h_live (empty: every chunk is live)
    rl::DevArray<uint32_t> live_row_bits;    // the same expanded to rows
    int64_t n_dead_chunks = 0, n_dead_rows = 0;
    rl::Pool maskbuf;                     // per-call row masks (the distinct filters of a sub-batch) and the query -> mask map
    rl::Pool qsplit;                      // fp16 (hi, lo) query fragments of a MaxSim batch (maxsim_stream.hip)
    // SPLIT arithmetic of the stream kernel (fp32 storage only): range of the row norms, and what follows from it
    rl::DevArray<uint32_t> d_range;       // device scratch of launch_row_range
    float max_abs = 0.f, min_row_max = std::numeric_limits<float>::infinity();  // over rows that are not all zero
    bool nonfinite = false;
    int arithmetic = RL_ARITH_AUTO;
    float split_scale = 0.f;              // > 0: power of two applied to the corpus inside the kernel; 0: exact fp32 MFMAs
    // Pre-split corpus image of maxsim_gemm.hip (fp16 hi | lo planes in the kernel's LDS layout, 4 B per element) and
    // the "last row of its chunk" bitmap; built with the index, extended on append, rebuilt when split_scale changes.
    rl::Image planes;
    rl::Pool ends, qplanes;
    rl::Pool q32;                         // rl_maxsim_topk_batch_f16: the fp16 queries widened to fp32 (what the query-side kernels read)
    rl::Pool cand;                        // rl_maxsim_rerank: sanitised candidate ordinals
    rl::Pool fused;                       // fused batched top-k: sample scores, thresholds, candidate lists, counters
    rl::Pool pp_work;                     // ... on the sixteen-group tile: wave-private record logs, block norm ranges (maxsim_pp.hip MODE 2)
    rl::Pool rankbuf;                     // rank cut (order-first-then-filter): histogram levels + tie counts
    rl::Pool hybrid;                      // rl_hybrid_search: the ranked lists the fusion reads, their scores and counts
    rl::Pool rerank;                      // rl_search_rerank_per_query: the fused candidates, their fused and MaxSim scores, positions
    rl::Pool ragged;                      // rl_maxsim_rerank_ragged's backstop: one (query, slab)'s scores
    // HI plane (round 2): fp16(e * split_scale) rounded to nearest (toward zero until round 3), row-major [n_rows x dim] -- the hi halves of the fp16
    // split as a matrix of their own, 2 B per element: what the single-query search streams (search_rows_hi).
    rl::Image hiplane;
    rl::Pool hibuf;
    // ... and the same halves in the one-plane IMAGE layout (maxsim_gemm.hip HALF): what the approximate MaxSim pass of a
    // batch multiplies (maxsim_batch_hi); the row-norm statistics are for the error bounds of both
    rl::Image hi_image;
    rl::NormStats norm_stats;
    rl::DevArray<uint32_t> d_norms;       // device scratch of launch_max_row_norm (4 words)
    // The scratch above is shared by all calls on this handle; `mu` serialises only their host side.
    rl::LastStream last_stream;
    int64_t ends_rows = -1;               // rows the `ends` bitmap covers (-1: not built); kept by both images
    // What the last bound-filtered search on this handle left behind (rl_index_filter_stats): per-query candidate counters and the
    // device flag its guarded full-precision fallback waits on.  Pointers into the scratch above, valid until the next call.
    // rl_rank_cut_*: the staged rank cut of a SHARDED corpus keeps its queries and scores here between the calls
    int32_t rank_B = 0;                   // queries of the running rl_rank_cut_begin (0: none)
    bool scores_direct = false;           // the scores score_rows left in `scores` came from the VALU scan: l2 summed (e - q)^2 directly (select_from_scores)
    int32_t mb_B = 0, mb_nq = 0, mb_k = 0;  // rl_maxsim_batch_begin in progress: queries, vectors per query, k (0: none)
    uint64_t scratch_epoch = 0, mb_epoch = 0;  // calls that used the scratch so far; the value right after that rl_maxsim_batch_begin
    rl::Pool rank_q;                      // their device copy (the l2 re-scoring of rl_rank_cut_finish needs them)
    struct FilterRecord { int kind = 0; int32_t n = 0, cap = 0; const uint32_t* cnt = nullptr; const uint32_t* flag = nullptr; } filt;
    rl::Options opt;                      // route options (rl_index_set_option)
    // RL_OPT_LAZY_IMAGES (round 5, the default): an image is built by the first call whose route reads it -- which images this index
    // has been asked for so far (IMG_* bits); with the option off every image the KEEP_* options allow is built with the index
    uint32_t demanded = 0;
    uint32_t no_room = 0;                 // IMG_* bits whose last build was skipped because it would not have left the headroom free
    uint64_t no_room_retry_epoch = 0;     // ... and the scratch epoch from which demand_images asks for them again
    // ... and a pinned host word every bound-filtered MaxSim batch copies its fallback flag to when it is done (asynchronously): a batch
    // that finds the previous one fell back asks for the pre-split image, so that an index whose data keeps defeating the bound runs its
    // full-precision passes through the eight-query kernel instead of the streaming kernels (3-4 x faster) from the second batch on
    std::unique_ptr<uint32_t, hipError_t (*)(void*)> h_fell_back{nullptr, hipHostFree};
    uint32_t* d_fell_back = nullptr;  // the device's view of that word (written by guarded_select_kernel)
    // rl_time_kernel kind 8: what the candidate pass of the last fused-HI row search ran with (pointers into misc / fused / pp_work: valid
    // while those pools have not been re-reserved, which `pools` pins down)
    struct FusedReplay {
        bool valid = false, pp = false, row_test = false; int32_t B = 0, log_cap = 0; int mode = 0; float* qs = nullptr; rl::CandArgs ca{}; uint32_t* cnt = nullptr;
        const float* thr1 = nullptr; int64_t round1_tiles = 0;  // two-round candidate pass: the first round's thresholds and tiles
        const void* pools[3] = {nullptr, nullptr, nullptr};
    } replay;
    ~rl_index() { rl::select_workspace_free(ws); }  // (every other member frees itself)
};

// ---- BM25 keyword search (include/raglite_hip.h; kernels in keyword.hip) -------------------------------------------------------
struct rl_keyword_index {
    int32_t n_terms = 0;
    int64_t n_postings = 0;
    int64_t n_chunks = 0;
    int n_cu = 256;
    rl::DevArray<int64_t> term_off;     // [n_terms + 1]
    rl::DevArray<int32_t> post_chunk;   // [n_postings], ascending within a term
    rl::DevArray<float> post_impact;    // [n_postings]
    std::mutex mu;
    rl::SelectWorkspace ws;
    rl::Pool scores;                    // [B x ld] chunk scores of a (sub-)batch
    rl::Pool qmap;                      // [B] the chunk bitset of each query of a per-query filtered call
    rl::LastStream last_stream;         // (the scratch above is shared by all calls on this handle)
    ~rl_keyword_index() { rl::select_workspace_free(ws); }
};

// ---- native encoder forward (include/raglite_hip.h; kernels in encoder.hip, entry points in api_ingest.hip) -----------------------
struct rl_encoder {
    int32_t vocab = 0, hidden = 0, layers = 0, heads = 0, ffn = 0, max_positions = 0, type_vocab = 0, dtype = 0;
    float eps = 0.f;
    const void *tok = nullptr, *pos = nullptr, *typ = nullptr, *ln_w = nullptr, *ln_b = nullptr;  // borrowed, like everything in `layer`
    struct Layer { const void *qkv_w, *qkv_b, *out_w, *out_b, *ln1_w, *ln1_b, *up_w, *up_b, *down_w, *down_b, *ln2_w, *ln2_b; };
    std::vector<Layer> layer;
    const void *pooler_w = nullptr, *pooler_b = nullptr, *head_w = nullptr, *head_b = nullptr;  // rl_encoder_set_head: borrowed; all null = no head
    int32_t ksplit = 1;          // the larger of the out and down projections' K slices: what `part` of the scratch is sized by
    std::mutex mu;
    rl::Pool scratch;             // rl::EncoderScratch over RL_ENCODER_MAX_TOKENS rows; every call walks a prefix of it
    rl::LastStream last_stream;
};

// ---- SentencePiece Unigram on the device (include/raglite_hip.h; kernels in sentencepiece.hip, entry points in api_ingest.hip) --------
struct rl_sentencepiece {
    std::mutex mu;
    int hash_bits = 0;
    int64_t n_table = 0, n_pool = 0, n_pieces = 0, n_slots = 0, table_bytes = 0;
    int32_t longest = 0, unk_id = 0;
    float unk_score = 0.f;
    rl::DevArray<int32_t> image_off;    // [n_table]
    rl::DevArray<uint8_t> image_len;    // [n_table]
    rl::DevArray<uint32_t> image_pool;  // [n_pool]
    rl::DevArray<uint32_t> piece_cp;    // the kept pieces' code points, back to back
    rl::DevArray<int32_t> piece_off;    // [n_pieces + 1]
    rl::DevArray<uint8_t> piece_flags;  // [n_pieces], all 0: no piece is a continuation
    rl::DevArray<int32_t> piece_ids;    // [n_pieces]
    rl::DevArray<float> piece_scores;   // [n_pieces]
    rl::DevArray<int32_t> slots;        // [n_slots]
    // what the last rl_sentencepiece_encode left (nothing until then)
    bool encoded = false;
    int64_t n_texts = 0, n_tokens = 0;
    // device arrays of a call, kept between calls with amortised capacity
    rl::Pool count, scan_scratch, raw, start, rtext_off, keep, sym, sym_off, bp_start, bp_id, tmp, tok_count, ids, offsets, status, counters;
    rl::LastStream last_stream;
    rl::SpImage image() const { return {image_off, image_len, image_pool, n_table, n_pool}; }
    rl::SpTable table() const { return {{piece_cp, piece_off, piece_flags, slots, n_slots, hash_bits}, piece_scores, piece_ids}; }
};

namespace rl {

// The process-wide default of a route option (api.hip keeps the table and its mutex to itself).
int64_t default_option(int key);

// api.hip, for the files that drive an rl_index from outside: the argument checks take no lock; use_scratch, then the *_device
// functions, under idx->mu
int use_scratch(rl_index* idx, hipStream_t s);
int check_search_args(const rl_index* idx, const float* q, int32_t B, int32_t k, const char* who);
int check_query_filters(int32_t B, const uint32_t* chunk_filters, int32_t n_filters, const int32_t* query_filter, const int64_t* rank_limits,
                        const char* who);
int search_chunks_device(rl_index* idx, const float* d_q, int32_t B, int32_t num_hits, int32_t k, const BatchFilters& f,
                         float* d_s, int32_t* d_c, int32_t* d_n, hipStream_t s);
int maxsim_rerank_device(rl_index* idx, const float* d_q, int32_t n_queries, int32_t nq, const int32_t* d_c, int32_t n_cand, float* d_o,
                         hipStream_t s);
// ... with a number of vectors per query: check_qv_off takes no lock and makes no HIP call (qv_off: HOST memory); the device half takes
// the table on both sides
int check_qv_off(const int64_t* qv_off, int32_t n_queries, const char* who);
int maxsim_rerank_ragged_device(rl_index* idx, const float* d_q, const int64_t* h_qv_off, const int64_t* d_qv_off, int32_t n_queries,
                                const int32_t* d_c, int32_t n_cand, float* d_o, hipStream_t s, const char* who);

// api_keyword.hip, for the hybrid and rerank calls: check_host_q_off takes no lock; keyword_use_stream, then the other two, under kw->mu
int keyword_use_stream(rl_keyword_index* kw, hipStream_t s);
int keyword_mask(rl_keyword_index* kw, const uint32_t* d_filters, int32_t n_filters, const int32_t* query_filter, int32_t B, hipStream_t s,
                 QueryMask* out);
int keyword_search_device(rl_keyword_index* kw, const int64_t* d_off, const int32_t* d_terms, int32_t n_queries, int32_t k, const QueryMask& d_f,
                          float* d_s, int32_t* d_c, int32_t* d_n, hipStream_t s);
int check_host_q_off(const int64_t* q_off, const int32_t* q_terms, int32_t n_queries, const char* who);

}  // namespace rl
