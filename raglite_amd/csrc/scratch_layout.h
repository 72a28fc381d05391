// How the search routes cut their device scratch blocks (the index's grow-only pools) into sub-buffers.  Plain C++ with no HIP
// dependency, so that tests/test_scratch_layout_host.py compiles this same code on the host, under the sanitizers, and checks every
// layout for alignment, bounds and overlap.
//
// One walk gives size and pointers: a layout is a struct of typed pointers with one function, lay(Carver, sizes...), that takes its
// sub-buffers front to back and returns the bytes walked.  Over no block (Carver()) that is the size to reserve; over the reserved block
// it fills the pointers (rl::carve in device_mem.h does both).  There is no second formula.
// Contiguity a kernel or a memset relies on is ONE take with named offsets inside it (Carver::sub), never two takes: every take starts on
// its own 16-byte boundary.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace rl {

struct Carver {
    uintptr_t base;  // 0: the sizing walk (every take returns nullptr; offsets are integers, nothing is added to a null pointer)
    size_t off = 0, align;  // align: 16 everywhere in the library (the host test also walks search_rows_hi at 4, the layout that had the bug)
    explicit Carver(void* block = nullptr, size_t align_ = 16) : base(reinterpret_cast<uintptr_t>(block)), align(align_) {}
    template <class T>
    T* take(size_t count) {  // the next `count` items of T, on a boundary of max(align, alignof(T)) bytes from the block's start
        const size_t a = align > alignof(T) ? align : alignof(T);
        off = (off + a - 1) / a * a;
        const size_t at = off;
        off += count * sizeof(T);
        return base ? reinterpret_cast<T*>(base + at) : nullptr;
    }
    template <class T>
    static T* sub(T* p, size_t i) { return p ? p + i : nullptr; }  // a named offset inside one take
};

// ---- owned by a launcher: the callers read into them -----------------------------------------------------------------------------------
// The query side of the row-score modes, written by launch_score_planes_queries (maxsim_gemm.hip), read by the passes of maxsim_gemm.hip
// and maxsim_pp.hip and by search_rows_fused_hi.  score_planes_scratch_floats() is this walk.
struct ScoreQueries {
    float *frag, *unscale, *anylo, *q_sumsq;  // fragments (dim * 32 per group of 32 queries), [nb] 2^(ex - 14), [groups], [nb] |q|^2
    size_t lay(Carver c, size_t nb, size_t dim) {
        const size_t groups = (nb + 31) / 32;
        frag = c.take<float>(groups * 32 * dim);
        unscale = c.take<float>(nb);
        anylo = c.take<float>(groups);
        q_sumsq = c.take<float>(nb);
        c.take<float>(64);  // (slack behind the last array, as the formula always had)
        return c.off;
    }
};
// The query image of the MaxSim passes, written by launch_query_planes (maxsim_gemm.hip).  query_planes_bytes() is this walk.
struct QueryPlanes {
    char* frag;    // dim * 128 bytes per query
    float* meta;   // [2 n] per query: 2^(ex - 14), any lo half != 0
    float* qsum;   // [2 n] per query: sum_i |q_i|, sum_i |q_lo,i|
    size_t lay(Carver c, size_t n_queries, size_t dim) {
        frag = c.take<char>(n_queries * dim * 128);
        meta = c.take<float>(2 * n_queries);
        qsum = c.take<float>(2 * n_queries);
        c.take<char>(64);
        return c.off;
    }
};

// ---- row search (api.hip) ---------------------------------------------------------------------------------------------------------------
struct FusedRows {  // search_rows_fused, pool `fused`
    float *S_s, *top_s, *c_s;  // [B x ld_s] sample scores, [B x k] their top-k, [B x cap] candidate scores
    int32_t *top_i, *c_i;
    uint32_t *cnt, *flag;      // [B] list lengths, then the overflow flag (16 words): ONE take -- a single memset clears cnt[0 .. B]
    size_t lay(Carver c, size_t B, size_t ld_s, size_t k, size_t cap) {
        S_s = c.take<float>(B * ld_s);
        top_s = c.take<float>(B * k);
        top_i = c.take<int32_t>(B * k);
        c_s = c.take<float>(B * cap);
        c_i = c.take<int32_t>(B * cap);
        cnt = c.take<uint32_t>(B + 16);
        flag = Carver::sub(cnt, B);
        return c.off;
    }
};
struct FusedHiRows : FusedRows {  // search_rows_fused_hi, pool `fused`: FusedRows' lists, then
    int32_t* r_i;                 // [B x cap2] rows to re-score
    float *r_s, *thr, *window, *thr1;  // [B x cap2] their exact similarities; [B] thresholds, windows, the first round's thresholds
    uint32_t* cnt2;               // [B]  (row_threshold_kernel clears cnt[b], cnt2[b] and the flag word one by one: no adjacency needed;
                                  // cnt and flag stay FusedRows' one take)
    size_t lay(Carver c, size_t B, size_t ld_s, size_t k, size_t cap, size_t cap2) {
        c.off = FusedRows::lay(c, B, ld_s, k, cap);
        r_i = c.take<int32_t>(B * cap2);
        r_s = c.take<float>(B * cap2);
        thr = c.take<float>(B);
        window = c.take<float>(B);
        thr1 = c.take<float>(B);
        cnt2 = c.take<uint32_t>(B);
        return c.off;
    }
};
struct HiRows {  // search_rows_hi, pool `hibuf`; nc = nb * cap candidates
    float *ts, *thr, *mb;  // [nb x k] approximate top-k; 16 words of thresholds; 16 words: each query's error bound
    int32_t *ti, *ci;      // [nb x k]; [nc] candidate rows
    float *gn, *G;         // [nc] their norms; [nc x dim] the gathered rows -- the kernels that score them take 16-byte loads: misaligned, the
                           // stream kernel declines and the scan sums in another order than the full pass (odd nb * k, before the takes aligned)
    float *xs, *es;        // [nb x nc] the exact score block; [nc] its diagonal
    uint32_t *cnt, *flag;  // ONE take of 32 words, flag = cnt + 16: launch_transform_hist / launch_pivot_route clear cnt[0 .. 32)
    uint64_t* bmax;        // [n_bmax] group maxima of the pivot route (pivot_scratch_words)
    size_t lay(Carver c, size_t nb, size_t k, size_t dim, size_t cap, size_t n_bmax) {
        const size_t nc = nb * cap;
        ts = c.take<float>(nb * k);
        ti = c.take<int32_t>(nb * k);
        thr = c.take<float>(16);
        mb = c.take<float>(16);
        cnt = c.take<uint32_t>(32);
        flag = Carver::sub(cnt, 16);
        ci = c.take<int32_t>(nc);
        gn = c.take<float>(nc);
        G = c.take<float>(nc * dim);
        xs = c.take<float>(nb * nc);
        es = c.take<float>(nc);
        bmax = c.take<uint64_t>(n_bmax);
        return c.off;
    }
};
struct L2Rescore {  // the l2 re-scoring of select_from_scores, pool `misc`: [items] each
    float* re;
    int32_t *pos, *tmp_rows;
    size_t lay(Carver c, size_t items) {
        re = c.take<float>(items);
        pos = c.take<int32_t>(items);
        tmp_rows = c.take<int32_t>(items);
        return c.off;
    }
};
struct RowMasks {  // search_rows_device, pool `maskbuf`
    uint32_t* row_sets;  // [most x rw] the row bitsets of a sub-batch's distinct filters
    int32_t* d_map;      // [most + 2 batch] the maps a sub-batch uploads in one copy: filter ids, query -> bitset, limits
    size_t lay(Carver c, size_t most, size_t rw, size_t batch) {
        row_sets = c.take<uint32_t>(most * rw);
        d_map = c.take<int32_t>(most + 2 * batch);
        return c.off;
    }
};

// ---- MaxSim (api.hip) -------------------------------------------------------------------------------------------------------------------
struct HiBatchScratch {  // the bound-filtered MaxSim batch of n queries, pool `hibuf` (the same in every call that works on the batch)
    float *ts, *thr, *es, *m, *es_top;  // [n x k] approximate top-k; [n]; [n x cap] exact scores; [n] bounds; [n x k] exact scores of ts
    int32_t *ti, *ci;                   // [n x k]; [n x cap] candidate chunks
    uint32_t *cnt, *flag;  // ONE take of n + 16 words, flag = cnt + n: the pivot route clears n + 16 words from cnt; launch_scale_f32,
                           // gemm_prepare and a memset clear the 16 flag words
    uint64_t* bmax;        // [n_bmax] group maxima of the few-queries pivot route
    size_t lay(Carver c, size_t n, size_t k, size_t cap, size_t n_bmax) {
        ts = c.take<float>(n * k);
        ti = c.take<int32_t>(n * k);
        thr = c.take<float>(n);
        cnt = c.take<uint32_t>(n + 16);
        flag = Carver::sub(cnt, n);
        ci = c.take<int32_t>(n * cap);
        es = c.take<float>(n * cap);
        m = c.take<float>(n);
        es_top = c.take<float>(n * k);
        bmax = c.take<uint64_t>(n_bmax);
        return c.off;
    }
};
struct ApproxBound {  // the bound of rl_maxsim_approx_scores, pool `hibuf`
    float *top, *thr;      // [n] "k-th best" = 0; [n] 0 - 2 m
    uint32_t *cnt, *flag;  // [n]; 16 words
    size_t lay(Carver c, size_t n) {
        top = c.take<float>(n);
        thr = c.take<float>(n);
        cnt = c.take<uint32_t>(n);
        flag = c.take<uint32_t>(16);
        return c.off;
    }
};

// ---- retrieval (api_retrieval.hip) ------------------------------------------------------------------------------------------------------
struct HybridLists {  // hybrid_search_device, pool `hybrid`: R = 1 (vector search) or 2 (+ keyword search), list r at r * B * n_each
    int32_t *lists, *counts;  // [R x B x n_each] what the fusion reads; [R x B]
    float* scores;            // [R x B x n_each]
    size_t lay(Carver c, size_t R, size_t B, size_t n_each) {
        lists = c.take<int32_t>(R * B * n_each);
        scores = c.take<float>(R * B * n_each);
        counts = c.take<int32_t>(R * B);
        return c.off;
    }
};
struct RerankScratch {  // search_rerank_device, pool `rerank`
    double* fused_scores;                // [B x n_cand]
    int32_t *fused, *fused_counts, *pos;  // [B x n_cand] candidates; [B]; [B x k] positions of the first k
    float *maxsim, *own_scores;          // [B x n_cand] MaxSim scores; [B x k] where the caller takes no scores, else nullptr
    size_t lay(Carver c, size_t B, size_t n_cand, size_t k, bool keep_scores) {
        fused_scores = c.take<double>(B * n_cand);
        fused = c.take<int32_t>(B * n_cand);
        maxsim = c.take<float>(B * n_cand);
        fused_counts = c.take<int32_t>(B);
        pos = c.take<int32_t>(B * k);
        own_scores = keep_scores ? c.take<float>(B * k) : nullptr;
        return c.off;
    }
};

struct RaggedScratch {  // maxsim_rerank_ragged_device, pool `ragged`
    float* slab;  // [n_cand] the backstop's scores of one (query, slab), summed into the result before the next one overwrites them
    size_t lay(Carver c, size_t n_cand) {
        slab = c.take<float>(n_cand);
        return c.off;
    }
};

// ---- native encoder forward (api_ingest.hip, encoder.hip) -------------------------------------------------------------------------------
struct EncoderScratch {  // rl_encoder_forward, the handle's one block: reserved for RL_ENCODER_MAX_TOKENS rows, walked per call with the
                         // call's own `rows`, so that a call writes a prefix of the block and nothing behind it.  rl_encoder_forward_pack
                         // walks the same layout over the caller's workspace, with up to RL_ENCODER_MAX_PACK_TOKENS rows
    uint16_t *x, *x1;    // [rows x hidden] a layer's input; the same after the attention half (ln1)
    uint16_t *qkv, *attn, *mid;  // [rows x 3 hidden] fused projection; [rows x hidden] attention output; [rows x ffn] gelu(up)
    float* part;         // [ksplit x rows x hidden] the K slices of the out / down projections, summed in order by the layer norm
    size_t lay(Carver c, size_t rows, size_t hidden, size_t ffn, size_t ksplit) {
        x = c.take<uint16_t>(rows * hidden);
        x1 = c.take<uint16_t>(rows * hidden);
        qkv = c.take<uint16_t>(rows * 3 * hidden);
        attn = c.take<uint16_t>(rows * hidden);
        mid = c.take<uint16_t>(rows * ffn);
        part = c.take<float>(ksplit * rows * hidden);
        return c.off;
    }
};

struct EncoderClassifyScratch {  // rl_encoder_classify_pack, over the caller's workspace: the pack's own scratch FIRST (so the trunk's
                                 // launches see the block rl_encoder_forward_pack would give them), then the rows the trunk writes and the head reads
    EncoderScratch trunk;
    uint16_t* final_rows;  // [rows x hidden] the last layer's output
    size_t lay(Carver c, size_t rows, size_t hidden, size_t ffn, size_t ksplit) {
        c.off = trunk.lay(c, rows, hidden, ffn, ksplit);
        final_rows = c.take<uint16_t>(rows * hidden);
        return c.off;
    }
};

// ---- Markdown block structure (markdown.hip) ----------------------------------------------------------------------------------------------
struct MarkdownScratch {  // launch_markdown_blocks: n characters in n_docs documents have at most n + n_docs lines
    int32_t *bm, *em, *ts, *sc;  // [lines] the line table: begin, end, first non-space character, indent
    uint8_t* lazy;               // [lines] the quote frame that made the line a lazy continuation
    int32_t* flags;              // [n_docs] undecided before the parse: a foreign line separator, a tab in a line's indent
    int32_t* save;               // [save_entries x 4] the quotes' save stacks: (line, bm, ts, sc)
    int64_t* scan;               // [scan_items] the scratch of the line counts' exclusive scan
    size_t lay(Carver c, size_t n, size_t n_docs, size_t save_entries, size_t scan_items) {
        const size_t lines = n + n_docs;
        bm = c.take<int32_t>(lines);
        em = c.take<int32_t>(lines);
        ts = c.take<int32_t>(lines);
        sc = c.take<int32_t>(lines);
        lazy = c.take<uint8_t>(lines);
        flags = c.take<int32_t>(n_docs);
        save = c.take<int32_t>(save_entries * 4);
        scan = c.take<int64_t>(scan_items);
        return c.off;
    }
};
struct MarkdownKnownScratch {  // launch_markdown_sentence_known: ONE take, cleared by a single memset
    uint8_t *body, *behind;    // [lines] the line is a heading's; the line follows a heading's last
    size_t lay(Carver c, size_t lines) {
        body = c.take<uint8_t>(2 * lines);
        behind = Carver::sub(body, lines);
        return c.off;
    }
};

}  // namespace rl
