// BERT WordPiece on the device (rl_wordpiece_encode / rl_wordpiece_pairs; driven from api_ingest.hip): what the
// `tokenizers` library's BertNormalizer + BertPreTokenizer + WordPiece do for many texts, on their UTF-32 code points, from tables the
// host probed out of that tokenizer (raglite_amd/_wordpiece.py: WordPieceTables.encode_tables states the same algorithm).
//   1. expand   every code point has an image of 0 .. WP_IMAGE_MAX code points (three 21-bit fields of a uint64: code point + 1, 0 = no
//               further one): count, exclusive scan, write -> the normalised stream `sym`, one uint32 per symbol, and its class per
//               symbol.  The count carries a second field from bit 32 up: 1 for a code point whose image may depend on its neighbours
//               (the context flag of `cls`), so the same scan says how many of those lie in front of every code point, and a text
//               that holds one gets status 1
//   2. words    a word is a maximal run of word characters inside one text, or one punctuation symbol; white space separates and is
//               dropped.  Heads are counted, scanned, and every word gets its position
//   3. match    one lane per word: its length (a word of more than max_word_chars symbols is one unk_id), the prefix sums of its
//               polynomial hash in LDS -- one pass, after which the hash of any [start, end) is two loads and a multiply
//               (wordpiece_table.h) -- then greedy longest match from the left, end - start bounded by the longest piece, every hit
//               compared code point by code point.  The ids of word w go to tmp[word_pos .. ) (a word has at most as many pieces as
//               symbols) and their number to tok_count: the matches are made ONCE, the second pass only moves them
//   4. emit     scan of tok_count -> every word's ids to their place, and the texts' token offsets
// Every phase is its own launch: no kernel waits on another workgroup.  The only atomics are integer adds of two counters (unknown
// words, flagged texts): sums, so the same run to run.  Every position is 64-bit and is checked against its array before it is written.
#include "common.h"
#include "wordpiece_table.h"

namespace rl {
namespace {

constexpr int WP_THREADS = 256;
constexpr int WP_MATCH_THREADS = 64;  // one wave: the prefix sums of its 64 words are (max_word_chars + 1) x 64 x 4 bytes of LDS
constexpr uint8_t WP_WORD = 0, WP_SPACE = 1, WP_PUNCT = 2;  // cls & 3
constexpr uint8_t WP_CONTEXT = 4;                           // cls & 4: the image may depend on a neighbour
constexpr int WP_FLAG_SHIFT = 32;
constexpr int64_t WP_LOW = (int64_t(1) << WP_FLAG_SHIFT) - 1;

unsigned wp_blocks(int64_t n, int64_t per) { return (unsigned)((n + per - 1) / per); }

__device__ __forceinline__ uint64_t wp_image(const uint64_t* __restrict__ image, int64_t n_table, uint32_t cp) {
    return (int64_t)cp < n_table ? image[cp] : 0ull;
}
__device__ __forceinline__ uint8_t wp_class(const uint8_t* __restrict__ cls, int64_t n_table, uint32_t c) {
    return (int64_t)c < n_table ? cls[c] : WP_WORD;
}

// count[i] = symbols of code point i + (its context flag << 32) for i < n, count[n] = 0: the scan's last entry is then the length of
// the normalised stream and the number of flagged code points
__global__ __launch_bounds__(WP_THREADS) void wp_expand_count_kernel(const uint32_t* __restrict__ cp, int64_t n, const uint64_t* __restrict__ image,
                                                                      const uint8_t* __restrict__ cls, int64_t n_table, int64_t* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * WP_THREADS + threadIdx.x;
    if (i > n) return;
    int64_t c = 0;
    if (i < n) {
        uint64_t e = wp_image(image, n_table, cp[i]);
        for (; c < WP_IMAGE_MAX && (e & 0x1FFFFFull); ++c) e >>= 21;
        if (wp_class(cls, n_table, cp[i]) & WP_CONTEXT) c |= int64_t(1) << WP_FLAG_SHIFT;
    }
    count[i] = c;
}

// sym [m]: the normalised stream; kind [m]: the class of every symbol (cls & 3)
__global__ __launch_bounds__(WP_THREADS) void wp_expand_write_kernel(const uint32_t* __restrict__ cp, int64_t n, const uint64_t* __restrict__ image,
                                                                      const uint8_t* __restrict__ cls, int64_t n_table,
                                                                      const int64_t* __restrict__ scan, int64_t m, uint32_t* __restrict__ sym,
                                                                      uint8_t* __restrict__ kind) {
    const int64_t i = (int64_t)blockIdx.x * WP_THREADS + threadIdx.x;
    if (i >= n) return;
    uint64_t e = wp_image(image, n_table, cp[i]);
    const int64_t at = scan[i] & WP_LOW;
    for (int j = 0; j < WP_IMAGE_MAX && (e & 0x1FFFFFull); ++j, e >>= 21) {
        const int64_t p = at + j;
        const uint32_t c = (uint32_t)(e & 0x1FFFFFull) - 1u;
        if (p >= 0 && p < m) {
            sym[p] = c;
            kind[p] = wp_class(cls, n_table, c) & 3u;
        }
    }
}

// ftext_off[t] = where text t begins in the normalised stream (t <= n_texts); start[p] = 1 where some text begins (start: zero on entry;
// several texts may begin at one symbol -- empty ones -- and all store the same byte); status[t] = 1: the text holds a flagged code point
__global__ __launch_bounds__(WP_THREADS) void wp_text_kernel(const int64_t* __restrict__ text_off, int64_t n_texts, int64_t n,
                                                              const int64_t* __restrict__ scan, int64_t m, int64_t* __restrict__ ftext_off,
                                                              uint8_t* __restrict__ start, uint8_t* __restrict__ status,
                                                              unsigned long long* __restrict__ counters) {
    const int64_t t = (int64_t)blockIdx.x * WP_THREADS + threadIdx.x;
    if (t > n_texts) return;
    const int64_t c = std::min<int64_t>(std::max<int64_t>(text_off[t], 0), n);
    const int64_t p = std::min<int64_t>(scan[c] & WP_LOW, m);
    ftext_off[t] = p;
    if (t == n_texts) return;
    if (p < m) start[p] = 1;
    const int64_t c1 = std::min<int64_t>(std::max<int64_t>(text_off[t + 1], c), n);
    const bool flagged = (scan[c1] >> WP_FLAG_SHIFT) != (scan[c] >> WP_FLAG_SHIFT);
    status[t] = flagged ? 1 : 0;
    if (flagged) atomicAdd(&counters[WP_COUNT_FLAGGED], 1ull);
}

__device__ __forceinline__ bool wp_is_head(const uint8_t* __restrict__ kind, const uint8_t* __restrict__ start, int64_t p) {
    const uint8_t k = kind[p];
    if (k == WP_SPACE) return false;
    return k == WP_PUNCT || p == 0 || start[p] || kind[p - 1] != WP_WORD;
}

// head[p] = 1 where a word begins (p < m), head[m] = 0
__global__ __launch_bounds__(WP_THREADS) void wp_heads_kernel(const uint8_t* __restrict__ kind, const uint8_t* __restrict__ start, int64_t m,
                                                               int64_t* __restrict__ head) {
    const int64_t p = (int64_t)blockIdx.x * WP_THREADS + threadIdx.x;
    if (p > m) return;
    head[p] = (p < m && wp_is_head(kind, start, p)) ? 1 : 0;
}

// word_pos[k] = the position of word k's first symbol (word_idx: the scanned heads)
__global__ __launch_bounds__(WP_THREADS) void wp_word_pos_kernel(const uint8_t* __restrict__ kind, const uint8_t* __restrict__ start,
                                                                  const int64_t* __restrict__ word_idx, int64_t m, int64_t n_words,
                                                                  int64_t* __restrict__ word_pos) {
    const int64_t p = (int64_t)blockIdx.x * WP_THREADS + threadIdx.x;
    if (p >= m || !wp_is_head(kind, start, p)) return;
    const int64_t k = word_idx[p];
    if (k >= 0 && k < n_words) word_pos[k] = p;
}

// One lane per word (the block is one wave; dynamic LDS: (max_word_chars + 1) rows of 64 prefix sums, lane-minor, so a row is one
// conflict-free access).  tok_count[w] = the pieces of word w (w < n_words), 0 at w = n_words; tmp[word_pos[w] + j] = the id of piece j.
__global__ __launch_bounds__(WP_MATCH_THREADS) void wp_match_kernel(const uint32_t* __restrict__ sym, const uint8_t* __restrict__ kind,
                                                                     const uint8_t* __restrict__ start, int64_t m,
                                                                     const int64_t* __restrict__ word_pos, int64_t n_words, WpTable table,
                                                                     const int32_t* __restrict__ piece_ids, int32_t max_piece, int32_t unk_id,
                                                                     int32_t max_word_chars, int32_t* __restrict__ tmp,
                                                                     int64_t* __restrict__ tok_count, unsigned long long* __restrict__ counters) {
    extern __shared__ __attribute__((aligned(16))) char wp_smem[];
    uint32_t* prefix = reinterpret_cast<uint32_t*>(wp_smem) + threadIdx.x;  // this lane's column: prefix[j * 64]
    const int64_t w = (int64_t)blockIdx.x * WP_MATCH_THREADS + threadIdx.x;
    if (w > n_words) return;
    if (w == n_words) {
        tok_count[w] = 0;
        return;
    }
    const int64_t p = word_pos[w];
    if (p < 0 || p >= m) {  // (cannot happen with the positions wp_word_pos_kernel wrote)
        tok_count[w] = 0;
        return;
    }
    int32_t len = 1;
    if (kind[p] == WP_WORD)
        while (len <= max_word_chars && p + len < m && kind[p + len] == WP_WORD && !start[p + len]) ++len;
    const uint32_t* word = sym + p;
    int32_t n_tok = 0;
    bool bad = len > max_word_chars;  // (len stops at max_word_chars + 1: longer words are all alike)
    if (!bad) {
        uint32_t h = 0, pw = 1;
        prefix[0] = 0;
        for (int32_t j = 0; j < len; ++j, pw *= WP_B) {
            h = wp_poly_add(h, word[j], pw);
            prefix[(j + 1) * WP_MATCH_THREADS] = h;
        }
        uint32_t inv = 1;  // B^-at
        for (int32_t at = 0; at < len && !bad;) {
            const uint32_t base = prefix[at * WP_MATCH_THREADS];
            int32_t end = std::min(len, at + max_piece), piece = WP_EMPTY;
            for (; end > at; --end) {
                const uint32_t poly = (prefix[end * WP_MATCH_THREADS] - base) * inv;
                piece = wp_table_find(table, word + at, end - at, at > 0 ? 1u : 0u, poly);
                if (piece != WP_EMPTY) break;
            }
            if (piece == WP_EMPTY) {
                bad = true;
                break;
            }
            tmp[p + n_tok++] = piece_ids[piece];  // n_tok <= at < len: inside the word's own symbols
            for (; at < end; ++at) inv *= WP_B_INV;
        }
    }
    if (bad) {
        tmp[p] = unk_id;
        n_tok = 1;
        atomicAdd(&counters[WP_COUNT_UNK], 1ull);
    }
    tok_count[w] = n_tok;
}

// ids[tok_scan[w] + j] = tmp[word_pos[w] + j] for the tok_scan[w + 1] - tok_scan[w] pieces of word w
__global__ __launch_bounds__(WP_THREADS) void wp_emit_kernel(const int64_t* __restrict__ word_pos, const int64_t* __restrict__ tok_scan,
                                                              int64_t n_words, const int32_t* __restrict__ tmp, int64_t m, int64_t n_tokens,
                                                              int32_t* __restrict__ ids) {
    const int64_t w = (int64_t)blockIdx.x * WP_THREADS + threadIdx.x;
    if (w >= n_words) return;
    const int64_t p = word_pos[w], at = tok_scan[w], cnt = tok_scan[w + 1] - at;
    for (int64_t j = 0; j < cnt; ++j)
        if (p + j >= 0 && p + j < m && at + j >= 0 && at + j < n_tokens) ids[at + j] = tmp[p + j];
}

// offsets[t] = the tokens in front of text t (t <= n_texts): word_idx [m + 1] the scanned heads, tok_scan [n_words + 1]
__global__ __launch_bounds__(WP_THREADS) void wp_offsets_kernel(const int64_t* __restrict__ ftext_off, int64_t n_texts,
                                                                 const int64_t* __restrict__ word_idx, int64_t m,
                                                                 const int64_t* __restrict__ tok_scan, int64_t n_words,
                                                                 int64_t* __restrict__ offsets) {
    const int64_t t = (int64_t)blockIdx.x * WP_THREADS + threadIdx.x;
    if (t > n_texts) return;
    const int64_t p = std::min<int64_t>(std::max<int64_t>(ftext_off[t], 0), m);
    const int64_t k = std::min<int64_t>(std::max<int64_t>(word_idx[p], 0), n_words);
    offsets[t] = tok_scan[k];
}

// ---- pair assembly: [CLS] q [SEP] d [SEP] rows from the token lists of texts ---------------------------------------------------------
// _cross_encoder.truncate_pair: one token at a time from the longer list, from the passage on a tie, in closed form
__device__ __forceinline__ void wp_truncate_pair(int64_t nq, int64_t nd, int64_t budget, int64_t* out_q, int64_t* out_d) {
    int64_t over = nq + nd - budget;
    if (over > 0) {
        if (nq > nd) {
            const int64_t cut = std::min(over, nq - nd);
            nq -= cut;
            over -= cut;
        } else if (nd > nq) {
            const int64_t cut = std::min(over, nd - nq);
            nd -= cut;
            over -= cut;
        }
        nd -= (over + 1) / 2;
        nq -= over / 2;
    }
    *out_q = std::max<int64_t>(nq, 0);
    *out_d = std::max<int64_t>(nd, 0);
}

// the tokens of text t (0 for an index outside [0, n_texts): host callers were checked, device callers own their indices)
__device__ __forceinline__ int64_t wp_text_tokens(const int64_t* __restrict__ tok_off, int64_t n_texts, int32_t t, int64_t* begin) {
    if (t < 0 || t >= n_texts) {
        *begin = 0;
        return 0;
    }
    *begin = tok_off[t];
    return std::max<int64_t>(tok_off[t + 1] - tok_off[t], 0);
}

__device__ __forceinline__ void wp_pair_shape(const int64_t* __restrict__ tok_off, int64_t n_texts, int32_t a, int32_t b, int64_t budget,
                                              int64_t* q_begin, int64_t* d_begin, int64_t* nq, int64_t* nd) {
    const int64_t cq = wp_text_tokens(tok_off, n_texts, a, q_begin), cd = wp_text_tokens(tok_off, n_texts, b, d_begin);
    wp_truncate_pair(cq, cd, budget, nq, nd);
}

// len[p] = the row length of pair p (p < n_pairs), len[n_pairs] = 0
__global__ __launch_bounds__(WP_THREADS) void wp_pair_len_kernel(const int64_t* __restrict__ tok_off, int64_t n_texts,
                                                                  const int32_t* __restrict__ query_text, const int32_t* __restrict__ doc_text,
                                                                  int64_t n_pairs, int64_t budget, int64_t* __restrict__ len) {
    const int64_t p = (int64_t)blockIdx.x * WP_THREADS + threadIdx.x;
    if (p > n_pairs) return;
    int64_t v = 0;
    if (p < n_pairs) {
        int64_t qb, db, nq, nd;
        wp_pair_shape(tok_off, n_texts, query_text[p], doc_text[p], budget, &qb, &db, &nq, &nd);
        v = nq + nd + 3;
    }
    len[p] = v;
}

__global__ __launch_bounds__(WP_THREADS) void wp_pair_offsets_kernel(const int64_t* __restrict__ row_scan, int64_t n_pairs,
                                                                      int32_t* __restrict__ seq_offsets) {
    const int64_t p = (int64_t)blockIdx.x * WP_THREADS + threadIdx.x;
    if (p <= n_pairs) seq_offsets[p] = (int32_t)row_scan[p];
}

// One lane per output token: its pair by binary search in the scanned row lengths (every row has at least three tokens)
__global__ __launch_bounds__(WP_THREADS) void wp_pair_write_kernel(const int32_t* __restrict__ ids, const int64_t* __restrict__ tok_off,
                                                                    int64_t n_texts, const int32_t* __restrict__ query_text,
                                                                    const int32_t* __restrict__ doc_text, int64_t n_pairs, int64_t budget,
                                                                    int32_t cls_id, int32_t sep_id, int32_t position_offset,
                                                                    const int64_t* __restrict__ row_scan, int64_t total,
                                                                    int32_t* __restrict__ out_ids, int32_t* __restrict__ out_positions,
                                                                    int32_t* __restrict__ out_type_ids) {
    const int64_t i = (int64_t)blockIdx.x * WP_THREADS + threadIdx.x;
    if (i >= total) return;
    int64_t lo = 0, hi = n_pairs;  // the first p with row_scan[p + 1] > i
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (row_scan[mid + 1] > i) hi = mid;
        else lo = mid + 1;
    }
    const int64_t p = lo;
    if (p >= n_pairs) return;
    const int64_t j = i - row_scan[p];
    int64_t qb, db, nq, nd;
    wp_pair_shape(tok_off, n_texts, query_text[p], doc_text[p], budget, &qb, &db, &nq, &nd);
    const int64_t n_tokens = tok_off[n_texts];
    int32_t v = sep_id;
    int64_t src = -1;
    if (j == 0) v = cls_id;
    else if (j <= nq) src = qb + j - 1;
    else if (j >= nq + 2 && j < nq + 2 + nd) src = db + j - nq - 2;
    if (src >= 0 && src < n_tokens) v = ids[src];
    out_ids[i] = v;
    out_positions[i] = position_offset + (int32_t)j;
    out_type_ids[i] = j < nq + 2 ? 0 : 1;
}

}  // namespace

#define WP_LAUNCH(kernel, items, ...)                                                                          \
    do {                                                                                                       \
        hipLaunchKernelGGL(kernel, dim3(wp_blocks((items), WP_THREADS)), dim3(WP_THREADS), 0, s, __VA_ARGS__); \
        RL_HIP(hipGetLastError());                                                                             \
    } while (0)

int launch_wp_expand_count(const uint32_t* cp, int64_t n, const uint64_t* image, const uint8_t* cls, int64_t n_table, int64_t* count, hipStream_t s) {
    WP_LAUNCH(wp_expand_count_kernel, n + 1, cp, n, image, cls, n_table, count);
    return RL_OK;
}

int launch_wp_expand_write(const uint32_t* cp, int64_t n, const uint64_t* image, const uint8_t* cls, int64_t n_table, const int64_t* scan, int64_t m,
                           uint32_t* sym, uint8_t* kind, hipStream_t s) {
    if (n <= 0 || m <= 0) return RL_OK;
    WP_LAUNCH(wp_expand_write_kernel, n, cp, n, image, cls, n_table, scan, m, sym, kind);
    return RL_OK;
}

int launch_wp_texts(const int64_t* text_off, int64_t n_texts, int64_t n, const int64_t* scan, int64_t m, int64_t* ftext_off, uint8_t* start,
                    uint8_t* status, unsigned long long* counters, hipStream_t s) {
    WP_LAUNCH(wp_text_kernel, n_texts + 1, text_off, n_texts, n, scan, m, ftext_off, start, status, counters);
    return RL_OK;
}

int launch_wp_heads(const uint8_t* kind, const uint8_t* start, int64_t m, int64_t* head, hipStream_t s) {
    WP_LAUNCH(wp_heads_kernel, m + 1, kind, start, m, head);
    return RL_OK;
}

size_t wp_match_lds_bytes(int32_t max_word_chars) { return (size_t)(max_word_chars + 1) * WP_MATCH_THREADS * sizeof(uint32_t); }

int launch_wp_match(const uint32_t* sym, const uint8_t* kind, const uint8_t* start, const int64_t* word_idx, int64_t m, int64_t n_words,
                    const WpTable& table, const int32_t* piece_ids, int32_t max_piece, int32_t unk_id, int32_t max_word_chars, int64_t* word_pos,
                    int32_t* tmp, int64_t* tok_count, unsigned long long* counters, hipStream_t s) {
    if (max_word_chars < 1 || max_word_chars > WP_MAX_WORD_CHARS) return fail(RL_ERR_INVALID, "launch_wp_match: max_word_chars out of range");
    if (m > 0 && n_words > 0) WP_LAUNCH(wp_word_pos_kernel, m, kind, start, word_idx, m, n_words, word_pos);
    hipLaunchKernelGGL(wp_match_kernel, dim3(wp_blocks(n_words + 1, WP_MATCH_THREADS)), dim3(WP_MATCH_THREADS), wp_match_lds_bytes(max_word_chars), s,
                       sym, kind, start, m, word_pos, n_words, table, piece_ids, max_piece, unk_id, max_word_chars, tmp, tok_count, counters);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

int launch_wp_emit(const int64_t* word_pos, const int64_t* tok_scan, int64_t n_words, const int32_t* tmp, int64_t m, int64_t n_tokens, int32_t* ids,
                   hipStream_t s) {
    if (n_words <= 0 || n_tokens <= 0) return RL_OK;
    WP_LAUNCH(wp_emit_kernel, n_words, word_pos, tok_scan, n_words, tmp, m, n_tokens, ids);
    return RL_OK;
}

int launch_wp_offsets(const int64_t* ftext_off, int64_t n_texts, const int64_t* word_idx, int64_t m, const int64_t* tok_scan, int64_t n_words,
                      int64_t* offsets, hipStream_t s) {
    WP_LAUNCH(wp_offsets_kernel, n_texts + 1, ftext_off, n_texts, word_idx, m, tok_scan, n_words, offsets);
    return RL_OK;
}

int launch_wp_pair_lengths(const int64_t* tok_off, int64_t n_texts, const int32_t* query_text, const int32_t* doc_text, int64_t n_pairs, int32_t max_length,
                           int64_t* len, hipStream_t s) {
    WP_LAUNCH(wp_pair_len_kernel, n_pairs + 1, tok_off, n_texts, query_text, doc_text, n_pairs, (int64_t)max_length - 3, len);
    return RL_OK;
}

int launch_wp_pair_offsets(const int64_t* row_scan, int64_t n_pairs, int32_t* seq_offsets, hipStream_t s) {
    WP_LAUNCH(wp_pair_offsets_kernel, n_pairs + 1, row_scan, n_pairs, seq_offsets);
    return RL_OK;
}

int launch_wp_pair_write(const int32_t* ids, const int64_t* tok_off, int64_t n_texts, const int32_t* query_text, const int32_t* doc_text, int64_t n_pairs,
                         int32_t max_length, int32_t cls_id, int32_t sep_id, int32_t position_offset, const int64_t* row_scan, int64_t total,
                         int32_t* out_ids, int32_t* out_positions, int32_t* out_type_ids, hipStream_t s) {
    if (n_pairs <= 0 || total <= 0) return RL_OK;
    WP_LAUNCH(wp_pair_write_kernel, total, ids, tok_off, n_texts, query_text, doc_text, n_pairs, (int64_t)max_length - 3, cls_id, sep_id, position_offset,
              row_scan, total, out_ids, out_positions, out_type_ids);
    return RL_OK;
}

}  // namespace rl
