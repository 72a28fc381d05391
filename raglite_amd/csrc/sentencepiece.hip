// SentencePiece Unigram on the device (rl_sentencepiece_encode / rl_sentencepiece_rows; driven from api_ingest.hip):
// what a SentencePieceProcessor over a Unigram model with nmt_nfkc-style normalisation does for many texts, on their UTF-32 code
// points, from tables the host read out of that model (raglite_amd/_sentencepiece.py: UnigramTables.encode_tables states the same
// algorithm).
//   1. expand   every code point has an image of 0 .. SP_MAX_IMAGE code points in a pool (none = itself): count, exclusive scan, write
//               -> the expanded stream `raw`.  The count carries a second field from bit 32 up: 1 for a code point of the trailing set,
//               so the same scan says how many of those lie in front of every code point, and a text that holds one gets status 1
//   2. spaces   the white-space rule is a predicate per symbol of `raw` (sentencepiece_table.h: sp_keep_count): count, scan, write
//               -> the normalised stream `sym` (a kept space is U+2581, a text's first non-space symbol brings the dummy prefix) and
//               the texts' symbol offsets.  Nothing carries across a text boundary
//   3. search   sp_viterbi_kernel, one text per wave, walked in order with the best score carried in float32 ACROSS the whole text
//               (per word, from 0, the rounding at 1e4 .. 1e5 decides near-ties differently: DESIGN.md 4.25).  For end position j the
//               lanes take the starts j - 1, j - 2, ..., j - L: lane k looks s[j-1-k .. j) up in the exact-compare hash table from the
//               rolling prefix hashes, adds its score to best[start] (ONE float32 addition), and the wave keeps the greatest sum, the
//               smallest start among equals.  best, the prefix hashes, the inverse powers and the symbols live in LDS rings of
//               SP_RING positions; the (start, id) back-pointers go to the text's own symbols of bp_start / bp_id.  Then lane 0
//               backtracks: the ids reversed into tmp at the text's own symbols, a run of unknowns as ONE, and the count
//   4. emit     scan of the counts -> every text's ids to their place in the id layout asked for, and the int64 token offsets
// rl_sentencepiece_rows then assembles `bos, ids[:max_len - 2], eos` rows from any token lists.
// Every phase is its own launch: no kernel waits on another workgroup.  No float atomics; the only atomics are integer adds of two
// counters (unknown ids, flagged texts) and an integer maximum (the longest text): the same run to run.  Every position is 64-bit and is
// checked against its array before it is written.
#include "common.h"
#include "sentencepiece_table.h"

namespace rl {
namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_WAVE = 64;
constexpr int SP_FLAG_SHIFT = 32;
constexpr int64_t SP_LOW = (int64_t(1) << SP_FLAG_SHIFT) - 1;

unsigned sp_blocks(int64_t n, int64_t per) { return (unsigned)((n + per - 1) / per); }

// count[i] = symbols of code point i's image + (its trailing-set flag << 32) for i < n, count[n] = 0
__global__ __launch_bounds__(SP_THREADS) void sp_expand_count_kernel(const uint32_t* __restrict__ cp, int64_t n, SpImage im, int64_t* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
    if (i > n) return;
    int64_t c = 0;
    if (i < n) {
        int32_t first;
        bool flagged;
        c = sp_image_len(im, cp[i], &first, &flagged);
        if (flagged) c |= int64_t(1) << SP_FLAG_SHIFT;
    }
    count[i] = c;
}

// raw [m0]: the expanded stream
__global__ __launch_bounds__(SP_THREADS) void sp_expand_write_kernel(const uint32_t* __restrict__ cp, int64_t n, SpImage im,
                                                                      const int64_t* __restrict__ scan, int64_t m0, uint32_t* __restrict__ raw) {
    const int64_t i = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
    if (i >= n) return;
    int32_t first;
    bool flagged;
    const uint32_t c = cp[i];
    const int32_t len = sp_image_len(im, c, &first, &flagged);
    const int64_t at = scan[i] & SP_LOW;
    for (int32_t j = 0; j < len; ++j) {
        const int64_t p = at + j;
        if (p >= 0 && p < m0) raw[p] = first < 0 ? c : im.pool[first + j];
    }
}

// rtext_off[t] = where text t begins in the expanded stream (t <= n_texts); start[p] = 1 where some text begins (start: zero on entry;
// several texts may begin at one symbol -- empty ones -- and all store the same byte); status[t] = 1: the text holds a flagged code point
__global__ __launch_bounds__(SP_THREADS) void sp_text_kernel(const int64_t* __restrict__ text_off, int64_t n_texts, int64_t n,
                                                              const int64_t* __restrict__ scan, int64_t m0, int64_t* __restrict__ rtext_off,
                                                              uint8_t* __restrict__ start, uint8_t* __restrict__ status,
                                                              unsigned long long* __restrict__ counters) {
    const int64_t t = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
    if (t > n_texts) return;
    const int64_t c = std::min<int64_t>(std::max<int64_t>(text_off[t], 0), n);
    const int64_t p = std::min<int64_t>(scan[c] & SP_LOW, m0);
    rtext_off[t] = p;
    if (t == n_texts) return;
    if (p < m0) start[p] = 1;
    const int64_t c1 = std::min<int64_t>(std::max<int64_t>(text_off[t + 1], c), n);
    const bool flagged = (scan[c1] >> SP_FLAG_SHIFT) != (scan[c] >> SP_FLAG_SHIFT);
    status[t] = flagged ? 1 : 0;
    if (flagged) atomicAdd(&counters[SP_COUNT_FLAGGED], 1ull);
}

__device__ __forceinline__ int32_t sp_keep_at(const uint32_t* __restrict__ raw, const uint8_t* __restrict__ start, int64_t m0, int64_t p) {
    const bool next_in_text = p + 1 < m0 && !start[p + 1];
    return sp_keep_count(raw[p] == SP_SPACE, p == 0 || start[p] != 0, next_in_text, next_in_text && raw[p + 1] == SP_SPACE);
}

// keep[p] = the normalised symbols raw symbol p leaves (p < m0), keep[m0] = 0
__global__ __launch_bounds__(SP_THREADS) void sp_keep_count_kernel(const uint32_t* __restrict__ raw, const uint8_t* __restrict__ start, int64_t m0,
                                                                    int64_t* __restrict__ keep) {
    const int64_t p = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
    if (p > m0) return;
    keep[p] = p < m0 ? sp_keep_at(raw, start, m0, p) : 0;
}

// sym [m]: the normalised stream
__global__ __launch_bounds__(SP_THREADS) void sp_keep_write_kernel(const uint32_t* __restrict__ raw, const uint8_t* __restrict__ start, int64_t m0,
                                                                    const int64_t* __restrict__ keep_scan, int64_t m, uint32_t* __restrict__ sym) {
    const int64_t p = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
    if (p >= m0) return;
    const int32_t k = sp_keep_at(raw, start, m0, p);
    const uint32_t c = raw[p];
    int64_t at = keep_scan[p];
    if (k == 2) {
        if (at >= 0 && at < m) sym[at] = SP_MARK;
        ++at;
    }
    if (k >= 1 && at >= 0 && at < m) sym[at] = c == SP_SPACE ? SP_MARK : c;
}

// sym_off[t] = where text t begins in the normalised stream (t <= n_texts)
__device__ __forceinline__ int64_t sp_sym_begin(const int64_t* __restrict__ rtext_off, const int64_t* __restrict__ keep_scan, int64_t m0, int64_t m,
                                                int64_t t) {
    const int64_t p = std::min<int64_t>(std::max<int64_t>(rtext_off[t], 0), m0);
    return std::min<int64_t>(std::max<int64_t>(keep_scan[p], 0), m);
}

__global__ __launch_bounds__(SP_THREADS) void sp_sym_off_kernel(const int64_t* __restrict__ rtext_off, int64_t n_texts, const int64_t* __restrict__ keep_scan,
                                                                 int64_t m0, int64_t m, int64_t* __restrict__ sym_off,
                                                                 unsigned long long* __restrict__ counters) {
    const int64_t t = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
    if (t > n_texts) return;
    const int64_t b = sp_sym_begin(rtext_off, keep_scan, m0, m, t);
    sym_off[t] = b;
    if (t == n_texts) return;
    const int64_t len = sp_sym_begin(rtext_off, keep_scan, m0, m, t + 1) - b;
    if (len > 0) atomicMax(&counters[SP_COUNT_LONGEST], (unsigned long long)len);  // (an integer maximum: the same whatever the order)
}

__device__ __forceinline__ float sp_wave_max(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, SP_WAVE));
    return v;
}

// One text per wave (the block is one wave).  tok_count[t] = the ids of text t (t < n_texts), 0 at t = n_texts; tmp[sym_off[t] + k] = id k
// from the END of the text (SP_UNK for the unknown piece).  longest: the longest piece in code points, 1 .. SP_MAX_PIECE.
__global__ __launch_bounds__(SP_WAVE) void sp_viterbi_kernel(const uint32_t* __restrict__ sym, const int64_t* __restrict__ sym_off, int64_t n_texts,
                                                              int64_t m, SpTable table, int32_t longest, float unk_score,
                                                              int32_t* __restrict__ bp_start, int32_t* __restrict__ bp_id, int32_t* __restrict__ tmp,
                                                              int64_t* __restrict__ tok_count, unsigned long long* __restrict__ counters) {
    __shared__ float best[SP_RING];       // best[j & (SP_RING - 1)]: the best score of a path that ends at position j
    __shared__ uint32_t prefix[SP_RING];  // the polynomial prefix sum at position j
    __shared__ uint32_t inv_pow[SP_RING]; // B^-j
    __shared__ uint32_t win[SP_RING];     // symbol j, in chunks of 64: the current chunk and the one before it
    const int lane = threadIdx.x;
    const int64_t t = blockIdx.x;
    if (t > n_texts) return;
    if (t == n_texts) {
        if (lane == 0) tok_count[t] = 0;
        return;
    }
    const int64_t base = std::min<int64_t>(std::max<int64_t>(sym_off[t], 0), m);
    const int64_t end = std::min<int64_t>(std::max<int64_t>(sym_off[t + 1], base), m);
    const int32_t n = (int32_t)std::min<int64_t>(end - base, INT32_MAX);  // (the caller keeps m below 2^31)
    if (n == 0) {
        if (lane == 0) tok_count[t] = 0;
        return;
    }
    if (lane == 0) {
        best[0] = 0.f;
        prefix[0] = 0u;
        inv_pow[0] = 1u;
    }
    uint32_t h = 0u, pw = 1u, inv = 1u;  // wave-uniform: the prefix sum at j - 1, B^(j-1), B^-(j-1)
    for (int32_t j = 1; j <= n; ++j) {
        if (((j - 1) & (SP_WAVE - 1)) == 0) {  // symbols j - 1 .. j + 62 into their half of the window (the other half keeps the 64 before them)
            const int32_t q = j - 1 + lane;
            win[q & (SP_RING - 1)] = q < n ? sym[base + q] : 0u;
        }
        __syncthreads();  // (one wave: orders the LDS writes of this wave -- the window, and position j - 1's best / prefix / inv_pow)
        const uint32_t c = win[(j - 1) & (SP_RING - 1)];
        h = wp_poly_add(h, c, pw);
        pw *= WP_B;
        inv *= WP_B_INV;
        // lane k: the span [i, j) of length k + 1
        const int32_t k = lane, i = j - 1 - k;
        float cand = -INFINITY;
        int32_t id = SP_UNK;
        if (k < longest && i >= 0) {
            const uint32_t poly = (h - prefix[i & (SP_RING - 1)]) * inv_pow[i & (SP_RING - 1)];
            const WpTable& pt = table.pieces;
            int64_t s = wp_first_slot(wp_hash(poly, k + 1, 0u, pt.hash_bits), pt.n_slots);
            int32_t piece = WP_EMPTY;
            for (int64_t probes = 0; probes < pt.n_slots; ++probes, s = wp_next_slot(s, pt.n_slots)) {
                const int32_t at = pt.slots[s];
                if (at == WP_EMPTY) break;
                const int32_t b = pt.off[at];
                if (pt.off[at + 1] - b != k + 1) continue;
                bool same = true;
                for (int32_t q = 0; q <= k && same; ++q) same = pt.cp[b + q] == win[(i + q) & (SP_RING - 1)];
                if (same) {
                    piece = at;
                    break;
                }
            }
            if (piece != WP_EMPTY) {
                cand = table.score[piece] + best[i & (SP_RING - 1)];
                id = table.id[piece];
            } else if (k == 0) {
                cand = unk_score + best[i & (SP_RING - 1)];  // no piece of length 1 at j - 1: the unknown piece, one symbol long
            }
        }
        // the winner: the greatest candidate, among equals the smallest start = the highest lane (sp_better's order); lane 0 always offers one
        const float top = sp_wave_max(cand);
        const unsigned long long at_top = __ballot(cand == top && k < longest && i >= 0);
        const int winner = 63 - __clzll(at_top);
        if (lane == winner) {
            best[j & (SP_RING - 1)] = cand;
            const int64_t p = base + j - 1;
            if (p >= 0 && p < m) {
                bp_start[p] = i;
                bp_id[p] = id;
            }
        }
        if (lane == 0) {
            prefix[j & (SP_RING - 1)] = h;
            inv_pow[j & (SP_RING - 1)] = inv;
        }
    }
    __syncthreads();
    __threadfence_block();  // the back-pointers other lanes stored are read by lane 0 below
    if (lane != 0) return;
    int64_t n_tok = 0;
    unsigned long long n_unk = 0;
    bool prev_unk = false;
    for (int32_t j = n; j > 0;) {
        const int64_t p = base + j - 1;
        const int32_t id = bp_id[p], i = bp_start[p];
        if (!(id == SP_UNK && prev_unk)) {  // a run of unknowns is one
            tmp[base + n_tok++] = id;       // n_tok <= n - j < n: inside the text's own symbols
            n_unk += id == SP_UNK;
        }
        prev_unk = id == SP_UNK;
        j = (i >= 0 && i < j) ? i : j - 1;  // (always i < j with the pointers stored above)
    }
    tok_count[t] = n_tok;
    if (n_unk) atomicAdd(&counters[SP_COUNT_UNK], n_unk);
}

// One lane per output token: its text by binary search in the scanned counts; ids[i] in the layout asked for
__global__ __launch_bounds__(SP_THREADS) void sp_emit_kernel(const int32_t* __restrict__ tmp, const int64_t* __restrict__ sym_off,
                                                              const int64_t* __restrict__ tok_scan, int64_t n_texts, int64_t m, int64_t n_tokens,
                                                              int32_t id_offset, int32_t unk_out, int32_t* __restrict__ ids) {
    const int64_t i = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
    if (i >= n_tokens) return;
    int64_t lo = 0, hi = n_texts;  // the first t with tok_scan[t + 1] > i
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (tok_scan[mid + 1] > i) hi = mid;
        else lo = mid + 1;
    }
    if (lo >= n_texts) return;
    const int64_t cnt = tok_scan[lo + 1] - tok_scan[lo], src = sym_off[lo] + (cnt - 1 - (i - tok_scan[lo]));
    int32_t v = SP_UNK;
    if (src >= 0 && src < m) v = tmp[src];
    ids[i] = v == SP_UNK ? unk_out : v + id_offset;
}

__global__ __launch_bounds__(SP_THREADS) void sp_copy_offsets_kernel(const int64_t* __restrict__ tok_scan, int64_t n_texts, int64_t* __restrict__ offsets) {
    const int64_t t = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
    if (t <= n_texts) offsets[t] = tok_scan[t];
}

// ---- row assembly: bos, ids[:max_len - 2], eos from the token lists of texts ----------------------------------------------------------
__device__ __forceinline__ int64_t sp_row_tokens(const int64_t* __restrict__ tok_off, int64_t t, int64_t budget) {
    return std::min<int64_t>(std::max<int64_t>(tok_off[t + 1] - tok_off[t], 0), budget);
}

// len[t] = the row length of text t (t < n_texts), len[n_texts] = 0
__global__ __launch_bounds__(SP_THREADS) void sp_row_len_kernel(const int64_t* __restrict__ tok_off, int64_t n_texts, int64_t budget, int64_t* __restrict__ len) {
    const int64_t t = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
    if (t > n_texts) return;
    len[t] = t < n_texts ? sp_row_tokens(tok_off, t, budget) + 2 : 0;
}

__global__ __launch_bounds__(SP_THREADS) void sp_row_offsets_kernel(const int64_t* __restrict__ row_scan, int64_t n_texts, int32_t* __restrict__ seq_offsets) {
    const int64_t t = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
    if (t <= n_texts) seq_offsets[t] = (int32_t)row_scan[t];
}

// One lane per output token: its row by binary search in the scanned row lengths (every row has at least two tokens)
__global__ __launch_bounds__(SP_THREADS) void sp_row_write_kernel(const int32_t* __restrict__ ids, const int64_t* __restrict__ tok_off, int64_t n_texts,
                                                                   int64_t budget, int32_t bos_id, int32_t eos_id, int32_t position_offset,
                                                                   const int64_t* __restrict__ row_scan, int64_t total, int32_t* __restrict__ out_ids,
                                                                   int32_t* __restrict__ out_positions) {
    const int64_t i = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
    if (i >= total) return;
    int64_t lo = 0, hi = n_texts;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (row_scan[mid + 1] > i) hi = mid;
        else lo = mid + 1;
    }
    if (lo >= n_texts) return;
    const int64_t j = i - row_scan[lo], kept = sp_row_tokens(tok_off, lo, budget), n_tokens = tok_off[n_texts];
    int32_t v = eos_id;
    if (j == 0) v = bos_id;
    else if (j <= kept) {
        const int64_t src = tok_off[lo] + j - 1;
        if (src >= 0 && src < n_tokens) v = ids[src];
    }
    out_ids[i] = v;
    out_positions[i] = position_offset + (int32_t)j;
}

}  // namespace

#define SP_LAUNCH(kernel, items, ...)                                                                          \
    do {                                                                                                       \
        hipLaunchKernelGGL(kernel, dim3(sp_blocks((items), SP_THREADS)), dim3(SP_THREADS), 0, s, __VA_ARGS__); \
        RL_HIP(hipGetLastError());                                                                             \
    } while (0)

int launch_sp_expand_count(const uint32_t* cp, int64_t n, const SpImage& im, int64_t* count, hipStream_t s) {
    SP_LAUNCH(sp_expand_count_kernel, n + 1, cp, n, im, count);
    return RL_OK;
}

int launch_sp_expand_write(const uint32_t* cp, int64_t n, const SpImage& im, const int64_t* scan, int64_t m0, uint32_t* raw, hipStream_t s) {
    if (n <= 0 || m0 <= 0) return RL_OK;
    SP_LAUNCH(sp_expand_write_kernel, n, cp, n, im, scan, m0, raw);
    return RL_OK;
}

int launch_sp_texts(const int64_t* text_off, int64_t n_texts, int64_t n, const int64_t* scan, int64_t m0, int64_t* rtext_off, uint8_t* start,
                    uint8_t* status, unsigned long long* counters, hipStream_t s) {
    SP_LAUNCH(sp_text_kernel, n_texts + 1, text_off, n_texts, n, scan, m0, rtext_off, start, status, counters);
    return RL_OK;
}

int launch_sp_keep_count(const uint32_t* raw, const uint8_t* start, int64_t m0, int64_t* keep, hipStream_t s) {
    SP_LAUNCH(sp_keep_count_kernel, m0 + 1, raw, start, m0, keep);
    return RL_OK;
}

int launch_sp_keep_write(const uint32_t* raw, const uint8_t* start, int64_t m0, const int64_t* keep_scan, int64_t m, const int64_t* rtext_off,
                         int64_t n_texts, uint32_t* sym, int64_t* sym_off, unsigned long long* counters, hipStream_t s) {
    if (m0 > 0 && m > 0) SP_LAUNCH(sp_keep_write_kernel, m0, raw, start, m0, keep_scan, m, sym);
    SP_LAUNCH(sp_sym_off_kernel, n_texts + 1, rtext_off, n_texts, keep_scan, m0, m, sym_off, counters);
    return RL_OK;
}

int launch_sp_viterbi(const uint32_t* sym, const int64_t* sym_off, int64_t n_texts, int64_t m, const SpTable& table, int32_t longest, float unk_score,
                      int32_t* bp_start, int32_t* bp_id, int32_t* tmp, int64_t* tok_count, unsigned long long* counters, hipStream_t s) {
    if (longest < 1 || longest > SP_MAX_PIECE) return fail(RL_ERR_INVALID, "launch_sp_viterbi: the longest piece must be 1 .. 64 code points");
    if (n_texts + 1 > INT32_MAX) return fail(RL_ERR_UNSUPPORTED, "launch_sp_viterbi: too many texts for one grid");
    hipLaunchKernelGGL(sp_viterbi_kernel, dim3((unsigned)(n_texts + 1)), dim3(SP_WAVE), 0, s, sym, sym_off, n_texts, m, table, longest, unk_score, bp_start,
                       bp_id, tmp, tok_count, counters);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

int launch_sp_emit(const int32_t* tmp, const int64_t* sym_off, const int64_t* tok_scan, int64_t n_texts, int64_t m, int64_t n_tokens, int32_t id_offset,
                   int32_t unk_out, int32_t* ids, int64_t* offsets, hipStream_t s) {
    if (n_texts > 0 && n_tokens > 0) SP_LAUNCH(sp_emit_kernel, n_tokens, tmp, sym_off, tok_scan, n_texts, m, n_tokens, id_offset, unk_out, ids);
    SP_LAUNCH(sp_copy_offsets_kernel, n_texts + 1, tok_scan, n_texts, offsets);
    return RL_OK;
}

int launch_sp_row_lengths(const int64_t* tok_off, int64_t n_texts, int32_t max_len, int64_t* len, hipStream_t s) {
    SP_LAUNCH(sp_row_len_kernel, n_texts + 1, tok_off, n_texts, (int64_t)max_len - 2, len);
    return RL_OK;
}

int launch_sp_row_offsets(const int64_t* row_scan, int64_t n_texts, int32_t* seq_offsets, hipStream_t s) {
    SP_LAUNCH(sp_row_offsets_kernel, n_texts + 1, row_scan, n_texts, seq_offsets);
    return RL_OK;
}

int launch_sp_row_write(const int32_t* ids, const int64_t* tok_off, int64_t n_texts, int32_t max_len, int32_t bos_id, int32_t eos_id, int32_t position_offset,
                        const int64_t* row_scan, int64_t total, int32_t* out_ids, int32_t* out_positions, hipStream_t s) {
    if (n_texts <= 0 || total <= 0) return RL_OK;
    SP_LAUNCH(sp_row_write_kernel, total, ids, tok_off, n_texts, (int64_t)max_len - 2, bos_id, eos_id, position_offset, row_scan, total, out_ids,
              out_positions);
    return RL_OK;
}

}  // namespace rl
