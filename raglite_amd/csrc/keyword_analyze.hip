// The BM25 index analyzer on the device (rl_keyword_analyze_begin / _finish; driven from api_keyword.hip): what
// raglite_amd._keyword.index_stems + stems_to_store_ids do for many chunk bodies, on their UTF-32 code points.
//   1. fold      every code point has an image of 0 .. KA_IMAGE_MAX symbols over {a-z, separator, backslash, newline} (the host builds
//                the table from _keyword.normalize): count, exclusive scan, write -> the folded stream, one byte per symbol
//   2. tokenize  a letter preceded, inside its text, by an odd run of backslashes is consumed (DuckDB's `(\\.|[^a-z])+`); the other
//                letters are token letters; a head is a token letter whose predecessor is none, or that starts a text.  Heads are
//                counted, scanned, and every token gets its position
//   3. stem      one lane per token: its length, the stopword test (binary search in the sorted list), the Porter stemmer -- the rules
//                edit a tail of at most KA_TAIL letters kept in LDS, the measure and vowel tests stream the untouched head from the
//                folded text -- then the stem's bytes and hash
//   4. distinct  an open-addressing table of token numbers: a compare-and-swap claims an empty slot, a slot whose token has other
//                bytes is passed by, an integer min leaves the FIRST token of each stem in its slot (a plain look comes first: the
//                read-modify-writes are issued only where they can change the slot).  Which slot a stem gets depends on arrival
//                order; which token ends up in it does not, and nothing else is read from the table.  The stems are then
//                numbered by their first token (a scan), which is the order the host's vocabulary numbers them in
//   5. emit      the host's id per distinct stem -> the term id of every kept token, and the texts' offsets
// Every phase is its own launch: no kernel waits on another workgroup.  The atomics are a 64-bit integer compare-and-swap and min in
// global memory from vector lanes; no float atomics.  Every position is 64-bit and is checked against its array before it is written.
#include "common.h"

namespace rl {
namespace {

constexpr int KA_THREADS = 256;
constexpr int KA_TAIL = 32;  // letters of a token the stemmer may edit: its rules remove at most 22 and read 7 back from the end
constexpr uint8_t KA_SEP = 26, KA_BSL = 27, KA_NL = 28;  // symbols 0 .. 25 are a .. z
constexpr unsigned long long KA_EMPTY = ~0ull;

unsigned blocks_of(int64_t n, int64_t per) { return (unsigned)((n + per - 1) / per); }

// The table entry of a code point: KA_IMAGE_MAX fields of 5 bits from bit 0, field = symbol + 1, 0 = no further symbol.  A value
// outside the table (no Unicode code point) is a separator.
__device__ __forceinline__ uint32_t fold_entry(const uint32_t* __restrict__ table, int64_t n_table, uint32_t cp) {
    return (int64_t)cp < n_table ? table[cp] : (uint32_t)(KA_SEP + 1);
}

// count[i] = symbols of code point i (i < n), count[n] = 0: the scan's last entry is then the length of the folded stream
__global__ __launch_bounds__(KA_THREADS) void ka_fold_count_kernel(const uint32_t* __restrict__ cp, int64_t n, const uint32_t* __restrict__ table,
                                                                    int64_t n_table, int64_t* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * KA_THREADS + threadIdx.x;
    if (i > n) return;
    int c = 0;
    if (i < n) {
        uint32_t e = fold_entry(table, n_table, cp[i]);
        for (; c < KA_IMAGE_MAX && (e & 31u); ++c) e >>= 5;
    }
    count[i] = c;
}

__global__ __launch_bounds__(KA_THREADS) void ka_fold_write_kernel(const uint32_t* __restrict__ cp, int64_t n, const uint32_t* __restrict__ table,
                                                                    int64_t n_table, const int64_t* __restrict__ sym_off, int64_t m,
                                                                    uint8_t* __restrict__ sym) {
    const int64_t i = (int64_t)blockIdx.x * KA_THREADS + threadIdx.x;
    if (i >= n) return;
    uint32_t e = fold_entry(table, n_table, cp[i]);
    const int64_t at = sym_off[i];
    for (int j = 0; j < KA_IMAGE_MAX && (e & 31u); ++j, e >>= 5) {
        const int64_t p = at + j;
        if (p >= 0 && p < m) sym[p] = (uint8_t)((e & 31u) - 1u);
    }
}

// ftext_off[t] = where text t begins in the folded stream (t <= n_texts); start[p] = 1 where some text begins (start: zero on entry;
// several texts may begin at one symbol -- empty ones -- and all store the same byte)
__global__ __launch_bounds__(KA_THREADS) void ka_text_starts_kernel(const int64_t* __restrict__ text_off, int64_t n_texts, int64_t n,
                                                                     const int64_t* __restrict__ sym_off, int64_t m, int64_t* __restrict__ ftext_off,
                                                                     uint8_t* __restrict__ start) {
    const int64_t t = (int64_t)blockIdx.x * KA_THREADS + threadIdx.x;
    if (t > n_texts) return;
    const int64_t c = std::min<int64_t>(std::max<int64_t>(text_off[t], 0), n);
    const int64_t p = std::min<int64_t>(std::max<int64_t>(sym_off[c], 0), m);
    ftext_off[t] = p;
    if (t < n_texts && p < m) start[p] = 1;
}

// letter[p] = 1: symbol p is a letter that no backslash consumes.  With r backslashes in front of it inside its text, the backslashes
// pair up from the left and an odd one out consumes the letter; only the letter's own lane walks the run.
__global__ __launch_bounds__(KA_THREADS) void ka_letters_kernel(const uint8_t* __restrict__ sym, const uint8_t* __restrict__ start, int64_t m,
                                                                 uint8_t* __restrict__ letter) {
    const int64_t p = (int64_t)blockIdx.x * KA_THREADS + threadIdx.x;
    if (p >= m) return;
    uint8_t out = 0;
    if (sym[p] < KA_SEP) {
        int64_t r = 0;
        if (!start[p]) {
            for (int64_t q = p - 1; q >= 0 && sym[q] == KA_BSL; --q) {
                ++r;
                if (start[q]) break;
            }
        }
        out = (r & 1) ? 0 : 1;
    }
    letter[p] = out;
}

// head[p] = 1 where a token begins (p < m), head[m] = 0
__global__ __launch_bounds__(KA_THREADS) void ka_heads_kernel(const uint8_t* __restrict__ letter, const uint8_t* __restrict__ start, int64_t m,
                                                               int64_t* __restrict__ head) {
    const int64_t p = (int64_t)blockIdx.x * KA_THREADS + threadIdx.x;
    if (p > m) return;
    head[p] = (p < m && letter[p] && (p == 0 || start[p] || !letter[p - 1])) ? 1 : 0;
}

// tok_pos[k] = the folded position of token k's first letter (tok_idx: the scanned heads)
__global__ __launch_bounds__(KA_THREADS) void ka_token_pos_kernel(const uint8_t* __restrict__ letter, const uint8_t* __restrict__ start,
                                                                   const int64_t* __restrict__ tok_idx, int64_t m, int64_t n_tok,
                                                                   int64_t* __restrict__ tok_pos) {
    const int64_t p = (int64_t)blockIdx.x * KA_THREADS + threadIdx.x;
    if (p >= m) return;
    if (!(letter[p] && (p == 0 || start[p] || !letter[p - 1]))) return;
    const int64_t k = tok_idx[p];
    if (k >= 0 && k < n_tok) tok_pos[k] = p;
}

// ---- the Porter stemmer of _keyword.stem, rule for rule ------------------------------------------------------------------------
struct Rule {
    char suf[8], rep[5];
    int8_t ns, nr;
};
__device__ const Rule KA_STEP2[20] = {{"ational", "ate", 7, 3}, {"tional", "tion", 6, 4}, {"enci", "ence", 4, 4},   {"anci", "ance", 4, 4},
                                      {"izer", "ize", 4, 3},    {"abli", "able", 4, 4},   {"alli", "al", 4, 2},     {"entli", "ent", 5, 3},
                                      {"eli", "e", 3, 1},       {"ousli", "ous", 5, 3},   {"ization", "ize", 7, 3}, {"ation", "ate", 5, 3},
                                      {"ator", "ate", 4, 3},    {"alism", "al", 5, 2},    {"iveness", "ive", 7, 3}, {"fulness", "ful", 7, 3},
                                      {"ousness", "ous", 7, 3}, {"aliti", "al", 5, 2},    {"iviti", "ive", 5, 3},   {"biliti", "ble", 6, 3}};
__device__ const Rule KA_STEP3[7] = {{"icate", "ic", 5, 2}, {"ative", "", 5, 0}, {"alize", "al", 5, 2}, {"iciti", "ic", 5, 2},
                                     {"ical", "ic", 4, 2},  {"ful", "", 3, 0},   {"ness", "", 4, 0}};
__device__ const Rule KA_STEP4[19] = {{"al", "", 2, 0},  {"ance", "", 4, 0}, {"ence", "", 4, 0},  {"er", "", 2, 0},   {"ic", "", 2, 0},
                                      {"able", "", 4, 0}, {"ible", "", 4, 0}, {"ant", "", 3, 0},   {"ement", "", 5, 0}, {"ment", "", 4, 0},
                                      {"ent", "", 3, 0},  {"ion", "", 3, 0},  {"ou", "", 2, 0},    {"ism", "", 3, 0},  {"ate", "", 3, 0},
                                      {"iti", "", 3, 0},  {"ous", "", 3, 0},  {"ive", "", 3, 0},   {"ize", "", 3, 0}};
constexpr int KA_ION = 11;  // the rule of step 4 with the extra condition

// A word being stemmed: letters [0, base) are the token's own, read from the folded text; letters [base, ...) live in `tail`.
struct Word {
    const uint8_t* src;  // the token's first letter in the folded stream
    uint8_t* tail;       // KA_TAIL bytes of LDS
    int64_t base, len;
    __device__ __forceinline__ uint8_t at(int64_t i) const { return i >= base ? tail[i - base] : src[i]; }
    __device__ __forceinline__ void put(int64_t i, uint8_t c) {
        if (i >= base && i - base < KA_TAIL) tail[i - base] = c;
    }
    __device__ bool ends(const char* suf, int n) const {
        if (len < n) return false;
        for (int j = 0; j < n; ++j)
            if (at(len - n + j) != (uint8_t)(suf[j] - 'a')) return false;
        return true;
    }
};

__device__ __forceinline__ bool ka_vowel(uint8_t c) { return c == 0 || c == 4 || c == 8 || c == 14 || c == 20; }  // a e i o u
constexpr uint8_t KA_Y = 24;

// _measure and _has_vowel of w[:k] in one walk: y is a consonant at the start and after a vowel
__device__ void ka_prefix(const Word& w, int64_t k, int64_t* measure, bool* has_vowel) {
    int64_t m = 0;
    bool hv = false, prev = false;
    for (int64_t i = 0; i < k; ++i) {
        const uint8_t c = w.at(i);
        const bool cons = ka_vowel(c) ? false : (c == KA_Y ? (i == 0 || !prev) : true);
        if (cons && i > 0 && !prev) ++m;
        hv |= !cons;
        prev = cons;
    }
    *measure = m;
    *has_vowel = hv;
}
__device__ int64_t ka_measure(const Word& w, int64_t k) {
    int64_t m;
    bool hv;
    ka_prefix(w, k, &m, &hv);
    return m;
}
__device__ bool ka_has_vowel(const Word& w, int64_t k) {
    int64_t m;
    bool hv;
    ka_prefix(w, k, &m, &hv);
    return hv;
}
// _consonant(w, i) without the recursion: a run of y's alternates from its first one
__device__ bool ka_consonant(const Word& w, int64_t i) {
    const uint8_t c = w.at(i);
    if (ka_vowel(c)) return false;
    if (c != KA_Y) return true;
    int64_t j = i;
    while (j > 0 && w.at(j - 1) == KA_Y) --j;
    const bool first = j == 0 ? true : ka_vowel(w.at(j - 1));  // the run's first y: a consonant at the start and after a vowel
    return ((i - j) & 1) ? !first : first;
}
__device__ bool ka_double_consonant(const Word& w, int64_t n) { return n >= 2 && w.at(n - 1) == w.at(n - 2) && ka_consonant(w, n - 1); }
__device__ bool ka_cvc(const Word& w, int64_t n) {
    if (n < 3) return false;
    const uint8_t last = w.at(n - 1);
    return ka_consonant(w, n - 3) && !ka_consonant(w, n - 2) && ka_consonant(w, n - 1) && last != 22 && last != 23 && last != KA_Y;  // w x y
}
// _longest: the rule with the longest matching suffix, -1 without one
__device__ int ka_longest(const Word& w, const Rule* rules, int n_rules) {
    int best = -1;
    for (int r = 0; r < n_rules; ++r)
        if (w.ends(rules[r].suf, rules[r].ns) && (best < 0 || rules[r].ns > rules[best].ns)) best = r;
    return best;
}
__device__ void ka_replace(Word& w, const Rule& rule) {
    w.len -= rule.ns;
    for (int j = 0; j < rule.nr; ++j) w.put(w.len + j, (uint8_t)(rule.rep[j] - 'a'));
    w.len += rule.nr;
}

__device__ void ka_stem(Word& w) {
    // step 1a
    if (w.ends("sses", 4) || w.ends("ies", 3)) w.len -= 2;
    else if (w.ends("s", 1) && !w.ends("ss", 2)) w.len -= 1;
    // step 1b
    bool again = false;
    if (w.ends("eed", 3)) {
        if (ka_measure(w, w.len - 3) > 0) w.len -= 1;
    } else if (w.ends("ed", 2) && ka_has_vowel(w, w.len - 2)) {
        w.len -= 2;
        again = true;
    } else if (w.ends("ing", 3) && ka_has_vowel(w, w.len - 3)) {
        w.len -= 3;
        again = true;
    }
    if (again) {
        if (w.ends("at", 2) || w.ends("bl", 2) || w.ends("iz", 2)) {
            w.put(w.len, 4);
            w.len += 1;
        } else if (ka_double_consonant(w, w.len) && w.at(w.len - 1) != 11 && w.at(w.len - 1) != 18 && w.at(w.len - 1) != 25) {  // l s z
            w.len -= 1;
        } else if (ka_measure(w, w.len) == 1 && ka_cvc(w, w.len)) {
            w.put(w.len, 4);
            w.len += 1;
        }
    }
    // step 1c
    if (w.ends("y", 1) && ka_has_vowel(w, w.len - 1)) w.put(w.len - 1, 8);
    // steps 2 and 3
    int r = ka_longest(w, KA_STEP2, 20);
    if (r >= 0 && ka_measure(w, w.len - KA_STEP2[r].ns) > 0) ka_replace(w, KA_STEP2[r]);
    r = ka_longest(w, KA_STEP3, 7);
    if (r >= 0 && ka_measure(w, w.len - KA_STEP3[r].ns) > 0) ka_replace(w, KA_STEP3[r]);
    // step 4
    r = ka_longest(w, KA_STEP4, 19);
    if (r >= 0) {
        const int64_t b = w.len - KA_STEP4[r].ns;
        const bool st = b >= 1 && (w.at(b - 1) == 18 || w.at(b - 1) == 19);  // s t
        if (ka_measure(w, b) > 1 && (r != KA_ION || st)) w.len = b;
    }
    // step 5a
    if (w.ends("e", 1)) {
        const int64_t m = ka_measure(w, w.len - 1);
        if (m > 1 || (m == 1 && !ka_cvc(w, w.len - 1))) w.len -= 1;
    }
    // step 5b
    if (w.ends("l", 1) && ka_double_consonant(w, w.len) && ka_measure(w, w.len) > 1) w.len -= 1;
}

// Is the token (letters src[0 .. len)) in the sorted stopword list (stop_off [n_stop + 1] into stop_bytes, symbols 0 .. 25)?
__device__ bool ka_is_stopword(const uint8_t* __restrict__ src, int64_t len, const uint8_t* __restrict__ stop_bytes,
                               const int32_t* __restrict__ stop_off, int32_t n_stop, int32_t stop_max_len) {
    if (len > stop_max_len) return false;
    int32_t lo = 0, hi = n_stop;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        const int32_t b = stop_off[mid], wl = stop_off[mid + 1] - b;
        int cmp = 0;  // the token against word mid
        for (int32_t j = 0; j < wl && j < (int32_t)len && cmp == 0; ++j) cmp = (int)src[j] - (int)stop_bytes[b + j];
        if (cmp == 0) cmp = (int32_t)len < wl ? -1 : ((int32_t)len > wl ? 1 : 0);
        if (cmp == 0) return true;
        if (cmp < 0) hi = mid;
        else lo = mid + 1;
    }
    return false;
}

// One lane per token: tok_len[k] = -1 for a stopword, else the stem's length, its letters at stem[tok_pos[k] ..] (a stem is never
// longer than its token) and its hash.
__global__ __launch_bounds__(KA_THREADS) void ka_stem_kernel(const uint8_t* __restrict__ sym, const uint8_t* __restrict__ letter,
                                                              const uint8_t* __restrict__ start, int64_t m, const int64_t* __restrict__ tok_pos,
                                                              int64_t n_tok, const uint8_t* __restrict__ stop_bytes,
                                                              const int32_t* __restrict__ stop_off, int32_t n_stop, int32_t stop_max_len,
                                                              int hash_bits, uint8_t* __restrict__ stem, int64_t* __restrict__ tok_len,
                                                              uint64_t* __restrict__ tok_hash) {
    __shared__ uint8_t tails[KA_THREADS * KA_TAIL];
    const int64_t k = (int64_t)blockIdx.x * KA_THREADS + threadIdx.x;
    if (k >= n_tok) return;
    const int64_t p = tok_pos[k];
    if (p < 0 || p >= m) {  // (cannot happen with the positions ka_token_pos_kernel wrote)
        tok_len[k] = -1;
        return;
    }
    int64_t len = 1;
    while (p + len < m && letter[p + len] && !start[p + len]) ++len;
    if (ka_is_stopword(sym + p, len, stop_bytes, stop_off, n_stop, stop_max_len)) {
        tok_len[k] = -1;
        return;
    }
    Word w;
    w.src = sym + p;
    w.tail = tails + threadIdx.x * KA_TAIL;
    w.base = len > KA_TAIL ? len - KA_TAIL : 0;
    w.len = len;
    for (int64_t i = w.base; i < len; ++i) w.tail[i - w.base] = w.src[i];
    ka_stem(w);
    uint64_t h = 0xcbf29ce484222325ull;  // FNV-1a over the letters, then a finalizer
    for (int64_t i = 0; i < w.len; ++i) {
        const uint8_t c = w.at(i);
        if (p + i < m) stem[p + i] = c;
        h = (h ^ (uint64_t)(c + 1)) * 0x100000001b3ull;
    }
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33;
    if (hash_bits > 0 && hash_bits < 64) h &= (uint64_t(1) << hash_bits) - 1;
    tok_len[k] = w.len;
    tok_hash[k] = h;
}

__device__ bool ka_same_stem(const uint8_t* __restrict__ stem, const int64_t* __restrict__ tok_pos, const int64_t* __restrict__ tok_len, int64_t a,
                             int64_t b) {
    const int64_t n = tok_len[a];
    if (n != tok_len[b]) return false;
    const uint8_t *x = stem + tok_pos[a], *y = stem + tok_pos[b];
    for (int64_t i = 0; i < n; ++i)
        if (x[i] != y[i]) return false;
    return true;
}

// slots [cap] (cap a power of two > the kept tokens, KA_EMPTY on entry): token k finds the slot of its stem and leaves the smallest
// token number of that stem there.  A slot's stem never changes once claimed: only a token of the same bytes lowers its value.
__global__ __launch_bounds__(KA_THREADS) void ka_distinct_kernel(const uint8_t* __restrict__ stem, const int64_t* __restrict__ tok_pos,
                                                                  const int64_t* __restrict__ tok_len, const uint64_t* __restrict__ tok_hash,
                                                                  int64_t n_tok, unsigned long long* __restrict__ slots, int64_t cap,
                                                                  int64_t* __restrict__ tok_slot) {
    const int64_t k = (int64_t)blockIdx.x * KA_THREADS + threadIdx.x;
    if (k >= n_tok) return;
    if (tok_len[k] < 0) {
        tok_slot[k] = -1;
        return;
    }
    int64_t s = (int64_t)(tok_hash[k] & (uint64_t)(cap - 1));
    int64_t found = -1;
    for (int64_t probes = 0; probes < cap; ++probes) {  // (the table is never full: cap > the kept tokens)
        // A look before the compare-and-swap: under a Zipf law hundreds of thousands of tokens meet in the slots of a few stems, and a
        // load does not queue where a read-modify-write does.  A stale value is harmless: it is KA_EMPTY (the swap then tells) or a
        // token that was in the slot, so of the slot's stem, and never smaller than the one there now.
        unsigned long long cur = __hip_atomic_load(&slots[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == KA_EMPTY) cur = atomicCAS(&slots[s], KA_EMPTY, (unsigned long long)k);
        if (cur == KA_EMPTY) {
            found = s;
            break;
        }
        if ((int64_t)cur < n_tok && ka_same_stem(stem, tok_pos, tok_len, (int64_t)cur, k)) {
            if ((unsigned long long)k < cur) atomicMin(&slots[s], (unsigned long long)k);
            found = s;
            break;
        }
        s = (s + 1) & (cap - 1);
    }
    tok_slot[k] = found;
}

// kept[k] = 1: token k is no stopword; first[k] = 1: it is the first token of its stem (k < n_tok); both 0 at k = n_tok
__global__ __launch_bounds__(KA_THREADS) void ka_flags_kernel(const int64_t* __restrict__ tok_len, const int64_t* __restrict__ tok_slot,
                                                               const unsigned long long* __restrict__ slots, int64_t cap, int64_t n_tok,
                                                               int64_t* __restrict__ kept, int64_t* __restrict__ first) {
    const int64_t k = (int64_t)blockIdx.x * KA_THREADS + threadIdx.x;
    if (k > n_tok) return;
    int64_t kp = 0, f = 0;
    if (k < n_tok && tok_len[k] >= 0) {
        kp = 1;
        const int64_t s = tok_slot[k];
        f = (s >= 0 && s < cap && slots[s] == (unsigned long long)k) ? 1 : 0;
    }
    kept[k] = kp;
    first[k] = f;
}

// Distinct stem d (the d-th in order of first appearance): its first token, that token's place among the kept ones, its length
// (dist_len[n_distinct] = 0: the scan's last entry is then the byte total)
__global__ __launch_bounds__(KA_THREADS) void ka_distinct_out_kernel(const int64_t* __restrict__ tok_len, const int64_t* __restrict__ tok_slot,
                                                                      const unsigned long long* __restrict__ slots, int64_t cap, int64_t n_tok,
                                                                      const int64_t* __restrict__ kept_scan, const int64_t* __restrict__ rank,
                                                                      int64_t n_distinct, int64_t* __restrict__ dist_tok,
                                                                      int64_t* __restrict__ dist_first, int64_t* __restrict__ dist_len) {
    const int64_t k = (int64_t)blockIdx.x * KA_THREADS + threadIdx.x;
    if (k == n_tok) dist_len[n_distinct] = 0;
    if (k >= n_tok || tok_len[k] < 0) return;
    const int64_t s = tok_slot[k];
    if (s < 0 || s >= cap || slots[s] != (unsigned long long)k) return;
    const int64_t d = rank[k];
    if (d < 0 || d >= n_distinct) return;
    dist_tok[d] = k;
    dist_first[d] = kept_scan[k];
    dist_len[d] = tok_len[k];
}

// the stems' letters as ASCII, stem d at bytes[dist_off[d] .. dist_off[d + 1])
__global__ __launch_bounds__(KA_THREADS) void ka_distinct_bytes_kernel(const uint8_t* __restrict__ stem, const int64_t* __restrict__ tok_pos,
                                                                        const int64_t* __restrict__ tok_len, const int64_t* __restrict__ dist_tok,
                                                                        const int64_t* __restrict__ dist_off, int64_t n_distinct, int64_t n_bytes,
                                                                        uint8_t* __restrict__ bytes) {
    const int64_t d = (int64_t)blockIdx.x * KA_THREADS + threadIdx.x;
    if (d >= n_distinct) return;
    const int64_t k = dist_tok[d], at = dist_off[d];
    const uint8_t* src = stem + tok_pos[k];
    const int64_t n = tok_len[k];
    for (int64_t i = 0; i < n; ++i)
        if (at + i >= 0 && at + i < n_bytes) bytes[at + i] = (uint8_t)('a' + src[i]);
}

// term_ids[kept_scan[k]] = ids[rank of the stem of token k]
__global__ __launch_bounds__(KA_THREADS) void ka_emit_kernel(const int64_t* __restrict__ tok_len, const int64_t* __restrict__ tok_slot,
                                                              const unsigned long long* __restrict__ slots, int64_t cap, int64_t n_tok,
                                                              const int64_t* __restrict__ kept_scan, const int64_t* __restrict__ rank,
                                                              const int32_t* __restrict__ ids, int64_t n_distinct, int64_t n_kept,
                                                              int32_t* __restrict__ term_ids) {
    const int64_t k = (int64_t)blockIdx.x * KA_THREADS + threadIdx.x;
    if (k >= n_tok || tok_len[k] < 0) return;
    const int64_t s = tok_slot[k], j = kept_scan[k];
    if (s < 0 || s >= cap || j < 0 || j >= n_kept) return;
    const unsigned long long f = slots[s];
    if (f >= (unsigned long long)n_tok) return;
    const int64_t d = rank[f];
    if (d >= 0 && d < n_distinct) term_ids[j] = ids[d];
}

// offsets[c] = the kept tokens in front of text c (c <= n_texts): tok_idx [m + 1] the scanned heads, kept_scan [n_tok + 1]
__global__ __launch_bounds__(KA_THREADS) void ka_offsets_kernel(const int64_t* __restrict__ ftext_off, int64_t n_texts, const int64_t* __restrict__ tok_idx,
                                                                 int64_t m, const int64_t* __restrict__ kept_scan, int64_t n_tok,
                                                                 int64_t* __restrict__ offsets) {
    const int64_t c = (int64_t)blockIdx.x * KA_THREADS + threadIdx.x;
    if (c > n_texts) return;
    const int64_t p = std::min<int64_t>(std::max<int64_t>(ftext_off[c], 0), m);
    const int64_t k = std::min<int64_t>(std::max<int64_t>(tok_idx[p], 0), n_tok);
    offsets[c] = kept_scan[k];
}

}  // namespace

#define KA_LAUNCH(kernel, items, ...)                                                                          \
    do {                                                                                                       \
        hipLaunchKernelGGL(kernel, dim3(blocks_of((items), KA_THREADS)), dim3(KA_THREADS), 0, s, __VA_ARGS__); \
        RL_HIP(hipGetLastError());                                                                             \
    } while (0)

int launch_ka_fold_count(const uint32_t* cp, int64_t n, const uint32_t* table, int64_t n_table, int64_t* count, hipStream_t s) {
    KA_LAUNCH(ka_fold_count_kernel, n + 1, cp, n, table, n_table, count);
    return RL_OK;
}

int launch_ka_fold_write(const uint32_t* cp, int64_t n, const uint32_t* table, int64_t n_table, const int64_t* sym_off, int64_t m, uint8_t* sym,
                         hipStream_t s) {
    if (n <= 0 || m <= 0) return RL_OK;
    KA_LAUNCH(ka_fold_write_kernel, n, cp, n, table, n_table, sym_off, m, sym);
    return RL_OK;
}

int launch_ka_text_starts(const int64_t* text_off, int64_t n_texts, int64_t n, const int64_t* sym_off, int64_t m, int64_t* ftext_off, uint8_t* start,
                          hipStream_t s) {
    KA_LAUNCH(ka_text_starts_kernel, n_texts + 1, text_off, n_texts, n, sym_off, m, ftext_off, start);
    return RL_OK;
}

int launch_ka_heads(const uint8_t* sym, const uint8_t* start, int64_t m, uint8_t* letter, int64_t* head, hipStream_t s) {
    if (m > 0) KA_LAUNCH(ka_letters_kernel, m, sym, start, m, letter);
    KA_LAUNCH(ka_heads_kernel, m + 1, letter, start, m, head);
    return RL_OK;
}

int launch_ka_stem(const uint8_t* sym, const uint8_t* letter, const uint8_t* start, const int64_t* tok_idx, int64_t m, int64_t n_tok,
                   const uint8_t* stop_bytes, const int32_t* stop_off, int32_t n_stop, int32_t stop_max_len, int hash_bits, int64_t* tok_pos,
                   uint8_t* stem, int64_t* tok_len, uint64_t* tok_hash, hipStream_t s) {
    if (m <= 0 || n_tok <= 0) return RL_OK;
    KA_LAUNCH(ka_token_pos_kernel, m, letter, start, tok_idx, m, n_tok, tok_pos);
    KA_LAUNCH(ka_stem_kernel, n_tok, sym, letter, start, m, tok_pos, n_tok, stop_bytes, stop_off, n_stop, stop_max_len, hash_bits, stem, tok_len,
              tok_hash);
    return RL_OK;
}

int64_t ka_table_slots(int64_t n_tok) {
    int64_t cap = 64;
    while (cap < 2 * n_tok) cap <<= 1;
    return cap;
}

int launch_ka_distinct(const uint8_t* stem, const int64_t* tok_pos, const int64_t* tok_len, const uint64_t* tok_hash, int64_t n_tok, uint64_t* slots,
                       int64_t cap, int64_t* tok_slot, int64_t* kept, int64_t* first, hipStream_t s) {
    if (n_tok <= 0) return RL_OK;
    RL_HIP(hipMemsetAsync(slots, 0xff, (size_t)cap * sizeof(uint64_t), s));
    KA_LAUNCH(ka_distinct_kernel, n_tok, stem, tok_pos, tok_len, tok_hash, n_tok, reinterpret_cast<unsigned long long*>(slots), cap, tok_slot);
    KA_LAUNCH(ka_flags_kernel, n_tok + 1, tok_len, tok_slot, reinterpret_cast<const unsigned long long*>(slots), cap, n_tok, kept, first);
    return RL_OK;
}

int launch_ka_distinct_out(const int64_t* tok_len, const int64_t* tok_slot, const uint64_t* slots, int64_t cap, int64_t n_tok, const int64_t* kept_scan,
                           const int64_t* rank, int64_t n_distinct, int64_t* dist_tok, int64_t* dist_first, int64_t* dist_len, hipStream_t s) {
    KA_LAUNCH(ka_distinct_out_kernel, n_tok + 1, tok_len, tok_slot, reinterpret_cast<const unsigned long long*>(slots), cap, n_tok, kept_scan, rank,
              n_distinct, dist_tok, dist_first, dist_len);
    return RL_OK;
}

int launch_ka_distinct_bytes(const uint8_t* stem, const int64_t* tok_pos, const int64_t* tok_len, const int64_t* dist_tok, const int64_t* dist_off,
                             int64_t n_distinct, int64_t n_bytes, uint8_t* bytes, hipStream_t s) {
    if (n_distinct <= 0 || n_bytes <= 0) return RL_OK;
    KA_LAUNCH(ka_distinct_bytes_kernel, n_distinct, stem, tok_pos, tok_len, dist_tok, dist_off, n_distinct, n_bytes, bytes);
    return RL_OK;
}

int launch_ka_emit(const int64_t* tok_len, const int64_t* tok_slot, const uint64_t* slots, int64_t cap, int64_t n_tok, const int64_t* kept_scan,
                   const int64_t* rank, const int32_t* ids, int64_t n_distinct, int64_t n_kept, int32_t* term_ids, hipStream_t s) {
    if (n_tok <= 0 || n_kept <= 0) return RL_OK;
    KA_LAUNCH(ka_emit_kernel, n_tok, tok_len, tok_slot, reinterpret_cast<const unsigned long long*>(slots), cap, n_tok, kept_scan, rank, ids,
              n_distinct, n_kept, term_ids);
    return RL_OK;
}

int launch_ka_offsets(const int64_t* ftext_off, int64_t n_texts, const int64_t* tok_idx, int64_t m, const int64_t* kept_scan, int64_t n_tok,
                      int64_t* offsets, hipStream_t s) {
    KA_LAUNCH(ka_offsets_kernel, n_texts + 1, ftext_off, n_texts, tok_idx, m, kept_scan, n_tok, offsets);
    return RL_OK;
}

}  // namespace rl
