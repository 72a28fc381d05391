// The tables of the device SentencePiece Unigram tokenizer (sentencepiece.hip), stated once for the host builder
// (rl_sentencepiece_create) and the kernels.  Plain C++: no HIP header is needed to read it, so a host program can build the tables,
// probe every piece back and run the white-space rule and the search's ordering (tests/test_sentencepiece_host.py).
//
//   - the per-code-point image: (offset, length) into a pool of code points; offset < 0 = the code point itself; bit 7 of the length
//     byte flags a code point of the trailing set (it may be consumed together with its predecessor: the text goes to the host)
//   - the white-space rule, per symbol of the expanded stream: how many normalised symbols it leaves (0, 1 or 2)
//   - the vocabulary: wordpiece_table.h's open-addressing table over the NORMAL pieces (no piece is a continuation here), with a
//     float32 score and a SentencePiece id per piece
//   - the order in which candidates for one end position win: greatest sum first, then the smallest start
#pragma once
#include <cstdint>

#include "wordpiece_table.h"

namespace rl {

constexpr uint32_t SP_SPACE = 0x20u;    // a space of the expanded stream ...
constexpr uint32_t SP_MARK = 0x2581u;   // ... is this symbol of the normalised one
constexpr int32_t SP_MAX_PIECE = 64;    // the longest piece in code points: one lane of the search's wave per start
constexpr int32_t SP_MAX_IMAGE = 127;   // the longest image in code points (7 bits of the length byte)
constexpr uint8_t SP_FLAG = 0x80u;      // image_len bit 7: the trailing set
constexpr int32_t SP_UNK = -1;          // the unknown piece in the search's back-pointers and in its reversed ids
constexpr int32_t SP_RING = 128;        // positions the search keeps in LDS: a power of two >= 2 * SP_MAX_PIECE (two symbol chunks of 64)
static_assert((SP_RING & (SP_RING - 1)) == 0 && SP_RING >= 2 * SP_MAX_PIECE, "the ring holds the current and the previous chunk of 64 symbols");

struct SpImage {
    const int32_t* off;    // [n_table]
    const uint8_t* len;    // [n_table]
    const uint32_t* pool;  // [n_pool]
    int64_t n_table, n_pool;
};

// the image of code point c: its length, and *first = where it begins in the pool (-1: the code point itself)
RL_WP_HD inline int32_t sp_image_len(const SpImage& im, uint32_t c, int32_t* first, bool* flagged) {
    *first = -1;
    *flagged = false;
    if ((int64_t)c >= im.n_table) return 1;
    const uint8_t l = im.len[c];
    *flagged = (l & SP_FLAG) != 0;
    const int32_t o = im.off[c];
    if (o < 0) return 1;
    const int32_t n = l & 0x7F;
    if ((int64_t)o + n > im.n_pool) return 0;  // (rl_sentencepiece_create has rejected such a table)
    *first = o;
    return n;
}

// How many normalised symbols symbol p of the expanded stream leaves.  A space is kept iff the next symbol of the same text exists and is
// no space (so of a run of spaces the last one stays, and trailing spaces go); a non-space symbol stays, and one that is its text's first
// symbol is preceded by the dummy prefix.  Leading spaces: the last of them IS the prefix.  An empty or all-space text leaves nothing.
RL_WP_HD inline int32_t sp_keep_count(bool is_space, bool first_of_text, bool next_in_text, bool next_is_space) {
    if (is_space) return (next_in_text && !next_is_space) ? 1 : 0;
    return first_of_text ? 2 : 1;
}

struct SpTable {
    WpTable pieces;       // flags all 0
    const float* score;   // [n_pieces]
    const int32_t* id;    // [n_pieces]
};

// Does candidate (c, start) beat (best_c, best_start) for one end position?  The recurrence offers candidates in ascending start and
// takes one only when it is strictly greater, so among equal sums the earliest start stays.
RL_WP_HD inline bool sp_better(float c, int32_t start, float best_c, int32_t best_start) { return c > best_c || (c == best_c && start < best_start); }

}  // namespace rl
