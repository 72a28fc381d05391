// The vocabulary table of the device WordPiece tokenizer (wordpiece.hip): the hash of a piece, the probe sequence and
// the comparison on a hit, stated once.  rl_wordpiece_create builds the table with wp_table_insert on the host, the match kernel looks
// pieces up with wp_table_find.  Plain C++: no HIP header is needed to read it, so a host program can build a table and probe every
// piece back (tests/test_wordpiece_host.py).
//
// A piece is its code points (the continuation prefix stripped) and one bit: is it a continuation?  Its hash starts from the
// polynomial sum of (c_j + 1) * B^j mod 2^32, which the kernel gets for every [start, end) of a word from ONE pass of prefix sums:
//     poly(start, end) = (prefix[end] - prefix[start]) * B^-start          (B is odd, so it has an inverse mod 2^32)
// then the length and the bit go in and a finalizer spreads the 32 bits over 64.  hash_bits > 0 keeps only that many low bits (the
// tests' knob: with 4 every lookup collides).  Collisions cost probes, never correctness: every hit compares the code points.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RL_WP_HD __host__ __device__
#else
#define RL_WP_HD
#endif

namespace rl {

constexpr uint32_t WP_B = 0x9E3779B1u;  // odd
constexpr uint32_t wp_inverse(uint32_t b) {  // Newton's iteration mod 2^32: every step doubles the correct low bits (b * b = 1 mod 8)
    uint32_t x = b;
    for (int i = 0; i < 5; ++i) x *= 2u - b * x;
    return x;
}
constexpr uint32_t WP_B_INV = wp_inverse(WP_B);
static_assert(WP_B * WP_B_INV == 1u, "WP_B_INV is the inverse of WP_B mod 2^32");

constexpr int32_t WP_EMPTY = -1;          // an empty slot
constexpr int64_t WP_MIN_SLOTS = 64;
constexpr int32_t WP_MAX_WORD_CHARS = 200;  // the longest word the match kernel keeps prefix sums for (rl_wordpiece_create's cap)

// The vocabulary as the table sees it: piece i is cp[off[i] .. off[i + 1]) with flags[i] & 1 = continuation; slots [n_slots] hold piece
// numbers (WP_EMPTY: none), n_slots a power of two > n_pieces.
struct WpTable {
    const uint32_t* cp;
    const int32_t* off;
    const uint8_t* flags;
    const int32_t* slots;
    int64_t n_slots;
    int hash_bits;
};

// slots for n_pieces pieces: a power of two >= 2 n_pieces (load <= 1/2), at least WP_MIN_SLOTS
RL_WP_HD inline int64_t wp_table_slots(int64_t n_pieces) {
    int64_t cap = WP_MIN_SLOTS;
    while (cap < 2 * n_pieces) cap <<= 1;
    return cap;
}

// One more symbol at position j of a prefix sum: prefix[j + 1] = wp_poly_add(prefix[j], c_j, B^j)
RL_WP_HD inline uint32_t wp_poly_add(uint32_t prefix, uint32_t c, uint32_t pow_j) { return prefix + (c + 1u) * pow_j; }

// The polynomial sum of a whole piece (what the host hashes at build time)
RL_WP_HD inline uint32_t wp_poly(const uint32_t* cp, int32_t len) {
    uint32_t h = 0, pw = 1;
    for (int32_t j = 0; j < len; ++j, pw *= WP_B) h = wp_poly_add(h, cp[j], pw);
    return h;
}

RL_WP_HD inline uint64_t wp_hash(uint32_t poly, int32_t len, uint32_t continuation, int hash_bits) {
    uint64_t h = ((uint64_t)poly << 32) | ((uint64_t)(uint32_t)len << 1) | (continuation & 1u);
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33;
    h *= 0xc4ceb9fe1a85ec53ull;
    h ^= h >> 33;
    if (hash_bits > 0 && hash_bits < 64) h &= (uint64_t(1) << hash_bits) - 1;
    return h;
}

// The probe sequence: linear from the hash's slot.
RL_WP_HD inline int64_t wp_first_slot(uint64_t hash, int64_t n_slots) { return (int64_t)(hash & (uint64_t)(n_slots - 1)); }
RL_WP_HD inline int64_t wp_next_slot(int64_t s, int64_t n_slots) { return (s + 1) & (n_slots - 1); }

RL_WP_HD inline bool wp_same_piece(const WpTable& t, int32_t piece, const uint32_t* cp, int32_t len, uint32_t continuation) {
    const int32_t b = t.off[piece];
    if (t.off[piece + 1] - b != len || (uint32_t)(t.flags[piece] & 1u) != (continuation & 1u)) return false;
    for (int32_t j = 0; j < len; ++j)
        if (t.cp[b + j] != cp[j]) return false;
    return true;
}

// The piece with these code points and this bit, or WP_EMPTY.  `poly` is wp_poly(cp, len), however the caller came by it.  The walk
// ends at the first empty slot; the table is never full, and the bound on the probes only guards a malformed one.
RL_WP_HD inline int32_t wp_table_find(const WpTable& t, const uint32_t* cp, int32_t len, uint32_t continuation, uint32_t poly) {
    int64_t s = wp_first_slot(wp_hash(poly, len, continuation, t.hash_bits), t.n_slots);
    for (int64_t probes = 0; probes < t.n_slots; ++probes, s = wp_next_slot(s, t.n_slots)) {
        const int32_t piece = t.slots[s];
        if (piece == WP_EMPTY) return WP_EMPTY;
        if (wp_same_piece(t, piece, cp, len, continuation)) return piece;
    }
    return WP_EMPTY;
}

// Host: put piece `piece` into slots (the table's own, writable).  Returns the slot, or -1 when an equal piece is there already
// (the first one stays) or the table is full.
inline int64_t wp_table_insert(const WpTable& t, int32_t* slots, int32_t piece) {
    const int32_t b = t.off[piece], len = t.off[piece + 1] - b;
    const uint32_t continuation = t.flags[piece] & 1u;
    int64_t s = wp_first_slot(wp_hash(wp_poly(t.cp + b, len), len, continuation, t.hash_bits), t.n_slots);
    for (int64_t probes = 0; probes < t.n_slots; ++probes, s = wp_next_slot(s, t.n_slots)) {
        if (slots[s] == WP_EMPTY) {
            slots[s] = piece;
            return s;
        }
        if (wp_same_piece(t, slots[s], t.cp + b, len, continuation)) return -1;
    }
    return -1;
}

}  // namespace rl
