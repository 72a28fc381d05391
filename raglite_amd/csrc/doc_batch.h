// What the document-batched kernels share (partition_sim.hip, partition_dp.hip, chunklet_dp.hip, sentence_dp.hip; DESIGN.md
// section 4.13b): a batch is n rows and a CSR `off` of n_docs + 1 offsets, document d owning rows [off[d], off[d + 1]).
//
// Host callers' offsets are checked before the first HIP call (api_ingest.hip: check_doc_offsets).  Device callers' offsets cannot be read
// without a synchronisation, so they are not validated: every kernel takes a document's rows from doc_rows, which forces them into
// [0, n], and doc_of returns a document in [0, n_docs) for any row.  With malformed offsets the results are unspecified, but no kernel
// indexes past n.
#pragma once
#include "common.h"

#include <limits>

namespace rl {

// The last document d with off[d] <= row, so empty documents in front of the row's own are skipped.
__device__ __forceinline__ int64_t doc_of(const int64_t* __restrict__ off, int64_t n_docs, int64_t row) {
    int64_t lo = 0, hi = n_docs;  // off[lo] <= row < off[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] <= row) lo = mid; else hi = mid;
    }
    return lo;
}

// Rows [b, e) of a document, forced into [0, n] and to at most max_rows (a kernel whose per-document indices are narrower than 64 bits).
__device__ __forceinline__ void doc_rows(const int64_t* __restrict__ off, int64_t doc, int64_t n, int64_t* b, int64_t* e,
                                         int64_t max_rows = std::numeric_limits<int64_t>::max()) {
    const int64_t lo = off[doc], hi = off[doc + 1];
    *b = lo < 0 ? 0 : (lo > n ? n : lo);
    *e = hi < *b ? *b : (hi > n ? n : hi);
    if (*e - *b > max_rows) *e = *b + max_rows;
}

// One step of a prefix sum that a wave carries over blocks of 64 values: lane l gets carry + x[0] + ... + x[l], and carry grows by the
// block's total.  Integers: any order gives the same sum.
__device__ __forceinline__ long long wave_prefix_step(long long x, int lane, long long* carry) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long t = __shfl_up(x, o, 64);
        if (lane >= o) x += t;
    }
    const long long incl = *carry + x;
    *carry += __shfl(x, 63, 64);
    return incl;
}

// The grid of a kernel that gives every item (a row, a document) one wave: four waves per block, at most 256 * 16 blocks (the kernels
// stride over the rest).
inline int wave_per_item_blocks(int64_t items) { return (int)std::max<int64_t>(1, std::min<int64_t>((items + 3) / 4, 256 * 16)); }

}  // namespace rl
