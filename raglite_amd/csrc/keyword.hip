// BM25 keyword search: the keyword half of the reference's hybrid search (src/raglite/_search.py:156-230, DuckDB FTS
// `match_bm25` over chunk.body).  The host (raglite_amd/_keyword.py) analyses the text and computes the statistics; the device
// holds the postings and scores a batch of queries.
//
// Postings are term-major CSR: term t owns [term_off[t], term_off[t+1]) of post_chunk (chunk ordinals, strictly ascending within a
// term) and post_impact (its BM25 contribution, computed once at build time by bm25_impact_kernel):
//     impact = idf_t * ((tf * (k1 + 1)) / (tf + nrm_c))          (float32, in exactly this order, every step rounded)
// A chunk's score is the sum of the impacts of the query's terms it contains, in ascending term id order, starting from the first
// impact; a chunk that contains none scores -inf and is not a result.  Every operation below is rounded to nearest with no
// contraction, so the scores are bitwise those of the NumPy restatement in tests/keyword_ref.py.
#include "common.h"

namespace rl {
namespace {

constexpr float BM25_K1 = 1.2f;
constexpr int KW_THREADS = 256;
constexpr int KW_TERM_GROUP = 64;  // query terms whose posting ranges a block looks up at once

__global__ __launch_bounds__(256) void bm25_impact_kernel(const int32_t* __restrict__ post_chunk, const int32_t* __restrict__ post_tf,
                                                          const int32_t* __restrict__ post_term, const float* __restrict__ idf,
                                                          const float* __restrict__ nrm, int64_t n_postings, int32_t n_terms,
                                                          int64_t n_chunks, float* __restrict__ post_impact) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_postings) return;
    const int32_t t = post_term[p], c = post_chunk[p];
    if (t < 0 || t >= n_terms || c < 0 || c >= n_chunks) {  // (the host validates host postings; device postings are taken as given)
        post_impact[p] = 0.f;
        return;
    }
    const float tf = (float)post_tf[p];
    post_impact[p] = __fmul_rn(idf[t], __fdiv_rn(__fmul_rn(tf, BM25_K1 + 1.0f), __fadd_rn(tf, nrm[c])));
}

// First position p in [a, e) with arr[p] >= x (e when there is none), by a 32-ary search of one half-wave: each round every lane
// reads one probe, so a range of 1 M postings takes four dependent reads instead of twenty.  `half` is the lane's half of the wave
// (0: lanes 0-31, 1: lanes 32-63); the two halves search independently, with their own x.  Every lane of the wave must call.
__device__ __forceinline__ int64_t lower_bound_32(const int32_t* __restrict__ arr, int64_t a, int64_t e, int32_t x, int lane, int half) {
    const int sub = lane & 31;
    for (;;) {
        const int64_t len = e - a;
        const int64_t step = len > 0 ? (len + 31) / 32 : 1;
        const int64_t p = a + (int64_t)sub * step;
        const bool below = len > 0 && p < e && arr[p] < x;
        const uint64_t m = __builtin_amdgcn_ballot_w64(below);
        const uint32_t mine = (uint32_t)(half ? (m >> 32) : m);
        // both halves loop until both are done (the ballot needs the whole wave)
        const bool done = len <= 0 || mine == 0;
        const uint64_t busy = __builtin_amdgcn_ballot_w64(!done);
        if (done) e = a;  // (keeps this half's answer, a, while the other half finishes)
        if (busy == 0) return a;
        if (!done) {
            const int j = __builtin_popcount(mine);        // probes below x form a prefix
            const int64_t last = a + (int64_t)(j - 1) * step;  // arr[last] < x
            a = last + 1;
            e = std::min<int64_t>(e, last + step);         // the next probe (if inside the range) is >= x
        }
    }
}

// grid (chunk tiles, queries); block KW_THREADS; dynamic LDS: `tile` floats (the tile's scores).
// q_off [B + 1] / q_terms: each query's term ids, ascending and distinct (ids outside [0, n_terms) are skipped).
// filter: query b's chunk bitset (none: no filter), bit c cleared -> -inf.  Writes scores[b * ld + c] for c < n_chunks.
__global__ __launch_bounds__(KW_THREADS) void bm25_score_kernel(const int64_t* __restrict__ term_off, const int32_t* __restrict__ post_chunk,
                                                                const float* __restrict__ post_impact, int32_t n_terms, int64_t n_chunks,
                                                                const int64_t* __restrict__ q_off, const int32_t* __restrict__ q_terms,
                                                                QueryMask filter_of, int32_t tile, float* __restrict__ scores,
                                                                int64_t ld) {
    extern __shared__ float s[];
    __shared__ int64_t range[KW_TERM_GROUP][2];
    const int b = blockIdx.y;
    const int64_t lo = (int64_t)blockIdx.x * tile;
    const int32_t width = (int32_t)std::min<int64_t>(tile, n_chunks - lo);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
    for (int i = threadIdx.x; i < width; i += KW_THREADS) s[i] = -INFINITY;
    const int64_t q0 = q_off[b], q1 = q_off[b + 1];
    for (int64_t g = q0; g < q1; g += KW_TERM_GROUP) {
        const int ng = (int)std::min<int64_t>(KW_TERM_GROUP, q1 - g);
        // posting range of every term of the group inside [lo, lo + width): one term per wave at a time, lanes 0-31 find the
        // start and lanes 32-63 the end
        for (int j = wave; j < ng; j += KW_THREADS / 64) {
            const int32_t t = q_terms[g + j];
            int64_t a = 0, e = 0;
            if (t >= 0 && t < n_terms) {
                a = term_off[t];
                e = term_off[t + 1];
            }
            const int64_t at = lower_bound_32(post_chunk, a, e, (int32_t)(lo + (half ? width : 0)), lane, half);
            if (lane == 0) range[j][0] = at;
            if (lane == 32) range[j][1] = at;
        }
        __syncthreads();  // (also orders the -inf fill before the first update)
        for (int j = 0; j < ng; ++j) {
            const int64_t pa = range[j][0], pb = range[j][1];
            // a chunk appears at most once per term: no two threads touch one score within a term, and the barrier below orders
            // the terms.  Four postings per thread per round, their loads issued before the updates.
            for (int64_t p = pa + threadIdx.x; p < pb; p += 4 * KW_THREADS) {
                int32_t c[4];
                float v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int64_t q = p + (int64_t)u * KW_THREADS;
                    c[u] = q < pb ? post_chunk[q] : -1;
                    v[u] = q < pb ? post_impact[q] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int64_t r = (int64_t)c[u] - lo;
                    if (r < 0 || r >= width) continue;  // padding, or postings that are not sorted as the contract says
                    const float old = s[r];
                    s[r] = old == -INFINITY ? v[u] : __fadd_rn(old, v[u]);
                }
            }
            __syncthreads();
        }
    }
    float* out = scores + (int64_t)b * ld + lo;
    const uint32_t* __restrict__ filter = filter_of.of(b);
    for (int i = threadIdx.x; i < width; i += KW_THREADS) {
        float v = s[i];
        if (filter) {
            const int64_t c = lo + i;
            if (!((filter[c >> 5] >> (c & 31)) & 1u)) v = -INFINITY;
        }
        out[i] = v;
    }
}

// counts[b] = the finite entries of the selected row b (they lead it: the selection is ordered by score)
__global__ __launch_bounds__(64) void bm25_count_kernel(const float* __restrict__ sel, int32_t k, int32_t* __restrict__ counts) {
    const float* r = sel + (int64_t)blockIdx.x * k;
    int n = 0;
    for (int i = threadIdx.x; i < k; i += 64) n += r[i] != -INFINITY;
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (threadIdx.x == 0) counts[blockIdx.x] = n;
}

}  // namespace

int launch_bm25_impact(const int32_t* post_chunk, const int32_t* post_tf, const int32_t* post_term, const float* idf, const float* nrm,
                       int64_t n_postings, int32_t n_terms, int64_t n_chunks, float* post_impact, hipStream_t s) {
    if (n_postings <= 0) return RL_OK;
    hipLaunchKernelGGL(bm25_impact_kernel, dim3((unsigned)((n_postings + 255) / 256)), dim3(256), 0, s, post_chunk, post_tf, post_term, idf, nrm,
                       n_postings, n_terms, n_chunks, post_impact);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

int32_t bm25_tile(int64_t n_chunks, int32_t n_queries, int n_cu) {
    // the widest tile (fewest posting-range look-ups) that still gives every CU two blocks; never below 1024 chunks
    int32_t tile = BM25_TILE_MAX;
    while (tile > 1024 && (int64_t)n_queries * ((n_chunks + tile - 1) / tile) < 2 * (int64_t)n_cu) tile >>= 1;
    return tile;
}

int launch_bm25_score(const int64_t* term_off, const int32_t* post_chunk, const float* post_impact, int32_t n_terms, int64_t n_chunks,
                      const int64_t* q_off, const int32_t* q_terms, int32_t n_queries, const QueryMask& filter, int32_t tile, float* scores,
                      int64_t ld, hipStream_t s) {
    if (n_queries <= 0 || n_chunks <= 0) return RL_OK;
    if (tile < 256 || tile > BM25_TILE_MAX || (tile & 255)) return fail(RL_ERR_INVALID, "launch_bm25_score: bad tile");
    const int64_t tiles = (n_chunks + tile - 1) / tile;
    hipLaunchKernelGGL(bm25_score_kernel, dim3((unsigned)tiles, (unsigned)n_queries), dim3(KW_THREADS), (size_t)tile * sizeof(float), s, term_off,
                       post_chunk, post_impact, n_terms, n_chunks, q_off, q_terms, filter, tile, scores, ld);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

int launch_bm25_count(const float* sel, int32_t n_queries, int32_t k, int32_t* counts, hipStream_t s) {
    if (n_queries <= 0) return RL_OK;
    hipLaunchKernelGGL(bm25_count_kernel, dim3((unsigned)n_queries), dim3(64), 0, s, sel, k, counts);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

}  // namespace rl
