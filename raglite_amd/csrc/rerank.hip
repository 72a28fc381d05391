// The order of a reranked candidate list: what `MaxSimRanker.rank` (raglite_amd/_search.py) does on the host with
// `np.lexsort((arange, -key))`, key = where(isnan(s), -inf, s), for a batch of queries -- the step between rl_maxsim_rerank's
// scores and the reference's `chunks[result.doc_id]` (src/raglite/_search.py:394-396).
//
// Per query b there are n_cand (score, candidate) pairs.  A candidate < 0 is padding: it comes after every real candidate and is
// not counted.  The real ones are ordered by score descending, NaN ranking as -inf, -0.0 equal to +0.0 (NumPy's comparison), equal
// keys by position (stable).  The first k are written: the score's own bits (a NaN stays that NaN, -0.0 stays -0.0), the candidate
// and its position in the input list, each re-read from the inputs through the position.
//
// One workgroup per query; one 64-bit key per entry in LDS at the sort size N (n_cand rounded up to a power of two): the high word
// is the order-preserving score key turned round for descending, the low word the position, padding all-ones.  The keys of the real
// entries are distinct, so a key-only bitonic sort gives the stable order.
#include "common.h"

namespace rl {
namespace {

constexpr uint64_t NONE64 = ~0ull;
constexpr int RERANK_MAX_THREADS = 512;

// Ascending in this key = descending in the ranker's key.  NaN -> -inf and -0.0 -> +0.0 are folded on the bits (what `s + 0.0f`
// does to -0.0, without an addition that a flushed denormal could change).  Never 0xffffffff: score_key is 0 for NaN alone.
__device__ __forceinline__ uint32_t rank_key_desc(uint32_t bits) {
    const uint32_t mag = bits & 0x7fffffffu;
    if (mag > 0x7f800000u) bits = 0xff800000u;  // NaN ranks as -inf
    if (mag == 0u) bits = 0u;                   // -0.0 == +0.0
    return ~score_key(__uint_as_float(bits));
}

// grid n_queries, block T (a power of two, 64 .. 512); dynamic LDS 8 * N bytes, N a power of two >= n_cand, k <= n_cand.
__global__ __launch_bounds__(RERANK_MAX_THREADS) void rerank_order_kernel(const uint32_t* __restrict__ scores, const int32_t* __restrict__ cand,
                                                                           int32_t n_cand, int32_t k, int32_t N,
                                                                           uint32_t* __restrict__ out_scores, int32_t* __restrict__ out_chunks,
                                                                           int32_t* __restrict__ out_pos, int32_t* __restrict__ out_counts) {
    extern __shared__ uint64_t key[];
    const int T = blockDim.x, tid = threadIdx.x;
    const int64_t in = (int64_t)blockIdx.x * n_cand, out = (int64_t)blockIdx.x * k;

    for (int p = tid; p < N; p += T) {
        uint64_t x = NONE64;
        if (p < n_cand && cand[in + p] >= 0) x = ((uint64_t)rank_key_desc(scores[in + p]) << 32) | (uint32_t)p;
        key[p] = x;
    }
    __syncthreads();

    for (int size = 2; size <= N; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (N >> 1); t += T) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const uint64_t a = key[i], e = key[j];
                if ((a > e) == ((i & size) == 0)) {
                    key[i] = e;
                    key[j] = a;
                }
            }
            __syncthreads();
        }
    }

    for (int t = tid; t < k; t += T) {
        const uint64_t x = key[t];
        const bool filled = x != NONE64;
        const int32_t p = (int32_t)(uint32_t)x;  // (< n_cand when filled)
        out_scores[out + t] = filled ? scores[in + p] : 0xff800000u;
        out_chunks[out + t] = filled ? cand[in + p] : -1;
        out_pos[out + t] = filled ? p : -1;
        if (out_counts) {
            if (filled && (t + 1 == k || key[t + 1] == NONE64)) out_counts[blockIdx.x] = t + 1;
            if (!filled && t == 0) out_counts[blockIdx.x] = 0;
        }
    }
}

}  // namespace

int launch_rerank_order(const float* scores, const int32_t* candidates, int32_t n_queries, int32_t n_cand, int32_t k, float* out_scores,
                        int32_t* out_chunks, int32_t* out_pos, int32_t* out_counts, hipStream_t s) {
    if (n_queries <= 0) return RL_OK;
    if (k < 1 || k > n_cand || n_cand > RERANK_MAX_ENTRIES) return fail(RL_ERR_INVALID, "launch_rerank_order: bad sizes");
    int32_t N = 1;
    while (N < n_cand) N <<= 1;
    const int T = std::min(RERANK_MAX_THREADS, std::max(64, N / 8));
    hipLaunchKernelGGL(rerank_order_kernel, dim3((unsigned)n_queries), dim3((unsigned)T), (size_t)N * 8, s,
                       reinterpret_cast<const uint32_t*>(scores), candidates, n_cand, k, N, reinterpret_cast<uint32_t*>(out_scores), out_chunks,
                       out_pos, out_counts);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

}  // namespace rl
