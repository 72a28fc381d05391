// Weighted Reciprocal Rank Fusion: the fusion step of the reference's hybrid search (src/raglite/_search.py:233-252,
// `reciprocal_rank_fusion`), for a batch of queries, bit for bit what the Python function returns on the same lists.
//
// Per query b there are R <= 4 ranked lists of chunk ordinals, list r at lists[(r * n_queries + b) * len ..], padded with
// entries < 0 (not results; they take no rank: rank i is the count of results before the entry in its list).  An ordinal's
// score is the float64 sum of w_r / (rrf_k + i) over its occurrences, added in the order Python's loop meets them (list 0
// first, each list in rank order), starting from +0.0, every division and addition rounded to nearest.  The result is ordered
// by score descending, equal scores by first occurrence in list 0 || list 1 || ... (Python's stable sort over the dict's
// insertion order).
//
// One workgroup per query; its n = R * len <= 4096 entries sit in LDS, 16 B each at the sort size N (n rounded up to a power of
// two, at least 8, so the usual hybrid shapes -- R = 2, len <= 100 -- sort at most 256 entries, not 4096):
//   1. an exclusive scan of the result flags gives each entry its rank i;
//   2. a bitonic sort by (ordinal, position) puts each ordinal's occurrences next to each other in position order;
//   3. the first entry of each run sums the run in that order;
//   4. a bitonic sort of the run heads by (order-preserving key of the score, descending; first position, ascending);
//   5. the first k are written.
#include <atomic>

#include "common.h"

namespace rl {
namespace {

constexpr uint32_t NONE32 = 0xffffffffu;
constexpr uint64_t NONE64 = ~0ull;
constexpr int FUSE_MAX_THREADS = 512;

struct FuseWeights {
    double w[RRF_MAX_LISTS];
};

__device__ __forceinline__ uint64_t score_key_desc(double x) {  // ascending in this key = descending in x (x finite, never -0.0)
    const uint64_t u = (uint64_t)__double_as_longlong(x);
    const uint64_t key = (u >> 63) ? ~u : (u | (1ull << 63));
    return ~key;
}

__device__ __forceinline__ double score_of_key(uint64_t desc) {
    const uint64_t key = ~desc;
    const uint64_t u = (key >> 63) ? (key & ~(1ull << 63)) : ~key;
    return __longlong_as_double((long long)u);
}

template <class T>
__device__ __forceinline__ T pick4(int r, T a, T b, T c, T d) {  // (a select chain: a runtime index into an array would go to scratch)
    return r == 0 ? a : r == 1 ? b : r == 2 ? c : d;
}

// Steps 1-5 for query b, by the whole workgroup (T = blockDim.x, a power of two, 64 .. 512); `at(p)` reads entry p of the
// concatenation list 0 || list 1 || ... (n_lists * len entries).  smem: 16 * N bytes, N >= 8:
//   sk u64[N] (the score keys of step 4; before step 3 the scan's 12 words of scratch), ord u32[N], pe u32[N] (position << 12 | rank).
// What rrf_fuse_kernel and shard_hybrid_fuse_kernel both run: the fusion rules exist once.
template <class At>
__device__ __forceinline__ void rrf_fuse_block(At at, int32_t n_lists, int32_t len, const FuseWeights& wt, int32_t rrf_k, int32_t k,
                                               int32_t N, uint64_t* smem, int b, double* __restrict__ out_scores,
                                               int32_t* __restrict__ out_ids, int32_t* __restrict__ out_counts) {
    uint64_t* sk = smem;
    uint32_t* ord = reinterpret_cast<uint32_t*>(smem + N);
    uint32_t* pe = ord + N;
    uint32_t* scratch = reinterpret_cast<uint32_t*>(sk);  // [0, 8): wave totals, [8, 12): the result count before each list
    const int T = blockDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = n_lists * len;

    // 1. ranks: thread tid owns positions [lo, hi) of the concatenation
    const int per = (n + T - 1) / T;
    const int lo = min(n, tid * per), hi = min(n, lo + per);
    int c = 0;
    for (int p = lo; p < hi; ++p) c += at(p) >= 0;
    int incl = c;
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(incl, o, 64);
        if (lane >= o) incl += y;
    }
    if (lane == 63) scratch[wave] = (uint32_t)incl;
    __syncthreads();
    int run = incl - c;
    for (int w = 0; w < wave; ++w) run += (int)scratch[w];
    for (int p = lo; p < hi; ++p) {
        const int32_t v = at(p);
        if (p % len == 0) scratch[8 + p / len] = (uint32_t)run;
        ord[p] = v >= 0 ? (uint32_t)v : NONE32;
        pe[p] = ((uint32_t)p << 12) | (uint32_t)run;  // (the global count here; the list's own base comes off in step 3)
        run += v >= 0;
    }
    for (int p = n + tid; p < N; p += T) {
        ord[p] = NONE32;
        pe[p] = NONE32;
    }
    __syncthreads();
    const uint32_t base0 = scratch[8], base1 = scratch[9], base2 = scratch[10], base3 = scratch[11];

    // 2. bitonic sort by (ordinal, position), ascending; padding (NONE32) sorts last
    for (int size = 2; size <= N; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (N >> 1); t += T) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const uint64_t a = ((uint64_t)ord[i] << 32) | pe[i], e = ((uint64_t)ord[j] << 32) | pe[j];
                if ((a > e) == ((i & size) == 0)) {
                    ord[i] = (uint32_t)(e >> 32); pe[i] = (uint32_t)e;
                    ord[j] = (uint32_t)(a >> 32); pe[j] = (uint32_t)a;
                }
            }
            __syncthreads();
        }
    }

    // 3. the head of each run sums it, in position order, from +0.0
    for (int i = tid; i < N; i += T) {
        const uint32_t o = ord[i];
        uint64_t key = NONE64;
        if (o != NONE32 && (i == 0 || ord[i - 1] != o)) {
            double s = 0.0;
            for (int j = i; j < N && ord[j] == o; ++j) {
                const uint32_t x = pe[j];
                const int p = (int)(x >> 12), r = p / len;
                const int rank = (int)((x & 0xfffu) - pick4(r, base0, base1, base2, base3));
                const double w = pick4(r, wt.w[0], wt.w[1], wt.w[2], wt.w[3]);
                s = __dadd_rn(s, __ddiv_rn(w, (double)(rrf_k + rank)));
            }
            key = score_key_desc(s);
        }
        sk[i] = key;
    }
    __syncthreads();
    for (int i = tid; i < N; i += T) pe[i] = sk[i] != NONE64 ? (pe[i] >> 12) : NONE32;  // a head's position is its first occurrence
    __syncthreads();

    // 4. bitonic sort of the heads by (score descending, first position ascending); the rest sorts last
    for (int size = 2; size <= N; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (N >> 1); t += T) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const uint64_t a = sk[i], e = sk[j];
                const uint32_t pa = pe[i], pb = pe[j];
                const bool greater = a > e || (a == e && pa > pb);
                if (greater == ((i & size) == 0)) {
                    sk[i] = e; pe[i] = pb;
                    sk[j] = a; pe[j] = pa;
                }
            }
            __syncthreads();
        }
    }

    // 5. the top k (k <= n <= N)
    for (int t = tid; t < k; t += T) {
        const uint64_t key = sk[t];
        const bool filled = key != NONE64;
        out_ids[(int64_t)b * k + t] = filled ? at((int)pe[t]) : -1;
        out_scores[(int64_t)b * k + t] = filled ? score_of_key(key) : -INFINITY;
        if (out_counts) {
            if (filled && (t + 1 == k || sk[t + 1] == NONE64)) out_counts[b] = t + 1;
            if (!filled && t == 0) out_counts[b] = 0;
        }
    }
}

// grid n_queries, block T (a power of two, 64 .. 512, T >= N / 8); dynamic LDS 16 * N bytes, N >= 8 (rrf_fuse_block's layout).
__global__ __launch_bounds__(FUSE_MAX_THREADS) void rrf_fuse_kernel(const int32_t* __restrict__ lists, int32_t n_lists, int32_t n_queries,
                                                                     int32_t len, FuseWeights wt, int32_t rrf_k, int32_t k, int32_t N,
                                                                     double* __restrict__ out_scores, int32_t* __restrict__ out_ids,
                                                                     int32_t* __restrict__ out_counts) {
    extern __shared__ uint64_t smem[];
    const int b = blockIdx.x;
    auto at = [&](int p) { return lists[((int64_t)(p / len) * n_queries + b) * len + (p % len)]; };
    rrf_fuse_block(at, n_lists, len, wt, rrf_k, k, N, smem, b, out_scores, out_ids, out_counts);
}

// ---- the fusion step of a sharded hybrid batch (rl_shard_hybrid_fuse) ----------------------------------------------------------
// Ascending bitonic sort of (key, val) pairs over [0, N) by the whole workgroup; N a power of two.
__device__ __forceinline__ void bitonic_pairs(uint64_t* key, uint32_t* val, int N) {
    const int T = blockDim.x, tid = threadIdx.x;
    for (int size = 2; size <= N; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (N >> 1); t += T) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const uint64_t a = key[i], e = key[j];
                const uint32_t va = val[i], ve = val[j];
                const bool greater = a > e || (a == e && va > ve);
                if (greater == ((i & size) == 0)) {
                    key[i] = e; val[i] = ve;
                    key[j] = a; val[j] = va;
                }
            }
            __syncthreads();
        }
    }
}

// (score desc, id asc) as an ASCENDING key (make_key64's order turned round: NaN after -inf); padding is NONE64 and sorts last
__device__ __forceinline__ uint64_t asc_key(float score, int32_t id) {
    return id >= 0 ? ~make_key64(score, (uint32_t)id) : NONE64;
}

// grid n_queries, block T (a power of two, 64 .. 512).  g: the all-gather of every rank's packed records, rank r's record block of
// query b at g + (r * n_queries + b) * W, W = 3 num_hits + (n_lists == 2 ? 2 n_each : 0): num_hits row records (score bits, global row,
// global chunk), then n_each keyword records (score bits, global chunk).  Dynamic LDS (bytes): `region` (the sorts, then the fusion's
// 16 Nf) followed by the two fused lists, int32 [n_lists * n_each]:
//   rows      key u64[Na] + val u32[Na] (val: the chunk), Na = pow2 >= world * num_hits; then k2 u64[Nh], Nh = pow2 >= num_hits
//   keywords  key u64[Nk] + val u32[Nk], Nk = pow2 >= world * n_each (reuses the start of the region)
//   fusion    rrf_fuse_block's 16 Nf bytes, Nf = pow2 >= n_lists * n_each (the start of the region again)
__global__ __launch_bounds__(FUSE_MAX_THREADS) void shard_hybrid_fuse_kernel(const int32_t* __restrict__ g, int32_t world, int32_t n_queries,
                                                                              int32_t num_hits, int32_t n_each, int32_t n_lists, FuseWeights wt,
                                                                              int32_t rrf_k, int32_t k, int32_t Na, int32_t Nh, int32_t Nk,
                                                                              int32_t Nf, int32_t region, double* __restrict__ out_scores,
                                                                              int32_t* __restrict__ out_ids, int32_t* __restrict__ out_counts) {
    extern __shared__ uint64_t smem[];
    const int b = blockIdx.x;
    const int T = blockDim.x, tid = threadIdx.x;
    const int64_t W = 3 * (int64_t)num_hits + (n_lists == 2 ? 2 * (int64_t)n_each : 0);
    int32_t* lists = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(smem) + region);
    uint64_t* key = smem;
    uint32_t* val = reinterpret_cast<uint32_t*>(key + Na);
    uint64_t* k2 = reinterpret_cast<uint64_t*>(val + Na);  // (Na >= 8: 8-byte aligned)

    // 1. load the rows; a rank that failed in its local step sent RL_ID_SHARD_MISSING somewhere in its records
    const int nr = world * num_hits;
    int missing = 0;
    for (int e = tid; e < Na; e += T) {
        uint64_t kk = NONE64;
        uint32_t c = NONE32;
        if (e < nr) {
            const int32_t* rec = g + ((int64_t)(e / num_hits) * n_queries + b) * W + 3 * (e % num_hits);
            const int32_t row = rec[1], chunk = rec[2];
            missing |= row == RL_ID_SHARD_MISSING || chunk == RL_ID_SHARD_MISSING;
            kk = asc_key(__int_as_float(rec[0]), row);
            c = (uint32_t)chunk;
        }
        key[e] = kk;
        val[e] = c;
    }
    if (n_lists == 2)
        for (int e = tid; e < world * n_each; e += T)
            missing |= g[((int64_t)(e / n_each) * n_queries + b) * W + 3 * num_hits + 2 * (e % n_each) + 1] == RL_ID_SHARD_MISSING;
    if (__syncthreads_or(missing)) {  // poisoned: a fusion that lacks a shard never looks like an answer (as rl_allgather_merge_topk)
        for (int t = tid; t < k; t += T) {
            out_scores[(int64_t)b * k + t] = __longlong_as_double(0x7ff8000000000000ll);
            out_ids[(int64_t)b * k + t] = -1;
        }
        if (out_counts && tid == 0) out_counts[b] = 0;
        return;
    }
    // ... merged by (score desc, row asc): the first num_hits real entries are the global top rows
    bitonic_pairs(key, val, Na);

    // 2. the first hit of each chunk in rank order, up to n_each: sort the top rows by (chunk, position), take the head of each run,
    //    sort the heads by position
    for (int i = tid; i < Nh; i += T) {
        const bool hit = i < num_hits && key[i] != NONE64 && (int32_t)val[i] >= 0;
        k2[i] = hit ? (((uint64_t)val[i] << 32) | (uint32_t)i) : NONE64;
        val[i] = 0;
    }
    __syncthreads();
    bitonic_pairs(k2, val, Nh);
    for (int i = tid; i < Nh; i += T) {
        const uint64_t x = k2[i];
        const bool head = x != NONE64 && (i == 0 || (k2[i - 1] >> 32) != (x >> 32));
        key[i] = head ? ((x << 32) | (x >> 32)) : NONE64;  // (position, chunk)
    }
    __syncthreads();
    bitonic_pairs(key, val, Nh);
    for (int j = tid; j < n_each; j += T) lists[j] = (j < Nh && key[j] != NONE64) ? (int32_t)(uint32_t)key[j] : -1;
    __syncthreads();

    // 3. the keyword lists merged by (score desc, chunk asc), the first n_each
    if (n_lists == 2) {
        const int nk = world * n_each;
        uint64_t* kkey = smem;
        uint32_t* kval = reinterpret_cast<uint32_t*>(kkey + Nk);
        for (int e = tid; e < Nk; e += T) {
            uint64_t kk = NONE64;
            if (e < nk) {
                const int32_t* rec = g + ((int64_t)(e / n_each) * n_queries + b) * W + 3 * num_hits + 2 * (e % n_each);
                kk = asc_key(__int_as_float(rec[0]), rec[1]);
            }
            kkey[e] = kk;
            kval[e] = 0;
        }
        __syncthreads();
        bitonic_pairs(kkey, kval, Nk);
        for (int j = tid; j < n_each; j += T) lists[n_each + j] = kkey[j] != NONE64 ? (int32_t)(0xffffffffu - (uint32_t)~kkey[j]) : -1;
        __syncthreads();
    }

    // 4. the fusion of rl_rrf_fuse over (vector list, keyword list)
    auto at = [&](int p) { return lists[p]; };
    rrf_fuse_block(at, n_lists, n_each, wt, rrf_k, k, Nf, smem, b, out_scores, out_ids, out_counts);
}

}  // namespace

int launch_rrf_fuse(const int32_t* lists, int32_t n_lists, int32_t n_queries, int32_t len, const double* weights, int32_t rrf_k, int32_t k,
                    double* out_scores, int32_t* out_ids, int32_t* out_counts, hipStream_t s) {
    if (n_queries <= 0) return RL_OK;
    if (n_lists < 1 || n_lists > RRF_MAX_LISTS || len < 1 || (int64_t)n_lists * len > RRF_MAX_ENTRIES || k < 1 || k > n_lists * len)
        return fail(RL_ERR_INVALID, "launch_rrf_fuse: bad sizes");
    FuseWeights wt{};
    for (int r = 0; r < n_lists; ++r) wt.w[r] = weights[r];
    int32_t N = 8;  // (at least 8: the scan's 12 words of scratch live in sk, 8 N bytes)
    while (N < n_lists * len) N <<= 1;
    const int T = std::min(FUSE_MAX_THREADS, std::max(64, N / 8));
    hipLaunchKernelGGL(rrf_fuse_kernel, dim3((unsigned)n_queries), dim3((unsigned)T), (size_t)N * 16, s, lists, n_lists, n_queries, len, wt, rrf_k,
                       k, N, out_scores, out_ids, out_counts);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

int launch_shard_hybrid_fuse(const int32_t* gathered, int32_t world, int32_t n_queries, int32_t num_hits, int32_t n_each, int32_t n_lists,
                             const double* weights, int32_t rrf_k, int32_t k, double* out_scores, int32_t* out_ids, int32_t* out_counts,
                             hipStream_t s) {
    if (n_queries <= 0) return RL_OK;
    if (world < 1 || num_hits < 1 || n_each < 1 || n_lists < 1 || n_lists > 2 || k < 1 || k > n_lists * n_each)
        return fail(RL_ERR_INVALID, "launch_shard_hybrid_fuse: bad sizes");
    if ((int64_t)world * num_hits > SHARD_FUSE_MAX_ENTRIES || (n_lists == 2 && (int64_t)world * n_each > SHARD_FUSE_MAX_ENTRIES))
        return fail(RL_ERR_UNSUPPORTED, "rl_shard_hybrid_fuse: world * num_hits and world * n_each must be <= 4096");
    FuseWeights wt{};
    for (int r = 0; r < n_lists; ++r) wt.w[r] = weights[r];
    auto pow2 = [](int64_t x) { int32_t N = 8; while (N < x) N <<= 1; return N; };
    const int32_t Na = pow2((int64_t)world * num_hits), Nh = pow2(num_hits), Nk = n_lists == 2 ? pow2((int64_t)world * n_each) : 8;
    const int32_t Nf = pow2((int64_t)n_lists * n_each);
    const int32_t region = std::max({12 * Na + 8 * Nh, 12 * Nk, 16 * Nf});
    const size_t lds = (size_t)region + (size_t)4 * n_lists * n_each;
    const int32_t T = std::min(FUSE_MAX_THREADS, std::max(64, std::max({Na, Nk, Nf}) / 8));
    // (at most 12 * 4096 + 8 * 4096 + 4 * 4096 = 96 KiB; the kernel's own static LDS counts against the 160 KiB too)
    static std::atomic<size_t> lds_allowed{64 * 1024};
    if (lds > lds_allowed.load()) {
        RL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(shard_hybrid_fuse_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        lds_allowed.store(lds);
    }
    hipLaunchKernelGGL(shard_hybrid_fuse_kernel, dim3((unsigned)n_queries), dim3((unsigned)T), lds, s, gathered, world, n_queries, num_hits,
                       n_each, n_lists, wt, rrf_k, k, Na, Nh, Nk, Nf, region, out_scores, out_ids, out_counts);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

}  // namespace rl
