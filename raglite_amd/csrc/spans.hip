// Chunk spans: what the reference's `retrieve_chunk_spans` (src/raglite/_search.py:323-361) does to a ranked list of chunks, for a
// batch of queries, on chunk ordinals: score the chunks by their place in the list, add their neighbours, deduplicate, order by
// (document, index), cut into runs of consecutive indices, sum each run's scores and order the runs by that sum.
//
// The span table (rl_span_table, api_retrieval.hip) holds the live chunks sorted by (doc, pos), doc being the dense number of the chunk's
// document_id in sorted order: rank_of[ordinal] (-1: no position), tab_key[rank] = doc << 32 | pos and tab_ord[rank].
//
// Per query b there are n_in entries, best first, and n_off offsets; E = n_in * (1 + n_off) <= 4096 slots.
//   1. An entry is kept if its ordinal is in range and has a position; its rank i is the number of kept entries before it (`:324`,
//      after retrieve_chunks dropped unknown ids) and its score 1.0 / (i + 1).  Slot p * (1 + n_off) takes the key
//      table rank << 32 | (n_in - 1 - p) << 12 | i; slot p * (1 + n_off) + 1 + j the chunk at (doc, pos + offsets[j]) if the table
//      holds one (`:328-340`), as table rank << 32 | 0x80000000.  The chunk lies within |offset| ranks of the entry's own, so the
//      lookup is a binary search over that window of tab_key.
//   2. A bitonic sort of the keys: by table rank, i.e. (doc, pos) (`:342`); within a chunk the last appearance in the input comes
//      first -- the one whose score stands (`:324`, a dict written in list order) -- and neighbours, which carry no score, last.
//   3. The head of each run of equal ranks is that chunk (`set(chunks)`, `:342`): compacted to rank[u] and info[u] (i, or "neighbour").
//   4. Chunk u starts a span unless tab_key[rank[u]] == tab_key[rank[u - 1]] + 1: the same doc and the next pos (`:345-353`).
//   5. One lane walks one span and adds its members' scores in ascending pos order from 0.0 (`:356-358`, `sum()` before CPython
//      3.12): __dadd_rn / __ddiv_rn, no reassociation.  A neighbour adds 0.0 (`.get(chunk.id, 0.0)`).
//   6. A bitonic sort of the spans by (score descending, first chunk ascending) (`:355-360`, a stable sort(reverse=True)).  The
//      scores are finite and >= +0.0, so their bits order as integers.
//   7. The spans are written in that order: their scores and lengths, and their chunks' ordinals in ascending pos.
//
// One workgroup per query, 16 bytes of LDS per slot at the sort size N (E rounded up to a power of two, at least 16):
//   X u64[N]   the keys of steps 1-3; from step 5 the span keys (the complemented score bits)
//   R u32[N]   the table rank of unique chunk u
//   I u16[N]   its info: bits 0-11 the rank i of the entry whose score stands, bit 12 neighbour only, bit 15 starts a span
//   S u16[N]   the first chunk u of span s (the payload of step 6)
// The wave totals of the four scans sit in whichever of these the step at hand does not use.
#include "common.h"

namespace rl {
namespace {

constexpr uint64_t NONE64 = ~0ull;
constexpr uint32_t NEIGHBOUR_LOW = 0x80000000u;
constexpr uint32_t INFO_RANK = 0x0fffu, INFO_NEIGHBOUR = 0x1000u, INFO_START = 0x8000u;
constexpr int SPANS_MAX_THREADS = 512;

struct SpanOffsets {
    int32_t v[SPANS_MAX_OFFSETS];
};

// Exclusive scan of v over the workgroup (blockDim.x a multiple of 64, at most 512); `total` is the sum.  scratch: 8 words that no
// thread reads or writes for anything else between the two barriers.  Every thread of the workgroup calls it.
__device__ __forceinline__ int block_scan_excl(int v, uint32_t* scratch, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    int incl = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(incl, o, 64);
        if (lane >= o) incl += y;
    }
    __syncthreads();  // (what the callers wrote before may alias scratch)
    if (lane == 63) scratch[wave] = (uint32_t)incl;
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < n_waves; ++w) {
        const int x = (int)scratch[w];
        if (w < wave) base += x;
        tot += x;
    }
    __syncthreads();
    total = tot;
    return base + incl - v;
}

// grid n_queries, block T (a power of two, 64 .. 512); dynamic LDS 16 * N bytes, N a power of two, max(16, E) <= N <= 4096.
__global__ __launch_bounds__(SPANS_MAX_THREADS) void chunk_spans_kernel(
    const int32_t* __restrict__ rank_of, const uint64_t* __restrict__ tab_key, const int32_t* __restrict__ tab_ord, int32_t n_chunks,
    int32_t n_live, const int32_t* __restrict__ chunks, int32_t n_in, SpanOffsets offs, int32_t n_off, int32_t N,
    int32_t* __restrict__ out_chunks, int32_t* __restrict__ out_span_len, double* __restrict__ out_span_scores,
    int32_t* __restrict__ out_n_spans, int32_t* __restrict__ out_n_chunks) {
    extern __shared__ uint64_t smem[];
    uint64_t* X = smem;
    uint32_t* R = reinterpret_cast<uint32_t*>(smem + N);
    uint16_t* I = reinterpret_cast<uint16_t*>(R + N);
    uint16_t* S = I + N;
    const int T = blockDim.x, tid = threadIdx.x;
    const int stride = 1 + n_off, E = n_in * stride;
    const int64_t in = (int64_t)blockIdx.x * n_in, out = (int64_t)blockIdx.x * E;

    // 1. the kept entries, their ranks and keys (scan scratch: R), then their neighbours
    for (int e = tid; e < N; e += T) X[e] = NONE64;
    int run = 0;
    for (int p0 = 0; p0 < n_in; p0 += T) {
        const int p = p0 + tid;
        int32_t r = -1;
        if (p < n_in) {
            const int32_t c = chunks[in + p];
            if (c >= 0 && c < n_chunks) r = rank_of[c];
        }
        int total;
        const int i = run + block_scan_excl(r >= 0, R, total);
        run += total;
        if (r >= 0) X[p * stride] = ((uint64_t)(uint32_t)r << 32) | ((uint32_t)(n_in - 1 - p) << 12) | (uint32_t)i;
    }
    __syncthreads();
    for (int e = tid; e < E; e += T) {
        const int p = e / stride, j = e - p * stride;
        if (j == 0) continue;
        const uint64_t own = X[p * stride];
        if (own == NONE64) continue;
        const int64_t r = (int64_t)(own >> 32), off = offs.v[j - 1];
        const uint64_t tk = tab_key[r];
        const int64_t pos = (int64_t)(uint32_t)tk + off;
        if (pos < 0 || pos > 0x7fffffffll) continue;
        const uint64_t want = (tk & 0xffffffff00000000ull) | (uint64_t)pos;
        const int64_t d = off < 0 ? -off : off;
        int64_t lo = max((int64_t)0, r - d), hi = min((int64_t)n_live, r + d + 1);  // [lo, hi): where (doc, pos + off) can be
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (tab_key[mid] < want) lo = mid + 1; else hi = mid;
        }
        if (lo < n_live && lo <= r + d && tab_key[lo] == want) X[e] = ((uint64_t)lo << 32) | NEIGHBOUR_LOW;
    }
    __syncthreads();

    // 2. by (doc, pos); within a chunk the entry whose score stands first
    for (int size = 2; size <= N; size <<= 1) {
        for (int st = size >> 1; st > 0; st >>= 1) {
            for (int t = tid; t < (N >> 1); t += T) {
                const int i = 2 * t - (t & (st - 1)), j = i + st;
                const uint64_t a = X[i], e = X[j];
                if ((a > e) == ((i & size) == 0)) {
                    X[i] = e;
                    X[j] = a;
                }
            }
            __syncthreads();
        }
    }

    // 3. the unique chunks (scan scratch: S)
    int nu = 0;
    for (int t0 = 0; t0 < N; t0 += T) {
        const int t = t0 + tid;  // (< N: T divides N or N < T)
        uint64_t x = NONE64;
        bool head = false;
        if (t < N) {
            x = X[t];
            head = x != NONE64 && (t == 0 || (uint32_t)(X[t - 1] >> 32) != (uint32_t)(x >> 32));
        }
        int total;
        const int u = nu + block_scan_excl(head, reinterpret_cast<uint32_t*>(S), total);
        nu += total;
        if (head) {
            const uint32_t low = (uint32_t)x;
            R[u] = (uint32_t)(x >> 32);
            I[u] = (uint16_t)((low & NEIGHBOUR_LOW) ? INFO_NEIGHBOUR : (low & INFO_RANK));
        }
    }
    __syncthreads();

    // 4. the span starts (scan scratch: X, which step 3 was the last to read)
    int ns = 0;
    for (int u0 = 0; u0 < nu; u0 += T) {
        const int u = u0 + tid;
        bool start = false;
        if (u < nu) start = u == 0 || tab_key[R[u]] != tab_key[R[u - 1]] + 1;
        int total;
        const int s = ns + block_scan_excl(start, reinterpret_cast<uint32_t*>(X), total);
        ns += total;
        if (start) {
            S[s] = (uint16_t)u;
            I[u] = (uint16_t)(I[u] | INFO_START);
        }
    }
    __syncthreads();

    // 5. one lane sums one span, left to right
    int N2 = 1;
    while (N2 < ns) N2 <<= 1;
    for (int s = tid; s < N2; s += T) {
        uint64_t key = NONE64;
        if (s < ns) {
            double sum = 0.0;
            int u = S[s];
            do {
                const uint32_t info = I[u];
                const double x = (info & INFO_NEIGHBOUR) ? 0.0 : __ddiv_rn(1.0, (double)((int)(info & INFO_RANK) + 1));
                sum = __dadd_rn(sum, x);
                ++u;
            } while (u < nu && !(I[u] & INFO_START));
            key = ~(uint64_t)__double_as_longlong(sum);
        } else {
            S[s] = 0xffffu;  // (after every real span: their S is < 4096)
        }
        X[s] = key;
    }
    __syncthreads();

    // 6. by (score descending, first chunk ascending)
    for (int size = 2; size <= N2; size <<= 1) {
        for (int st = size >> 1; st > 0; st >>= 1) {
            for (int t = tid; t < (N2 >> 1); t += T) {
                const int i = 2 * t - (t & (st - 1)), j = i + st;
                const uint64_t a = X[i], e = X[j];
                const uint16_t sa = S[i], se = S[j];
                const bool greater = a > e || (a == e && sa > se);
                if (greater == ((i & size) == 0)) {
                    X[i] = e; S[i] = se;
                    X[j] = a; S[j] = sa;
                }
            }
            __syncthreads();
        }
    }

    // 7. the scores and lengths, then (scan scratch: X) the chunks; the rest of the slots is padding
    auto span_len = [&](int s) {
        const int first = S[s];
        int u = first + 1;
        while (u < nu && !(I[u] & INFO_START)) ++u;
        return u - first;
    };
    for (int s = tid; s < E; s += T) {
        out_span_scores[out + s] = s < ns ? __longlong_as_double((long long)~X[s]) : 0.0;
        out_span_len[out + s] = s < ns ? span_len(s) : 0;
    }
    for (int u = nu + tid; u < E; u += T) out_chunks[out + u] = -1;
    __syncthreads();
    int at = 0;
    for (int s0 = 0; s0 < ns; s0 += T) {
        const int s = s0 + tid;
        const int len = s < ns ? span_len(s) : 0;
        int total;
        const int to = at + block_scan_excl(len, reinterpret_cast<uint32_t*>(X), total);
        at += total;
        if (s < ns) {
            const int first = S[s];
            for (int j = 0; j < len; ++j) out_chunks[out + to + j] = tab_ord[R[first + j]];
        }
    }
    if (tid == 0) {
        out_n_spans[blockIdx.x] = ns;
        out_n_chunks[blockIdx.x] = nu;
    }
}

}  // namespace

int launch_chunk_spans(const int32_t* rank_of, const uint64_t* tab_key, const int32_t* tab_ord, int32_t n_chunks, int32_t n_live,
                       const int32_t* chunks, int32_t n_queries, int32_t n_in, const int32_t* offsets, int32_t n_off, int32_t* out_chunks,
                       int32_t* out_span_len, double* out_span_scores, int32_t* out_n_spans, int32_t* out_n_chunks, hipStream_t s) {
    if (n_queries <= 0) return RL_OK;
    if (n_in < 1 || n_off < 0 || n_off > SPANS_MAX_OFFSETS || (int64_t)n_in * (1 + n_off) > SPANS_MAX_ENTRIES)
        return fail(RL_ERR_INVALID, "launch_chunk_spans: bad sizes");
    SpanOffsets offs{};
    for (int32_t j = 0; j < n_off; ++j) offs.v[j] = offsets[j];
    const int32_t E = n_in * (1 + n_off);
    int32_t N = 16;
    while (N < E) N <<= 1;
    const int T = std::min(SPANS_MAX_THREADS, std::max(64, N / 8));
    hipLaunchKernelGGL(chunk_spans_kernel, dim3((unsigned)n_queries), dim3((unsigned)T), (size_t)N * 16, s, rank_of, tab_key, tab_ord, n_chunks,
                       n_live, chunks, n_in, offs, n_off, N, out_chunks, out_span_len, out_span_scores, out_n_spans, out_n_chunks);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

}  // namespace rl
