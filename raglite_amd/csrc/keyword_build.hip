// Building the BM25 postings on the device (rl_keyword_store_count; driven from api_keyword.hip).  The store keeps each chunk's term ids
// chunk-major (tok_off / tok_term); the postings are term-major.  The transposition is
//   1. emit     (key = term_rank[tok_term], value = chunk) for the tokens of live chunks, in token order
//   2. sort     stable LSD radix sort on the key alone, 8-bit digits: per pass a per-block digit histogram, an exclusive scan of the
//               (digit, block) table and a scatter with a stable in-block rank.  Stability keeps the chunks ascending within a term.
//   3. encode   equal neighbouring (term, chunk) pairs form one posting; its run length is the term frequency
//   4. derive   term_off[t] = lower bound of t in post_term; df = its differences
// Every phase is its own launch: no kernel waits on another workgroup.  The only atomics are integer min / max of kb_minmax_kernel,
// whose result does not depend on arrival order.  Positions and totals are 64-bit throughout.
#include "common.h"

namespace rl {
namespace {

constexpr int KB_THREADS = 256;
constexpr int KB_SCAN_ITEMS = 8;                            // consecutive items per thread of the scan and encode kernels
constexpr int KB_SCAN_TILE = KB_THREADS * KB_SCAN_ITEMS;    // 2048
constexpr int KB_SORT_ROUNDS = 16;                          // keys per thread of a sort block, one per round
constexpr int KB_SORT_TILE = KB_THREADS * KB_SORT_ROUNDS;   // 4096

// Inclusive scan of one int64 per thread over the block (the shape of block_inclusive_scan in select.hip); scratch: one slot per wave.
__device__ __forceinline__ int64_t block_inclusive_scan64(int64_t v, int64_t* scratch, int64_t& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int64_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    __syncthreads();
    if (lane == 63) scratch[w] = x;
    __syncthreads();
    int64_t base = 0, t = 0;
    for (int i = 0; i < nw; ++i) {
        if (i < w) base += scratch[i];
        t += scratch[i];
    }
    total = t;
    return x + base;
}

// data[tile] -> its exclusive scan within the tile; sums[block] = the tile's total
__global__ __launch_bounds__(KB_THREADS) void kb_scan_tile_kernel(int64_t* __restrict__ data, int64_t n, int64_t* __restrict__ sums) {
    __shared__ int64_t scratch[KB_THREADS / 64];
    const int64_t first = (int64_t)blockIdx.x * KB_SCAN_TILE + (int64_t)threadIdx.x * KB_SCAN_ITEMS;
    int64_t v[KB_SCAN_ITEMS], s = 0;
#pragma unroll
    for (int j = 0; j < KB_SCAN_ITEMS; ++j) {
        v[j] = first + j < n ? data[first + j] : 0;
        s += v[j];
    }
    int64_t total;
    int64_t run = block_inclusive_scan64(s, scratch, total) - s;
#pragma unroll
    for (int j = 0; j < KB_SCAN_ITEMS; ++j) {
        if (first + j < n) data[first + j] = run;
        run += v[j];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// data[i] += base[i / KB_SCAN_TILE] (base: the scanned tile totals)
__global__ __launch_bounds__(KB_THREADS) void kb_add_base_kernel(int64_t* __restrict__ data, int64_t n, const int64_t* __restrict__ base) {
    const int64_t i = (int64_t)blockIdx.x * KB_THREADS + threadIdx.x;
    if (i < n) data[i] += base[i / KB_SCAN_TILE];
}

// length[c] = the tokens of a live chunk, 0 for a dead one
__global__ __launch_bounds__(KB_THREADS) void kb_length_kernel(const int64_t* __restrict__ tok_off, const uint8_t* __restrict__ live, int64_t n_chunks,
                                                                int64_t* __restrict__ length) {
    const int64_t c = (int64_t)blockIdx.x * KB_THREADS + threadIdx.x;
    if (c < n_chunks) length[c] = live[c] ? tok_off[c + 1] - tok_off[c] : 0;
}

// Token i of the store belongs to the chunk c with tok_off[c] <= i < tok_off[c + 1] (binary search: a chunk of any length, and a run
// of empty chunks, take the same route); a live chunk's tokens go to out_off[c] + (i - tok_off[c]), in token order.
__global__ __launch_bounds__(KB_THREADS) void kb_emit_kernel(const int64_t* __restrict__ tok_off, const int32_t* __restrict__ tok_term,
                                                              const uint8_t* __restrict__ live, const int64_t* __restrict__ out_off,
                                                              const int32_t* __restrict__ term_rank, int32_t n_terms, int64_t n_chunks,
                                                              int64_t n_tokens, int64_t m, uint32_t* __restrict__ keys, int32_t* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * KB_THREADS + threadIdx.x;
    if (i >= n_tokens) return;
    int64_t lo = 0, hi = n_chunks;  // the first c in (0, n_chunks] with tok_off[c] > i, minus one
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (tok_off[mid + 1] > i) hi = mid;
        else lo = mid + 1;
    }
    const int64_t c = lo;
    if (c >= n_chunks || !live[c]) return;
    const int64_t dst = out_off[c] + (i - tok_off[c]);
    if (dst < 0 || dst >= m) return;  // (cannot happen with the store's own arrays)
    const int32_t id = tok_term[i];
    int32_t key = id;
    if (term_rank) key = (id >= 0 && id < n_terms) ? term_rank[id] : 0;  // (the store checks its ids against n_terms before any launch)
    keys[dst] = (uint32_t)key;
    vals[dst] = (int32_t)c;
}

// The lanes of the wave that hold the same digit as this one (valid lanes only): one wave64 ballot per digit bit.  Every lane of the
// wave must call.
__device__ __forceinline__ uint64_t digit_peers(uint32_t d, bool valid) {
    uint64_t peers = __builtin_amdgcn_ballot_w64(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const uint64_t m = __builtin_amdgcn_ballot_w64(bit);
        peers &= bit ? m : ~m;
    }
    return peers;
}

// table[digit * n_blocks + block] = the keys of the block's tile with that digit
__global__ __launch_bounds__(KB_THREADS) void kb_hist_kernel(const uint32_t* __restrict__ keys, int64_t m, int shift, int64_t n_blocks,
                                                              int64_t* __restrict__ table) {
    __shared__ uint32_t wave_cnt[KB_THREADS / 64][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int i = 0; i < KB_THREADS / 64; ++i) wave_cnt[i][threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * KB_SORT_TILE;
#pragma unroll 4
    for (int r = 0; r < KB_SORT_ROUNDS; ++r) {
        const int64_t i = base + (int64_t)r * KB_THREADS + threadIdx.x;
        const bool valid = i < m;
        const uint32_t d = valid ? (keys[i] >> shift) & 255u : 0u;
        const uint64_t peers = digit_peers(d, valid);
        // the first lane of each group of peers counts for all of them; each wave owns its row, so no atomics
        if (valid && (peers & ((uint64_t(1) << lane) - 1)) == 0) wave_cnt[w][d] += (uint32_t)__builtin_popcountll(peers);
    }
    __syncthreads();
    uint32_t n = 0;
    for (int i = 0; i < KB_THREADS / 64; ++i) n += wave_cnt[i][threadIdx.x];
    table[(int64_t)threadIdx.x * n_blocks + blockIdx.x] = n;
}

// table: the exclusive scan of kb_hist_kernel's counts = where the block's first key of each digit goes.  Within the tile, keys are
// taken in index order (round, wave, lane), so equal digits keep their order: the sort is stable.
__global__ __launch_bounds__(KB_THREADS) void kb_scatter_kernel(const uint32_t* __restrict__ keys_in, const int32_t* __restrict__ vals_in, int64_t m,
                                                                 int shift, int64_t n_blocks, const int64_t* __restrict__ table,
                                                                 uint32_t* __restrict__ keys_out, int32_t* __restrict__ vals_out) {
    __shared__ int64_t running[256];                       // per digit: the next free output position of this block
    __shared__ uint32_t wave_cnt[KB_THREADS / 64][256];    // per wave and digit: the keys of the current round
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    running[threadIdx.x] = table[(int64_t)threadIdx.x * n_blocks + blockIdx.x];
    for (int i = 0; i < KB_THREADS / 64; ++i) wave_cnt[i][threadIdx.x] = 0;
    const int64_t base = (int64_t)blockIdx.x * KB_SORT_TILE;
    uint32_t key[KB_SORT_ROUNDS];
    int32_t val[KB_SORT_ROUNDS];
#pragma unroll
    for (int r = 0; r < KB_SORT_ROUNDS; ++r) {  // (all loads issued before the first barrier)
        const int64_t i = base + (int64_t)r * KB_THREADS + threadIdx.x;
        key[r] = i < m ? keys_in[i] : 0u;
        val[r] = i < m ? vals_in[i] : 0;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < KB_SORT_ROUNDS; ++r) {
        const int64_t i = base + (int64_t)r * KB_THREADS + threadIdx.x;
        const bool valid = i < m;
        const uint32_t d = (key[r] >> shift) & 255u;
        const uint64_t peers = digit_peers(d, valid);
        const int rank = __builtin_popcountll(peers & ((uint64_t(1) << lane) - 1));
        if (valid && rank == 0) wave_cnt[w][d] = (uint32_t)__builtin_popcountll(peers);
        __syncthreads();
        if (valid) {
            int64_t pos = running[d] + rank;
            for (int j = 0; j < w; ++j) pos += wave_cnt[j][d];
            if (pos >= 0 && pos < m) {  // (always, with a table scanned from this pass's histogram)
                keys_out[pos] = key[r];
                vals_out[pos] = val[r];
            }
        }
        __syncthreads();
        uint32_t n = 0;
        for (int j = 0; j < KB_THREADS / 64; ++j) {
            n += wave_cnt[j][threadIdx.x];
            wave_cnt[j][threadIdx.x] = 0;
        }
        running[threadIdx.x] += n;
        __syncthreads();
    }
}

__device__ __forceinline__ bool is_head(const uint32_t* __restrict__ keys, const int32_t* __restrict__ vals, int64_t i) {
    return i == 0 || keys[i] != keys[i - 1] || vals[i] != vals[i - 1];
}

// heads[block] = the postings that start inside the block's tile
__global__ __launch_bounds__(KB_THREADS) void kb_rle_count_kernel(const uint32_t* __restrict__ keys, const int32_t* __restrict__ vals, int64_t m,
                                                                   int64_t* __restrict__ heads) {
    __shared__ int64_t scratch[KB_THREADS / 64];
    const int64_t first = (int64_t)blockIdx.x * KB_SCAN_TILE + (int64_t)threadIdx.x * KB_SCAN_ITEMS;
    int64_t n = 0;
#pragma unroll
    for (int j = 0; j < KB_SCAN_ITEMS; ++j)
        if (first + j < m) n += is_head(keys, vals, first + j);
    int64_t total;
    (void)block_inclusive_scan64(n, scratch, total);
    if (threadIdx.x == 0) heads[blockIdx.x] = total;
}

// heads: the exclusive scan of kb_rle_count_kernel's counts.  Posting p starts at head_pos[p] of the sorted stream.
__global__ __launch_bounds__(KB_THREADS) void kb_rle_write_kernel(const uint32_t* __restrict__ keys, const int32_t* __restrict__ vals, int64_t m,
                                                                   const int64_t* __restrict__ heads, int64_t n_postings,
                                                                   int32_t* __restrict__ post_term, int32_t* __restrict__ post_chunk,
                                                                   int64_t* __restrict__ head_pos) {
    __shared__ int64_t scratch[KB_THREADS / 64];
    const int64_t first = (int64_t)blockIdx.x * KB_SCAN_TILE + (int64_t)threadIdx.x * KB_SCAN_ITEMS;
    bool head[KB_SCAN_ITEMS];
    int64_t n = 0;
#pragma unroll
    for (int j = 0; j < KB_SCAN_ITEMS; ++j) {
        head[j] = first + j < m && is_head(keys, vals, first + j);
        n += head[j];
    }
    int64_t total;
    int64_t p = heads[blockIdx.x] + block_inclusive_scan64(n, scratch, total) - n;
#pragma unroll
    for (int j = 0; j < KB_SCAN_ITEMS; ++j) {
        if (!head[j]) continue;
        if (p >= 0 && p < n_postings) {  // (always)
            post_term[p] = (int32_t)keys[first + j];
            post_chunk[p] = vals[first + j];
            head_pos[p] = first + j;
        }
        ++p;
    }
}

// post_tf[p] = the run length of posting p (runs cross tiles: the next head may be anywhere)
__global__ __launch_bounds__(KB_THREADS) void kb_tf_kernel(const int64_t* __restrict__ head_pos, int64_t n_postings, int64_t m,
                                                            int32_t* __restrict__ post_tf) {
    const int64_t p = (int64_t)blockIdx.x * KB_THREADS + threadIdx.x;
    if (p >= n_postings) return;
    const int64_t next = p + 1 < n_postings ? head_pos[p + 1] : m;
    post_tf[p] = (int32_t)(next - head_pos[p]);
}

// term_off[t] = the first posting whose term is >= t, t in [0, n_terms]: one thread per term
__global__ __launch_bounds__(KB_THREADS) void kb_term_off_kernel(const int32_t* __restrict__ post_term, int64_t n_postings, int32_t n_terms,
                                                                  int64_t* __restrict__ term_off) {
    const int64_t t = (int64_t)blockIdx.x * KB_THREADS + threadIdx.x;
    if (t > n_terms) return;
    int64_t lo = 0, hi = n_postings;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)post_term[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    term_off[t] = lo;
}

__global__ __launch_bounds__(KB_THREADS) void kb_df_kernel(const int64_t* __restrict__ term_off, int32_t n_terms, int64_t* __restrict__ df) {
    const int64_t t = (int64_t)blockIdx.x * KB_THREADS + threadIdx.x;
    if (t < n_terms) df[t] = term_off[t + 1] - term_off[t];
}

// out[0] = min(out[0], ids), out[1] = max(out[1], ids): integer min / max, the same whatever the arrival order
__global__ __launch_bounds__(KB_THREADS) void kb_minmax_kernel(const int32_t* __restrict__ ids, int64_t n, int32_t* __restrict__ out) {
    int32_t lo = 0x7fffffff, hi = -0x7fffffff - 1;
    for (int64_t i = (int64_t)blockIdx.x * KB_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * KB_THREADS) {
        const int32_t v = ids[i];
        lo = std::min(lo, v);
        hi = std::max(hi, v);
    }
    for (int o = 32; o > 0; o >>= 1) {
        lo = std::min(lo, __shfl_xor(lo, o, 64));
        hi = std::max(hi, __shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(out, lo);
        atomicMax(out + 1, hi);
    }
}

unsigned blocks_of(int64_t n, int64_t per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

size_t kb_scan_scratch_items(int64_t n) {
    size_t items = 0;
    do {
        n = (n + KB_SCAN_TILE - 1) / KB_SCAN_TILE;
        items += (size_t)n;
    } while (n > 1);
    return items;
}

int launch_kb_exclusive_scan(int64_t* data, int64_t n, int64_t* scratch, const int64_t** total, hipStream_t s) {
    if (n <= 0) return fail(RL_ERR_INVALID, "launch_kb_exclusive_scan: nothing to scan");
    int64_t* level[8];
    int64_t level_n[8];
    int levels = 0;
    int64_t* cur = data;
    int64_t cur_n = n;
    for (;;) {  // 2048-fold per level: 2^63 items would take six
        const int64_t nb = (cur_n + KB_SCAN_TILE - 1) / KB_SCAN_TILE;
        hipLaunchKernelGGL(kb_scan_tile_kernel, dim3((unsigned)nb), dim3(KB_THREADS), 0, s, cur, cur_n, scratch);
        level[levels] = cur;
        level_n[levels] = cur_n;
        ++levels;
        if (nb == 1) break;
        cur = scratch;
        cur_n = nb;
        scratch += nb;
    }
    *total = scratch;
    for (int l = levels - 2; l >= 0; --l)
        hipLaunchKernelGGL(kb_add_base_kernel, dim3(blocks_of(level_n[l], KB_THREADS)), dim3(KB_THREADS), 0, s, level[l], level_n[l], level[l + 1]);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

int launch_kb_lengths(const int64_t* tok_off, const uint8_t* live, int64_t n_chunks, int64_t* length, hipStream_t s) {
    if (n_chunks <= 0) return RL_OK;
    hipLaunchKernelGGL(kb_length_kernel, dim3(blocks_of(n_chunks, KB_THREADS)), dim3(KB_THREADS), 0, s, tok_off, live, n_chunks, length);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

int launch_kb_emit(const int64_t* tok_off, const int32_t* tok_term, const uint8_t* live, const int64_t* out_off, const int32_t* term_rank,
                   int32_t n_terms, int64_t n_chunks, int64_t n_tokens, int64_t m, uint32_t* keys, int32_t* vals, hipStream_t s) {
    if (n_tokens <= 0 || m <= 0) return RL_OK;
    hipLaunchKernelGGL(kb_emit_kernel, dim3(blocks_of(n_tokens, KB_THREADS)), dim3(KB_THREADS), 0, s, tok_off, tok_term, live, out_off, term_rank,
                       n_terms, n_chunks, n_tokens, m, keys, vals);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

int kb_sort_passes(int32_t n_terms) {
    int bits = 0;
    for (uint32_t top = n_terms > 1 ? (uint32_t)(n_terms - 1) : 0u; top; top >>= 1) ++bits;
    return std::max(1, (bits + 7) / 8);
}

int64_t kb_sort_blocks(int64_t m) { return (m + KB_SORT_TILE - 1) / KB_SORT_TILE; }

int launch_kb_sort_pass(const uint32_t* keys_in, const int32_t* vals_in, int64_t m, int pass, int64_t* table, int64_t* scan_scratch,
                        uint32_t* keys_out, int32_t* vals_out, hipStream_t s) {
    if (m <= 0) return RL_OK;
    const int64_t nb = kb_sort_blocks(m);
    hipLaunchKernelGGL(kb_hist_kernel, dim3((unsigned)nb), dim3(KB_THREADS), 0, s, keys_in, m, 8 * pass, nb, table);
    RL_HIP(hipGetLastError());
    const int64_t* total;
    RL_TRY(launch_kb_exclusive_scan(table, 256 * nb, scan_scratch, &total, s));
    hipLaunchKernelGGL(kb_scatter_kernel, dim3((unsigned)nb), dim3(KB_THREADS), 0, s, keys_in, vals_in, m, 8 * pass, nb, table, keys_out, vals_out);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

int64_t kb_rle_blocks(int64_t m) { return (m + KB_SCAN_TILE - 1) / KB_SCAN_TILE; }

int launch_kb_rle_count(const uint32_t* keys, const int32_t* vals, int64_t m, int64_t* heads, hipStream_t s) {
    if (m <= 0) return RL_OK;
    hipLaunchKernelGGL(kb_rle_count_kernel, dim3((unsigned)kb_rle_blocks(m)), dim3(KB_THREADS), 0, s, keys, vals, m, heads);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

int launch_kb_rle_write(const uint32_t* keys, const int32_t* vals, int64_t m, const int64_t* heads, int64_t n_postings, int32_t* post_term,
                        int32_t* post_chunk, int32_t* post_tf, int64_t* head_pos, hipStream_t s) {
    if (m <= 0 || n_postings <= 0) return RL_OK;
    hipLaunchKernelGGL(kb_rle_write_kernel, dim3((unsigned)kb_rle_blocks(m)), dim3(KB_THREADS), 0, s, keys, vals, m, heads, n_postings, post_term,
                       post_chunk, head_pos);
    hipLaunchKernelGGL(kb_tf_kernel, dim3(blocks_of(n_postings, KB_THREADS)), dim3(KB_THREADS), 0, s, head_pos, n_postings, m, post_tf);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

int launch_kb_term_off(const int32_t* post_term, int64_t n_postings, int32_t n_terms, int64_t* term_off, int64_t* df, hipStream_t s) {
    hipLaunchKernelGGL(kb_term_off_kernel, dim3(blocks_of((int64_t)n_terms + 1, KB_THREADS)), dim3(KB_THREADS), 0, s, post_term, n_postings, n_terms,
                       term_off);
    if (n_terms > 0 && df) hipLaunchKernelGGL(kb_df_kernel, dim3(blocks_of(n_terms, KB_THREADS)), dim3(KB_THREADS), 0, s, term_off, n_terms, df);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

int launch_kb_minmax(const int32_t* ids, int64_t n, int32_t* out, hipStream_t s) {
    if (n <= 0) return RL_OK;
    const unsigned grid = (unsigned)std::min<int64_t>(1024, (n + KB_THREADS - 1) / KB_THREADS);
    hipLaunchKernelGGL(kb_minmax_kernel, dim3(grid), dim3(KB_THREADS), 0, s, ids, n, out);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

}  // namespace rl
