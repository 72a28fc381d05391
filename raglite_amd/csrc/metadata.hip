// Metadata filters on the device: the reference's JSON containment `metadata @> filter` (src/raglite/_search.py:82-94) over tag ids.
// The host numbers the (key, value) pairs (raglite_amd/_metadata.py); a chunk is the ascending, duplicate-free list of its tags, a
// filter the tags it wants, and a chunk matches a filter when its list holds every one of them.  One launch evaluates a batch of
// filters and writes each one's bitset over chunk ordinals -- the `chunk_filters` table the *_per_query searches read -- together with
// the number of matching chunks and of their embedding rows.
#include "common.h"

namespace rl {
namespace {

// Is t in the ascending list L[0 .. n)?
__device__ __forceinline__ bool holds_tag(const int32_t* __restrict__ L, int32_t n, int32_t t) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (L[mid] < t) lo = mid + 1; else hi = mid;
    }
    return lo < n && L[lo] == t;
}

// One lane per chunk (grid x), MF_GROUP filters per grid y.  The chunk side is read once for all filters of the group: the workgroup
// stages the contiguous slice of its chunks' tags in LDS (a chunk whose list ends past the staged part reads HBM), then walks the
// filters, whose tags come through LDS in pieces of whole filters.  Per 64 chunks and filter: one ballot, lanes 0 and 32 store one word
// each (every word of the table is written; chunks past n_chunks vote no, so the tail bits are zero).  The counts go through a wave
// reduction and LDS into one 64-bit integer atomic per (workgroup, filter that matched).
__global__ __launch_bounds__(MF_BLOCK) void metadata_filters_kernel(const int64_t* __restrict__ tag_off, const int32_t* __restrict__ tags,
                                                                     int64_t n_chunks, const int64_t* __restrict__ row_off,
                                                                     const int64_t* __restrict__ f_off, const int32_t* __restrict__ f_tags,
                                                                     int32_t n_filters, uint32_t* __restrict__ bits, int64_t words,
                                                                     unsigned long long* __restrict__ counts) {
    __shared__ int32_t s_tags[MF_STAGE_TAGS];
    __shared__ int32_t s_ftags[MF_FILTER_TAGS];
    __shared__ int32_t s_foff[MF_GROUP + 1];
    __shared__ unsigned long long s_cnt[2 * MF_GROUP];  // (chunks, rows) per filter of the group
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int64_t c0 = (int64_t)blockIdx.x * MF_BLOCK;  // (< n_chunks: the grid covers no more)
    const int64_t c = c0 + tid;
    const int64_t c1 = c0 + MF_BLOCK < n_chunks ? c0 + MF_BLOCK : n_chunks;
    const int64_t t0 = tag_off[c0];
    const int64_t span = tag_off[c1] - t0;
    const int32_t staged = (int32_t)(span < MF_STAGE_TAGS ? span : MF_STAGE_TAGS);
    for (int32_t i = tid; i < staged; i += MF_BLOCK) s_tags[i] = tags[t0 + i];
    const int32_t j0 = (int32_t)blockIdx.y * MF_GROUP;
    const int32_t nj = n_filters - j0 < MF_GROUP ? n_filters - j0 : MF_GROUP;
    const int64_t fbase = f_off[j0];
    for (int32_t i = tid; i <= nj; i += MF_BLOCK) s_foff[i] = (int32_t)(f_off[j0 + i] - fbase);
    for (int32_t i = tid; i < 2 * nj; i += MF_BLOCK) s_cnt[i] = 0;
    // this lane's chunk: its list [lo, lo + n) of `tags`, in LDS at lo - t0 when it ends inside the staged part
    const bool valid = c < n_chunks;
    int64_t lo = 0;
    int32_t n = 0;
    unsigned long long rows = 0;
    if (valid) {
        lo = tag_off[c];
        n = (int32_t)(tag_off[c + 1] - lo);
        rows = (unsigned long long)(row_off[c + 1] - row_off[c]);
    }
    const bool in_lds = valid && lo - t0 + n <= staged;
    const int32_t* g_list = tags + lo;
    const int32_t* s_list = s_tags + (in_lds ? (int32_t)(lo - t0) : 0);
    const int64_t w = c >> 5;
    __syncthreads();  // s_tags, s_foff and s_cnt are written
    int32_t jp = 0;
    while (jp < nj) {
        // the next piece: the filters [jp, je) whose tags fit the LDS piece together; a single filter with more tags reads them from HBM
        int32_t je = jp;
        while (je < nj && s_foff[je + 1] - s_foff[jp] <= MF_FILTER_TAGS) ++je;
        const bool big = je == jp;
        if (big) je = jp + 1;
        const int32_t pbase = s_foff[jp];
        const int32_t pn = big ? 0 : s_foff[je] - pbase;
        __syncthreads();  // (the previous piece has been read)
        for (int32_t i = tid; i < pn; i += MF_BLOCK) s_ftags[i] = f_tags[fbase + pbase + i];
        __syncthreads();
        for (int32_t j = jp; j < je; ++j) {
            const int32_t fb = s_foff[j], m = s_foff[j + 1] - fb;
            bool ok = valid;
            for (int32_t i = 0; i < m && ok; ++i) {
                const int32_t t = big ? f_tags[fbase + fb + i] : s_ftags[fb - pbase + i];
                ok = in_lds ? holds_tag(s_list, n, t) : holds_tag(g_list, n, t);
            }
            const uint64_t b = __builtin_amdgcn_ballot_w64(ok);
            if ((lane & 31) == 0 && w < words) bits[(int64_t)(j0 + j) * words + w] = (uint32_t)(lane ? (b >> 32) : b);
            if (b) {  // (wave-uniform)
                unsigned long long r = ok ? rows : 0ull;
                for (int o = 32; o > 0; o >>= 1) r += __shfl_xor(r, o, 64);
                if (lane == 0) {
                    atomicAdd(&s_cnt[2 * j], (unsigned long long)__builtin_popcountll(b));
                    atomicAdd(&s_cnt[2 * j + 1], r);
                }
            }
        }
        jp = je;
    }
    __syncthreads();
    for (int32_t j = tid; j < nj; j += MF_BLOCK) {
        if (s_cnt[2 * j]) {
            atomicAdd(counts + (j0 + j), s_cnt[2 * j]);
            atomicAdd(counts + n_filters + (j0 + j), s_cnt[2 * j + 1]);
        }
    }
}

}  // namespace

int launch_metadata_filters(const int64_t* tag_off, const int32_t* tags, int64_t n_chunks, const int64_t* row_off, const int64_t* f_off,
                            const int32_t* f_tags, int32_t n_filters, uint32_t* bits, unsigned long long* counts, hipStream_t s) {
    if (n_filters <= 0) return RL_OK;
    RL_HIP(hipMemsetAsync(counts, 0, (size_t)2 * n_filters * sizeof(unsigned long long), s));
    if (n_chunks <= 0) return RL_OK;
    const int64_t words = (n_chunks + 31) >> 5;
    const dim3 grid((unsigned)((n_chunks + MF_BLOCK - 1) / MF_BLOCK), (unsigned)((n_filters + MF_GROUP - 1) / MF_GROUP));
    hipLaunchKernelGGL(metadata_filters_kernel, grid, dim3(MF_BLOCK), 0, s, tag_off, tags, n_chunks, row_off, f_off, f_tags, n_filters, bits,
                       words, counts);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

}  // namespace rl
