// The chunk partition of src/raglite/_split_chunks.py:87-113 without a MILP solver.  The reference minimises
// cost . x over binary x (x[j] = split after chunklet j) such that every window of chunklets that overflows max_size holds a split.
// The windows [i, end[i]) have ascending ends, so the optimum is a shortest path over split positions:
//   g[j] = cost[j] + min over the admissible predecessors p of g[p]   (float64, one addition per step, nothing re-associated)
// where p < j is admissible when no window lies strictly between p and j (p + 1 >= W or end[p + 1] > j), "no predecessor" (0.0)
// when window 0 reaches past j.  The admissible p are the range [lo(j), j - 1] with lo non-decreasing.  Ties: "no predecessor"
// beats an equal g[p]; among predecessors, and among last cuts, the smallest p wins.  raglite_amd/_chunking.py: partition_dp is
// the host statement of the same recurrence, and the two agree bit for bit.
// Batched over documents (doc_batch.h), every phase its own launch:
//   pd_prefix_kernel  one wave per document: inclusive prefix sums of the sizes, status (1: a size > max_size; 2: a non-finite cost
//                     or, from rl_split_chunks, a row of zero / NaN norm)
//   pd_ends_kernel    one lane per chunklet: end[i] = #{k : csum[k] <= start[i] + max_size} by binary search
//   ps_headings_kernel  (rl_split_chunks only) the Markdown-heading adjustments of :73-86, elementwise
//   partition_dp_kernel  one wave per document: W, the recurrence, the last cut, the backtrack
// Scratch per chunklet: csum, end, prev int64 + g float64 (32 bytes).  No per-document length limit.
#include "doc_batch.h"

#include <cmath>
#include <limits>

namespace rl {
namespace {

constexpr int64_t I64_MAX = std::numeric_limits<int64_t>::max();

__global__ __launch_bounds__(256) void pd_prefix_kernel(const int64_t* __restrict__ sizes, const float* __restrict__ cost,
                                                         const float* __restrict__ inv_norm, const int64_t* __restrict__ off,
                                                         int64_t n_docs, int64_t n, int64_t max_size, int64_t* __restrict__ csum,
                                                         int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
    for (int64_t doc = wave0; doc < n_docs; doc += n_waves) {
        int64_t b, e;
        doc_rows(off, doc, n, &b, &e);
        long long carry = 0;
        int bad = 0;
        for (int64_t base = b; base < e; base += 64) {
            const int64_t i = base + lane;
            const bool ok = i < e;
            long long x = ok ? (long long)sizes[i] : 0;
            if (ok) {
                if (x > max_size) bad |= 1;
                if (i + 1 < e && !isfinite(cost[i])) bad |= 2;
                if (inv_norm && !(inv_norm[i] < INFINITY)) bad |= 2;  // 1 / |x_i|: inf for a zero row, NaN for a NaN row
            }
            const long long incl = wave_prefix_step(x, lane, &carry);
            if (ok) csum[i] = incl;
        }
        const int any1 = __any(bad & 1), any2 = __any(bad & 2);
        if (lane == 0) status[doc] = any1 ? 1 : (any2 ? 2 : 0);
    }
}

__global__ __launch_bounds__(256) void pd_ends_kernel(const int64_t* __restrict__ csum, const int64_t* __restrict__ off, int64_t n_docs,
                                                       int64_t n, int64_t max_size, int64_t* __restrict__ end) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int64_t b, e;
    doc_rows(off, doc_of(off, n_docs, i), n, &b, &e);
    if (i < b || i >= e) { end[i] = 0; return; }
    const int64_t start = i > b ? csum[i - 1] : 0;
    const int64_t target = start > I64_MAX - max_size ? I64_MAX : start + max_size;
    int64_t lo = 0, hi = e - b;  // the count of k with csum[b + k] <= target (np.searchsorted, side="right")
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (csum[b + mid] <= target) lo = mid + 1; else hi = mid;
    }
    end[i] = lo;
}

// _chunking._apply_headings elementwise.  The sequential loop sets sim[i] = 1 at a heading i <= n_doc - 2 and divides sim[i - 1] by 4
// when chunklet i - 1 is none: entry i ends as 1 if it is a heading (the division at step i + 1 needs "previous is no heading"),
// else as sim[i] / 4 if i + 1 <= n_doc - 2 is one, else untouched; the first step never reaches back (prev_is_heading starts true).
// In place: entry i depends on sim[i] and the flags alone.
__global__ __launch_bounds__(256) void ps_headings_kernel(float* __restrict__ cost, const uint8_t* __restrict__ heading,
                                                           const int64_t* __restrict__ off, int64_t n_docs, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int64_t b, e;
    doc_rows(off, doc_of(off, n_docs, i), n, &b, &e);
    if (i < b || i + 1 >= e) return;  // i <= n_doc - 2 only
    if (heading[i]) cost[i] = 1.0f;
    else if (i + 2 < e && heading[i + 1]) cost[i] = cost[i] / 4;
}

// The smallest-p minimum of g[b + lo .. b + hi): every lane keeps its own (strict <, ascending p), the wave takes the minimum value and
// then the smallest p among the lanes that hold it; *val = g at that p, taken from the lane that read it.  -1 when the range is empty.
__device__ __forceinline__ int64_t pd_wave_argmin(const double* g, int64_t b, int64_t lo, int64_t hi, int lane, double* val) {
    double bv = INFINITY;
    long long bp = -1;
    for (int64_t p = lo + lane; p < hi; p += 64) {
        const double v = g[b + p];
        if (bp < 0 || v < bv) { bv = v; bp = p; }
    }
    double mv = bv;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double t = __shfl_xor(mv, o, 64);
        if (t < mv) mv = t;
    }
    long long cand = (bp >= 0 && bv == mv) ? bp : (long long)I64_MAX;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long t = __shfl_xor(cand, o, 64);
        if (t < cand) cand = t;
    }
    if (cand == (long long)I64_MAX) { *val = INFINITY; return -1; }
    const unsigned long long holders = __ballot(bp == cand);
    *val = __shfl(bv, __ffsll((long long)holders) - 1, 64);
    return cand;
}

__global__ __launch_bounds__(256) void partition_dp_kernel(const float* __restrict__ cost, const int64_t* __restrict__ off, int64_t n_docs,
                                                            int64_t n, const int64_t* __restrict__ end,
                                                            const int32_t* __restrict__ status, double* g, int64_t* prev,
                                                            uint8_t* __restrict__ cut, double* __restrict__ objective) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
    for (int64_t doc = wave0; doc < n_docs; doc += n_waves) {
        int64_t b, e;
        doc_rows(off, doc, n, &b, &e);
        const int64_t nd = e - b, m = nd - 1;  // m split positions
        if (status[doc] != 0) {
            if (lane == 0 && objective) objective[doc] = NAN;
            continue;
        }
        int64_t W = 0;  // windows i < W: the first i in [0, m) whose end reaches nd (ends ascend), m if none does
        if (m > 0) {
            int64_t lo = 0, hi = m;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (end[b + mid] >= nd) hi = mid; else lo = mid + 1;
            }
            W = lo;
        }
        if (W == 0) {  // nd <= 1, or everything fits: no cut
            if (lane == 0 && objective) objective[doc] = 0.0;
            continue;
        }
        int64_t lo = 0;
        const int64_t end0 = end[b];
        for (int64_t j = 0; j < m; ++j) {
            while (lo < j - 1 && lo + 1 < W && end[b + lo + 1] <= j) ++lo;
            double pv = INFINITY;
            int64_t pp = -1;
            if (j > 0 && (lo + 1 >= W || end[b + lo + 1] > j)) pp = pd_wave_argmin(g, b, lo, j, lane, &pv);
            if (end0 > j && !(pv < 0.0)) { pv = 0.0; pp = -1; }  // "no predecessor" wins a tie
            if (lane == 0) {
                g[b + j] = (double)cost[b + j] + pv;
                prev[b + j] = pp;
            }
            __threadfence_block();  // lane 0's g[j] before the other lanes' reads of the next step
        }
        double best;
        const int64_t last = pd_wave_argmin(g, b, W - 1, m, lane, &best);
        if (lane == 0) {
            if (objective) objective[doc] = best;
            int64_t p = last;
            for (int64_t steps = 0; p >= 0 && p < m && steps < m; ++steps) {  // prev[p] < p: at most m steps
                cut[b + p] = 1;
                p = prev[b + p];
            }
        }
    }
}
}  // namespace

// scratch: int64 csum[n], end[n], prev[n] + double g[n]
size_t partition_dp_scratch_bytes(int64_t n) { return (size_t)n * 32 + 64; }

int launch_partition_headings(float* cost, const uint8_t* heading, const int64_t* doc_off, int64_t n_docs, int64_t n, hipStream_t s) {
    if (n <= 0 || n_docs <= 0) return RL_OK;
    hipLaunchKernelGGL(ps_headings_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, cost, heading, doc_off, n_docs, n);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

int launch_partition_dp(const float* cost, const int64_t* sizes, const float* inv_norm, const int64_t* doc_off, int64_t n, int64_t n_docs,
                        int64_t max_size, uint8_t* cut, double* objective, int32_t* status, void* scratch, hipStream_t s) {
    if (n <= 0 || n_docs <= 0) return RL_OK;
    int64_t* csum = static_cast<int64_t*>(scratch);
    int64_t* end = csum + n;
    int64_t* prev = end + n;
    double* g = reinterpret_cast<double*>(prev + n);
    RL_HIP(hipMemsetAsync(cut, 0, (size_t)n, s));
    const int wblocks = wave_per_item_blocks(n_docs);
    hipLaunchKernelGGL(pd_prefix_kernel, dim3(wblocks), dim3(256), 0, s, sizes, cost, inv_norm, doc_off, n_docs, n, max_size, csum, status);
    hipLaunchKernelGGL(pd_ends_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, csum, doc_off, n_docs, n, max_size, end);
    hipLaunchKernelGGL(partition_dp_kernel, dim3(wblocks), dim3(256), 0, s, cost, doc_off, n_docs, n, end, status, g, prev, cut, objective);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

}  // namespace rl
