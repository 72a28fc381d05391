// The chunklet partition of src/raglite/_split_chunklets.py:136-178.  The reference cuts a document's sentences
// into chunklets by an exact shortest path over split positions, in float64:
//   dp[0] = 0,   dp[i] = min over j in [lo(i), i) of dp[j] + cost(j, i),   lo(i) = the smallest j with chars(j .. i) <= max_size
//   cost(j, i) = ((1.0 - p[j]) + (pb[i] - pb[j + 1])) + (s - 3.0)^2 / sqrt(max(s, 1e-6)) / 2.0,   s = ps[i] - ps[j]
// with p the Markdown boundary probabilities, pb / ps the prefix sums of p and of the sentences' statement counts (taken strictly left
// to right, np.cumsum's order).  The smallest j wins a tie (the reference's `<=` under backward iteration); +inf takes part in ties, so
// behind a sentence longer than max_size the back-pointers go to the window's first position, and an empty window leaves dp[i] = inf,
// back[i] = -1; NaN never wins.  The backtrack is `i = back[n]; while i > 0`.  raglite_amd/_chunklets.py: chunklet_dp is the host
// statement of the same recurrence, and the two agree bit for bit.  The square is x * x (the reference's NumPy scalar `** 2` goes
// through libm pow, which differs from x * x in the last bit for about one value in a thousand): objectives are pinned against the
// statement, partitions against the reference.
// Batched over documents (doc_batch.h), every phase its own launch, no atomics:
//   cd_prefix_kernel  one wave per document: the character prefix by a wave scan (integers: any order gives the same sum); the two
//                     float64 prefixes by ONE running sum that every lane carries through the 64 values of a block in order
//                     (a scan would re-associate); status (2: a non-finite input, else 1: a sentence longer than max_size)
//   cd_lo_kernel      one lane per sentence: lo(i) by binary search over the character prefix
//   chunklet_dp_kernel  one wave per document: the recurrence (lanes stride over the window), the backtrack (lane 0)
// Prefix arrays hold n_d + 1 entries per document: document d (rows [b, e)) owns entries [b + d, e + d] of each, and e <= n keeps
// entry e + d inside their n + n_docs.  Scratch per entry:
// pc, lo, back int64 + pb, ps, dp float64 (48 bytes).  dp lives in global memory (L2-resident for the window a step reads): an LDS
// ring over the window would cap the window's width, and the kernel has no per-document limit.
//
// Bits: no operation in this file may be fused or re-associated.  `#pragma clang fp contract(off)` below covers every expression of
// the file (hipcc's default contracts a * b + c into an fma across statements); the build has no -ffast-math, so `/` and sqrt are the
// IEEE double operations.
#include "doc_batch.h"

#include <cmath>
#include <limits>

#pragma clang fp contract(off)

namespace rl {
namespace {

constexpr long long CD_NONE = std::numeric_limits<long long>::max();

__global__ __launch_bounds__(256) void cd_prefix_kernel(const double* __restrict__ boundary, const double* __restrict__ statements,
                                                         const int64_t* __restrict__ lengths, const int64_t* __restrict__ off,
                                                         int64_t n_docs, int64_t n, int64_t max_size, int64_t* __restrict__ pc,
                                                         double* __restrict__ pb, double* __restrict__ ps, int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
    for (int64_t doc = wave0; doc < n_docs; doc += n_waves) {
        int64_t b, e;
        doc_rows(off, doc, n, &b, &e);
        const int64_t base = b + doc;
        if (lane == 0) { pc[base] = 0; pb[base] = 0.0; ps[base] = 0.0; }
        long long carry = 0;
        double run_b = 0.0, run_s = 0.0;  // the running sums, the same value in every lane
        int bad = 0;
        for (int64_t blk = b; blk < e; blk += 64) {
            const int64_t i = blk + lane;
            const bool ok = i < e;
            long long x = ok ? (long long)lengths[i] : 0;
            const double vb = ok ? boundary[i] : 0.0, vs = ok ? statements[i] : 0.0;
            if (ok) {
                if (x > max_size) bad |= 1;
                if (!isfinite(vb) || !isfinite(vs)) bad |= 2;
            }
            const long long incl = wave_prefix_step(x, lane, &carry);
            double mine_b = 0.0, mine_s = 0.0;
#pragma unroll 1  // unrolled, the 64 broadcast values fill the register file (256 VGPRs, spilled SGPRs)
            for (int k = 0; k < 64; ++k) {  // left to right; np.cumsum starts from the first element itself, not from 0.0 + it
                const double tb = __shfl(vb, k, 64), ts = __shfl(vs, k, 64);
                const bool first = blk == b && k == 0;
                run_b = first ? tb : run_b + tb;
                run_s = first ? ts : run_s + ts;
                if (lane == k) { mine_b = run_b; mine_s = run_s; }
            }
            if (ok) {
                pc[base + (i - b) + 1] = incl;
                pb[base + (i - b) + 1] = mine_b;
                ps[base + (i - b) + 1] = mine_s;
            }
        }
        const int any1 = __any(bad & 1), any2 = __any(bad & 2);
        if (lane == 0) status[doc] = any2 ? 2 : (any1 ? 1 : 0);
    }
}

__global__ __launch_bounds__(256) void cd_lo_kernel(const int64_t* __restrict__ pc, const int64_t* __restrict__ off, int64_t n_docs,
                                                     int64_t n, int64_t max_size, int64_t* __restrict__ lo_out) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    int64_t b, e;
    const int64_t doc = doc_of(off, n_docs, r);
    doc_rows(off, doc, n, &b, &e);
    if (r < b || r >= e) return;
    const int64_t base = b + doc, i = r - b + 1;  // position i in 1 .. n_d
    const int64_t pci = pc[base + i];
    int64_t lo = 0, hi = i;  // the smallest j in [0, i] with pc[i] - pc[j] <= max_size (j = i always holds; pc does not descend)
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (pci - pc[base + mid] <= max_size) hi = mid; else lo = mid + 1;
    }
    lo_out[base + i] = lo;
}

__global__ __launch_bounds__(256) void chunklet_dp_kernel(const double* __restrict__ boundary, const int64_t* __restrict__ off,
                                                           int64_t n_docs, int64_t n, const double* __restrict__ pb,
                                                           const double* __restrict__ ps, const int64_t* __restrict__ lo_in,
                                                           const int32_t* __restrict__ status, double* dp, int64_t* back,
                                                           uint8_t* __restrict__ cut, double* __restrict__ objective) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
    for (int64_t doc = wave0; doc < n_docs; doc += n_waves) {
        int64_t b, e;
        doc_rows(off, doc, n, &b, &e);
        const int64_t nd = e - b, base = b + doc;
        if (status[doc] == 2) {
            if (lane == 0 && objective) objective[doc] = NAN;
            continue;
        }
        const double* P = boundary + b;
        const double* PB = pb + base;
        const double* PS = ps + base;
        const int64_t* LO = lo_in + base;
        double* DP = dp + base;
        int64_t* BK = back + base;
        if (lane == 0) { DP[0] = 0.0; BK[0] = -1; }
        __threadfence_block();  // lane 0's dp[0] before the other lanes' reads
        double last = 0.0;      // dp[n_d]: 0 for an empty document
        for (int64_t i = 1; i <= nd; ++i) {
            int64_t lo = LO[i];
            lo = lo < 0 ? 0 : (lo > i ? i : lo);
            const double pbi = PB[i], psi = PS[i];
            double bv = INFINITY;
            long long bj = CD_NONE;
            for (int64_t j = lo + lane; j < i; j += 64) {  // the lane's own best: strict <, ascending j; +inf selectable, NaN not
                const double bc = (1.0 - P[j]) + (pbi - PB[j + 1]);
                const double s = psi - PS[j];
                const double d = s - 3.0;
                const double sc = d * d / sqrt(1e-6 > s ? 1e-6 : s) / 2.0;
                const double v = DP[j] + (bc + sc);
                if (!(v != v) && (bj == CD_NONE || v < bv)) { bv = v; bj = j; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {  // the minimum value, then the smallest j that holds it; a lane without a candidate is (inf, none)
                const double tv = __shfl_xor(bv, o, 64);
                const long long tj = __shfl_xor(bj, o, 64);
                if (tv < bv || (tv == bv && tj < bj)) { bv = tv; bj = tj; }
            }
            if (lane == 0) {
                DP[i] = bv;
                BK[i] = bj == CD_NONE ? -1 : bj;
            }
            last = bv;
            __threadfence_block();  // lane 0's dp[i] before the other lanes' reads of the next step
        }
        if (lane == 0) {
            if (objective) objective[doc] = last;
            int64_t i = nd > 0 ? BK[nd] : -1;
            for (int64_t steps = 0; i > 0 && i < nd && steps < nd; ++steps) {  // back[i] < i: at most n_d steps
                cut[b + i - 1] = 1;
                i = BK[i];
            }
        }
    }
}
}  // namespace

// scratch: int64 pc, lo, back + double pb, ps, dp, each of n + n_docs entries
size_t chunklet_dp_scratch_bytes(int64_t n, int64_t n_docs) { return (size_t)(n + n_docs) * 48 + 64; }

int launch_chunklet_dp(const double* boundary, const double* statements, const int64_t* lengths, const int64_t* doc_off, int64_t n,
                       int64_t n_docs, int64_t max_size, uint8_t* cut, double* objective, int32_t* status, void* scratch, hipStream_t s) {
    if (n <= 0 || n_docs <= 0) return RL_OK;
    const int64_t m = n + n_docs;
    int64_t* pc = static_cast<int64_t*>(scratch);
    int64_t* lo = pc + m;
    int64_t* back = lo + m;
    double* pb = reinterpret_cast<double*>(back + m);
    double* ps = pb + m;
    double* dp = ps + m;
    RL_HIP(hipMemsetAsync(cut, 0, (size_t)n, s));
    const int wblocks = wave_per_item_blocks(n_docs);
    hipLaunchKernelGGL(cd_prefix_kernel, dim3(wblocks), dim3(256), 0, s, boundary, statements, lengths, doc_off, n_docs, n, max_size, pc,
                       pb, ps, status);
    hipLaunchKernelGGL(cd_lo_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pc, doc_off, n_docs, n, max_size, lo);
    hipLaunchKernelGGL(chunklet_dp_kernel, dim3(wblocks), dim3(256), 0, s, boundary, doc_off, n_docs, n, pb, ps, lo, status, dp, back, cut,
                       objective);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

}  // namespace rl
