// The sentence partition of src/raglite/_split_sentences.py:183-218: everything the reference does with the
// model's boundary probability per character, batched over documents (doc_batch.h).
//   override     probas[k] = known[k] where known[k] is finite, cast to the dtype of probas (:185-186)
//   propagation  a range [i, j): i a non-space character followed by a space, j the first non-space character after that run;
//                probas[i : j-1] = min(probas[i : j]), probas[j-1] = max(probas[i : j]) (:188-196).  A run without a character before
//                it, or without one after it in the document, stays as it is.  min and max are exact and the ranges are disjoint (a
//                range writes nothing at j), so every range is one thread's and the phase works in place.
//   scores       probas - 0.25 in the dtype of probas, widened to float64 (:74)
//   phase 1      dp[i] = s[i], or best_prev + s[i] if best_prev > -inf and best_prev + s[i] > s[i]; best_prev the running maximum of
//                dp[first_valid .. i - min_len] under strict > (the EARLIEST of equals); the final boundary the earliest maximum under
//                strict > from 0.0 (:79-94, :115-125)
//   phase 2      every phase-1 sentence longer than max_len again, on its slice of the propagated probabilities, with the predecessor
//                the maximum of the finite dp[j], j in [i - max_len, i - min_len], the LATEST of equals (the reference's deque pops
//                on <=); a first boundary only if i + 1 <= max_len; the final boundary the earliest maximum over
//                [max(first_valid, n - max_len - 1), last_valid] from -inf (:95-125)
// Every float64 add is the reference's, in its order.  raglite_amd/_sentences.py: sentence_partition is the host statement of the whole
// call and agrees bit for bit.
// Every phase its own launch on the caller's stream, no atomics, no kernel waits on another workgroup:
//   sd_classify_kernel   one thread per character: the white-space class of the code point (str.isspace: 29 code points), the
//                        override, the value widened to float64 (exact), and bad[doc] = 1 by a plain store where the value is not
//                        finite (every writer stores the same word)
//   sd_propagate_kernel  one thread per character; the thread at a range's first character walks the run (of any length) twice
//   sd_phase1_kernel     one document per wave, 64 positions per block: the scores come in one coalesced load, then all lanes walk the
//                        64 positions in order with the same state (the reference's loop; lane k keeps position k's dp and back);
//                        dp[i - min_len] comes from the block's own lanes or from one coalesced load at the block's start.  The final
//                        maximum is tracked on the way; lane 0 backtracks.
//   sd_phase2_kernel     one document per wave walks its phase-1 sentences in turn (64 cut bytes per ballot) and solves the long ones
//                        one after the other: lanes stride over the window, one butterfly on (value, index).  A compacted list of
//                        long sentences with a wave each would need a count, a scan and two more launches for what is the exception
//                        (a table, a line without punctuation); the price is that one document's long sentences are solved in series.
// Scratch per character: the propagated probability float64, dp float64, back int32 (relative to the document in phase 1, to the
// sentence in phase 2), the space byte; per document the bad word.  dp lives in global memory, as in chunklet_dp.hip.
#include "doc_batch.h"

#include <cmath>
#include <limits>

#pragma clang fp contract(off)

namespace rl {
namespace {

constexpr int64_t SD_DOC_MAX = 2147483647;  // back is int32: the cap every doc_rows of this file passes

__device__ __forceinline__ bool sd_is_space(uint32_t c) {  // str.isspace
    return (c >= 0x0009u && c <= 0x000Du) || (c >= 0x001Cu && c <= 0x0020u) || c == 0x0085u || c == 0x00A0u || c == 0x1680u ||
           (c >= 0x2000u && c <= 0x200Au) || c == 0x2028u || c == 0x2029u || c == 0x202Fu || c == 0x205Fu || c == 0x3000u;
}

// probas - 0.25 in the dtype of probas, widened (p holds a float exactly when f32)
__device__ __forceinline__ double sd_score(double p, int f32) { return f32 ? (double)((float)p - 0.25f) : p - 0.25; }

// Lane k's value in every lane; k is the same in all lanes (a loop counter), so this is two v_readlane_b32 and not a trip through the
// LDS crossbar: the walk of phase 1 waits on it 64 times per block.
__device__ __forceinline__ double sd_lane(double v, int k) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), k), hi = __builtin_amdgcn_readlane(__double2hiint(v), k);
    return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(256) void sd_classify_kernel(const uint32_t* __restrict__ cp, const void* __restrict__ probas, int f32,
                                                           const double* __restrict__ known, const int64_t* __restrict__ off,
                                                           int64_t n_docs, int64_t n, double* __restrict__ P, uint8_t* __restrict__ SP,
                                                           int32_t* bad) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        SP[i] = sd_is_space(cp[i]) ? 1 : 0;
        const double k = known ? known[i] : NAN;
        double p;
        if (f32) {
            float q = static_cast<const float*>(probas)[i];
            if (isfinite(k)) q = (float)k;
            p = (double)q;
        } else {
            p = static_cast<const double*>(probas)[i];
            if (isfinite(k)) p = k;
        }
        P[i] = p;
        if (!isfinite(p)) {
            int64_t b, e;
            const int64_t doc = doc_of(off, n_docs, i);
            doc_rows(off, doc, n, &b, &e, SD_DOC_MAX);
            if (i >= b && i < e) bad[doc] = 1;
        }
    }
}

__global__ __launch_bounds__(256) void sd_propagate_kernel(const uint8_t* __restrict__ SP, const int64_t* __restrict__ off,
                                                            int64_t n_docs, int64_t n, double* P) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        if (SP[i] || i + 1 >= n || !SP[i + 1]) continue;  // a range starts at a non-space character followed by a space
        int64_t b, e;
        const int64_t doc = doc_of(off, n_docs, i);
        doc_rows(off, doc, n, &b, &e, SD_DOC_MAX);
        if (i < b || i + 1 >= e) continue;
        double lo = P[i], hi = lo;
        int64_t j = i + 1;
        for (; j < e && SP[j]; ++j) {
            const double v = P[j];
            lo = v < lo ? v : lo;
            hi = v > hi ? v : hi;
        }
        if (j >= e) continue;  // no character after the run: the reference drops the range
        for (int64_t k = i; k < j - 1; ++k) P[k] = lo;
        P[j - 1] = hi;
    }
}

__global__ __launch_bounds__(256) void sd_phase1_kernel(const double* __restrict__ P, int f32, const int64_t* __restrict__ off,
                                                         int64_t n_docs, int64_t n, int64_t min_len, const int32_t* __restrict__ bad,
                                                         double* dp, int32_t* back, uint8_t* __restrict__ cut,
                                                         double* __restrict__ objective, int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
    for (int64_t doc = wave0; doc < n_docs; doc += n_waves) {
        int64_t b, e;
        doc_rows(off, doc, n, &b, &e, SD_DOC_MAX);
        if (bad[doc]) {
            if (lane == 0) {
                status[doc] = 2;
                if (objective) objective[doc] = NAN;
            }
            continue;
        }
        const int64_t nd = e - b, first = min_len - 1, last = nd - min_len - 1;
        const double* S = P + b;
        double* DP = dp + b;
        int32_t* BK = back + b;
        double best_score = 0.0, best_prev = -INFINITY;  // the state of the reference's loop, the same in every lane
        int64_t best_last = -1, best_prev_idx = -1;
        for (int64_t blk = first; blk <= last; blk += 64) {
            const int64_t i = blk + lane, jm = i - min_len;
            const bool ok = i <= last;
            const double s = ok ? sd_score(S[i], f32) : 0.0;
            const double pre = (ok && jm >= first && jm < blk) ? DP[jm] : -INFINITY;  // written by an earlier block of this wave
            double cur = -INFINITY;
            int32_t cur_back = -1;
            const int cnt = (int)(last - blk + 1 < 64 ? last - blk + 1 : 64);
#pragma unroll 1
            for (int k = 0; k < cnt; ++k) {
                const double sk = sd_lane(s, k);
                const int64_t jk = blk + k - min_len;
                if (jk >= first) {  // position jk becomes a valid predecessor
                    const double pv = (int64_t)k >= min_len ? sd_lane(cur, (int)(k - min_len)) : sd_lane(pre, k);
                    if (pv > best_prev) { best_prev = pv; best_prev_idx = jk; }
                }
                double d = sk;
                int32_t bk = -1;
                if (best_prev > -INFINITY && best_prev + sk > d) { d = best_prev + sk; bk = (int32_t)best_prev_idx; }
                if (d > best_score) { best_score = d; best_last = blk + k; }
                if (lane == k) { cur = d; cur_back = bk; }
            }
            if (ok) { DP[i] = cur; BK[i] = cur_back; }
            __threadfence_block();  // this block's dp and back before the next block's loads and lane 0's backtrack
        }
        if (lane == 0) {
            status[doc] = 0;
            if (objective) objective[doc] = best_score;
            int64_t pos = best_last;
            for (int64_t steps = 0; pos >= 0 && pos < nd - 1 && steps < nd; ++steps) {  // back[pos] < pos: at most n_d steps
                cut[b + pos] = 1;
                const int64_t prev = BK[pos];
                pos = prev < pos ? prev : -1;
            }
        }
    }
}

// One sentence of m > max_len characters under max_len.  Returns 0, 1 (shorter than 2 * min_len: unsplit) or 3 (no valid split), the
// same in every lane.
__device__ __forceinline__ int sd_window_dp(const double* __restrict__ S, int f32, int64_t m, int64_t min_len, int64_t max_len,
                                            double* DP, int32_t* BK, uint8_t* __restrict__ cut, int lane) {
    const int64_t first = min_len - 1, last = m - min_len - 1;
    if (last < first) return 1;
    for (int64_t i = first; i <= last; ++i) {
        const int64_t hi = i - min_len, lo = i - max_len > first ? i - max_len : first;
        double bv = -INFINITY;
        int64_t bj = -1;
        for (int64_t j = lo + lane; j <= hi; j += 64) {  // the lane's own best: ascending j, >= keeps the latest; finite values only
            const double v = DP[j];
            if (isfinite(v) && (bj < 0 || v >= bv)) { bv = v; bj = j; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {  // the larger value, then the larger index; a lane without a candidate has index -1
            const double tv = __shfl_xor(bv, o, 64);
            const long long tj = __shfl_xor((long long)bj, o, 64);
            if (tj >= 0 && (bj < 0 || tv > bv || (tv == bv && tj > bj))) { bv = tv; bj = tj; }
        }
        const double s = sd_score(S[i], f32);
        double d = -INFINITY;
        int32_t bk = -1;
        if (i + 1 <= max_len) d = s;
        if (bj >= 0 && bv + s > d) { d = bv + s; bk = (int32_t)bj; }
        if (lane == 0) { DP[i] = d; BK[i] = bk; }
        __threadfence_block();  // lane 0's dp[i] before the other lanes' reads of the next step
    }
    const int64_t amin = m - max_len - 1 > first ? m - max_len - 1 : first;
    double bv = -INFINITY;
    int64_t bj = -1;
    for (int64_t i = amin + lane; i <= last; i += 64) {  // strict > from -inf, ascending i: the earliest maximum
        const double v = DP[i];
        if (v > bv) { bv = v; bj = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {  // the larger value, then the smaller index
        const double tv = __shfl_xor(bv, o, 64);
        const long long tj = __shfl_xor((long long)bj, o, 64);
        if (tj >= 0 && (bj < 0 || tv > bv || (tv == bv && tj < bj))) { bv = tv; bj = tj; }
    }
    if (bj < 0) return 3;
    if (lane == 0) {
        int64_t pos = bj;
        for (int64_t steps = 0; pos >= 0 && pos < m - 1 && steps < m; ++steps) {
            cut[pos] = 1;
            const int64_t prev = BK[pos];
            pos = prev < pos ? prev : -1;
        }
    }
    return 0;
}

__global__ __launch_bounds__(256) void sd_phase2_kernel(const double* __restrict__ P, int f32, const int64_t* __restrict__ off,
                                                         int64_t n_docs, int64_t n, int64_t min_len, int64_t max_len, double* dp,
                                                         int32_t* back, uint8_t* cut, int32_t* status) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
    for (int64_t doc = wave0; doc < n_docs; doc += n_waves) {
        int64_t b, e;
        doc_rows(off, doc, n, &b, &e, SD_DOC_MAX);
        const int64_t nd = e - b;
        if (nd <= max_len || status[doc] == 2) continue;
        int st = 0;
        int64_t seg = 0;
        while (seg < nd) {
            int64_t end = nd;  // one past the sentence's last character: behind the first cut at or after seg
            for (int64_t p = seg; p < nd; p += 64) {
                const int64_t i = p + lane;
                const unsigned long long hit = __ballot(i < nd && cut[b + i] != 0);
                if (hit) { end = p + (__ffsll(hit) - 1) + 1; break; }
            }
            if (end - seg > max_len) {
                const int r = sd_window_dp(P + b + seg, f32, end - seg, min_len, max_len, dp + b + seg, back + b + seg, cut + b + seg, lane);
                if (r == 3) { st = 3; break; }  // the reference raises at the first such sentence
                st = r > st ? r : st;
            }
            seg = end;
        }
        if (st == 3) {
            __threadfence_block();  // lane 0's cuts before the stores that clear them
            for (int64_t i = lane; i < nd; i += 64) cut[b + i] = 0;
        }
        if (lane == 0 && st) status[doc] = st;
    }
}
}  // namespace

// scratch: double P, dp + int32 back + uint8 space per character, int32 bad per document
size_t sentence_dp_scratch_bytes(int64_t n, int64_t n_docs) { return (size_t)n * 21 + (size_t)n_docs * 4 + 64; }

int launch_sentence_dp(const uint32_t* codepoints, const void* probas, int probas_f64, const double* known, const int64_t* doc_off,
                       int64_t n, int64_t n_docs, int64_t min_len, int64_t max_len, uint8_t* cut, double* objective, int32_t* status,
                       void* scratch, hipStream_t s) {
    if (n <= 0 || n_docs <= 0) return RL_OK;
    double* P = static_cast<double*>(scratch);
    double* dp = P + n;
    int32_t* back = reinterpret_cast<int32_t*>(dp + n);
    int32_t* bad = back + n;
    uint8_t* SP = reinterpret_cast<uint8_t*>(bad + n_docs);
    const int f32 = probas_f64 ? 0 : 1;
    RL_HIP(hipMemsetAsync(cut, 0, (size_t)n, s));
    RL_HIP(hipMemsetAsync(bad, 0, (size_t)n_docs * sizeof(int32_t), s));
    const int cblocks = (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 256 * 64));
    const int wblocks = wave_per_item_blocks(n_docs);
    hipLaunchKernelGGL(sd_classify_kernel, dim3(cblocks), dim3(256), 0, s, codepoints, probas, f32, known, doc_off, n_docs, n, P, SP, bad);
    hipLaunchKernelGGL(sd_propagate_kernel, dim3(cblocks), dim3(256), 0, s, SP, doc_off, n_docs, n, P);
    hipLaunchKernelGGL(sd_phase1_kernel, dim3(wblocks), dim3(256), 0, s, P, f32, doc_off, n_docs, n, min_len, bad, dp, back, cut, objective,
                       status);
    if (max_len > 0)
        hipLaunchKernelGGL(sd_phase2_kernel, dim3(wblocks), dim3(256), 0, s, P, f32, doc_off, n_docs, n, min_len, max_len, dp, back, cut,
                           status);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

}  // namespace rl
