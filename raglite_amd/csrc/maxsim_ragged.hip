// Ragged MaxSim rerank: exact MaxSim of (query, candidate chunk) pairs where every query carries its OWN number of
// token vectors -- query b owns Q[qv_off[b] .. qv_off[b + 1]) -- so that a batch of text queries of mixed lengths is one launch, and a
// query of more than 32 vectors is scored at all on an fp16-stored index.
//
//   maxsim_ragged_kernel    : dim % 16 == 0, 16 <= dim <= 1024, fp32 or fp16-stored rows; any number of vectors per query
//   slab_accumulate_kernel  : out = slab (first) or out + slab: the sum of the backstop (api.hip: maxsim_rerank_ragged_device), which
//                             scores the shapes this kernel does not take one (query, slab) at a time through rl_maxsim_rerank's own
//                             kernels.  The backstop is correct and unhurried: a launch pair per (query, slab).
//
// The contract (include/raglite_hip.h, rl_maxsim_rerank_ragged): a query's scores are, bit for bit, the fp32 sum in slab order of what
// rl_maxsim_rerank returns for each slab of 32 of its vectors alone (the last slab with its own shorter nq).
//
// The arithmetic is maxsim_pairs_kernel's (maxsim_generic.hip), copied here so that the kernels behind the headline's re-scoring step
// keep their code and their schedule: one workgroup of eight waves per (candidate slice, query); the slab's [32 x dim] fp32 matrix in
// LDS at a pitch of dim + 8 floats (a ds_read_b128 serves 8 rows x 2 k-quads per cycle; + 32 B per row spreads them over all 64 banks),
// rows past the slab's end zero (their maxima are 0 and add nothing); per 16-row tile of a chunk and 16-wide k step one 16-B global
// load per lane feeds four v_mfma_f32_16x16x4_f32 steps per 16-column half, k ascending; the masked max over the chunk's rows; the
// 4-step butterfly over 16 columns, then s0 + s1.  A query's bits therefore do not depend on any other query of the launch: nq is a
// load bound, read from the table.
// The software pipeline is that kernel's too: the rows of the NEXT block of KB k are requested before the MFMAs of the current one
// (sched_barrier keeps the loads above them), the query fragments of step j + 1 are read from LDS before the MFMAs of step j.
//
// Slabs: a workgroup walks its query 32 vectors at a time: load the slab, barrier, walk its candidates, barrier (before the next slab
// overwrites LDS).  Slab 0 stores a candidate's score, slab s > 0 stores out + score: one fp32 addition per slab, in slab order.  Which
// wave takes a candidate depends on blockIdx.x, the wave id and the stride alone, so the same lane of the same wave writes a slot in
// every slab and the read-modify-write follows that thread's own earlier store: no atomics, the same bits run to run.  Candidates < 0
// and empty chunks get -inf once, in slab 0, and are not touched again.
#include <mutex>

#include "common.h"

namespace rl {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int RAGGED_SLAB = 32;  // query vectors per slab: the columns of two 16 x 16 MFMA tiles

template <bool FULL, int KB, bool ROW16>
__global__ __launch_bounds__(512) void maxsim_ragged_kernel(const float* __restrict__ D, int dim, const float* __restrict__ Q,
                                                             const int64_t* __restrict__ qv_off, const int64_t* __restrict__ offsets,
                                                             const int32_t* __restrict__ candidates, int64_t n_items, float* out) {
    extern __shared__ __attribute__((aligned(16))) float qs[];  // [32][dim + 8]
    const int pitch = dim + 8;
    const int64_t v_begin = qv_off[blockIdx.y], v_end = qv_off[blockIdx.y + 1];  // this query's vectors
    const int32_t* cb = candidates + (int64_t)blockIdx.y * n_items;
    float* ob = out + (int64_t)blockIdx.y * n_items;
    const int lane = threadIdx.x & 63, w = wave_id();
    const int m = lane & 15, g = lane >> 4;  // A: row m of the tile, k quad g;  B / C: query column m, k quad / row quad g
    const float* q0 = qs + m * pitch + 4 * g;
    const float* q1 = qs + (16 + m) * pitch + 4 * g;
    const int64_t stride = (int64_t)gridDim.x * 8;
    // the 16 rows x KB k of a block, one 16-B load per lane and 16-wide k step (rows past the chunk: its last row again, masked later)
    constexpr int NL = KB / 16;
    auto request = [&](f32x4 (&x)[NL], int64_t e, int64_t r0, int t0) __attribute__((always_inline)) {
        const int64_t row = r0 + m < e ? r0 + m : e - 1;
        if constexpr (ROW16) {
            typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
            const _Float16* a = reinterpret_cast<const _Float16*>(D) + row * (int64_t)dim + 4 * g + t0;
#pragma unroll
            for (int j = 0; j < NL; ++j) {
                h16x4 h = (h16x4){0, 0, 0, 0};
                if (FULL || t0 + 16 * j < dim) h = *reinterpret_cast<const h16x4*>(a + 16 * j);
                x[j] = (f32x4){(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
            }
        } else {
            const float* a = D + row * (int64_t)dim + 4 * g + t0;
#pragma unroll
            for (int j = 0; j < NL; ++j) x[j] = (FULL || t0 + 16 * j < dim) ? *reinterpret_cast<const f32x4*>(a + 16 * j) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    };
    auto lane_i64 = [](int64_t v, int k) __attribute__((always_inline)) {  // lane k's value, k wave-uniform
        const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)(uint64_t)v, k), hi = __builtin_amdgcn_readlane((uint32_t)((uint64_t)v >> 32), k);
        return (int64_t)(((uint64_t)hi << 32) | lo);
    };
    f32x4 xc[NL], xn[NL];
    for (int64_t v0 = v_begin; v0 < v_end; v0 += RAGGED_SLAB) {
        const bool first = v0 == v_begin;  // (uniform)
        const int nq = (int)(v_end - v0 < RAGGED_SLAB ? v_end - v0 : RAGGED_SLAB);
        const float* Qb = Q + v0 * (int64_t)dim;
        for (int i = threadIdx.x * 4; i < RAGGED_SLAB * dim; i += 512 * 4) {
            const int n = i / dim, c = i - n * dim;
            f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};  // rows past the slab's end: zeros (their maxima are 0 and add nothing)
            if (n < nq) v = *reinterpret_cast<const f32x4*>(Qb + (int64_t)n * dim + c);
            *reinterpret_cast<f32x4*>(qs + n * pitch + c) = v;
        }
        __syncthreads();
        // 64 of this wave's candidates at a time: lane L looks up the L-th one's row range (two dependent loads, once per 64 candidates
        // and for all of them at the same time), candidates without rows get their -inf (slab 0), the others are walked in lane order
        for (int64_t base = (int64_t)blockIdx.x * 8 + w; base < n_items; base += 64 * stride) {
            const int64_t mine = base + (int64_t)lane * stride;
            int64_t vb = 0, ve = 0;
            if (mine < n_items) {
                const int64_t chunk = cb[mine];
                if (chunk >= 0) { vb = offsets[chunk]; ve = offsets[chunk + 1]; }
                if (ve <= vb && first) ob[mine] = -INFINITY;
            }
            const uint64_t todo = __builtin_amdgcn_ballot_w64(ve > vb);
            if (todo == 0ull) continue;  // (wave-uniform)
            int k = __builtin_ctzll(todo);
            int64_t e = lane_i64(ve, k), r0 = lane_i64(vb, k);
            int t0 = 0;
            request(xc, e, r0, 0);
            f32x4 y0 = *reinterpret_cast<const f32x4*>(q0), y1 = *reinterpret_cast<const f32x4*>(q1);  // query fragments of the step being multiplied
            float best0 = -INFINITY, best1 = -INFINITY;  // running max over the chunk's rows of this lane's column (both halves)
            f32x4 acc0 = (f32x4){0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
            for (;;) {
                // the block after this one -- same tile, next tile, the next candidate's first -- chosen without a branch and requested
                // before this block's 8 NL MFMAs (after the last block of the 64 candidates: the current candidate's first block again, unused)
                const bool more_k = t0 + KB < dim, more_rows = r0 + 16 < e;
                const uint64_t rest = todo & ~((2ull << k) - 1ull);
                const int nk = rest ? __builtin_ctzll(rest) : k;
                const int64_t ne = lane_i64(ve, nk), nb = lane_i64(vb, nk);
                const int64_t n_e = (more_k || more_rows) ? e : ne;
                const int64_t n_r0 = more_k ? r0 : (more_rows ? r0 + 16 : nb);
                const int n_t0 = more_k ? t0 + KB : 0;
                request(xn, n_e, n_r0, n_t0);
                __builtin_amdgcn_sched_barrier(0);  // (the scheduler would sink the loads below the MFMAs: they have to be in flight DURING them)
#pragma unroll
                for (int j = 0; j < NL; ++j) {
                    if (!FULL && t0 + 16 * j >= dim) break;  // (uniform)
                    const int tn = j + 1 < NL ? t0 + 16 * (j + 1) : n_t0;  // (a partial block's steps past dim: a fragment nobody multiplies)
                    const int tr = (FULL || tn < dim) ? tn : 0;
                    const f32x4 z0 = *reinterpret_cast<const f32x4*>(q0 + tr);
                    const f32x4 z1 = *reinterpret_cast<const f32x4*>(q1 + tr);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xc[j][u], y0[u], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xc[j][u], y1[u], acc1, 0, 0, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    y0 = z0;
                    y1 = z1;
                }
                bool last = false;
                if (!more_k) {  // the tile is complete.  C layout: this lane holds rows 4 g + i (i = 0..3) of column m
                    float s0 = -INFINITY, s1 = -INFINITY;
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (r0 + 4 * g + i < e) { s0 = fmaxf(s0, acc0[i]); s1 = fmaxf(s1, acc1[i]); }
                    s0 = fmaxf(s0, __shfl_xor(s0, 16)); s0 = fmaxf(s0, __shfl_xor(s0, 32));
                    s1 = fmaxf(s1, __shfl_xor(s1, 16)); s1 = fmaxf(s1, __shfl_xor(s1, 32));
                    best0 = fmaxf(best0, s0);
                    best1 = fmaxf(best1, s1);
                    acc0 = acc1 = (f32x4){0.f, 0.f, 0.f, 0.f};
                    if (!more_rows) {  // ... and so is the candidate: sum over the slab's 32 columns, 16 per half by a 4-step butterfly,
                                       // then the two halves -- a fixed order -- and onto what the earlier slabs left
                        float t0s = best0, t1s = best1;
#pragma unroll
                        for (int o = 1; o < 16; o <<= 1) { t0s += __shfl_xor(t0s, o); t1s += __shfl_xor(t1s, o); }
                        if (lane == 0) {
                            float* slot = ob + base + (int64_t)k * stride;
                            const float score = t0s + t1s;
                            *slot = first ? score : *slot + score;
                        }
                        best0 = best1 = -INFINITY;
                        last = rest == 0ull;
                        k = nk;
                    }
                }
                if (last) break;
                e = n_e;
                r0 = n_r0;
                t0 = n_t0;
#pragma unroll
                for (int j = 0; j < NL; ++j) xc[j] = xn[j];
            }
        }
        __syncthreads();  // every wave is done with this slab before the next one overwrites it
    }
}

__global__ __launch_bounds__(256) void slab_accumulate_kernel(float* __restrict__ out, const float* __restrict__ slab, int64_t n, int add) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = add ? out[i] + slab[i] : slab[i];
}

int launch_slab_accumulate(float* out, const float* slab, int64_t n, bool add, hipStream_t s) {
    if (n <= 0) return RL_OK;
    hipLaunchKernelGGL(slab_accumulate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out, slab, n, add ? 1 : 0);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

namespace {
// > 64 KiB of dynamic LDS needs the opt-in, which is a property of the function ON a device: once per device, under a lock
int ragged_opt_in() {
    static std::mutex mu;
    static uint64_t done[4] = {0, 0, 0, 0};  // one bit per device ordinal
    int dev = 0;
    RL_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 256) return fail(RL_ERR_UNSUPPORTED, "maxsim_ragged: device ordinal beyond 255");
    std::lock_guard<std::mutex> lock(mu);
    if (done[dev >> 6] >> (dev & 63) & 1ull) return RL_OK;
#define RL_RAGGED_ATTR(...) RL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(maxsim_ragged_kernel<__VA_ARGS__>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024))
    RL_RAGGED_ATTR(true, 256, false);
    RL_RAGGED_ATTR(true, 128, false);
    RL_RAGGED_ATTR(false, 128, false);
    RL_RAGGED_ATTR(true, 256, true);
    RL_RAGGED_ATTR(true, 128, true);  // (no <false, 128, true>: an fp16-stored index has a dim % 128 == 0, rl_index_create_f16)
#undef RL_RAGGED_ATTR
    done[dev >> 6] |= 1ull << (dev & 63);
    return RL_OK;
}
}  // namespace

// d_qv_off: device [n_queries + 1]; candidates / out: [n_queries x n_cand] (candidates sanitised: < 0 or a chunk of the map).
// RL_ERR_UNSUPPORTED outside dim % 16 == 0, 16 <= dim <= 1024 (fp16 rows: dim % 128 == 0, the dims such an index has), beyond 65535
// queries (the grid's second dimension), or on misaligned rows / vectors.
int launch_maxsim_ragged(const RowsRef& rows, const float* Q, const int64_t* d_qv_off, int32_t n_queries, const ChunkMap& c,
                         const int32_t* candidates, int32_t n_cand, float* out, hipStream_t s) {
    const float* const D = static_cast<const float*>(rows.p);  // fp32 rows, or (rows.f16) IEEE halves
    const int32_t dim = rows.dim;
    if (n_cand <= 0 || n_queries <= 0) return RL_OK;
    if (dim % 16 || dim < 16 || dim > 1024 || (rows.f16 && dim % 128) || n_queries > 65535 || !candidates || !d_qv_off) return RL_ERR_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(D) & (rows.f16 ? 7 : 15)) || (reinterpret_cast<uintptr_t>(Q) & 15)) return RL_ERR_UNSUPPORTED;
    RL_TRY(ragged_opt_in());
    const size_t lds = (size_t)RAGGED_SLAB * (dim + 8) * sizeof(float);
    // workgroups per query as launch_maxsim_pairs sizes them: enough to fill the chip when there are few queries, at most one wave per candidate
    const int per_query = (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)n_cand + 7) / 8, std::max<int64_t>(1, 512 / n_queries)));
#define RL_RAGGED(FULL_, KB_, ROW16_)                                                                                                      \
    hipLaunchKernelGGL((maxsim_ragged_kernel<FULL_, KB_, ROW16_>), dim3(per_query, n_queries), dim3(512), lds, s, D, (int)dim, Q, d_qv_off,    \
                       c.offsets, candidates, (int64_t)n_cand, out)
    if (dim % 256 == 0) { if (rows.f16) RL_RAGGED(true, 256, true); else RL_RAGGED(true, 256, false); }
    else if (dim % 128 == 0) { if (rows.f16) RL_RAGGED(true, 128, true); else RL_RAGGED(true, 128, false); }
    else RL_RAGGED(false, 128, false);
#undef RL_RAGGED
    RL_HIP(hipGetLastError());
    return RL_OK;
}

}  // namespace rl
