// The head of a BERT cross-encoder on the native encoder's final hidden states (rl_encoder_head, rl_encoder_classify_pack; DESIGN.md
// 4.23): per sequence s, on the row of its FIRST token,
//     p[j] = tanh(sum_k Wp[j, k] x[k] + bp[j])   (the pooler: nn.Linear's own [hidden x hidden] matrix, read in place)
//     logit = sum_j wh[j] p[j] + bh               (the one-logit classifier)
// One workgroup of four waves per sequence.  16-bit loads (bf16 / fp16), everything after them in f32, ONE f32 store: nothing is rounded
// to 16 bits between the hidden states and the logit (the torch route rounds the pooler's sum, its tanh and the logit).
//
// The order of every sum, a function of `hidden` alone -- not of n_seqs, of s, or of where the row lies:
//   * The outputs go in groups of 8: group g = outputs 8 g .. 8 g + 7; wave w takes the groups g = w, w + 4, w + 8, ..  (hidden / 8 is a
//     multiple of 4: every wave makes the same number of turns).
//   * A pre-activation: lane l runs ONE fma chain from 0 over its elements k = 4 l + 256 i + {0, 1, 2, 3}, i ascending (acc = fma(W[j, k],
//     x[k], acc)); the 64 chains are summed by the butterfly of wave_sum (xor 32, 16, 8, 4, 2, 1); then + bp[j]; then tanhf.
//   * Lane i < 8 of wave w owns output 8 g + i of each of the wave's groups and keeps P[w][i] = the sum over the wave's turns, in order, of
//     wh[j] * p[j] (acc = fma(wh[j], p[j], acc), starting from 0).
//   * One thread adds the 32 values P[0][0], P[0][1], .., P[3][7] in that order from 0, then + bh.
// No atomics, no second workgroup: the same bits run to run, and the bits of a row whatever else the launch holds.
//
// Safety: the row index seq_offsets[s] is clamped into [0, n_tokens - 1] -- a bad offset gives a wrong number, never a read outside x --
// and an empty sequence (seq_offsets[s] == seq_offsets[s + 1]) writes a quiet NaN without reading x.
#include <cmath>

#include "common.h"

namespace rl {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <class T> __device__ __forceinline__ float widen(uint16_t bits);
template <> __device__ __forceinline__ float widen<__bf16>(uint16_t bits) { return __uint_as_float((uint32_t)bits << 16); }
template <> __device__ __forceinline__ float widen<_Float16>(uint16_t bits) { return (float)__builtin_bit_cast(_Float16, bits); }

template <class T>
__device__ __forceinline__ f32x4 widen4(u32x2 w) {
    return f32x4{widen<T>((uint16_t)w[0]), widen<T>((uint16_t)(w[0] >> 16)), widen<T>((uint16_t)w[1]), widen<T>((uint16_t)(w[1] >> 16))};
}
__device__ __forceinline__ u32x2 load4(const uint16_t* p) { return *reinterpret_cast<const u32x2*>(p); }

constexpr int HEAD_THREADS = 256;
constexpr int HEAD_WAVES = HEAD_THREADS / WAVE;
constexpr int HEAD_GROUP = 8;  // outputs a wave computes per turn: 8 independent rows of Wp in flight per lane

template <class T>
__global__ __launch_bounds__(HEAD_THREADS) void encoder_head_kernel(const uint16_t* __restrict__ x, const int32_t* __restrict__ seq_offsets,
                                                                    int n_tokens, int hidden, const uint16_t* __restrict__ Wp,
                                                                    const uint16_t* __restrict__ bp, const uint16_t* __restrict__ wh,
                                                                    const uint16_t* __restrict__ bh, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float xrow[];  // [hidden] the first token's row in f32
    __shared__ float part[HEAD_WAVES * HEAD_GROUP];
    const int s = blockIdx.x;
    const int begin = seq_offsets[s];
    if (begin == seq_offsets[s + 1]) {  // (uniform over the workgroup: nobody waits at a barrier below)
        if (threadIdx.x == 0) out[s] = __uint_as_float(0x7fc00000u);
        return;
    }
    const int row = begin < 0 ? 0 : (begin >= n_tokens ? n_tokens - 1 : begin);
    const uint16_t* xr = x + (int64_t)row * hidden;
    for (int e = 4 * threadIdx.x; e < hidden; e += 4 * HEAD_THREADS) *reinterpret_cast<f32x4*>(xrow + e) = widen4<T>(load4(xr + e));
    __syncthreads();

    const int w = wave_id(), lane = threadIdx.x & (WAVE - 1);
    float mine = 0.f;  // P[w][lane] for lane < HEAD_GROUP
    for (int g = w; g < hidden / HEAD_GROUP; g += HEAD_WAVES) {
        const uint16_t* w0 = Wp + (int64_t)g * HEAD_GROUP * hidden;
        float acc[HEAD_GROUP];
#pragma unroll
        for (int i = 0; i < HEAD_GROUP; ++i) acc[i] = 0.f;
        for (int e = 4 * lane; e < hidden; e += 4 * WAVE) {
            u32x2 wv[HEAD_GROUP];
#pragma unroll
            for (int i = 0; i < HEAD_GROUP; ++i) wv[i] = load4(w0 + (int64_t)i * hidden + e);
            const f32x4 xv = *reinterpret_cast<const f32x4*>(xrow + e);
#pragma unroll
            for (int i = 0; i < HEAD_GROUP; ++i) {
                const f32x4 v = widen4<T>(wv[i]);
                acc[i] = fmaf(v[3], xv[3], fmaf(v[2], xv[2], fmaf(v[1], xv[1], fmaf(v[0], xv[0], acc[i]))));
            }
        }
        float pre = 0.f;
#pragma unroll
        for (int i = 0; i < HEAD_GROUP; ++i) {
            const float sum = wave_sum(acc[i]);  // (the same value in every lane)
            pre = lane == i ? sum : pre;
        }
        if (lane < HEAD_GROUP) {
            const int j = g * HEAD_GROUP + lane;
            mine = fmaf(widen<T>(wh[j]), tanhf(pre + widen<T>(bp[j])), mine);
        }
    }
    if (lane < HEAD_GROUP) part[w * HEAD_GROUP + lane] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        float logit = 0.f;
#pragma unroll
        for (int i = 0; i < HEAD_WAVES * HEAD_GROUP; ++i) logit += part[i];
        out[s] = logit + widen<T>(bh[0]);
    }
}

}  // namespace

static_assert(ENC_HIDDEN_MAX * sizeof(float) <= 64 * 1024 - 256, "the f32 row and the partials fit a workgroup's default LDS");

int launch_encoder_head(const void* x, const int32_t* seq_offsets, int32_t n_seqs, int32_t n_tokens, int32_t hidden, const void* pooler_w,
                        const void* pooler_b, const void* head_w, const void* head_b, int32_t dtype, float* out_logits, hipStream_t s) {
    if (n_seqs <= 0) return RL_OK;
    const dim3 grid((unsigned)n_seqs), block(HEAD_THREADS);
    const size_t lds = (size_t)hidden * sizeof(float);
#define RL_ENC_HEAD(T)                                                                                                                    \
    hipLaunchKernelGGL((encoder_head_kernel<T>), grid, block, lds, s, static_cast<const uint16_t*>(x), seq_offsets, n_tokens, hidden,      \
                       static_cast<const uint16_t*>(pooler_w), static_cast<const uint16_t*>(pooler_b), static_cast<const uint16_t*>(head_w), \
                       static_cast<const uint16_t*>(head_b), out_logits)
    if (dtype == RL_ATTN_BF16) RL_ENC_HEAD(__bf16);
    else RL_ENC_HEAD(_Float16);
#undef RL_ENC_HEAD
    RL_HIP(hipGetLastError());
    return RL_OK;
}

}  // namespace rl
