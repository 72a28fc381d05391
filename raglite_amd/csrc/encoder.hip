// The kernels of the native encoder forward for short packs (rl_encoder_forward) and for packs of several token
// blocks (rl_encoder_forward_pack): embeddings + layer norm, the skinny linear layer, and the layer norm that closes a
// projection.  16-bit storage (bf16 / fp16), every sum in f32, one rounding per stored value.  Attention is attention_varlen.hip's, on
// the QKV buffer as the linear kernel leaves it.
//
// Skinny linear: out[M x N] = epi(x[M x K] . W[N x K]^T).  At these M a projection is a stream of W, not a GEMM: a workgroup owns a slab
// of 32 output columns -- 32 rows of W, read in place from nn.Linear's [N x K] layout, each byte once -- for ALL M rows, and, where the
// grid would otherwise leave most CUs idle, only one K slice of it (blockIdx.y; encoder_ksplit).  Inside the workgroup the four waves
// take the slice's 64-element K chunks in turn (its i-th chunk to wave i % 4), so all four stream W at once, and every wave keeps the whole
// [32 x M] tile in accumulators: MT = ceil(M / 32) <= 8 MFMA tiles of 16 registers, 128 of a wave's 512 at the cap -- that, and a
// [4 waves x 32 x 32] f32 reduction image in LDS, is what sets RL_ENCODER_MAX_TOKENS = 256.
//   mfma_f32_32x32x16(A = W fragment, B = x fragment): the swapped product of attention_varlen.hip, so a lane holds ONE token (column
//   lane & 31) against 16 output columns (rows (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)).  Both operands take their 8 elements of k-step j
//   of a chunk from k = chunk + (lane >> 5) * (chunk size / 2) + 8 j: the k order inside an MFMA is free as long as A and B agree, and this
//   one lets a lane read 64 contiguous bytes of its W row.  K % 64 == 32 ends in a chunk of 32 (two k-steps).
//   x rows past M are clamped to row M - 1 for the loads and never stored.
// More than RL_ENCODER_MAX_TOKENS rows: a TOKEN BLOCK per blockIdx.z.  Block z owns the rows [256 z, min(256 z + 256, M)) and runs on them
// exactly the loop above -- the same chunks to the same waves, the same k-steps, the same reductions -- so W is streamed once per block
// and a row's sums are the ones it has in a call of its own; `part` is indexed with the global row.
// The waves' tiles are summed through LDS in wave order, the K slices by launch_encoder_ln in slice order: a row's summation order is a
// function of (N, K) alone -- not of M, MT, the token block, the place in it, or what else is in the pack -- and there is no atomic anywhere.
// Epilogues, in f32 before the single rounding: + bias (QKV); gelu_erf(. + bias) (up); or the raw f32 slice into `part` (out, down),
// whose bias, residual and layer norm follow in encoder_ln_kernel.
//
// Layer norms: one workgroup per row, the f32 row kept in LDS (hidden <= ENC_HIDDEN_MAX); mean, then the variance of the centred values.
#include "common.h"

namespace rl {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <class T> struct Elem;
template <> struct Elem<__bf16> {
    typedef bf16x8 v8;
    static __device__ __forceinline__ f32x16 mfma(v8 a, v8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ float widen(uint16_t bits) { return __uint_as_float((uint32_t)bits << 16); }
};
template <> struct Elem<_Float16> {
    typedef f16x8 v8;
    static __device__ __forceinline__ f32x16 mfma(v8 a, v8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ float widen(uint16_t bits) { return (float)__builtin_bit_cast(_Float16, bits); }
};
template <class T>
__device__ __forceinline__ uint16_t narrow(float v) { return __builtin_bit_cast(uint16_t, (T)v); }  // round to nearest even

__device__ __forceinline__ int clamp_index(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// ---- layer norms: one workgroup of four waves per row --------------------------------------------------------------------------------
// A thread owns the elements 4 (tid + 256 i) .. + 3 of its row: one 8-byte (16-bit data) or 16-byte (f32) load each, all of an iteration's
// loads independent; at hidden = 1024 that is one iteration.  Sums: the thread's own elements in order, the wave's butterfly, the four
// waves in order -- a function of hidden alone.
constexpr int LN_THREADS = 256;

template <class T>
__device__ __forceinline__ f32x4 widen4(u32x2 w) {
    return f32x4{Elem<T>::widen((uint16_t)w[0]), Elem<T>::widen((uint16_t)(w[0] >> 16)), Elem<T>::widen((uint16_t)w[1]),
                 Elem<T>::widen((uint16_t)(w[1] >> 16))};
}
template <class T>
__device__ __forceinline__ u32x2 narrow4(f32x4 v) {
    return u32x2{(uint32_t)narrow<T>(v[0]) | ((uint32_t)narrow<T>(v[1]) << 16), (uint32_t)narrow<T>(v[2]) | ((uint32_t)narrow<T>(v[3]) << 16)};
}
__device__ __forceinline__ u32x2 load4(const uint16_t* p) { return *reinterpret_cast<const u32x2*>(p); }

__device__ __forceinline__ float block_sum(float v, float* slots) {  // slots: one float per wave, not in use by anything else
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) slots[wave_id()] = v;
    __syncthreads();
    return ((slots[0] + slots[1]) + slots[2]) + slots[3];
}

// row[e .. e + 3] holds the f32 values of this thread's elements, written by this thread: no barrier of its own; sum = its part of the row sum.
template <class T>
__device__ __forceinline__ void ln_finish(const float* row, int hidden, float sum, const uint16_t* w, const uint16_t* b, float eps,
                                          uint16_t* out, float* slots) {
    const float mean = block_sum(sum, slots) / (float)hidden;
    float sq = 0.f;
    for (int e = 4 * threadIdx.x; e < hidden; e += 4 * LN_THREADS) {
        const f32x4 d = *reinterpret_cast<const f32x4*>(row + e) - mean;
        sq += ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3];
    }
    const float rstd = 1.0f / sqrtf(block_sum(sq, slots + 4) / (float)hidden + eps);
    for (int e = 4 * threadIdx.x; e < hidden; e += 4 * LN_THREADS) {
        const f32x4 d = *reinterpret_cast<const f32x4*>(row + e) - mean;
        *reinterpret_cast<u32x2*>(out + e) = narrow4<T>(d * rstd * widen4<T>(load4(w + e)) + widen4<T>(load4(b + e)));
    }
}

template <class T>
__global__ __launch_bounds__(LN_THREADS) void encoder_embed_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ positions,
                                                                   const int32_t* __restrict__ type_ids, const uint16_t* __restrict__ tok,
                                                                   int vocab, const uint16_t* __restrict__ pos, int max_positions,
                                                                   const uint16_t* __restrict__ typ, int type_vocab,
                                                                   const uint16_t* __restrict__ ln_w, const uint16_t* __restrict__ ln_b,
                                                                   int hidden, float eps, uint16_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float row[];
    __shared__ float slots[8];
    const int t = blockIdx.x;
    const uint16_t* a = tok + (int64_t)clamp_index(ids[t], vocab) * hidden;
    const uint16_t* p = pos + (int64_t)clamp_index(positions[t], max_positions) * hidden;
    const uint16_t* y = typ + (int64_t)clamp_index(type_ids ? type_ids[t] : 0, type_vocab) * hidden;
    float sum = 0.f;
    for (int e = 4 * threadIdx.x; e < hidden; e += 4 * LN_THREADS) {
        const f32x4 v = widen4<T>(load4(a + e)) + widen4<T>(load4(p + e)) + widen4<T>(load4(y + e));
        *reinterpret_cast<f32x4*>(row + e) = v;
        sum += ((v[0] + v[1]) + v[2]) + v[3];
    }
    ln_finish<T>(row, hidden, sum, ln_w, ln_b, eps, out + (int64_t)t * hidden, slots);
}

template <class T>
__global__ __launch_bounds__(LN_THREADS) void encoder_ln_kernel(const float* __restrict__ part, int ksplit, int M, int hidden,
                                                                const uint16_t* __restrict__ bias, const uint16_t* __restrict__ resid,
                                                                const uint16_t* __restrict__ ln_w, const uint16_t* __restrict__ ln_b,
                                                                float eps, uint16_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float row[];
    __shared__ float slots[8];
    const int r = blockIdx.x;
    const float* p0 = part + (int64_t)r * hidden;
    const int64_t slice = (int64_t)M * hidden;
    const uint16_t* xr = resid + (int64_t)r * hidden;
    float sum = 0.f;
    for (int e = 4 * threadIdx.x; e < hidden; e += 4 * LN_THREADS) {
        f32x4 v = *reinterpret_cast<const f32x4*>(p0 + e);
        for (int s = 1; s < ksplit; ++s) v += *reinterpret_cast<const f32x4*>(p0 + s * slice + e);  // the K slices in order
        v += widen4<T>(load4(bias + e));
        v += widen4<T>(load4(xr + e));
        *reinterpret_cast<f32x4*>(row + e) = v;
        sum += ((v[0] + v[1]) + v[2]) + v[3];
    }
    ln_finish<T>(row, hidden, sum, ln_w, ln_b, eps, out + (int64_t)r * hidden, slots);
}

// ---- skinny linear ------------------------------------------------------------------------------------------------------------------
constexpr int LIN_SLAB = 32;    // output columns (rows of W) per workgroup
constexpr int LIN_CHUNK = 64;   // k elements per chunk: 128 bytes of a W row, 64 per lane half
constexpr int LIN_WAVES = 4;
constexpr int LIN_BLOCK_ROWS = 256;  // token rows per blockIdx.z: eight tiles of 32, the most a wave keeps in accumulators
constexpr int LIN_RED_LD = 36;  // floats per token row of a wave's reduction tile (32 + 4: the 16-byte writes of 32 lanes spread over the banks)

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

// G chunks of STEPS k-steps at the element offsets kb[g] of the rows: first all of this lane's W loads (8 G STEPS elements, G x STEPS
// independent 16-byte loads in flight: at these sizes a wave's time is load latency, not bandwidth), then per token tile its x loads and the
// MFMAs -- in chunk order, k-step order, whatever G is: grouping changes when loads are issued, never a sum.
template <class T, int MT, int STEPS, int G>
__device__ __forceinline__ void chunk_mac(const uint16_t* wrow, const uint16_t* (&xrow)[MT], const int (&kb)[G], f32x16 (&acc)[MT]) {
    typedef typename Elem<T>::v8 v8;
    v8 wf[G][STEPS];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int j = 0; j < STEPS; ++j) wf[g][j] = __builtin_bit_cast(v8, *reinterpret_cast<const u32x4*>(wrow + kb[g] + 8 * j));
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        v8 xf[G][STEPS];
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int j = 0; j < STEPS; ++j) xf[g][j] = __builtin_bit_cast(v8, *reinterpret_cast<const u32x4*>(xrow[mt] + kb[g] + 8 * j));
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int j = 0; j < STEPS; ++j) acc[mt] = Elem<T>::mfma(wf[g][j], xf[g][j], acc[mt]);
    }
}

template <class T, int MT, int EPI>
__global__ __launch_bounds__(WAVE * LIN_WAVES) void encoder_linear_kernel(const uint16_t* __restrict__ x, int M, int K,
                                                                          const uint16_t* __restrict__ W, int N,
                                                                          const uint16_t* __restrict__ bias, int chunks_per_slice,
                                                                          uint16_t* __restrict__ out16, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float red[LIN_WAVES * 32 * LIN_RED_LD];
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = wave_id();
    const int n0 = blockIdx.x * LIN_SLAB, slice = blockIdx.y;
    const int m0 = blockIdx.z * LIN_BLOCK_ROWS;  // this token block's first row (gridDim.z == 1, m0 == 0 wherever MT < 8)
    const int n_chunks = (K + LIN_CHUNK - 1) / LIN_CHUNK;
    const int c_begin = slice * chunks_per_slice;
    const int c_end = c_begin + chunks_per_slice < n_chunks ? c_begin + chunks_per_slice : n_chunks;

    const uint16_t* wrow = W + (int64_t)(n0 + r) * K;  // n0 + 31 < N: N is a multiple of the slab
    const uint16_t* xrow[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int m = m0 + mt * 32 + r;
        xrow[mt] = x + (int64_t)(m < M ? m : M - 1) * K;
    }
    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;

    // this wave's chunks c_begin + wave, + 4, ..: the full ones in groups of G, then one by one, then the 32-element tail of a K that is an
    // odd multiple of 32 (every bound is uniform per wave)
    constexpr int G = MT <= 2 ? 4 : 2;
    const int full_end = (K % LIN_CHUNK) == 0 || c_end < n_chunks ? c_end : n_chunks - 1;
    int c = c_begin + wave;
    for (; c + (G - 1) * LIN_WAVES < full_end; c += G * LIN_WAVES) {
        int kb[G];
#pragma unroll
        for (int g = 0; g < G; ++g) kb[g] = (c + g * LIN_WAVES) * LIN_CHUNK + h * (LIN_CHUNK / 2);
        chunk_mac<T, MT, LIN_CHUNK / 16, G>(wrow, xrow, kb, acc);
    }
    for (; c < full_end; c += LIN_WAVES) {
        const int kb[1] = {c * LIN_CHUNK + h * (LIN_CHUNK / 2)};
        chunk_mac<T, MT, LIN_CHUNK / 16, 1>(wrow, xrow, kb, acc);
    }
    if (c < c_end) {
        const int kb[1] = {c * LIN_CHUNK + h * (LIN_CHUNK / 4)};
        chunk_mac<T, MT, LIN_CHUNK / 32, 1>(wrow, xrow, kb, acc);
    }

    // the four waves' tiles, summed in wave order, 32 tokens at a time; thread tid then owns token tid / 8, columns 4 (tid % 8) .. + 3
    const int m_l = tid >> 3, nl = (tid & 7) * 4;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        if (m0 + mt * 32 >= M) break;  // (uniform)
        if (mt) __syncthreads();  // the previous tile has been read
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<f32x4*>(red + (wave * 32 + r) * LIN_RED_LD + 8 * g + 4 * h) =
                f32x4{acc[mt][4 * g], acc[mt][4 * g + 1], acc[mt][4 * g + 2], acc[mt][4 * g + 3]};
        __syncthreads();
        f32x4 v = *reinterpret_cast<const f32x4*>(red + m_l * LIN_RED_LD + nl);
#pragma unroll
        for (int w = 1; w < LIN_WAVES; ++w) v += *reinterpret_cast<const f32x4*>(red + (w * 32 + m_l) * LIN_RED_LD + nl);
        const int m = m0 + mt * 32 + m_l;
        if (m >= M) continue;
        if (EPI == ENC_EPI_PARTIAL) {
            *reinterpret_cast<f32x4*>(part + ((int64_t)slice * M + m) * N + n0 + nl) = v;
        } else {
            const u32x2 bb = *reinterpret_cast<const u32x2*>(bias + n0 + nl);
            uint16_t o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float y = v[e] + Elem<T>::widen((uint16_t)(bb[e >> 1] >> (16 * (e & 1))));
                if (EPI == ENC_EPI_GELU) y = gelu_erf(y);
                o[e] = narrow<T>(y);
            }
            *reinterpret_cast<u32x2*>(out16 + (int64_t)m * N + n0 + nl) =
                u32x2{(uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16)};
        }
    }
}

template <class T, int MT>
int linear_epi(const void* x, int32_t M, int32_t K, const void* W, int32_t N, const void* bias, int epilogue, void* out16, float* part,
               hipStream_t s) {
    const int chunks = (K + LIN_CHUNK - 1) / LIN_CHUNK;
    const int slices = epilogue == ENC_EPI_PARTIAL ? encoder_ksplit(N, K) : 1;
    const int per = (chunks + slices - 1) / slices;
    const dim3 grid((unsigned)(N / LIN_SLAB), (unsigned)slices, (unsigned)((M + LIN_BLOCK_ROWS - 1) / LIN_BLOCK_ROWS)), block(WAVE * LIN_WAVES);
    const uint16_t* x16 = static_cast<const uint16_t*>(x);
    const uint16_t* w16 = static_cast<const uint16_t*>(W);
    const uint16_t* b16 = static_cast<const uint16_t*>(bias);
    uint16_t* o16 = static_cast<uint16_t*>(out16);
    if (epilogue == ENC_EPI_BIAS)
        hipLaunchKernelGGL((encoder_linear_kernel<T, MT, ENC_EPI_BIAS>), grid, block, 0, s, x16, M, K, w16, N, b16, per, o16, part);
    else if (epilogue == ENC_EPI_GELU)
        hipLaunchKernelGGL((encoder_linear_kernel<T, MT, ENC_EPI_GELU>), grid, block, 0, s, x16, M, K, w16, N, b16, per, o16, part);
    else
        hipLaunchKernelGGL((encoder_linear_kernel<T, MT, ENC_EPI_PARTIAL>), grid, block, 0, s, x16, M, K, w16, N, b16, per, o16, part);
    RL_HIP(hipGetLastError());
    return RL_OK;
}

// The token tiles a wave keeps are a template argument (the accumulators are registers); a row's arithmetic is the same in all four.
// Up to 256 rows the grid has one token block; above, ceil(M / 256) blocks of the eight-tile kernel.
template <class T>
int linear_t(const void* x, int32_t M, int32_t K, const void* W, int32_t N, const void* bias, int epilogue, void* out16, float* part,
             hipStream_t s) {
    if (M <= 32) return linear_epi<T, 1>(x, M, K, W, N, bias, epilogue, out16, part, s);
    if (M <= 64) return linear_epi<T, 2>(x, M, K, W, N, bias, epilogue, out16, part, s);
    if (M <= 128) return linear_epi<T, 4>(x, M, K, W, N, bias, epilogue, out16, part, s);
    return linear_epi<T, 8>(x, M, K, W, N, bias, epilogue, out16, part, s);
}

}  // namespace

static_assert(RL_ENCODER_MAX_TOKENS == 8 * 32, "the linear kernel keeps at most eight token tiles of 32 in a wave's accumulators");
static_assert(LIN_BLOCK_ROWS == RL_ENCODER_MAX_TOKENS && RL_ENCODER_MAX_PACK_TOKENS % LIN_BLOCK_ROWS == 0 &&
                  RL_ENCODER_MAX_PACK_TOKENS / LIN_BLOCK_ROWS <= 65535,
              "a token block is the rows of one short pack; the pack cap is whole blocks on the grid's z axis");

// Slabs x slices near the CU count, every wave of a slice with at least one chunk of its own, at most ENC_KSPLIT_MAX slices -- and no
// empty slice: the launcher gives each ceil(chunks / slices) chunks.
int32_t encoder_ksplit(int32_t N, int32_t K) {
    const int chunks = (K + LIN_CHUNK - 1) / LIN_CHUNK;
    int want = 256 / std::max(1, N / LIN_SLAB);
    want = std::min(want, chunks / LIN_WAVES);
    want = std::max(1, std::min(want, ENC_KSPLIT_MAX));
    const int per = (chunks + want - 1) / want;
    return (chunks + per - 1) / per;
}

int launch_encoder_embed(const int32_t* ids, const int32_t* positions, const int32_t* type_ids, int32_t n_tokens, const void* tok,
                         int32_t vocab, const void* pos, int32_t max_positions, const void* typ, int32_t type_vocab, const void* ln_w,
                         const void* ln_b, int32_t hidden, float eps, int32_t dtype, void* out, hipStream_t s) {
    if (n_tokens <= 0) return RL_OK;
    const dim3 grid((unsigned)n_tokens), block(LN_THREADS);
    const size_t lds = (size_t)hidden * sizeof(float);
#define RL_ENC_EMBED(T)                                                                                                                   \
    hipLaunchKernelGGL((encoder_embed_kernel<T>), grid, block, lds, s, ids, positions, type_ids, static_cast<const uint16_t*>(tok), vocab, \
                       static_cast<const uint16_t*>(pos), max_positions, static_cast<const uint16_t*>(typ), type_vocab,                   \
                       static_cast<const uint16_t*>(ln_w), static_cast<const uint16_t*>(ln_b), hidden, eps, static_cast<uint16_t*>(out))
    if (dtype == RL_ATTN_BF16) RL_ENC_EMBED(__bf16);
    else RL_ENC_EMBED(_Float16);
#undef RL_ENC_EMBED
    RL_HIP(hipGetLastError());
    return RL_OK;
}

int launch_encoder_linear(const void* x, int32_t M, int32_t K, const void* W, int32_t N, const void* bias, int epilogue, int32_t dtype,
                          void* out16, float* part, hipStream_t s) {
    if (M <= 0) return RL_OK;
    if (dtype == RL_ATTN_BF16) return linear_t<__bf16>(x, M, K, W, N, bias, epilogue, out16, part, s);
    return linear_t<_Float16>(x, M, K, W, N, bias, epilogue, out16, part, s);
}

int launch_encoder_ln(const float* part, int32_t ksplit, int32_t M, int32_t hidden, const void* bias, const void* resid, const void* ln_w,
                      const void* ln_b, float eps, int32_t dtype, void* out, hipStream_t s) {
    if (M <= 0) return RL_OK;
    const dim3 grid((unsigned)M), block(LN_THREADS);
    const size_t lds = (size_t)hidden * sizeof(float);
#define RL_ENC_LN(T)                                                                                                                 \
    hipLaunchKernelGGL((encoder_ln_kernel<T>), grid, block, lds, s, part, ksplit, M, hidden, static_cast<const uint16_t*>(bias),     \
                       static_cast<const uint16_t*>(resid), static_cast<const uint16_t*>(ln_w), static_cast<const uint16_t*>(ln_b), \
                       eps, static_cast<uint16_t*>(out))
    if (dtype == RL_ATTN_BF16) RL_ENC_LN(__bf16);
    else RL_ENC_LN(_Float16);
#undef RL_ENC_LN
    RL_HIP(hipGetLastError());
    return RL_OK;
}

}  // namespace rl
