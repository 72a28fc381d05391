// Variable-length (packed, block-diagonal) softmax attention forward for gfx950.
//
//   out[t, h, :] = softmax_j(scale * q[t,h] . k[j,h]) . v[j,h],   j over the tokens of t's own sequence
//
// qkv is the fused projection as the encoder's `Layer.qkv` writes it, [n_tokens x 3 x heads x D] bf16 / fp16, read in place: q, k, v of
// head h at element offsets h*D, (heads + h)*D, (2*heads + h)*D of a token row of 3*heads*D elements.  out is [n_tokens x heads x D].
//
// One workgroup = one (query tile, head, sequence): NW waves of 32 query rows each -- NW = 2 (64 rows), or NW = 4 (128 rows) from
// max_len = 1024 on; workgroups past their sequence's end exit at once.  Keys / values arrive in tiles of 64 through LDS (the next
// tile's global loads in flight under this tile's arithmetic) and are consumed as two sub-tiles of 32:
//   S^T = K . Q^T   mfma_f32_32x32x16(A = K fragment from LDS, B = Q fragment in registers): the SWAPPED product, so a lane holds the
//                   scores of ONE query (column lane & 31) against 16 keys (rows (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)); the other 16
//                   keys sit in lane ^ 32, which is the one cross-lane step of the row maximum and of the final row sum.
//   online softmax in f32: t = score * (scale * log2 e), m' = max(m, max t), p = exp2(t - m'), O *= exp2(m - m'), l = l exp2(m - m') + sum p.
//                   `scale` touches f32 scores only; q is never rescaled in 16 bits.
//   O^T += V^T . P^T  mfma(A = V^T fragment from LDS, B = P): the accumulator of the first product IS the B operand of the second --
//                   registers 8s .. 8s+7 rounded to the input dtype are k-step s, whose k order is key 16 s + 8 (j >> 2) + 4 (lane >> 5)
//                   + (j & 3); V^T is laid out in LDS so that a lane reads exactly those keys as two 8-byte words.  No lane movement,
//                   no LDS round trip for P.  In bf16 P goes in as two operands, the rounded value and the rounded remainder (2 MFMAs).
// O^T again has the query on the lane, so the rescale factor and 1 / l are lane-local.
//
// LDS images (16 KiB at D = 64), both XOR-swizzled on 16-byte slots so that the 16 lanes of a ds_read group hit 16 different slots
// of the 256-byte bank row:
//   K   [64 keys][D]     slot c of row `key` stored at c ^ ((key / RP) & (D/8 - 1)), RP = rows per 256 B (2 at D = 64, 4 at D = 32)
//   V^T [D][64 keys]     slot (key / 8) of row d stored at (key / 8) ^ ((d >> 1 ^ d >> 3) & 7): conflict-free for the fragment read
//                        (lanes = 32 consecutive d) AND for the transposing 2-byte writes (lanes = 8 d-slots x 8 keys)
//
// Masking and safety.  Keys past the sequence end score -inf and their V rows are staged as zeros (0 * stale data of a neighbouring
// sequence could be NaN).  Key tile 0 of a non-empty sequence holds key 0, so m is finite from the first sub-tile on and exp2 never sees
// inf - inf.  Every token index is start + min(i, len - 1) with 0 <= start <= end <= n_tokens clamped from seq_offsets: offsets that
// break the contract give wrong numbers, never an access outside qkv / out.  Tiles are laid from the sequence's own start and nothing
// is accumulated across workgroups, so a sequence's output bits depend neither on its neighbours in the pack nor on max_len.
#include "common.h"

namespace rl {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <class T> struct Mfma;
template <> struct Mfma<__bf16> {
    typedef bf16x8 v8;
    // bf16 rounds with a relative error of up to 2^-8; a single rounded P next to the rounded output leaves up to 2^-7 A, twice what the
    // kernel is held to.  P.V therefore takes P as hi + rounded remainder (two MFMAs per k-step): the output's own rounding is then all
    // that is left.  fp16 (2^-11) needs none.
    static constexpr bool p_split = true;
    static __device__ __forceinline__ f32x16 run(v8 a, v8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <> struct Mfma<_Float16> {
    typedef f16x8 v8;
    static constexpr bool p_split = false;
    static __device__ __forceinline__ f32x16 run(v8 a, v8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};

constexpr int ATT_KT = 64;            // keys per LDS tile (two sub-tiles of 32)
constexpr int ATT_LONG = 1024;        // max_len from which a workgroup is four waves (128 query rows) instead of two (64)

// slot swizzle of the V^T image (see the header comment)
__device__ __forceinline__ int vt_swz(int d) { return ((d >> 1) ^ (d >> 3)) & 7; }

template <class T, int D, int NW>
__global__ __launch_bounds__(64 * NW) void attention_varlen_kernel(const uint16_t* __restrict__ qkv, const int32_t* __restrict__ seq_offsets,
                                                                       int64_t n_tokens, int heads, float c2, uint16_t* __restrict__ out) {
    typedef typename Mfma<T>::v8 v8;
    constexpr int NT = 64 * NW, ATT_QT = 32 * NW;
    constexpr int CH = D / 8;                 // 16-byte slots per K row
    constexpr int RP = 16 / CH;               // K rows per 256 bytes
    constexpr int NCH = ATT_KT * CH / NT;     // slots each thread stages per tile, of K and of V
    constexpr bool P_SPLIT = Mfma<T>::p_split;
    __shared__ __attribute__((aligned(16))) uint16_t k_lds[ATT_KT * D];
    __shared__ __attribute__((aligned(16))) uint16_t vt_lds[D * ATT_KT];

    const int seq = blockIdx.z, head = blockIdx.y;
    int64_t s0 = seq_offsets[seq], s1 = seq_offsets[seq + 1];
    s0 = s0 < 0 ? 0 : (s0 > n_tokens ? n_tokens : s0);
    s1 = s1 < s0 ? s0 : (s1 > n_tokens ? n_tokens : s1);
    const int len = (int)(s1 - s0);           // offsets are int32: fits
    const int q0 = blockIdx.x * ATT_QT;
    if (q0 >= len) return;                     // (uniform; also every empty sequence) -- from here on len >= 1 and s0 + len - 1 < n_tokens

    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = wave_id();
    const int64_t ld = (int64_t)3 * heads * D;
    const uint16_t* qbase = qkv + (int64_t)head * D;
    const uint16_t* kbase = qbase + (int64_t)heads * D;
    const uint16_t* vbase = kbase + (int64_t)heads * D;

    // Q fragments: B operand, lane (r, h) holds Q[query r][16 ks + 8 h .. + 7]
    const int qrow = q0 + wave * 32 + r;
    const int64_t tq = s0 + (qrow < len ? qrow : len - 1);
    v8 qf[D / 16];
#pragma unroll
    for (int ks = 0; ks < D / 16; ++ks)
        qf[ks] = __builtin_bit_cast(v8, *reinterpret_cast<const u32x4*>(qbase + tq * ld + ks * 16 + h * 8));

    f32x16 o[D / 32];
#pragma unroll
    for (int db = 0; db < D / 32; ++db)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[db][i] = 0.f;
    float m = -INFINITY, l = 0.f;

    const int n_tiles = (len + ATT_KT - 1) / ATT_KT;
    u32x4 kreg[NCH], vreg[NCH];
    auto fetch = [&](int kt) {
#pragma unroll
        for (int n = 0; n < NCH; ++n) {
            const int i = tid + n * NT, key = i / CH, c = i % CH;
            const int kk = kt * ATT_KT + key;
            const int64_t tk = s0 + (kk < len ? kk : len - 1);
            kreg[n] = *reinterpret_cast<const u32x4*>(kbase + tk * ld + c * 8);
            u32x4 v = *reinterpret_cast<const u32x4*>(vbase + tk * ld + c * 8);
            if (kk >= len) v = u32x4{0u, 0u, 0u, 0u};
            vreg[n] = v;
        }
    };
    fetch(0);
    for (int kt = 0; kt < n_tiles; ++kt) {
        __syncthreads();  // every wave is done reading the previous tile
#pragma unroll
        for (int n = 0; n < NCH; ++n) {
            const int i = tid + n * NT, key = i / CH, c = i % CH;
            *reinterpret_cast<u32x4*>(k_lds + key * D + ((c ^ ((key / RP) & (CH - 1))) << 3)) = kreg[n];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int d = c * 8 + e;
                const uint32_t w = vreg[n][e >> 1];
                vt_lds[d * ATT_KT + ((((key >> 3) ^ vt_swz(d))) << 3) + (key & 7)] = (uint16_t)((e & 1) ? (w >> 16) : (w & 0xffffu));
            }
        }
        __syncthreads();
        if (kt + 1 < n_tiles) fetch(kt + 1);  // in flight under this tile's arithmetic

#pragma unroll
        for (int st = 0; st < 2; ++st) {
            const int key0 = kt * ATT_KT + st * 32;
            if (key0 >= len) break;  // (uniform) a sub-tile with no real key
            f32x16 s;
#pragma unroll
            for (int i = 0; i < 16; ++i) s[i] = 0.f;
            const int krow = st * 32 + r;
#pragma unroll
            for (int ks = 0; ks < D / 16; ++ks) {
                const int c = ks * 2 + h;
                const v8 kf = __builtin_bit_cast(v8, *reinterpret_cast<const u32x4*>(k_lds + krow * D + ((c ^ ((krow / RP) & (CH - 1))) << 3)));
                s = Mfma<T>::run(kf, qf[ks], s);
            }
            float mx = -INFINITY;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int kk = key0 + (i & 3) + 8 * (i >> 2) + 4 * h;
                s[i] = kk < len ? s[i] * c2 : -INFINITY;
                mx = fmaxf(mx, s[i]);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float mn = fmaxf(m, mx);  // finite: sub-tile 0 of tile 0 holds key 0
            const float alpha = __builtin_amdgcn_exp2f(m - mn);
            m = mn;
            float sum = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                s[i] = __builtin_amdgcn_exp2f(s[i] - mn);  // v_exp_f32: arguments <= 0, results in [0, 1]
                sum += s[i];
            }
            l = l * alpha + sum;
            // P as the operand of P.V: rounded to the input dtype -- and, where that dtype keeps 8 bits (bf16), followed by the rounded
            // remainder as a second operand, so that what P's rounding costs drops from 2^-8 to 2^-16 of A (see P_SPLIT)
            v8 pf[2], pr[2];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const T hi = (T)s[i];
                pf[i >> 3][i & 7] = hi;
                if (P_SPLIT) pr[i >> 3][i & 7] = (T)(s[i] - (float)hi);
            }
#pragma unroll
            for (int db = 0; db < D / 32; ++db) {
#pragma unroll
                for (int i = 0; i < 16; ++i) o[db][i] *= alpha;
                const int d = db * 32 + r;
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const int kc = st * 4 + s2 * 2;
                    const u32x2 lo = *reinterpret_cast<const u32x2*>(vt_lds + d * ATT_KT + ((kc ^ vt_swz(d)) << 3) + 4 * h);
                    const u32x2 hi = *reinterpret_cast<const u32x2*>(vt_lds + d * ATT_KT + (((kc + 1) ^ vt_swz(d)) << 3) + 4 * h);
                    const v8 vf = __builtin_bit_cast(v8, u32x4{lo[0], lo[1], hi[0], hi[1]});
                    o[db] = Mfma<T>::run(vf, pf[s2], o[db]);
                    if (P_SPLIT) o[db] = Mfma<T>::run(vf, pr[s2], o[db]);
                }
            }
        }
    }

    l += __shfl_xor(l, 32, 64);
    if (qrow >= len) return;
    const float inv = 1.0f / l;
    uint16_t* orow = out + (tq * heads + head) * D;
#pragma unroll
    for (int db = 0; db < D / 32; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            typedef T t4 __attribute__((ext_vector_type(4)));
            t4 w;
#pragma unroll
            for (int e = 0; e < 4; ++e) w[e] = (T)(o[db][4 * g + e] * inv);
            *reinterpret_cast<u32x2*>(orow + db * 32 + 8 * g + 4 * h) = __builtin_bit_cast(u32x2, w);
        }
}

template <class T, int D, int NW>
int launch_nw(const void* qkv, const int32_t* off, int32_t n_seqs, int64_t n_tokens, int32_t max_len, int32_t heads, float scale, void* out,
              hipStream_t s) {
    const dim3 grid((unsigned)((max_len + 32 * NW - 1) / (32 * NW)), (unsigned)heads, (unsigned)n_seqs);
    hipLaunchKernelGGL((attention_varlen_kernel<T, D, NW>), grid, dim3(64 * NW), 0, s, static_cast<const uint16_t*>(qkv), off, n_tokens, heads,
                       scale * 1.4426950408889634f, static_cast<uint16_t*>(out));
    RL_HIP(hipGetLastError());
    return RL_OK;
}

// A query row's arithmetic does not depend on how many rows share its workgroup (the key tiles and their order are the same), so the
// choice below changes the time, never the bits: long sequences amortise each staged K / V tile over four waves, short ones keep the
// 64-row tile that wastes fewer rows past a sequence's end.
template <class T, int D>
int launch_t(const void* qkv, const int32_t* off, int32_t n_seqs, int64_t n_tokens, int32_t max_len, int32_t heads, float scale, void* out,
             hipStream_t s) {
    if (max_len >= ATT_LONG) return launch_nw<T, D, 4>(qkv, off, n_seqs, n_tokens, max_len, heads, scale, out, s);
    return launch_nw<T, D, 2>(qkv, off, n_seqs, n_tokens, max_len, heads, scale, out, s);
}

}  // namespace

int launch_attention_varlen(const void* qkv, const int32_t* seq_offsets, int32_t n_seqs, int64_t n_tokens, int32_t max_len, int32_t heads,
                            int32_t head_dim, int32_t dtype, float scale, void* out, hipStream_t s) {
    if (n_seqs <= 0 || n_tokens <= 0 || max_len <= 0) return RL_OK;
    if (dtype == RL_ATTN_BF16) {
        if (head_dim == 32) return launch_t<__bf16, 32>(qkv, seq_offsets, n_seqs, n_tokens, max_len, heads, scale, out, s);
        if (head_dim == 64) return launch_t<__bf16, 64>(qkv, seq_offsets, n_seqs, n_tokens, max_len, heads, scale, out, s);
    } else if (dtype == RL_ATTN_F16) {
        if (head_dim == 32) return launch_t<_Float16, 32>(qkv, seq_offsets, n_seqs, n_tokens, max_len, heads, scale, out, s);
        if (head_dim == 64) return launch_t<_Float16, 64>(qkv, seq_offsets, n_seqs, n_tokens, max_len, heads, scale, out, s);
    }
    return fail(RL_ERR_UNSUPPORTED, "rl_attention_varlen: head_dim must be 32 or 64, dtype bf16 or fp16");
}

}  // namespace rl
