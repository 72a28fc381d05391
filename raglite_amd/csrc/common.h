// Shared declarations for libraglite_hip.so (gfx950 only; wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <string>

#include "raglite_hip.h"

namespace rl {

// ---- host-side error plumbing ---------------------------------------------------------------
void set_error(const std::string& msg);
int fail(int code, const std::string& msg);

#define RL_HIP(expr)                                                                         \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess)                                                                \
            return ::rl::fail(_e == hipErrorOutOfMemory ? RL_ERR_NOMEM : RL_ERR_HIP,         \
                              std::string(#expr) + ": " + hipGetErrorString(_e));            \
    } while (0)

#define RL_TRY(expr)              \
    do {                          \
        int _s = (expr);          \
        if (_s != RL_OK) return _s; \
    } while (0)

// Experiment switches (kernel A/B variants, timing skeletons, s_memtime traces) are read from the environment ONLY in experiment
// builds (-DRAGLITE_EXPERIMENTS: raglite_amd._build.build(experiments=True) -> libraglite_hip_exp.so, used by scripts/gpu_calls/).  The
// shipped library reads no environment variable: there every switch folds to "off" at compile time.
#ifdef RAGLITE_EXPERIMENTS
inline const char* exp_env(const char* name) { return std::getenv(name); }
#else
inline const char* exp_env(const char*) { return nullptr; }
#endif

constexpr int WAVE = 64;
constexpr int K_MAX = 2048;       // largest top-k the selection stage supports
constexpr int HIST_BINS = 2048;   // top 11 bits of the orderable score key
constexpr int CAND_CAP = 4096;    // threshold-bin candidates kept per query before the slow path
constexpr int MERGE_CAP = 8192;   // n_lists * k_in accepted by rl_merge_topk

// ---- device helpers ----------------------------------------------------------------------------
#ifdef __HIPCC__

// Monotone map float -> uint32: larger float <=> larger key; every NaN -> 0 (ranks last).
__device__ __forceinline__ uint32_t score_key(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_score(uint32_t k) {
    uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __uint_as_float(u);
}
// 64-bit total order: (score desc, id asc)  <=>  key64 desc.  key64 == 0 is the padding value.
__device__ __forceinline__ uint64_t make_key64(float score, uint32_t id) {
    return ((uint64_t)score_key(score) << 32) | (uint64_t)(0xffffffffu - id);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}


// Wave-uniform id of the calling wave inside its block (provably uniform for the compiler).
__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

#endif  // __HIPCC__

// Grid of a persistent streaming kernel: exactly one resident generation of workgroups (CUs x the
// occupancy the runtime reports for this kernel), capped by the work available.  Measured on the B = 1
// scan: 5 blocks/CU (= its occupancy) 0.71 ms, 8 blocks/CU 0.81 ms -- a second, partial generation of
// blocks costs a tail.
template <class Kernel>
inline int persistent_grid(Kernel kernel, int block_threads, int64_t max_useful_blocks) {
    static thread_local int cached_cu = 0;
    if (cached_cu == 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cached_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cached_cu <= 0)
            cached_cu = 256;
    }
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block_threads, 0) != hipSuccess || per_cu <= 0)
        per_cu = 4;
    return (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)cached_cu * per_cu, max_useful_blocks));
}

// ---- kernel launchers (one per .hip file) -------------------------------------------------------
int launch_synth(float* dst, int64_t start, int64_t count, uint64_t seed, int kind, hipStream_t s);

int launch_pool_norm(const float* tokens, int32_t dim, const int64_t* span_begin, const int64_t* span_end,
                     int64_t n_spans, int normalize, double eps, float* out_f32, uint16_t* out_f16,
                     hipStream_t s);

// attention_varlen.hip: arguments as rl_attention_varlen takes them, already checked
int launch_attention_varlen(const void* qkv, const int32_t* seq_offsets, int32_t n_seqs, int64_t n_tokens, int32_t max_len, int32_t heads,
                            int32_t head_dim, int32_t dtype, float scale, void* out, hipStream_t s);

// encoder.hip: the kernels of rl_encoder_forward.  dtype: RL_ATTN_BF16 / RL_ATTN_F16, of every `void*` below;
// M, n_tokens <= RL_ENCODER_MAX_PACK_TOKENS rows (the linear kernel takes them in token blocks of RL_ENCODER_MAX_TOKENS, one per
// blockIdx.z); hidden, K, N multiples of 32; arguments already checked
constexpr int32_t ENC_KSPLIT_MAX = 8;
constexpr int32_t ENC_HIDDEN_MAX = 8192;        // a row of f32 in a workgroup's LDS (the layer norms)
int32_t encoder_ksplit(int32_t N, int32_t K);  // the K slices of a projection into f32 partials: a function of (N, K) alone
// out[t] = LN(tok[ids[t]] + pos[positions[t]] + typ[type_ids ? type_ids[t] : 0]), indices clamped into their tables
int launch_encoder_embed(const int32_t* ids, const int32_t* positions, const int32_t* type_ids, int32_t n_tokens, const void* tok,
                         int32_t vocab, const void* pos, int32_t max_positions, const void* typ, int32_t type_vocab, const void* ln_w,
                         const void* ln_b, int32_t hidden, float eps, int32_t dtype, void* out, hipStream_t s);
enum EncEpilogue { ENC_EPI_BIAS = 0, ENC_EPI_GELU = 1, ENC_EPI_PARTIAL = 2 };
// x [M x K] . W [N x K]^T: ENC_EPI_BIAS / ENC_EPI_GELU -> out16 [M x N] = (gelu_erf)(. + bias); ENC_EPI_PARTIAL -> part [encoder_ksplit(N, K) x
// M x N] f32, the raw K slices (bias, residual and their ordered sum belong to launch_encoder_ln)
int launch_encoder_linear(const void* x, int32_t M, int32_t K, const void* W, int32_t N, const void* bias, int epilogue, int32_t dtype,
                          void* out16, float* part, hipStream_t s);
// out[r] = LN(part[0][r] + .. + part[ksplit - 1][r] + bias + resid[r])
int launch_encoder_ln(const float* part, int32_t ksplit, int32_t M, int32_t hidden, const void* bias, const void* resid, const void* ln_w,
                      const void* ln_b, float eps, int32_t dtype, void* out, hipStream_t s);
// encoder_head.hip: out_logits[s] = head_w . tanh(pooler_w x[clamp(seq_offsets[s])] + pooler_b) + head_b in f32, a quiet
// NaN for an empty sequence; n_tokens >= 1, hidden a multiple of 32 and <= ENC_HIDDEN_MAX; arguments already checked
int launch_encoder_head(const void* x, const int32_t* seq_offsets, int32_t n_seqs, int32_t n_tokens, int32_t hidden, const void* pooler_w,
                        const void* pooler_b, const void* head_w, const void* head_b, int32_t dtype, float* out_logits, hipStream_t s);

// scan.hip
enum ScanMode { SCAN_RAW_DOT = 0, SCAN_COSINE = 1, SCAN_DOT = 2, SCAN_L2 = 3 };

// The metric transform of a raw dot product (transform_kernel in scan.hip and transform_hist_kernel in select.hip share
// these statements, so both give the same bits): qss = |q|^2 summed as block_query_sumsq does, qn = sqrtf(qss).
__device__ __forceinline__ float transform_score(float d, int mode, float row_norm, float row_sumsq, float qn, float qss) {
    if (mode == SCAN_COSINE) return 1.0f - (1.0f - d / (row_norm * qn));
    if (mode == SCAN_DOT) return 1.0f + d;
    if (mode == SCAN_L2) return 1.0f - sqrtf(fmaxf(row_sumsq + qss - 2.0f * d, 0.f));
    return d;
}
// scores[b * ld + row] for b < nb (nb <= 4 per launch handled inside), rows < n.
int launch_scan_rows(const float* E, int64_t n, int32_t dim, const float* queries, int32_t nb,
                     const float* row_norm, int mode, float* scores, int64_t ld, hipStream_t s, const uint32_t* run_if = nullptr);
// out[b] = A @ q[b] for b < nb in one launch, each with the bits of launch_scan_rows(A, dim, dim, q[b], 1, .., SCAN_RAW_DOT, ..)
int launch_adapter_rows(const float* A, int32_t dim, const float* queries, int32_t nb, float* out, hipStream_t s);
// scan16.hip: the same over an fp16-stored corpus (dim <= 1024) -- or over the HI plane of a WIDE fp32 index (dim <= 4096, nb <= 4: raw dots)
int launch_scan_rows16(const uint16_t* E, int64_t n, int32_t dim, const float* queries, int32_t nb,
                       const float* row_norm, int mode, float* scores, int64_t ld, hipStream_t s);
int launch_row_norms16(const uint16_t* E, int64_t n, int32_t dim, float* norm, float* sumsq, hipStream_t s);
int launch_row_norms(const float* E, int64_t n, int32_t dim, float* norm, float* sumsq, hipStream_t s);
int launch_cast_f16(const float* src, uint16_t* dst, int64_t count, hipStream_t s);
// dst = fp16(src * scale) rounded to nearest even (the HI plane); count % 8 == 0, 16-byte aligned pointers
int launch_cast_f16_scaled(const float* src, uint16_t* dst, int64_t count, float scale, hipStream_t s);
int launch_fill_f32(float* dst, float value, int64_t count, hipStream_t s);
int launch_scale_f32(const float* src, float* dst, float factor, int64_t count, hipStream_t s, uint32_t* zero_words = nullptr,
                     int n_zero = 0);  // hi_filter.hip: dst = src * factor (and n_zero words set to zero on the way)
// in-place metric transform of raw dots: scores[b*ld+i] (i<n), per-row norm / sumsq, per-query norm.
// (pre_scale: the raw dots are multiplied by it first -- a power of two, exact; run_if as in launch_topk)
int launch_transform(float* scores, int32_t nb, int64_t n, int64_t ld, const float* row_norm,
                     const float* row_sumsq, const float* queries, int32_t dim, int mode, hipStream_t s, float pre_scale = 1.0f,
                     const uint32_t* run_if = nullptr);

// select.hip
struct SelectWorkspace {      // device buffers sized for `capacity_queries`
    uint32_t* hist = nullptr; // [B][HIST_BINS + 8]  (bins, then counters).  ALL ZERO between selections: zeroed when
                              // allocated, and the final kernel of every selection zeroes its query's row again once it
                              // has read it -- no memset launch in front of every top-k
    uint64_t* sel = nullptr;  // [B][K_MAX]
    uint64_t* cand = nullptr; // [B][CAND_CAP]
    uint32_t* pv = nullptr;   // [3 B + 16] counters, flag block, bounds and thresholds of launch_topk_pivot
    int32_t capacity_queries = 0;
    bool dirty = false;       // a launch sequence was cut short by an error: re-zero `hist` before the next use
    int block_route = 2;      // RL_OPT_TOPK_BLOCK: selections of <= 256 k scores per query in ONE launch, one block per query (select.hip); 2: with the thread-maximum prefilter
};
int select_workspace_reserve(SelectWorkspace& ws, int32_t n_queries, hipStream_t s);
void select_workspace_free(SelectWorkspace& ws);
// run_if != nullptr: the three kernels return at once unless *run_if != 0 (the guarded dense fallback of the fused top-k).
// have_hist: the histogram of `scores` is already in ws.hist (launch_transform_hist) -- skip that pass.
// emit (the half-bytes row search, api.hip: search_rows_hi): the selection also lists every row whose score is within 2 m[q] of the k-th best
// -- the candidates of the exact re-scoring -- without another pass over the scores (topk_filter_kernel / topk_final_body have the argument)
struct HiEmit {
    const float* m = nullptr;         // [n_queries] error bound per query (launch_transform_hist: HiBound)
    int32_t cap = 0;                  // slots per candidate list
    int32_t* ids = nullptr;           // [n_queries x cap] rows; nullptr = no emission
    float* norms = nullptr;           // [n_queries x cap] their norms (with row_norm)
    const float* row_norm = nullptr;  // [n] (cosine) or nullptr
    uint32_t* cnt = nullptr;          // [n_queries], zero on entry
    uint32_t* flag = nullptr;         // set on overflow / unusable threshold
    float* thr = nullptr;             // [n_queries] (optional) the thresholds, for diagnostics
    int l2 = 0;                       // the scores are l2 similarities 1 - sqrt(D), m the bound of D: lower_threshold's other form
};
int launch_topk(const float* scores, int32_t n_queries, int64_t n, int64_t ld, int32_t k,
                SelectWorkspace& ws, float* out_scores, int32_t* out_ids, hipStream_t s, const uint32_t* run_if = nullptr,
                bool have_hist = false, const HiEmit* emit = nullptr);
// Transform + exact top-k of raw dots in ONE guarded launch, one block per query (slow: the fallback of the half-bytes row search)
int launch_guarded_select(float* scores, int32_t nb, int64_t n, int64_t ld, int32_t k, const float* row_norm, const float* row_sumsq,
                          const float* queries, int32_t dim, int mode, float pre_scale, float* out_scores, int32_t* out_ids,
                          const uint32_t* run_if, hipStream_t s, uint32_t* host_flag = nullptr);
// launch_transform (scan.hip) + the selection's histogram pass in ONE launch: raw dots -> similarities in place, and their
// 2048-bin key histogram into ws.hist (same statements as transform_kernel: same bits).  Follow with launch_topk(have_hist).
// pre_scale: the raw dots are multiplied by it first (a power of two: exact; 1 = the plain transform); run_if as in launch_topk.
// zero_words / n_zero (<= 256): words this launch also sets to zero (the candidate counters + flag of a B <= 16 row search: no memset launch).
// bound: m_out[b] = the half-bytes search's error bound of query b -- cosine: m_rel; dot: m_rel * e_norm_bound * |q_b| + 2^-22
// The half-bytes search's candidate threshold (hi_filter.hip has the derivation of the l2 form in front of approx_threshold_kernel)
__device__ __forceinline__ float l2_delta(float a, float eps, float e_max, float qn) {
    const float t = e_max + qn;
    return (2.0f * a * qn + 2.0f * eps * t * t) * 1.0001f;
}
// the candidate threshold under a lower bound P of the k-th best approximate similarity; m: the query's bound (l2: delta, in squared distance)
__device__ __forceinline__ float lower_threshold(float P, float m, bool l2) {
    if (!l2) return P - 2.0f * m;
    const float r = fmaxf(1.0f - P, 0.f);
    return 1.0f - sqrtf(fmaf(r, r, 2.0f * m)) * (1.0f + 0x1p-18f) - 0x1p-20f;
}

struct HiBound {
    float* m_out = nullptr;
    float m_rel = 0.f, e_norm_bound = 0.f;
    float e_max = 0.f;  // l2 (round 6): max |e|; m_rel = the rounding term per |q| |e| (sum_eps), e_norm_bound = the dot bound per |q| -- m_out[b] is then
                        // the bound of the SQUARED distance, hi_filter.hip: l2_delta
};
int launch_transform_hist(float* scores, int32_t nb, int64_t n, int64_t ld, const float* row_norm, const float* row_sumsq,
                          const float* queries, int32_t dim, int mode, SelectWorkspace& ws, hipStream_t s, float pre_scale = 1.0f,
                          const uint32_t* run_if = nullptr, uint32_t* zero_words = nullptr, int n_zero = 0, const HiBound* bound = nullptr);
int launch_group_chunk_max(const float* hit_scores, const int32_t* hit_rows, int32_t n_queries,
                           int32_t num_hits, const int64_t* chunk_offsets, int64_t n_chunks, int32_t k,
                           float* out_scores, int32_t* out_chunks, int32_t* out_counts, hipStream_t s);
// The metric transform of raw dots applied on the way into the merge (n_lists == 1): record j of query q is transform_score(in_scores, mode,
// row_norm[q * k_in + j], .., |queries[q]|) -- the statements of transform_kernel (same bits), without its launch.
struct MergeTransform {
    const float* row_norm = nullptr;  // [n_queries x k_in] (cosine), else unused
    const float* queries = nullptr;   // [n_queries x dim]; nullptr = no transform
    int dim = 0, mode = 0;
};
int launch_merge_topk(const float* in_scores, const int32_t* in_ids, int32_t n_lists, int32_t n_queries,
                      int32_t k_in, int32_t k, float* out_scores, int32_t* out_ids, hipStream_t s,
                      const uint32_t* counts = nullptr,  // counts (n_lists == 1): records list q really holds
                      const MergeTransform* transform = nullptr);

// The bitset each query of a batch is masked with (mask.hip, select.hip, keyword.hip): query b reads sets + set[b] * ld, or `none` where
// set[b] < 0; set == nullptr: every query reads `sets`.  A query whose bitset is nullptr is not masked.  A plain pointer converts to
// the mask every query shares.
struct QueryMask {
    const uint32_t* sets = nullptr;
    int64_t ld = 0;                  // words per bitset
    const int32_t* set = nullptr;    // device [n_queries]
    const uint32_t* none = nullptr;
    QueryMask() = default;
    QueryMask(const uint32_t* bits) : sets(bits) {}  // NOLINT(google-explicit-constructor)
    QueryMask(const uint32_t* sets_, int64_t ld_, const int32_t* set_, const uint32_t* none_) : sets(sets_), ld(ld_), set(set_), none(none_) {}
    __host__ __device__ const uint32_t* of(int64_t b) const {
        if (!set) return sets;
        const int32_t f = set[b];
        return f >= 0 ? sets + (int64_t)f * ld : none;
    }
    bool any() const { return sets || none; }  // (host) some query of the batch is masked
    QueryMask from(int32_t b0) const {         // the mask of the sub-batch that starts at query b0
        QueryMask m = *this;
        if (m.set) m.set += b0;
        return m;
    }
};

// select.hip, rank cut (order-first-then-filter, src/raglite/_search.py:120-141): rows outside the rank_limit best of their
// query, and rows whose keep bit is clear, become -inf
// the cut in stages (a corpus sharded over several indexes sums each level's histogram over the shards between them)
size_t rank_stage_scratch_bytes(int32_t n_queries, int64_t n);
int launch_rank_stage_level(const float* scores, int32_t n_queries, int64_t n, int64_t ld, int64_t rank_limit, int level, void* scratch,
                            uint32_t* level_out, hipStream_t s);
int launch_rank_stage_set_level(int32_t n_queries, int level, void* scratch, const uint32_t* level_in, hipStream_t s);
int launch_rank_stage_ties(const float* scores, int32_t n_queries, int64_t n, int64_t ld, int64_t rank_limit, void* scratch,
                           uint32_t* totals_out, hipStream_t s);
int launch_rank_stage_apply(float* scores, int32_t n_queries, int64_t n, int64_t ld, int64_t rank_limit, const uint32_t* keep_bits,
                            void* scratch, const uint32_t* tie_base, hipStream_t s);
size_t rank_cut_scratch_bytes(int32_t n_queries, int64_t n);
// limits != nullptr: query b cuts at limits[b] instead of rank_limit (device [n_queries]; >= n: no cut, only its keep bits)
int launch_rank_cut(float* scores, int32_t n_queries, int64_t n, int64_t ld, int64_t rank_limit, const uint32_t* limits, const QueryMask& keep,
                    void* scratch, hipStream_t s);

// hi_filter.hip: helpers of the half-bytes single-query search (api.hip: search_rows_hi)
int launch_approx_threshold(const float* topk, int32_t nb, int32_t k, const float* queries, int32_t dim, int mode, float m_rel,
                            float e_norm_bound, float* thr, uint32_t* cnt, uint32_t* flag, hipStream_t s, float e_max = 0.f);  // also zeroes cnt[0..nb) and *flag
// top_s / top_i [nb x k] (optional): the approximate top-k in selection order -- only entries ranking BELOW its k-th one are collected
struct PivotMaxSim {                  // the MaxSim flavour of the pivot route (hi_filter.hip: transform_bmax_kernel)
    int nq = 0;                       // query vectors per query (0: a row search)
    int64_t q_stride = 0;             // floats between two queries
    float m_abs = 0.f;                // m_b = m_abs * sum_i |q_i|
    int32_t* fill_ids = nullptr;      // [nb x cap] candidate lists to pre-fill with -1
    int64_t fill_n = 0;               // (set by the launcher)
    int per_wave = 0;                 // (set by the launcher)
    int read_only = 0;                // the scores are not rewritten (an identity transform: launch_topk_pivot)
};
size_t pivot_scratch_words(int32_t nb);
bool pivot_route_takes(int64_t n, int32_t k);
int launch_pivot_route(float* scores, int32_t nb, int64_t n, int64_t ld, int32_t k, const float* row_norm, const float* row_sumsq, const float* queries,
                       int32_t dim, int mode, float pre_scale, uint64_t* bmax, uint32_t* zero_words, int n_zero, const HiBound& bound, float* thr,
                       int32_t cap, int32_t* ids, float* norms, uint32_t* cnt, uint32_t* flag, hipStream_t s, const float* E = nullptr,
                       float* gather_out = nullptr, bool* gathered = nullptr, const PivotMaxSim* maxsim = nullptr, const float* aux_src = nullptr,
                       int64_t aux_ld = 0);
// Exact top-k of scores that CROWD (l2 similarities 1 - |e - q| of a big corpus share one exponent and a few mantissa bits: the radix selection's
// threshold bin then holds the whole corpus and its one-block slow path takes 2 ms per query): the pivot route's group maxima do not care how the
// scores are distributed.  k <= 128, >= 3 k groups, <= 240 queries; RL_ERR_UNSUPPORTED otherwise.  Same results as launch_topk.
int launch_topk_pivot(const float* scores, int32_t n_queries, int64_t n, int64_t ld, int32_t k, SelectWorkspace& ws, float* out_scores,
                      int32_t* out_ids, hipStream_t s);
int launch_collect_above(const float* scores, int32_t nb, int64_t n, int64_t ld, const float* thr, const float* row_norm, int32_t cap,
                         int32_t* ids, float* norms, uint32_t* cnt, uint32_t* flag, hipStream_t s, const float* top_s = nullptr,
                         const int32_t* top_i = nullptr, int32_t k = 0);
// thr[b] = min_j exact[b][j] - m[b] (the k-th best EXACT score of the approximate top-k bounds the k-th best overall from below);
// ids[b][0 .. k) = top_i[b], es[b][0 .. k) = exact[b], cnt[b] = k; unusable -> *flag, thr = +inf, cnt = 0.  See exact_threshold_kernel.
// fp16 queries over an fp16-stored corpus: widen the queries (exact), certify per query that the one-product pass lost nothing and hand its
// top-k out as the result (hi_filter.hip)
int launch_widen_f16(const uint16_t* src, float* dst, int64_t count, hipStream_t s);
int launch_f16_exact_finish(const float* Q, int32_t nq, int32_t dim, int64_t q_stride, const float* q_unscale, const float* top_s,
                            const int32_t* top_i, int32_t n_queries, int32_t k, float* out_s, int32_t* out_i, uint32_t* cnt, uint32_t* flag,
                            hipStream_t s);
int launch_exact_threshold(const float* exact, const int32_t* top_i, int32_t n_queries, int32_t k, float* m, int32_t cap, float* thr,
                           uint32_t* cnt, int32_t* ids, float* es, uint32_t* flag, hipStream_t s, const float* qsum = nullptr, float m_abs = 0.f,
                           float e_norm_max = 0.f, bool with_lo = false, const float* top_s = nullptr);  // top_s: the approximate top-k scores (-inf: masked)
// MaxSim flavour of the threshold: thr[b] = topk[b * k + k - 1] - 2 * m_rel * e_max * sum_i |q_i|; zeroes cnt[b]; sets *flag when
// the k-th score is unusable.  One block per query.
// q_unscale != nullptr (one-product pass: only the queries' fp16 hi halves were multiplied): q_unscale[2 * b] = 2^(ex - 14) of
// query b (the meta words of launch_query_planes), and the threshold drops by another 2 * e_norm_max * sum_i |q_lo,i| with
// q_lo,i = q_i - fp16(q_i * scale) / scale, recomputed here with the statement query_planes_kernel uses.
int launch_maxsim_threshold(const float* topk, int32_t n_queries, int32_t k, const float* Q, int32_t nq, int32_t dim, int64_t q_stride,
                            float m_rel, float e_max, float* thr, uint32_t* cnt, uint32_t* flag, hipStream_t s,
                            const float* q_unscale = nullptr, float e_norm_max = 0.f, float* m_out = nullptr);  // m_out[b] = the bound m_b
// A MaxSim batch over a sharded corpus (api.hip: rl_maxsim_batch_begin / _finish): out[b] = top[b][0 .. k) ++ {m_b} with neg2m[b] = -2 m_b;
// thr[b] = (k-th best of all shards' lists [world][B][k + 1]) - max_r m_r - m_rank, cnt[b] = 0, *flag on an unusable threshold
int launch_pack_approx(const float* top, const float* neg2m, int32_t B, int32_t k, float* out, hipStream_t s);
int launch_global_threshold(const float* lists, int32_t world, int32_t B, int32_t k, int32_t rank, float* thr, uint32_t* cnt, uint32_t* flag,
                            hipStream_t s);
// bits[0..2] = max |e|, max |e_lo|, max |e_lo| / |e| over the rows (float bit patterns, nudged up by 1e-6; start them at the
// values so far), e_lo = what the fp16 HI halves at `scale` drop
int launch_max_row_norm(const float* E, int64_t n_rows, int32_t dim, float scale, uint32_t* bits, hipStream_t s);
int launch_max_row_norm16(const uint16_t* E, int64_t n_rows, int32_t dim, uint32_t* bits, hipStream_t s);  // fp16-stored rows: bits[0] only
int launch_diag_blocks(const float* src, int64_t ld, int32_t k2, int64_t count, float* dst, hipStream_t s);
// Batched half-bytes search (experimental, api.hip: search_rows_fused_hi) -- see the kernels' comments in hi_filter.hip / select.hip
int launch_row_threshold(const float* topk, int32_t nb, int32_t k, const float* Q, int32_t dim, int mode, const float* q_unscale, float lo_ratio,
                         float lo_norm, float e_norm, float* thr, float* window, uint32_t* cnt, uint32_t* cnt2, uint32_t* flag, hipStream_t s,
                         float* thr_copy = nullptr, float sum_eps = 0x1p-12f);
int launch_row_dots(const float* E, int32_t dim, const float* Q, int32_t nb, const int32_t* rows, const uint32_t* cnt, int32_t cap, int mode,
                    const float* row_norm, const float* q_sumsq, float* out, hipStream_t s);
int launch_list_prefix(const float* in_scores, const int32_t* in_ids, int32_t nq, int32_t k_in, int32_t k, const uint32_t* counts,
                       const float* window, int32_t cap2, int32_t* out_ids, uint32_t* out_cnt, uint32_t* flag, hipStream_t s);
// the same contract by a radix SELECT of the list's k-th best score instead of a sort (round 5; out_ids in any order), and the step between
// the two rounds of the candidate pass -- thr[q] = max(thr[q], (k-th best of list q) - window[q]) -- as one launch of the same kernel
int launch_list_select(const float* in_scores, const int32_t* in_ids, int32_t nq, int32_t k_in, int32_t k, const uint32_t* counts,
                       const float* window, int32_t cap2, int32_t* out_ids, uint32_t* out_cnt, uint32_t* flag, hipStream_t s);
int launch_list_raise_threshold(const float* in_scores, const int32_t* in_ids, int32_t nq, int32_t k_in, int32_t k, const uint32_t* counts,
                                const float* window, float* thr, hipStream_t s);

// mask.hip: validity bitsets (metadata filter pushed down to the device, tombstones of deleted chunks)
// n_sets chunk bitsets -> row bitsets in one launch: row_bits [n_sets x (n_rows + 31) / 32] from chunk_bits + fid[j] * chunk_ld (fid
// nullptr: bitset j), each and-ed with and_rows when given
int launch_expand_chunk_bits(const uint32_t* chunk_bits, int64_t chunk_ld, const int32_t* fid, int32_t n_sets, const int32_t* row_to_chunk,
                             int64_t n_rows, const uint32_t* and_rows, uint32_t* row_bits, hipStream_t s);
int launch_mask_scores(float* scores, int32_t nb, int64_t n, int64_t ld, const QueryMask& bits, hipStream_t s);
int launch_fix_masked(const float* scores, int32_t* ids, int64_t count, hipStream_t s);
int launch_popcount(const uint32_t* bits, int64_t n, unsigned long long* out_dev, hipStream_t s);

// keyword.hip: BM25 over term-major postings (term_off [n_terms + 1], post_chunk ascending within a term, post_impact)
constexpr int32_t BM25_TILE_MAX = 8192;  // chunk scores per block, in LDS: 32 KiB, four blocks per CU
// post_impact[p] = idf[t] * ((tf * 2.2f) / (tf + nrm[c])) for posting p = (t, c, tf), float32 rounded at every step
int launch_bm25_impact(const int32_t* post_chunk, const int32_t* post_tf, const int32_t* post_term, const float* idf, const float* nrm,
                       int64_t n_postings, int32_t n_terms, int64_t n_chunks, float* post_impact, hipStream_t s);
int32_t bm25_tile(int64_t n_chunks, int32_t n_queries, int n_cu);  // the tile launch_bm25_score is given
// scores[b * ld + c] (c < n_chunks): the BM25 score of chunk c for query b (terms q_terms[q_off[b] .. q_off[b + 1]), ascending),
// -inf where the chunk has none of them or its filter bit is clear
int launch_bm25_score(const int64_t* term_off, const int32_t* post_chunk, const float* post_impact, int32_t n_terms, int64_t n_chunks,
                      const int64_t* q_off, const int32_t* q_terms, int32_t n_queries, const QueryMask& filter, int32_t tile, float* scores,
                      int64_t ld, hipStream_t s);
int launch_bm25_count(const float* sel, int32_t n_queries, int32_t k, int32_t* counts, hipStream_t s);  // finite entries per selected row

// keyword_build.hip: the postings of a device token store (rl_keyword_store_count drives these in this order)
int launch_kb_minmax(const int32_t* ids, int64_t n, int32_t* out /* [2]: min, max; folded into what they hold */, hipStream_t s);
int launch_kb_lengths(const int64_t* tok_off, const uint8_t* live, int64_t n_chunks, int64_t* length, hipStream_t s);
// data [n] (n >= 1) -> its exclusive scan, in place; scratch: kb_scan_scratch_items(n) int64; *total: where the sum of all lands (device)
size_t kb_scan_scratch_items(int64_t n);
int launch_kb_exclusive_scan(int64_t* data, int64_t n, int64_t* scratch, const int64_t** total, hipStream_t s);
// keys / vals [m]: (term_rank[tok_term] or tok_term itself, chunk) of the live chunks' tokens in token order; out_off: scanned lengths
int launch_kb_emit(const int64_t* tok_off, const int32_t* tok_term, const uint8_t* live, const int64_t* out_off, const int32_t* term_rank,
                   int32_t n_terms, int64_t n_chunks, int64_t n_tokens, int64_t m, uint32_t* keys, int32_t* vals, hipStream_t s);
int kb_sort_passes(int32_t n_terms);  // 8-bit digits that cover n_terms - 1, at least one
int64_t kb_sort_blocks(int64_t m);    // blocks of a sort pass; its table holds 256 * that many int64
// one stable pass on digit `pass` of the keys: histogram, scan of the (digit, block) table, scatter
int launch_kb_sort_pass(const uint32_t* keys_in, const int32_t* vals_in, int64_t m, int pass, int64_t* table, int64_t* scan_scratch,
                        uint32_t* keys_out, int32_t* vals_out, hipStream_t s);
int64_t kb_rle_blocks(int64_t m);
int launch_kb_rle_count(const uint32_t* keys, const int32_t* vals, int64_t m, int64_t* heads /* [kb_rle_blocks(m)] */, hipStream_t s);
// heads: scanned; post_term / post_chunk / post_tf [n_postings]; head_pos [n_postings]: scratch
int launch_kb_rle_write(const uint32_t* keys, const int32_t* vals, int64_t m, const int64_t* heads, int64_t n_postings, int32_t* post_term,
                        int32_t* post_chunk, int32_t* post_tf, int64_t* head_pos, hipStream_t s);
int launch_kb_term_off(const int32_t* post_term, int64_t n_postings, int32_t n_terms, int64_t* term_off /* [n_terms + 1] */,
                       int64_t* df /* [n_terms] or null */, hipStream_t s);

// keyword_analyze.hip: chunk bodies -> stable term ids (rl_keyword_analyze_begin / _finish drive these in this order; the scans
// between them are launch_kb_exclusive_scan's).  cp [n] UTF-32; table [n_table]: a code point's image, KA_IMAGE_MAX fields of 5 bits
// (symbol + 1; 0 ends it); symbols: 0 .. 25 = a .. z, 26 separator, 27 backslash, 28 newline.
constexpr int KA_IMAGE_MAX = 6;
int launch_ka_fold_count(const uint32_t* cp, int64_t n, const uint32_t* table, int64_t n_table, int64_t* count /* [n + 1] */, hipStream_t s);
int launch_ka_fold_write(const uint32_t* cp, int64_t n, const uint32_t* table, int64_t n_table, const int64_t* sym_off, int64_t m, uint8_t* sym,
                         hipStream_t s);
// ftext_off [n_texts + 1]: the texts' offsets in the folded stream; start [m] (zero on entry): 1 where a text begins
int launch_ka_text_starts(const int64_t* text_off, int64_t n_texts, int64_t n, const int64_t* sym_off, int64_t m, int64_t* ftext_off, uint8_t* start,
                          hipStream_t s);
// letter [m]: 1 = a letter no backslash consumes; head [m + 1]: 1 where a token begins (to be scanned: tok_idx)
int launch_ka_heads(const uint8_t* sym, const uint8_t* start, int64_t m, uint8_t* letter, int64_t* head, hipStream_t s);
// per token: tok_pos, tok_len (-1: a stopword, else its stem's length), the stem's letters at stem[tok_pos ..], tok_hash (hash_bits > 0:
// only that many low bits)
int launch_ka_stem(const uint8_t* sym, const uint8_t* letter, const uint8_t* start, const int64_t* tok_idx, int64_t m, int64_t n_tok,
                   const uint8_t* stop_bytes, const int32_t* stop_off, int32_t n_stop, int32_t stop_max_len, int hash_bits, int64_t* tok_pos,
                   uint8_t* stem, int64_t* tok_len, uint64_t* tok_hash, hipStream_t s);
int64_t ka_table_slots(int64_t n_tok);  // slots of the distinct table: a power of two >= 2 n_tok
// slots [cap]: set here; tok_slot [n_tok]; kept / first [n_tok + 1]: the flags to be scanned (kept_scan, rank)
int launch_ka_distinct(const uint8_t* stem, const int64_t* tok_pos, const int64_t* tok_len, const uint64_t* tok_hash, int64_t n_tok, uint64_t* slots,
                       int64_t cap, int64_t* tok_slot, int64_t* kept, int64_t* first, hipStream_t s);
int launch_ka_distinct_out(const int64_t* tok_len, const int64_t* tok_slot, const uint64_t* slots, int64_t cap, int64_t n_tok, const int64_t* kept_scan,
                           const int64_t* rank, int64_t n_distinct, int64_t* dist_tok, int64_t* dist_first, int64_t* dist_len /* [n_distinct + 1] */,
                           hipStream_t s);
int launch_ka_distinct_bytes(const uint8_t* stem, const int64_t* tok_pos, const int64_t* tok_len, const int64_t* dist_tok, const int64_t* dist_off,
                             int64_t n_distinct, int64_t n_bytes, uint8_t* bytes, hipStream_t s);
int launch_ka_emit(const int64_t* tok_len, const int64_t* tok_slot, const uint64_t* slots, int64_t cap, int64_t n_tok, const int64_t* kept_scan,
                   const int64_t* rank, const int32_t* ids, int64_t n_distinct, int64_t n_kept, int32_t* term_ids, hipStream_t s);
int launch_ka_offsets(const int64_t* ftext_off, int64_t n_texts, const int64_t* tok_idx, int64_t m, const int64_t* kept_scan, int64_t n_tok,
                      int64_t* offsets /* [n_texts + 1] */, hipStream_t s);

// wordpiece.hip: texts -> BERT WordPiece ids (rl_wordpiece_encode drives these in this order; the scans between them are
// launch_kb_exclusive_scan's), and the [CLS] q [SEP] d [SEP] rows of text pairs (rl_wordpiece_pairs).  cp [n] UTF-32; image [n_table]:
// a code point's normalised image, WP_IMAGE_MAX fields of 21 bits (code point + 1; 0 ends it); cls [n_table]: bits 0-1 the class of a
// SYMBOL of the normalised stream (0 word character, 1 white space, 2 punctuation), bit 2 the context flag of an INPUT code point.
constexpr int WP_IMAGE_MAX = 3;
constexpr int WP_COUNT_UNK = 0, WP_COUNT_FLAGGED = 1;  // counters [2]: words that became unk_id, texts with status 1 (zero on entry)
struct WpTable;                                        // wordpiece_table.h
// count [n + 1]: symbols per code point, + (context flag << 32); scanned, its last entry is (m, flagged code points) in the two fields
int launch_wp_expand_count(const uint32_t* cp, int64_t n, const uint64_t* image, const uint8_t* cls, int64_t n_table, int64_t* count, hipStream_t s);
int launch_wp_expand_write(const uint32_t* cp, int64_t n, const uint64_t* image, const uint8_t* cls, int64_t n_table, const int64_t* scan, int64_t m,
                           uint32_t* sym, uint8_t* kind, hipStream_t s);
// ftext_off [n_texts + 1]; start [m] (zero on entry): 1 where a text begins; status [n_texts]: 1 = holds a flagged code point
int launch_wp_texts(const int64_t* text_off, int64_t n_texts, int64_t n, const int64_t* scan, int64_t m, int64_t* ftext_off, uint8_t* start,
                    uint8_t* status, unsigned long long* counters, hipStream_t s);
int launch_wp_heads(const uint8_t* kind, const uint8_t* start, int64_t m, int64_t* head /* [m + 1], to be scanned: word_idx */, hipStream_t s);
// word_pos [n_words]; tmp [m]: the ids of word w from tmp[word_pos[w]] on; tok_count [n_words + 1]: to be scanned (tok_scan)
int launch_wp_match(const uint32_t* sym, const uint8_t* kind, const uint8_t* start, const int64_t* word_idx, int64_t m, int64_t n_words,
                    const WpTable& table, const int32_t* piece_ids, int32_t max_piece, int32_t unk_id, int32_t max_word_chars, int64_t* word_pos,
                    int32_t* tmp, int64_t* tok_count, unsigned long long* counters, hipStream_t s);
int launch_wp_emit(const int64_t* word_pos, const int64_t* tok_scan, int64_t n_words, const int32_t* tmp, int64_t m, int64_t n_tokens, int32_t* ids,
                   hipStream_t s);
int launch_wp_offsets(const int64_t* ftext_off, int64_t n_texts, const int64_t* word_idx, int64_t m, const int64_t* tok_scan, int64_t n_words,
                      int64_t* offsets /* [n_texts + 1] */, hipStream_t s);
// len [n_pairs + 1]: the row length of every pair, to be scanned (row_scan); then the int32 offsets and the three token arrays
int launch_wp_pair_lengths(const int64_t* tok_off, int64_t n_texts, const int32_t* query_text, const int32_t* doc_text, int64_t n_pairs, int32_t max_length,
                           int64_t* len, hipStream_t s);
int launch_wp_pair_offsets(const int64_t* row_scan, int64_t n_pairs, int32_t* seq_offsets, hipStream_t s);
int launch_wp_pair_write(const int32_t* ids, const int64_t* tok_off, int64_t n_texts, const int32_t* query_text, const int32_t* doc_text, int64_t n_pairs,
                         int32_t max_length, int32_t cls_id, int32_t sep_id, int32_t position_offset, const int64_t* row_scan, int64_t total,
                         int32_t* out_ids, int32_t* out_positions, int32_t* out_type_ids, hipStream_t s);

// sentencepiece.hip: texts -> SentencePiece Unigram ids (rl_sentencepiece_encode drives these in this order; the scans between them are
// launch_kb_exclusive_scan's), and the bos ids eos rows of texts (rl_sentencepiece_rows).  cp [n] UTF-32; SpImage / SpTable:
// sentencepiece_table.h.
constexpr int SP_COUNT_UNK = 0, SP_COUNT_FLAGGED = 1, SP_COUNT_LONGEST = 2, SP_COUNTERS = 3;  // counters [3], zero on entry: unknown ids written,
                                                                                             // texts with status 1, the longest text in symbols
struct SpImage;
struct SpTable;
// count [n + 1]: symbols per code point, + (trailing-set flag << 32); scanned, its last entry is (m0, flagged code points) in the two fields
int launch_sp_expand_count(const uint32_t* cp, int64_t n, const SpImage& im, int64_t* count, hipStream_t s);
int launch_sp_expand_write(const uint32_t* cp, int64_t n, const SpImage& im, const int64_t* scan, int64_t m0, uint32_t* raw, hipStream_t s);
// rtext_off [n_texts + 1]; start [m0] (zero on entry): 1 where a text begins; status [n_texts]: 1 = holds a flagged code point
int launch_sp_texts(const int64_t* text_off, int64_t n_texts, int64_t n, const int64_t* scan, int64_t m0, int64_t* rtext_off, uint8_t* start,
                    uint8_t* status, unsigned long long* counters, hipStream_t s);
// keep [m0 + 1]: normalised symbols per expanded symbol (0, 1, 2), to be scanned; then sym [m] and sym_off [n_texts + 1]
int launch_sp_keep_count(const uint32_t* raw, const uint8_t* start, int64_t m0, int64_t* keep, hipStream_t s);
int launch_sp_keep_write(const uint32_t* raw, const uint8_t* start, int64_t m0, const int64_t* keep_scan, int64_t m, const int64_t* rtext_off,
                         int64_t n_texts, uint32_t* sym, int64_t* sym_off, unsigned long long* counters, hipStream_t s);
// one text per wave; bp_start, bp_id, tmp [m]; tok_count [n_texts + 1]: to be scanned (tok_scan); tmp holds every text's ids REVERSED
int launch_sp_viterbi(const uint32_t* sym, const int64_t* sym_off, int64_t n_texts, int64_t m, const SpTable& table, int32_t longest, float unk_score,
                      int32_t* bp_start, int32_t* bp_id, int32_t* tmp, int64_t* tok_count, unsigned long long* counters, hipStream_t s);
// ids [n_tokens] = id + id_offset, the unknown piece unk_out; offsets [n_texts + 1] = tok_scan
int launch_sp_emit(const int32_t* tmp, const int64_t* sym_off, const int64_t* tok_scan, int64_t n_texts, int64_t m, int64_t n_tokens, int32_t id_offset,
                   int32_t unk_out, int32_t* ids, int64_t* offsets, hipStream_t s);
// len [n_texts + 1]: the row length of every text, to be scanned (row_scan); then the int32 offsets and the two token arrays
int launch_sp_row_lengths(const int64_t* tok_off, int64_t n_texts, int32_t max_len, int64_t* len, hipStream_t s);
int launch_sp_row_offsets(const int64_t* row_scan, int64_t n_texts, int32_t* seq_offsets, hipStream_t s);
int launch_sp_row_write(const int32_t* ids, const int64_t* tok_off, int64_t n_texts, int32_t max_len, int32_t bos_id, int32_t eos_id, int32_t position_offset,
                        const int64_t* row_scan, int64_t total, int32_t* out_ids, int32_t* out_positions, hipStream_t s);

// fuse.hip: weighted Reciprocal Rank Fusion of n_lists ranked lists per query (lists [n_lists x n_queries x len] int32, < 0 = padding)
// -> the top k by (float64 score desc, first occurrence asc), bit for bit the reference's reciprocal_rank_fusion
constexpr int32_t RRF_MAX_LISTS = 4;
constexpr int32_t RRF_MAX_ENTRIES = 4096;  // n_lists * len
constexpr int32_t RRF_MAX_K = 1 << 30;       // rrf_k + rank stays an exact int32 (and double)
constexpr double RRF_MAX_WEIGHT = 0x1p1000;  // |w| <= 2^1000: no sum of 4096 terms w / (rrf_k + i) overflows
int launch_rrf_fuse(const int32_t* lists, int32_t n_lists, int32_t n_queries, int32_t len, const double* weights /* host */, int32_t rrf_k,
                    int32_t k, double* out_scores, int32_t* out_ids, int32_t* out_counts, hipStream_t s);
// ... and the step after the one all-gather of a sharded hybrid batch (rl_shard_hybrid_fuse): merge the rows, group them by chunk, merge
// the keyword lists, then the same fusion; RL_ERR_UNSUPPORTED past world * num_hits or world * n_each > SHARD_FUSE_MAX_ENTRIES
constexpr int32_t SHARD_FUSE_MAX_ENTRIES = 4096;
int launch_shard_hybrid_fuse(const int32_t* gathered, int32_t world, int32_t n_queries, int32_t num_hits, int32_t n_each, int32_t n_lists,
                             const double* weights /* host */, int32_t rrf_k, int32_t k, double* out_scores, int32_t* out_ids,
                             int32_t* out_counts, hipStream_t s);

// rerank.hip: the order of reranked candidates (scores / candidates [n_queries x n_cand], candidate < 0 = padding) -> the first k by
// (score desc, NaN as -inf, -0.0 == +0.0; position asc), padding last: MaxSimRanker.rank's lexsort.  out_counts may be nullptr.
constexpr int32_t RERANK_MAX_ENTRIES = 4096;  // n_cand: one workgroup's LDS, as RRF_MAX_ENTRIES
int launch_rerank_order(const float* scores, const int32_t* candidates, int32_t n_queries, int32_t n_cand, int32_t k, float* out_scores,
                        int32_t* out_chunks, int32_t* out_pos, int32_t* out_counts, hipStream_t s);

// spans.hip: retrieve_chunk_spans on ordinals.  rank_of [n_chunks] (-1: no position), tab_key [n_live] = doc << 32 | pos ascending,
// tab_ord [n_live]: the span table's device arrays; chunks [n_queries x n_in] best first; offsets: host, n_off of them.
// E = n_in * (1 + n_off): out_chunks / out_span_len / out_span_scores [n_queries x E], out_n_spans / out_n_chunks [n_queries].
constexpr int32_t SPANS_MAX_ENTRIES = 4096;  // E: one workgroup's LDS, as RERANK_MAX_ENTRIES
constexpr int32_t SPANS_MAX_OFFSETS = 64;
int launch_chunk_spans(const int32_t* rank_of, const uint64_t* tab_key, const int32_t* tab_ord, int32_t n_chunks, int32_t n_live,
                       const int32_t* chunks, int32_t n_queries, int32_t n_in, const int32_t* offsets /* host */, int32_t n_off,
                       int32_t* out_chunks, int32_t* out_span_len, double* out_span_scores, int32_t* out_n_spans, int32_t* out_n_chunks,
                       hipStream_t s);

// metadata.hip: metadata filters as tag containment.  tag_off [n_chunks + 1] / tags: every chunk's ascending, duplicate-free tag ids;
// row_off [n_chunks + 1]: the index's chunk offsets; f_off [n_filters + 1] / f_tags: the filters' tags.  bits [n_filters x words],
// words = (n_chunks + 31) / 32, every word written; counts [2 x n_filters] (matching chunks, then their rows), zeroed here.
constexpr int32_t MF_BLOCK = 256;         // chunks per workgroup, one lane each
constexpr int32_t MF_STAGE_TAGS = 4096;   // chunk tags a workgroup stages in LDS (16 KiB); a chunk whose list ends past them reads HBM
constexpr int32_t MF_FILTER_TAGS = 1024;  // filter tags per LDS piece (4 KiB); a single filter with more reads HBM
constexpr int32_t MF_GROUP = 64;          // filters per blockIdx.y
int launch_metadata_filters(const int64_t* tag_off, const int32_t* tags, int64_t n_chunks, const int64_t* row_off, const int64_t* f_off,
                            const int32_t* f_tags, int32_t n_filters, uint32_t* bits, unsigned long long* counts, hipStream_t s);

// adapter_fit.hip: device half of update_query_adapter (best row per (query, chunk), row gather)
int launch_chunk_best_rows(const void* E, bool f16, int32_t dim, const float* Q, const int64_t* offsets,
                           int64_t n_chunks, const int32_t* cand, int32_t n_cand, int64_t n_items, int32_t* out_rows,
                           hipStream_t s);
int launch_rescore_l2(const void* E, bool f16, int32_t dim, const float* Q, const int32_t* rows, const float* ranked,
                      int32_t k, int64_t n_items, float* out, hipStream_t s);
int launch_permute_rows(const int32_t* rows_in, const int32_t* pos, int32_t k, int64_t n_items, int32_t* rows_out,
                        hipStream_t s);
// counts / cap (optional): rows[] is nq lists of cap slots of which list q holds min(counts[q], cap) -- the other slots are skipped (their
// output rows keep whatever they held)
int launch_gather_rows(const void* E, bool f16, int32_t dim, int64_t n_rows, const int32_t* rows, int64_t n, float* out,
                       hipStream_t s, const uint32_t* counts = nullptr, int32_t cap = 0);
int launch_compact_rows(const void* src, int64_t row_bytes, const int64_t* old_row, int64_t n, void* dst, hipStream_t s);

// query_targets.hip: the exact NNLS targets of update_query_adapter, batched over evals (Gram, solve, target: three launches)
size_t query_targets_scratch_bytes(int32_t B, int32_t k);
int launch_query_targets(const void* E, bool f16, int32_t dim, int64_t n_rows, const float* Q, int32_t B, const int32_t* rows,
                         const uint8_t* relevant, int32_t k, double gap, double* targets, double* weights, double* objective,
                         int32_t* status, int32_t* iterations, void* scratch, hipStream_t s);

// partition_sim.hip: semantic-chunking similarities (src/raglite/_split_chunks.py:54-72), batched over documents
size_t partition_sim_scratch_bytes(int64_t n, int64_t n_docs, int32_t dim);
int launch_partition_similarity(const float* X, int64_t n, int32_t dim, const int64_t* doc_off, int64_t n_docs,
                                const uint8_t* sel, float* out, void* scratch, hipStream_t s);

// partition_dp.hip: the chunk partition as a shortest path over split positions (`_split_chunks.py:87-113` without the MILP solver),
// batched over documents.  cost: the layout launch_partition_similarity writes; inv_norm (optional): 1 / |x_i| per row, a row where it
// is inf or NaN gives its document status 2.  cut [n] is zeroed here.
size_t partition_dp_scratch_bytes(int64_t n);
int launch_partition_headings(float* cost /* in: the similarities */, const uint8_t* heading, const int64_t* doc_off, int64_t n_docs,
                              int64_t n, hipStream_t s);
int launch_partition_dp(const float* cost, const int64_t* sizes, const float* inv_norm, const int64_t* doc_off, int64_t n, int64_t n_docs,
                        int64_t max_size, uint8_t* cut, double* objective, int32_t* status, void* scratch, hipStream_t s);

// chunklet_dp.hip: the chunklet partition of `_split_chunklets.py:136-178` (an exact shortest path over split positions in float64),
// batched over documents.  boundary / statements: one value per sentence; lengths: the sentences' characters.  cut [n] is zeroed here.
size_t chunklet_dp_scratch_bytes(int64_t n, int64_t n_docs);
int launch_chunklet_dp(const double* boundary, const double* statements, const int64_t* lengths, const int64_t* doc_off, int64_t n,
                       int64_t n_docs, int64_t max_size, uint8_t* cut, double* objective, int32_t* status, void* scratch, hipStream_t s);

// sentence_dp.hip: the sentence partition of `_split_sentences.py:183-218` (override, white-space propagation, the dynamic programme
// without and with a maximum length in float64), batched over documents.  codepoints / probas / known: one value per character.
// cut [n] is zeroed here.
size_t sentence_dp_scratch_bytes(int64_t n, int64_t n_docs);
int launch_sentence_dp(const uint32_t* codepoints, const void* probas, int probas_f64, const double* known, const int64_t* doc_off,
                       int64_t n, int64_t n_docs, int64_t min_len, int64_t max_len, uint8_t* cut, double* objective, int32_t* status,
                       void* scratch, hipStream_t s);

// markdown.hip: the block structure `MarkdownIt().parse` gives the splitters, batched over documents (the parser: markdown_blocks.h).
// first_open / heading_end / line_start have n + n_docs rows (a bound on the lines), line_off [n_docs + 1] says which are used;
// line_start is optional.  The two derived launchers take per-line arrays of n_lines rows (at least line_off[n_docs]).
size_t markdown_blocks_scratch_bytes(int64_t n, int64_t n_docs);
int launch_markdown_blocks(const uint32_t* codepoints, const int64_t* doc_off, int64_t n, int64_t n_docs, uint8_t* first_open,
                           int32_t* heading_end, int64_t* line_start, int64_t* line_off, int32_t* status, void* scratch, hipStream_t s);
size_t markdown_known_scratch_bytes(int64_t n_lines);
int launch_markdown_sentence_known(const int32_t* heading_end, const int64_t* line_start, const int64_t* line_off, const int32_t* status,
                                   const int64_t* doc_off, int64_t n, int64_t n_docs, int64_t n_lines, double* known, void* scratch,
                                   hipStream_t s);
size_t markdown_boundary_scratch_bytes(int64_t n_sent);
int launch_markdown_chunklet_boundary(const uint8_t* first_open, const int64_t* line_start, const int64_t* line_off, const int32_t* status,
                                      const int64_t* sent_off, const int64_t* sent_doc_off, int64_t n_sent, int64_t n_docs,
                                      int64_t n_lines, double* boundary, void* scratch, hipStream_t s);

// maxsim*.hip
// The launchers of this section take what they read and write as a few plain views (nothing owns memory; api.hip builds them from an index
// in one place: rows(idx), image(idx), chunks(idx), on(idx, s, run_if) ...), then what is their own.
// A corpus matrix: the stored rows, the row-major HI plane, or an image in the tiled layout of maxsim_gemm.hip.
struct RowsRef {
    const void* p = nullptr;
    bool f16 = false;  // fp16 elements: an fp16-stored corpus, the HI plane; of an image: ONE plane (the `half` layout) instead of hi | lo
    int64_t n_rows = 0;
    int32_t dim = 0;
    // An image or the HI plane: the power of two it was built at (the kernels undo it); that is 1 for an fp16-stored corpus.  fp32 rows:
    // the split scale the kernel applies (fp32 operands as fp16 hi + lo pairs, three fp16 MFMAs, fp32 accumulation), 0 = the exact fp32
    // MFMA chain.  Kernels that read fp16 rows directly take no scale.
    float scale = 0.f;
};
struct ChunkMap {  // the chunk structure over those rows
    const int32_t* row_to_chunk = nullptr;
    const int64_t* offsets = nullptr;  // [n_chunks + 1]
    int64_t n_chunks = 0;
    const uint32_t* ends_bits = nullptr;  // launch_chunk_ends' bitmap (the image passes)
};
struct QueryVecs {  // n_queries queries of nq vectors each, q_stride floats apart
    const float* Q = nullptr;
    int32_t nq = 0;
    int64_t q_stride = 0;
    int32_t n_queries = 1;
};
struct QueryImageRef {  // queries first .. first + n_q - 1, nq vectors each, of a launch_query_planes / launch_query_split buffer over n_queries
    const void* buf = nullptr;
    int32_t n_queries = 0, first = 0, n_q = 0, nq = 0;
};
struct RowMetric {  // the row side of a similarity (scan.hip conventions)
    int mode = SCAN_RAW_DOT;
    const float* row_norm = nullptr;   // [n_rows] (cosine)
    const float* row_sumsq = nullptr;  // [n_rows] (l2)
};
struct Scores {  // out[q * ld + row or chunk]
    float* p = nullptr;
    int64_t ld = 0;
};
struct Launch {
    int n_cu = 0;
    hipStream_t s = nullptr;
    const uint32_t* run_if = nullptr;  // the kernel returns at once unless *run_if != 0 (nullptr: always runs); a launcher whose kernel has no
                                       // such guard refuses one
};

int launch_row_to_chunk(const int64_t* chunk_offsets, int64_t n_chunks, int64_t n_rows, int32_t* row_to_chunk,
                        hipStream_t s);
// Fast path: dim in {128,256,384,512,768,1024}, q.nq <= 32 (wave-specialised MFMA streaming kernel; one query, q.n_queries == 1), fp32 or
// fp16 rows.  mode 0: chunk MaxSim scores out[n_chunks] (out.ld != 0: added to what `out` holds); mode 1: raw row dots out[q * ld + row].
// RL_ERR_UNSUPPORTED outside the fast path.
int launch_maxsim_stream(const RowsRef& D, const QueryVecs& q, const ChunkMap& c, int mode, Scores out, const Launch& on);
struct StreamSecondJob {  // launch_maxsim_stream_two: what grid row 1 runs
    const float* D = nullptr;
    int64_t n_rows = 0;
    float* out = nullptr;
    int64_t ld = 0;
    const uint32_t* run_if = nullptr;  // the row returns at once unless *run_if != 0 (nullptr: always runs)
};
int launch_maxsim_stream_two(const RowsRef& D, const QueryVecs& q, const ChunkMap& c, Scores out, const Launch& on, const StreamSecondJob& job2);
int launch_maxsim_stream_batch(const RowsRef& D, const QueryVecs& q, const ChunkMap& c, Scores out, const Launch& on);
size_t query_split_bytes(int32_t dim, int32_t n_queries);
int launch_query_split(const QueryVecs& q, int32_t dim, void* buf, bool f16_corpus, hipStream_t s);
int launch_maxsim_stream2(const RowsRef& D, const QueryImageRef& q, const ChunkMap& c, Scores out, const Launch& on);  // q.n_q == 2
// maxsim_gemm.hip: eight queries per corpus pass over the pre-split (fp16 hi | lo) corpus image, or (image.f16) a one-plane image
size_t planes_bytes(int64_t rows, int32_t dim, bool half = false);
// rows [first_row, E.n_rows) of E -> their place in the image `planes`
int launch_presplit_rows(const RowsRef& E, int64_t first_row, void* planes, hipStream_t s);
int launch_preformat_rows16(const RowsRef& E, int64_t first_row, void* planes, hipStream_t s);
int launch_presplit_hi_rows(const RowsRef& E, int64_t first_row, void* planes, hipStream_t s);
size_t chunk_ends_words(int64_t rows);
int launch_chunk_ends(const int32_t* row_to_chunk, int64_t n_rows, uint32_t* ends, hipStream_t s);
size_t query_planes_bytes(int32_t dim, int32_t n_queries);
int launch_query_planes(const QueryVecs& q, int32_t dim, void* buf, hipStream_t s, uint32_t* zero_words, int n_zero);
// hi_only: one product (q_hi . e_hi) per multiply; all_passes: q.n_q > 8 in one launch
int launch_maxsim_gemm(const RowsRef& image, const QueryImageRef& q, const ChunkMap& c, Scores out, const Launch& on, bool hi_only,
                       bool all_passes);
// maxsim_pp.hip: the approximate pass of the headline pipeline -- SIXTEEN queries per pass over a one-plane image, one product
constexpr int32_t PP_PASS_QUERIES = 16;
int launch_maxsim_pp(const RowsRef& image, const QueryImageRef& q, const ChunkMap& c, Scores out, const Launch& on,
                     int schedule, int xcd_passes, int loop);  // RL_OPT_PP_SCHEDULE, RL_OPT_PP_XCD_PASSES, RL_OPT_PP_LOOP
// the matrix pipe's sustained fp16 rate under the pass kernel's own MFMA stream (no loads, no epilogue): rl_time_kernel kind 9
constexpr int32_t MFMA_RATE_ITERS = 1000;  // x 32 MFMAs per wave: the MFMA count of a wave over one pass of 1 M rows x 1024
int launch_mfma_f16_rate(float* out, int n_cu, int32_t iters, hipStream_t s, double* flops);
// the candidate pass of the fused row top-k on that kernel's tile (MODE 2; see maxsim_pp.hip) -- declared after CandArgs below
size_t score_planes_scratch_floats(int32_t nb, int32_t dim);
int launch_score_planes(const RowsRef& image, const float* Q, int32_t nb, Scores out, const RowMetric& m, float* scratch, const Launch& on);
struct CandArgs { const float* tau; int32_t tau_stride; float* scores; int32_t* ids; uint32_t* cnt; uint32_t* overflow; int32_t cap; };
int launch_score_planes_queries(const float* Q, int32_t nb, int32_t dim, float* scratch, int mode, hipStream_t s, uint32_t* zero_word = nullptr);
size_t pp_rows_scratch_bytes(int64_t n_rows, int32_t nb, int n_cu, int32_t expected_per_query, int32_t* log_cap_out);
struct PpRowsPass {
    void* work = nullptr;  // pp_rows_scratch_bytes bytes, which also gives log_cap
    int32_t log_cap = 0;
    int64_t tile_begin = 0, tile_count = -1;  // row tiles (of 128 rows) [tile_begin, tile_begin + tile_count) only (tile_count < 0: to the end)
    bool norms_ready = false;                 // the block norm ranges in `work` are those of an earlier launch of the same search
    bool row_norm_test = false;               // cosine: test hits row by row against their own norms (wild norm spread)
};
int launch_pp_rows_pass(const RowsRef& image, int32_t nb, float* scratch, const RowMetric& m, const CandArgs* cand, const PpRowsPass& pass,
                        const Launch& on);
// the sample pass of the same search on that tile (MODE 1): S[q * ld + 256 j + r] = similarity of query q with row 256 stride j + r
int launch_pp_rows_sample(const RowsRef& image, int32_t nb, float* scratch, const RowMetric& m, Scores S, int32_t stride, const Launch& on);
// thr[q] = max(thr[q], kth[q * k + k - 1] - window[q]): the k-th best approximate similarity of ANY subset of the rows bounds the k-th best
// overall from below (select.hip; the second round of the fused top-k's candidate pass)
int launch_raise_threshold(float* thr, const float* kth, int32_t nq, int32_t k, const float* window, hipStream_t s);
struct ScorePass {
    int32_t tile_stride = 1;         // > 1: every tile_stride-th 256-row tile only, in compact columns (the sample pass)
    const CandArgs* cand = nullptr;  // the fused top-k's candidate lists instead of dense scores
    bool hi_only = false;            // one product per multiply over a one-plane image
};
int launch_score_planes_pass(const RowsRef& image, int32_t nb, float* scratch, Scores out, const RowMetric& m, const ScorePass& pass,
                             const Launch& on);
// [largest |element|, smallest non-zero row maximum, non-finite flag] of an fp32 corpus, as uint32 bit patterns (device, 3 words)
int launch_row_range(const float* E, int64_t n_rows, int32_t dim, uint32_t* range, hipStream_t s);
// score_gemm.hip: similarity of many queries at once (fp32 MFMA GEMM, 128 x 128 tiles, fused metric); dim % 32 == 0; fp32 rows.
// tile: 0 = the launcher's choice, 1 = 128 x 128, 2 = 128 x 256 (split arithmetic only) -- rl_score_gemm names one
int launch_score_gemm(const RowsRef& E, const float* Q, int32_t nb, Scores out, const RowMetric& m, float* q_sumsq_scratch, const Launch& on,
                      int tile = 0);
// |q|^2 per query as the GEMM epilogues read it (query_sumsq_kernel)
int launch_query_sumsq(const float* Q, int32_t nb, int32_t dim, float* out, hipStream_t s);
size_t score_gemm_scratch_floats(int32_t nb, int32_t dim, bool split);
// exact MaxSim of (query, candidate chunk) pairs, all queries in one launch: dim % 16 == 0 up to 1024, dim % 128 == 0 up to 4096 (wave-private query
// windows, maxsim_pairs_wide_kernel), nq <= 32, fp32 MFMA over fp32 or fp16 rows
struct PairsList {
    const int32_t* candidates = nullptr;
    int64_t n_items = 0;                       // entries scored per query
    int64_t item_stride = 0, first_item = 0;   // lists of `item_stride` (0: n_items) entries per query, of which first_item .. first_item + n_items - 1 are scored
    int packed = 1;  // 0: a chunk per tile; 1: rows packed into shared tiles; 2: ... by sixteen waves per workgroup  (dim % 128 == 0: same bits, about half the matrix work on short chunks)
};
int launch_maxsim_pairs(const RowsRef& D, const QueryVecs& q, const ChunkMap& c, const PairsList& list, float* out, hipStream_t s);
// 1024 < dim <= 4096 (dim % 128 == 0): launch_maxsim_pairs takes maxsim_pairs_wide_kernel; and the exact scores of EVERY chunk behind a run-if flag
int launch_maxsim_pairs_all_wide(const RowsRef& D, const QueryVecs& q, const ChunkMap& c, Scores out, const Launch& on);
// Any dim / nq: one wave per chunk (or per candidate), VALU dot products; fp32 rows.
int launch_maxsim_generic(const RowsRef& D, const QueryVecs& q, const ChunkMap& c, const int32_t* candidates, int64_t n_items, float* out,
                          hipStream_t s);
int launch_sanitize_candidates(const int32_t* in, int64_t n, int64_t n_chunks, const uint32_t* live_chunk_bits, int32_t* out,
                               hipStream_t s);
// Rerank fast path: dim == 128, nq <= 32 (MFMA, direct fragment loads), fp32 or fp16 rows.
int launch_maxsim_cand(const RowsRef& D, const QueryVecs& q, const ChunkMap& c, const int32_t* candidates, int32_t n_cand, float* out,
                       hipStream_t s);
// maxsim_ragged.hip: the rerank where query b owns the vectors Q[qv_off[b] .. qv_off[b + 1]) (d_qv_off: device [n_queries + 1]), any number
// of them, walked in slabs of 32: dim % 16 == 0 up to 1024, fp32 or fp16 rows; candidates / out [n_queries x n_cand].  RL_ERR_UNSUPPORTED elsewhere.
int launch_maxsim_ragged(const RowsRef& D, const float* Q, const int64_t* d_qv_off, int32_t n_queries, const ChunkMap& c,
                         const int32_t* candidates, int32_t n_cand, float* out, hipStream_t s);
// out[i] = slab[i] (add false) or out[i] + slab[i]: how the ragged rerank's backstop sums a query's slabs, in slab order
int launch_slab_accumulate(float* out, const float* slab, int64_t n, bool add, hipStream_t s);

}  // namespace rl
