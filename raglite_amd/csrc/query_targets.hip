// The target vectors of `update_query_adapter` on the device (src/raglite/_query_adapter.py:20-38).  Per eval the
// reference solves  t* = argmin |q + D^T mu|^2  over mu >= 0,  D = P_i - c N_j  (c = 1 + gap, P / N the positive / negative example
// rows): the projection of the origin onto q + cone(D).  Everything the solver needs comes from the Gram matrix of the eval's
// k <= 64 example rows, K = E E^T, and e = E q, in float64; pair (i, j) -> i * n + j:
//   G[(i,j),(i',j')] = K[i,i'] - c (K[i,j'] + K[j,i']) + c^2 K[j,j']        h[(i,j)] = e[i] - c e[j]
//   gradient g_ij = u_i - c u_j,  u = e + K w,  w the marginals (w_i = sum_j mu_ij, w_j = -c sum_i mu_ij)
// raglite_amd/_query_adapter.py: optimize_query_target_active_set is the host statement of the same Lawson-Hanson iteration.
// Every phase is its own launch, no atomics, nothing waits on another workgroup, every sum has a fixed order:
//   qt_gram_kernel    one workgroup per eval (grid-stride): the rows are read in place from the index by ordinal (-1 = padding), staged
//                     through LDS in 32-column tiles as float64; K, e and q.q are fma chains in ascending column order.  Flags the
//                     eval (status 2) for an ordinal outside the index or a non-finite row / query.
//   qt_solve_kernel   one wave64 per eval (a 64-thread workgroup, grid-stride): K, the packed Cholesky factor, mu, u and the passive
//                     list live in LDS; lanes over pairs for the gradient and its arg-max, lanes over rows for the factor and the
//                     substitutions.  Writes weights (the non-negative marginals by example slot), status, iterations.
//   qt_target_kernel  t = q + sum_i a_i P_i - c sum_j b_j N_j and |t|^2 in float64; status 3 when |t| <= 1e-9 |q|.
// Scratch: K [B x k x k], e [B x k], q.q [B] float64.
#include "common.h"

#include <cmath>

namespace rl {
namespace {

constexpr int QT_MAX = RL_QT_MAX_EXAMPLES;  // 64: one lane per example, one lane per passive slot
constexpr int QT_TILE = 32;                 // columns per Gram tile
constexpr int QT_LD = QT_MAX + 2;           // tile row: 64 examples + the query, padded to keep 16-byte alignment
constexpr int QT_GRID_CAP = 1024;           // workgroups per launch; every kernel strides over the evals beyond it

template <typename ET>
__device__ __forceinline__ double qt_elt(const ET* p);
template <>
__device__ __forceinline__ double qt_elt<float>(const float* p) { return (double)*p; }
template <>
__device__ __forceinline__ double qt_elt<uint16_t>(const uint16_t* p) {
    _Float16 h;
    __builtin_memcpy(&h, p, 2);
    return (double)h;
}

// ---- Gram --------------------------------------------------------------------------------------------------------------------------
// Thread t owns the 4 x 4 block of K at rows 4 (t / 16), columns 4 (t % 16); threads 0 .. 63 also own e[t], thread 64 owns q.q.
template <typename ET>
__global__ __launch_bounds__(256) void qt_gram_kernel(const ET* __restrict__ E, int dim, int64_t n_rows, const float* __restrict__ Q,
                                                       const int32_t* __restrict__ rows, int k, int B, double* __restrict__ Kout,
                                                       double* __restrict__ eout, double* __restrict__ qq, int32_t* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) double tile[QT_TILE * QT_LD];  // tile[c][slot]; slot 64 = the query
    __shared__ int64_t row_of[QT_MAX];                                     // -1: padding or outside the index (reads as zeros)
    __shared__ int bad;
    const int t = threadIdx.x, ti = t >> 4, tj = t & 15;
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        __syncthreads();  // the previous eval's tile and flags are done with
        if (t == 0) bad = 0;
        __syncthreads();
        if (t < QT_MAX) {
            int64_t r = -1;
            if (t < k) {
                r = rows[(int64_t)b * k + t];
                if (r < -1 || r >= n_rows) { bad = 1; r = -1; }
            }
            row_of[t] = r;
        }
        double acc[4][4] = {};
        double ev = 0.0;
        const bool live = 4 * ti < k && 4 * tj < k;
        const float* q = Q + (int64_t)b * dim;
        for (int c0 = 0; c0 < dim; c0 += QT_TILE) {
            __syncthreads();  // row_of is written; the previous tile is consumed
            const int c = t & (QT_TILE - 1), col = c0 + c;
            for (int s = t >> 5; s <= QT_MAX; s += 8) {  // 8 rows per pass, 32 consecutive columns of each
                double v = 0.0;
                if (col < dim) {
                    if (s == QT_MAX) v = (double)q[col];
                    else if (row_of[s] >= 0) v = qt_elt<ET>(E + row_of[s] * (int64_t)dim + col);
                }
                tile[c * QT_LD + s] = v;
            }
            __syncthreads();
            if (live) {
#pragma unroll 4
                for (int cc = 0; cc < QT_TILE; ++cc) {
                    const double* col_p = tile + cc * QT_LD;
                    double a[4], bb[4];
#pragma unroll
                    for (int x = 0; x < 4; ++x) { a[x] = col_p[4 * ti + x]; bb[x] = col_p[4 * tj + x]; }
#pragma unroll
                    for (int x = 0; x < 4; ++x)
#pragma unroll
                        for (int y = 0; y < 4; ++y) acc[x][y] = fma(a[x], bb[y], acc[x][y]);
                }
            }
            if (t <= QT_MAX) {  // e (threads 0 .. 63) and q.q (thread 64): slot t against the query
                for (int cc = 0; cc < QT_TILE; ++cc) ev = fma(tile[cc * QT_LD + t], tile[cc * QT_LD + QT_MAX], ev);
            }
        }
        if (live) {
            for (int x = 0; x < 4; ++x)
                for (int y = 0; y < 4; ++y) {
                    const int i = 4 * ti + x, j = 4 * tj + y;
                    if (i < k && j < k) {
                        Kout[((int64_t)b * k + i) * k + j] = acc[x][y];
                        if (i == j && !isfinite(acc[x][y])) bad = 1;
                    }
                }
        }
        if (t < k) eout[(int64_t)b * k + t] = ev;
        if (t == QT_MAX) {
            qq[b] = ev;
            if (!isfinite(ev)) bad = 1;
        }
        __syncthreads();
        if (t == 0) status[b] = bad ? 2 : 0;
    }
}

// ---- solve -------------------------------------------------------------------------------------------------------------------------
// LDS of one wave: K 32 KiB + packed factor 16.25 KiB + pair states 1 KiB + vectors and lists 3.5 KiB = 52.75 KiB, so three waves
// share a CU's 160 KiB.
struct QtLds {
    double K[QT_MAX * QT_MAX];            // by example slot; column reads (K is symmetric) keep the lanes on consecutive banks
    double L[QT_MAX * (QT_MAX + 1) / 2];  // row r of the Cholesky factor at r (r + 1) / 2
    double dinv[QT_MAX];                  // 1 / L[r][r]
    double e[QT_MAX], u[QT_MAX], mu[QT_MAX];
    int16_t lx[QT_MAX];                   // passive list: pair index ...
    uint8_t lp[QT_MAX], ln[QT_MAX];       // ... and the example slots of its positive and negative row
    uint8_t pslot[QT_MAX], nslot[QT_MAX]; // example slot of the i-th positive / j-th negative
    uint8_t state[QT_MAX * QT_MAX / 4];   // per pair (p n <= 1024): 0 free, 1 passive, 2 banned
};

__device__ __forceinline__ double qt_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double qt_wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}

// G between two pairs given by their example slots (a positive, a negative each).
__device__ __forceinline__ double qt_g(const double* K, int pa, int na, int pb, int nb, double c) {
    return K[pa * QT_MAX + pb] - c * (K[pa * QT_MAX + nb] + K[na * QT_MAX + pb]) + c * c * K[na * QT_MAX + nb];
}

// Row `s` of the factor for the pair (cp, cn) behind passive slots 0 .. s - 1: lane r < s ends with L[s][r]; returns the squared pivot.
__device__ __forceinline__ double qt_factor_row(const QtLds& m, int s, int cp, int cn, double gd, double c, int lane, double* y_out) {
    double a = 0.0;
    if (lane < s) a = qt_g(m.K, m.lp[lane], m.ln[lane], cp, cn, c);
    for (int col = 0; col < s; ++col) {
        const double y = __shfl(a, col, 64) * m.dinv[col];
        if (lane == col) a = y;
        else if (lane > col && lane < s) a = fma(-m.L[lane * (lane + 1) / 2 + col], y, a);
    }
    *y_out = a;
    return gd - wave_sum(lane < s ? a * a : 0.0);
}

// z = -(L L^T)^-1 h over the s passive slots; lane r < s returns z_r.
__device__ __forceinline__ double qt_passive_solve(const QtLds& m, int s, double c, int lane) {
    double b = 0.0;
    if (lane < s) b = -(m.e[m.lp[lane]] - c * m.e[m.ln[lane]]);
    for (int col = 0; col < s; ++col) {
        const double y = __shfl(b, col, 64) * m.dinv[col];
        if (lane == col) b = y;
        else if (lane > col && lane < s) b = fma(-m.L[lane * (lane + 1) / 2 + col], y, b);
    }
    for (int col = s - 1; col >= 0; --col) {
        const double z = __shfl(b, col, 64) * m.dinv[col];
        if (lane == col) b = z;
        else if (lane < col) b = fma(-m.L[col * (col + 1) / 2 + lane], z, b);
    }
    return b;
}

__global__ __launch_bounds__(64) void qt_solve_kernel(const double* __restrict__ Kin, const double* __restrict__ ein,
                                                       const int32_t* __restrict__ rows, const uint8_t* __restrict__ relevant, int k,
                                                       int B, double c, double* __restrict__ weights, int32_t* __restrict__ status,
                                                       int32_t* __restrict__ iterations) {
    __shared__ QtLds m;
    const int lane = threadIdx.x;
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        __syncthreads();
        // ---- the eval's examples: positives and negatives by slot, in slot order ----
        const bool present = lane < k && rows[(int64_t)b * k + lane] != -1;
        const bool pos = present && relevant[(int64_t)b * k + lane] != 0;
        const unsigned long long pmask = __ballot(pos), nmask = __ballot(present && !pos);
        const int p = __popcll(pmask), n = __popcll(nmask), kk = p + n, np = p * n;
        const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
        if (pos) m.pslot[__popcll(pmask & below)] = (uint8_t)lane;
        if (present && !pos) m.nslot[__popcll(nmask & below)] = (uint8_t)lane;
        const int flagged = status[b];
        if (p == 0 || n == 0 || flagged != 0) {
            if (lane < k) weights[(int64_t)b * k + lane] = 0.0;
            if (lane == 0) {
                status[b] = (p == 0 || n == 0) ? 1 : 2;
                iterations[b] = 0;
            }
            continue;
        }
        double kmax = 0.0;
        for (int x = lane; x < k * k; x += 64) {
            const double v = Kin[(int64_t)b * k * k + x];
            m.K[(x / k) * QT_MAX + x % k] = v;
            kmax = fmax(kmax, fabs(v));
        }
        if (lane < k) m.e[lane] = ein[(int64_t)b * k + lane];
        for (int x = lane; x < np; x += 64) m.state[x] = 0;
        __syncthreads();
        double hmax = 0.0;
        for (int x = lane; x < np; x += 64) hmax = fmax(hmax, fabs(m.e[m.pslot[x / n]] - c * m.e[m.nslot[x % n]]));
        const double tol = 64.0 * 2.220446049250313e-16 * qt_wave_max(fmax(kmax, hmax));

        int s = 0, iters = 0, st = 0;  // passive slots; entering steps; status
        bool banned = false;
        double mu = 0.0;  // lane r < s: mu of passive slot r (mirrored in m.mu for the marginals)
        for (;;) {
            // ---- u = e + K w, w the signed marginals ----
            if (lane < k) {
                double w = 0.0;
                for (int r = 0; r < s; ++r)
                    if (m.lp[r] == lane || m.ln[r] == lane) w += m.mu[r];
                if (!pos) w = -c * w;
                m.u[lane] = w;  // (w, for the moment)
            }
            __syncthreads();
            double u = 0.0;
            if (lane < k) {
                u = m.e[lane];
                for (int j = 0; j < k; ++j) u = fma(m.K[j * QT_MAX + lane], m.u[j], u);
            }
            __syncthreads();
            if (lane < k) m.u[lane] = u;
            __syncthreads();
            // ---- entering step: the free pair with the largest -g, the smallest index on a tie ----
            double best = -INFINITY;
            int bx = 0x7fffffff;
            for (int x = lane; x < np; x += 64) {
                const double v = -(m.u[m.pslot[x / n]] - c * m.u[m.nslot[x % n]]);
                if (m.state[x] == 0 && v > best) { best = v; bx = x; }
            }
            const double top = qt_wave_max(best);
            if (!(top > tol)) break;
            if (iters >= 4 * kk) { st = 4; break; }
            ++iters;
            int cand = best == top ? bx : 0x7fffffff;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
            const int cp = m.pslot[cand / n], cn = m.nslot[cand % n];
            const double gd = qt_g(m.K, cp, cn, cp, cn, c);
            // ---- the candidate's factor row, appended last; rejected (banned until the next accepted one) on a small pivot ----
            double y = 0.0;
            const double d = s < kk ? qt_factor_row(m, s, cp, cn, gd, c, lane, &y) : 0.0;
            if (!(d > 1e-12 * gd)) {
                if (lane == 0) m.state[cand] = 2;
                banned = true;
                __syncthreads();
                continue;
            }
            if (lane < s) m.L[s * (s + 1) / 2 + lane] = y;
            if (lane == s) {
                const double root = sqrt(d);
                m.L[s * (s + 1) / 2 + s] = root;
                m.dinv[s] = 1.0 / root;
                m.lx[s] = (int16_t)cand;
                m.lp[s] = (uint8_t)cp;
                m.ln[s] = (uint8_t)cn;
            }
            __syncthreads();
            double z = qt_passive_solve(m, s + 1, c, lane);
            if (!(__shfl(z, s, 64) > 0.0)) {  // ... or on its own z <= 0
                if (lane == 0) m.state[cand] = 2;
                banned = true;
                __syncthreads();
                continue;
            }
            if (banned) {
                for (int x = lane; x < np; x += 64)
                    if (m.state[x] == 2) m.state[x] = 0;
                banned = false;
            }
            if (lane == s) { m.state[cand] = 1; mu = 0.0; }
            ++s;
            __syncthreads();
            // ---- inner loop: step towards z as far as mu stays feasible, drop what reached 0, re-solve ----
            while (__ballot(lane < s && z <= 0.0)) {
                const bool neg = lane < s && z <= 0.0;
                const double ratio = neg ? mu / (mu - z) : INFINITY;
                const double step = qt_wave_min(ratio);
                if (lane < s) mu = mu + step * (z - mu);
                const bool drop = lane < s && ((neg && ratio == step) || mu <= 0.0);
                const unsigned long long dmask = __ballot(drop), kmask = __ballot(lane < s && !drop);
                if (!dmask) { st = 4; break; }  // (a step that frees nothing cannot end: unreachable with finite inputs)
                const int first = __ffsll((long long)dmask) - 1, slot = __popcll(kmask & below);
                const int x = m.lx[lane], xp = m.lp[lane], xn = m.ln[lane];  // (lanes >= s read stale slots and write nothing)
                __syncthreads();
                if (drop) m.state[x] = 0;
                if (lane < s && !drop) {
                    m.lx[slot] = (int16_t)x;
                    m.lp[slot] = (uint8_t)xp;
                    m.ln[slot] = (uint8_t)xn;
                    m.mu[slot] = mu;
                }
                s = __popcll(kmask);
                __syncthreads();
                mu = lane < s ? m.mu[lane] : 0.0;
                // rows before the first dropped slot keep their factor; a subset of a passive list keeps its pivots (they only grow)
                for (int r = first; r < s; ++r) {
                    const int rp = m.lp[r], rn = m.ln[r];
                    const double rg = qt_g(m.K, rp, rn, rp, rn, c);
                    double yr = 0.0;
                    const double dr = fmax(qt_factor_row(m, r, rp, rn, rg, c, lane, &yr), 1e-12 * rg);
                    if (lane < r) m.L[r * (r + 1) / 2 + lane] = yr;
                    if (lane == r) {
                        const double root = sqrt(dr);
                        m.L[r * (r + 1) / 2 + r] = root;
                        m.dinv[r] = 1.0 / root;
                    }
                    __syncthreads();
                }
                z = qt_passive_solve(m, s, c, lane);
            }
            if (st) break;
            if (lane < s) { mu = z; m.mu[lane] = z; }
            __syncthreads();
        }
        // ---- the non-negative marginals by example slot ----
        if (lane < k) {
            double w = 0.0;
            for (int r = 0; r < s; ++r)
                if (m.lp[r] == lane || m.ln[r] == lane) w += m.mu[r];
            weights[(int64_t)b * k + lane] = w;
        }
        if (lane == 0) {
            status[b] = st;
            iterations[b] = iters;
        }
    }
}

// ---- target ------------------------------------------------------------------------------------------------------------------------
template <typename ET>
__global__ __launch_bounds__(256) void qt_target_kernel(const ET* __restrict__ E, int dim, const float* __restrict__ Q,
                                                         const int32_t* __restrict__ rows, const uint8_t* __restrict__ relevant, int k,
                                                         int B, double c, const double* __restrict__ weights, const double* __restrict__ qq,
                                                         double* __restrict__ T, double* __restrict__ objective,
                                                         int32_t* __restrict__ status) {
    __shared__ double coef[QT_MAX];
    __shared__ int64_t row_of[QT_MAX];
    __shared__ double part[4];
    const int t = threadIdx.x;
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        const int st = status[b];
        double* out = T + (int64_t)b * dim;
        if (st == 1 || st == 2) {  // no problem was posed, or its rows may not be read: nothing but NaN
            for (int d = t; d < dim; d += 256) out[d] = NAN;
            if (t == 0) objective[b] = NAN;
            continue;
        }
        __syncthreads();
        if (t < k) {
            const double w = weights[(int64_t)b * k + t];
            coef[t] = relevant[(int64_t)b * k + t] ? w : -c * w;
            row_of[t] = rows[(int64_t)b * k + t];  // in range: the Gram kernel flagged the eval otherwise
        }
        __syncthreads();
        const float* q = Q + (int64_t)b * dim;
        double sum = 0.0;
        for (int d = t; d < dim; d += 256) {
            double acc = (double)q[d];
            for (int s = 0; s < k; ++s)
                if (coef[s] != 0.0) acc = fma(coef[s], qt_elt<ET>(E + row_of[s] * (int64_t)dim + d), acc);
            out[d] = acc;
            sum = fma(acc, acc, sum);
        }
        sum = wave_sum(sum);
        if ((t & 63) == 0) part[t >> 6] = sum;
        __syncthreads();
        if (t == 0) {
            const double tt = ((part[0] + part[1]) + part[2]) + part[3];
            objective[b] = tt;
            if (tt <= 1e-18 * qq[b]) status[b] = 3;  // |t| <= 1e-9 |q|: the constraints cannot be met
        }
    }
}
}  // namespace

// scratch: double K[B * k * k], e[B * k], qq[B]
size_t query_targets_scratch_bytes(int32_t B, int32_t k) { return ((size_t)B * k * k + (size_t)B * k + (size_t)B) * sizeof(double); }

int launch_query_targets(const void* E, bool f16, int32_t dim, int64_t n_rows, const float* Q, int32_t B, const int32_t* rows,
                         const uint8_t* relevant, int32_t k, double gap, double* targets, double* weights, double* objective,
                         int32_t* status, int32_t* iterations, void* scratch, hipStream_t s) {
    if (B <= 0) return RL_OK;
    double* K = static_cast<double*>(scratch);
    double* e = K + (size_t)B * k * k;
    double* qq = e + (size_t)B * k;
    const double c = 1.0 + gap;
    const int blocks = std::min<int>(B, QT_GRID_CAP);
    if (f16) {
        hipLaunchKernelGGL((qt_gram_kernel<uint16_t>), dim3(blocks), dim3(256), 0, s, static_cast<const uint16_t*>(E), (int)dim, n_rows,
                           Q, rows, (int)k, (int)B, K, e, qq, status);
    } else {
        hipLaunchKernelGGL((qt_gram_kernel<float>), dim3(blocks), dim3(256), 0, s, static_cast<const float*>(E), (int)dim, n_rows, Q,
                           rows, (int)k, (int)B, K, e, qq, status);
    }
    hipLaunchKernelGGL(qt_solve_kernel, dim3(blocks), dim3(64), 0, s, K, e, rows, relevant, (int)k, (int)B, c, weights, status,
                       iterations);
    if (f16) {
        hipLaunchKernelGGL((qt_target_kernel<uint16_t>), dim3(blocks), dim3(256), 0, s, static_cast<const uint16_t*>(E), (int)dim, Q,
                           rows, relevant, (int)k, (int)B, c, weights, qq, targets, objective, status);
    } else {
        hipLaunchKernelGGL((qt_target_kernel<float>), dim3(blocks), dim3(256), 0, s, static_cast<const float*>(E), (int)dim, Q, rows,
                           relevant, (int)k, (int)B, c, weights, qq, targets, objective, status);
    }
    RL_HIP(hipGetLastError());
    return RL_OK;
}

}  // namespace rl
