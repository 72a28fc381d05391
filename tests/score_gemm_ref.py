"""The dense score GEMMs (`rl_score_gemm`: score_gemm.hip's three kernels, and the row-score mode of maxsim_gemm.hip over an image)
stated in float64, NumPy only: the fp16 split restated, derived error bounds, the metric epilogue, planted defects, and the cases of
tests/test_gpu_score_gemm.py as data.  Reference, `gamma`, `rho`, the comparator and the integer / same-sign makers are tests/scan_ref.py's.

The split, restated (`split_rows`, `split_queries`).  With a power of two s, a row element e becomes x = fp32(e s), hi = fp16_rtz(x),
lo = fp16_rtz(fp32(x - hi)): `cvt_pkrtz` (split8, presplit_rows_kernel).  A query is scaled by q_scale = 2^(14 - max(ex, -100)), ex the
exponent of its largest |q| (frexp: |q| = m 2^ex, m in [0.5, 1); a zero query takes ex = 0), and split with round-to-nearest:
hi = fp16_rn(x), lo = fp16_rn(fp32(x - hi)) (query_presplit_kernel, query_rows_planes_kernel).  The kernels sum, per 32-wide K slab,
eh.qh, then el.qh, then eh.ql into one fp32 accumulator and multiply by 1 / (s q_scale) -- a power of two, exact:
    d_split = (sum eh qh + el qh + eh ql) / (s q_scale)                       (`d_split`; lo.lo is dropped by design)
Products of two fp16 halves have 22 significant bits, so they are exact in fp32 and in float64; float64 sums them here with an error
2^-30 of the bounds below.

Bounds -- derived, never fitted to device output.
  accumulation   Against d_split the only error is the fp32 accumulation inside the matrix pipe.  Its internal order and rounding mode are
                 not stated by the code, so every accumulated product is charged one rounding of unit 2^-23 (truncation's unit; it covers
                 round-to-nearest) for every product that can follow it: T = 3 dim products for the split kernels, dim for the exact fp32
                 kernel (whose products are fp32 x fp32 inside the pipe):  |acc - d_split| <= T 2^-23 sum |e q|  (`acc_bound`; first order:
                 sum |halves' products| exceeds sum |e q| by less than 2^-9 of it).
  representation Against the float64 dot the split's own error comes on top (`rep_bound`).  With X = e s and Y = q q_scale, X = eh + el + re
                 and Y = qh + ql + rq, so  X Y - (eh qh + el qh + eh ql) = X rq + re Y - re rq + el ql.  Truncation to 11 bits: |X - eh| <=
                 EL = max(2^-10 |X|, 2^-24) (the second term: fp16's smallest spacing, reached below 2^-14), |el| <= EL, |re| <= RE =
                 max(2^-10 EL, 2^-24).  Rounding to nearest: |Y - qh| <= DQ = max(2^-11 |Y|, 2^-25), |ql| <= QL = DQ (1 + 2^-11) + 2^-25,
                 |rq| <= RQ = max(2^-11 DQ, 2^-25); a zero has no error.  Summed over k and divided by s q_scale.  To first order that is
                 (2^-22 + 2^-20 + 2^-21) |e q| = 1.75 2^-20 |e q| per product.
  one-hot rows   A single nonzero product per (row, query): the whole error is per product, bound 2^-19 |e q| (`probe_bound`).  The restated
                 split stays below 0.47 of it at dim 1024 (tests/test_score_gemm_ref_host.py); the three accumulations cost at most
                 2 x 2^-23 more (the first product is exact in the accumulator), 0.125 of the bound.
  epilogue       `score_bound`: what the metric adds to a bound bd on the dot, in scan_ref.bound's terms with u = 2^-24.  The caller gives
                 row_norm / row_sumsq, so they carry no error.  |q|^2 comes from query_sumsq_kernel: a chain of ceil(dim / 256) fmas per
                 thread, six butterfly additions, two more for the four waves: relative error gq = gamma(ceil(dim / 256) + 8)
                 (`q_sumsq_bound`), its root rho(gq).
                     dot     one addition:  + u |result|
                     cosine  c = d / (rn |q|): the root, the product and the division move c by |c| R + bd / (rn |q|) (1 + R),
                             R = (1 + u) / ((1 - rho(gq)) (1 - u)) - 1; then the two subtractions, + u |1 - c| and + u |c|
                     l2      t = (rs + |q|^2) - 2 d (2 d is exact, so a contracted fma changes nothing): dt = gq |q|^2 + u |rs + |q|^2| + 2 bd +
                             u |t|, each u term on the perturbed value; the root of a value within dt of t is within sqrt(t) - sqrt(max(t -
                             dt, 0)) of sqrt(t) (concavity; the clamp at 0 only helps), + u for its rounding; then + u |result|.

Why probes.  On same-sign dense data a dropped el.qh leaves the accumulation bound on every element at dims 32, 64, 96 (error / bound about
7 at dim 96): the dropped sum grows with dim, the worst-case bound with dim^2.  At dim 1024 the ratio is 0.83: the worst-case bound no
longer separates the defect.  One-hot rows put ONE product in every sum, so the bound is per product at every dim, and every k position
of every chunk, both halves and both operands, is some row's only product.
"""

import functools
from dataclasses import dataclass

import numpy as np

from oracle import oracle
from tests import scan_ref
from tests.scan_ref import U, gamma, rho

U23 = 2.0 ** -23
GK = 32          # K per slab
NSLOT = 4        # LDS ring of the 128 x 128 kernel (3 in the 128 x 256 one)
KERNELS = {1: "128x128", 2: "128x256", 3: "image"}
METRICS = ("raw", "cosine", "dot", "l2")


# ---- the split ---------------------------------------------------------------------------------------------------------------------
def _f16_rtz(x32):
    """fp16 round-toward-zero of float32 values, as float64."""
    with np.errstate(over="ignore"):
        h = x32.astype(np.float16)
    over = np.abs(h.astype(np.float64)) > np.abs(x32.astype(np.float64))
    h[over] = np.nextafter(h[over], np.float16(0))
    assert np.all(np.isfinite(h)), "the split scale lets a row element overflow fp16"
    return h.astype(np.float64)


def _f16_rn(x32):
    h = x32.astype(np.float16)
    assert np.all(np.isfinite(h))
    return h.astype(np.float64)


def pow2_scale(x):
    """The power of two that brings the largest |x| into [2^13, 2^14): 2^(14 - max(ex, -100)); 2^14 for an all-zero x."""
    mx = float(np.max(np.abs(x))) if np.size(x) else 0.0
    ex = int(np.frexp(np.float32(mx))[1]) if 0.0 < mx < np.inf else 0
    return 2.0 ** (14 - max(ex, -100))


def split_rows(E, s):
    """(eh, el, x) of rows E at scale s, float64, in the scaled domain."""
    x = np.asarray(E, dtype=np.float32) * np.float32(s)
    hi = _f16_rtz(x)
    lo = _f16_rtz((x - hi.astype(np.float32)).astype(np.float32))
    return hi, lo, x.astype(np.float64)


def query_scale(Q):
    """q_scale [B], float64."""
    return np.array([pow2_scale(q) for q in np.atleast_2d(np.asarray(Q, dtype=np.float32))])


def split_queries(Q):
    """(qh, ql, y, q_scale) of queries Q, float64, in the scaled domain."""
    Q = np.atleast_2d(np.asarray(Q, dtype=np.float32))
    qs = query_scale(Q)
    y = Q * qs.astype(np.float32)[:, None]
    hi = _f16_rn(y)
    lo = _f16_rn((y - hi.astype(np.float32)).astype(np.float32))
    return hi, lo, y.astype(np.float64), qs


def slab_sums(E, Q, s, terms=("hh", "lh", "hl")):
    """The scaled split sums per K slab, float64 [dim / 32, B, n]: what one slab adds to an accumulator.  `terms`: the products kept
    (hh = eh.qh, lh = el.qh, hl = eh.ql)."""
    eh, el, _ = split_rows(E, s)
    qh, ql, _, _ = split_queries(Q)
    out = []
    for k0 in range(0, eh.shape[1], GK):
        k = slice(k0, k0 + GK)
        t = np.zeros((qh.shape[0], eh.shape[0]))
        if "hh" in terms:
            t += qh[:, k] @ eh[:, k].T
        if "lh" in terms:
            t += qh[:, k] @ el[:, k].T
        if "hl" in terms:
            t += ql[:, k] @ eh[:, k].T
        out.append(t)
    return np.stack(out)


def unscale(E, Q, s):
    """1 / (s q_scale) per query, [B, 1]."""
    return 1.0 / (float(s) * query_scale(Q))[:, None]


def d_split(E, Q, s, terms=("hh", "lh", "hl")):
    """What the split kernels compute in exact arithmetic, float64 [B, n]."""
    eh, el, _ = split_rows(E, s)
    qh, ql, _, _ = split_queries(Q)
    t = np.zeros((qh.shape[0], eh.shape[0]))
    for name, q, e in (("hh", qh, eh), ("lh", qh, el), ("hl", ql, eh)):
        if name in terms:
            t += q @ e.T
    return t * unscale(E, Q, s)


def d_exact(E, Q):
    return np.asarray(Q, dtype=np.float64) @ np.asarray(E, dtype=np.float64).T


def abs_dot(E, Q):
    return np.abs(np.asarray(Q, dtype=np.float64)) @ np.abs(np.asarray(E, dtype=np.float64)).T


# ---- bounds ------------------------------------------------------------------------------------------------------------------------
def acc_bound(E, Q, split):
    """|accumulator - exact sum of the products it was given|, [B, n]: T 2^-23 sum |e q|, T = 3 dim (split) or dim (fp32)."""
    dim = np.shape(E)[1]
    return (3 if split else 1) * dim * U23 * abs_dot(E, Q)


def rep_bound(E, Q, s):
    """|float64 dot - d_split|, [B, n], from the split rules (module docstring)."""
    _, _, X = split_rows(E, s)
    _, _, Y, _ = split_queries(Q)
    aX, aY = np.abs(X), np.abs(Y)
    nzx, nzy = aX > 0, aY > 0
    EL = np.where(nzx, np.maximum(2.0 ** -10 * aX, 2.0 ** -24), 0.0)  # noqa: N806
    RE = np.where(nzx, np.maximum(2.0 ** -10 * EL, 2.0 ** -24), 0.0)  # noqa: N806
    DQ = np.where(nzy, np.maximum(2.0 ** -11 * aY, 2.0 ** -25), 0.0)  # noqa: N806
    QL = np.where(nzy, DQ * (1.0 + 2.0 ** -11) + 2.0 ** -25, 0.0)  # noqa: N806
    RQ = np.where(nzy, np.maximum(2.0 ** -11 * DQ, 2.0 ** -25), 0.0)  # noqa: N806
    return (RQ @ aX.T + aY @ RE.T + RQ @ RE.T + QL @ EL.T) * unscale(E, Q, s)


def dot_bound(E, Q, s):
    """|device dot - float64 dot|, [B, n]; s = 0: the exact fp32 kernel."""
    return acc_bound(E, Q, True) + rep_bound(E, Q, s) if s else acc_bound(E, Q, False)


def probe_bound(E, Q):
    """One-hot rows: 2^-19 |e q| of the row's one product, [B, n]."""
    return 2.0 ** -19 * abs_dot(E, Q)


def q_sumsq_terms(dim):
    return -(-int(dim) // 256) + 8


def q_sumsq_bound(Q):
    """(|q|^2 float64, bound on query_sumsq_kernel's output), [B] each."""
    Q = np.atleast_2d(np.asarray(Q, dtype=np.float64))
    ss = np.sum(Q * Q, axis=1)
    return ss, ss * gamma(q_sumsq_terms(Q.shape[1]))


def score_ref(d, metric, Q, row_norm=None, row_sumsq=None):
    """The metric epilogue in float64 on dots d [B, n] with the caller's row norms: what `transform_score` states."""
    if metric == "raw":
        return d
    if metric == "dot":
        return 1.0 + d
    qss = q_sumsq_bound(Q)[0][:, None]
    if metric == "cosine":
        with np.errstate(invalid="ignore", divide="ignore"):
            return 1.0 - (1.0 - d / (np.asarray(row_norm, dtype=np.float64)[None, :] * np.sqrt(qss)))
    if metric == "l2":
        return 1.0 - np.sqrt(np.maximum(np.asarray(row_sumsq, dtype=np.float64)[None, :] + qss - 2.0 * d, 0.0))
    raise ValueError(f"Unsupported metric: {metric}")


def score_bound(d, bd, metric, Q, row_norm=None, row_sumsq=None):
    """|device score - score_ref(d)| given |device dot - d| <= bd, [B, n]."""
    if metric == "raw":
        return bd
    if metric == "dot":
        return bd + U * (np.abs(1.0 + d) + bd)
    qss = q_sumsq_bound(Q)[0][:, None]
    gq = gamma(q_sumsq_terms(np.shape(Q)[1]))
    if metric == "cosine":
        den = np.asarray(row_norm, dtype=np.float64)[None, :] * np.sqrt(qss)
        R = (1.0 + U) / ((1.0 - rho(gq)) * (1.0 - U)) - 1.0  # noqa: N806
        c = d / den
        dc = np.abs(c) * R + bd / np.abs(den) * (1.0 + R)
        e1 = dc + U * (np.abs(1.0 - c) + dc)
        return e1 + U * (np.abs(c) + e1)
    if metric == "l2":
        a = np.asarray(row_sumsq, dtype=np.float64)[None, :] + qss
        da = gq * qss + U * (np.abs(a) + gq * qss)
        t = a - 2.0 * d
        dt = da + 2.0 * bd + U * (np.abs(t) + da + 2.0 * bd)
        tc = np.maximum(t, 0.0)
        root = np.sqrt(tc)
        ds = root - np.sqrt(np.maximum(tc - dt, 0.0))
        ds = ds + U * (root + ds)
        return ds + U * (np.abs(1.0 - root) + ds)
    raise ValueError(f"Unsupported metric: {metric}")


def epilogue_f32(d32, metric, q_sumsq32, row_norm=None, row_sumsq=None):
    """`transform_score` in float32, operation by operation, on the raw launch's dots d32 [B, n] and the |q|^2 the device read: the bits
    the metric launches must give."""
    f = np.float32
    d32 = np.asarray(d32, dtype=f)
    if metric == "raw":
        return d32
    if metric == "dot":
        return f(1.0) + d32
    qss = np.asarray(q_sumsq32, dtype=f)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        if metric == "cosine":
            den = np.asarray(row_norm, dtype=f)[None, :] * np.sqrt(qss)
            return f(1.0) - (f(1.0) - d32 / den)
        if metric == "l2":
            t = (np.asarray(row_sumsq, dtype=f)[None, :] + qss) - f(2.0) * d32
            return f(1.0) - np.sqrt(np.maximum(t, f(0.0)))
    raise ValueError(f"Unsupported metric: {metric}")


def exact_scores(E, Q, metric):
    """Integer data: `tests.util.sim_fp32_exact` for every query at once, float32 [B, n] (tests/test_score_gemm_ref_host.py holds the two
    together), with the norms it takes: row_norm = sqrt(fp32 |e|^2), row_sumsq = |e|^2."""
    f = np.float32
    E64, Q64 = np.asarray(E, dtype=np.float64), np.asarray(Q, dtype=np.float64)  # noqa: N806
    dot = (Q64 @ E64.T).astype(f)
    if metric == "raw":
        return dot
    if metric == "dot":
        return f(1.0) + dot
    ess, qss = np.sum(E64 * E64, axis=1).astype(f), np.sum(Q64 * Q64, axis=1).astype(f)
    if metric == "l2":
        d2 = (ess[None, :].astype(np.float64) + qss[:, None].astype(np.float64) - 2.0 * dot.astype(np.float64)).astype(f)
        return f(1.0) - np.sqrt(d2)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = dot / (np.sqrt(ess)[None, :] * np.sqrt(qss)[:, None])
    return f(1.0) - (f(1.0) - c)


def int_norms(E):
    """(row_norm, row_sumsq) float32 of integer rows, as `exact_scores` takes them."""
    E64 = np.asarray(E, dtype=np.float64)  # noqa: N806
    ss = np.sum(E64 * E64, axis=1).astype(np.float32)
    return np.sqrt(ss), ss


# ---- planted defects (tests/test_score_gemm_ref_host.py: each leaves its bound on the input chosen for it) ---------------------------
def defect_dropped_slab(E, Q, s, g):
    sl = slab_sums(E, Q, s)
    return (sl.sum(axis=0) - sl[g]) * unscale(E, Q, s)


def defect_stale_slab(E, Q, s, g, nslot=NSLOT):
    """The ring slot of slab g still holds slab g - nslot (both operands share a slot)."""
    sl = slab_sums(E, Q, s)
    return (sl.sum(axis=0) - sl[g] + sl[g - nslot]) * unscale(E, Q, s)


def defect_stale_rows(E, Q, s, g, nslot=NSLOT):
    """Only the row loader is behind: E's slab g - nslot against Q's slab g."""
    E2 = np.array(E, dtype=np.float32)  # noqa: N806
    E2[:, g * GK:(g + 1) * GK] = E2[:, (g - nslot) * GK:(g - nslot + 1) * GK]
    return d_split(E2, Q, s)


def defect_kept_accumulator(E, Q, s, tile_rows=128):
    """The accumulator is not reset: a row tile's sums start from the previous row tile's (same lane: row r - tile_rows)."""
    d = d_split(E, Q, s)
    out = d.copy()
    out[:, tile_rows:] += d[:, :-tile_rows] * 1.0
    touched = np.zeros(d.shape, dtype=bool)
    touched[:, tile_rows:] = True
    return out, touched


def defect_neighbour_scale(E, Q, s):
    """Query b is unscaled by query b + 1's q_scale (the last by its own)."""
    qs = query_scale(Q)
    nb = np.concatenate((qs[1:], qs[-1:]))
    return d_split(E, Q, s) * (qs / nb)[:, None], (qs != nb)[:, None] & np.ones((1, len(E)), dtype=bool)


def defect_swapped_chunk(E, Q, s, slab, kq):
    """query_presplit_kernel writes the lo chunk where the hi chunk of (slab, kq) belongs and the other way round."""
    eh, el, _ = split_rows(E, s)
    qh, ql, _, _ = split_queries(Q)
    ks = chunk_positions(slab, kq)
    qh2, ql2 = qh.copy(), ql.copy()
    qh2[:, ks], ql2[:, ks] = ql[:, ks], qh[:, ks]
    return (qh2 @ eh.T + qh2 @ el.T + ql2 @ eh.T) * unscale(E, Q, s), ks


def chunk_positions(slab, kq):
    """The 8 k positions lane (., kq) holds of a slab: 32 slab + {4 kq .. 4 kq + 3, 16 + 4 kq .. 16 + 4 kq + 3}."""
    return np.array([GK * slab + 4 * kq + u for u in range(4)] + [GK * slab + 16 + 4 * kq + u for u in range(4)])


# ---- input makers (deterministic; shared arrays are read-only) --------------------------------------------------------------------
def _ro(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def uniform(seed, n, dim):
    """U(-1, 1) float32 (the counter-based generator of the project: fewer rows are a prefix of more)."""
    return _ro(oracle.synth_matrix(int(seed), int(n), int(dim)))


@functools.lru_cache(maxsize=None)
def positive(seed, n, dim):
    """U(0.25, 1) float32: the same-sign data of the planted-defect tests."""
    return _ro(np.random.default_rng(int(seed)).uniform(0.25, 1.0, (int(n), int(dim))))


@functools.lru_cache(maxsize=None)
def spread_rows(seed, n, dim):
    """U(-1, 1) rows, every other one scaled by 2^-9: both ends of the 2^10 window the split accepts (`tiny_and_big` of test_hi_bound.py)."""
    x = np.array(uniform(seed, n, dim))
    x[1::2] *= np.float32(2.0 ** -9)
    return _ro(x)


@functools.lru_cache(maxsize=None)
def scaled_queries(seed, B, dim):  # noqa: N803
    """U(-1, 1) queries, query b scaled by 2^((7 b) % 41 - 20): 2^-20 .. 2^20 side by side within one tile, neighbours never alike."""
    x = np.array(uniform(seed, B, dim))
    x *= (2.0 ** ((7 * np.arange(B)) % 41 - 20)).astype(np.float32)[:, None]
    return _ro(x)


@functools.lru_cache(maxsize=None)
def one_hot_rows(seed, n, dim):
    """Row r: U(0.25, 1) at k = r % dim, zero elsewhere; n >= dim puts every k position in some row."""
    v = np.random.default_rng(int(seed)).uniform(0.25, 1.0, int(n)).astype(np.float32)
    x = np.zeros((int(n), int(dim)), dtype=np.float32)
    x[np.arange(n), np.arange(n) % dim] = v
    return _ro(x)


@functools.lru_cache(maxsize=None)
def grouped_queries(seed, dim):
    """96 queries in three groups of 32 for the image kernel's per-group lo flag: integers (every lo half zero: the flag is clear), floats,
    integers with ONE float query (index 77)."""
    q = np.array(scan_ref.int_data(seed, 96, dim))
    f = uniform(seed + 1, 96, dim)
    q[32:64] = f[32:64]
    q[77] = f[77]
    return _ro(q)


def make(kind, seed, n, dim):
    if kind == "uniform":
        return uniform(seed, n, dim)
    if kind == "same_sign_rows":
        return scan_ref.same_sign_rows(seed, n, dim)
    if kind == "same_sign_queries":
        return scan_ref.same_sign_queries(seed, n, dim)
    if kind == "spread":
        return spread_rows(seed, n, dim)
    if kind == "scaled":
        return scaled_queries(seed, n, dim)
    if kind == "int":
        return scan_ref.int_data(seed, n, dim)
    if kind == "one_hot":
        return one_hot_rows(seed, n, dim)
    if kind == "grouped":
        assert n == 96
        return grouped_queries(seed, dim)
    raise ValueError(kind)


def given_norms(E):  # noqa: N803
    """The row norms a float-data test hands in: the true |e| and |e|^2 times a factor of their own per row (1 + (r % 7) / 16, exact in
    fp32 arithmetic up to one rounding), so an epilogue that reads row r' for row r is off by 6 % and more -- and l2's radicand stays
    positive: rs >= |e|^2."""
    E64 = np.asarray(E, dtype=np.float64)  # noqa: N806
    ss = np.sum(E64 * E64, axis=1)
    w = 1.0 + (np.arange(len(E64)) % 7) / 16.0
    return (np.sqrt(ss) * w).astype(np.float32), (ss * w).astype(np.float32)



# ---- the cases of tests/test_gpu_score_gemm.py ---------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str   # says which branch it takes
    n: int
    B: int
    dim: int
    rows: str = "uniform"
    queries: str = "uniform"

    def data(self):
        """(E [n, dim], Q [B, dim]) float32, read-only."""
        return make(self.rows, 100 + self.dim, self.n, self.dim), make(self.queries, 200 + self.dim, self.B, self.dim)


DIMS = (32, 64, 96, 128, 160, 288, 1024)   # slabs 1, 2, 3 (the look-ahead), 4 (the ring), 5, 9 (odd), 32
ROWS = (1, 127, 128, 129, 130, 1003)       # one row; both sides of a row tile; n % 4 = 2; eight row tiles with a ragged last
BATCHES = (1, 97, 128, 129, 255, 256, 257, 300)
SMALL_N, SMALL_B, SMALL_DIM = 130, 97, 96


def elementwise_cases():
    """Each value of a size at the others' smallest interesting values, plus corners; every case runs kernels 1, 2, 3 in split arithmetic
    and kernel 1 in exact fp32, in the four metrics."""
    out = [Case(f"dim{d}_slabs{d // GK}", SMALL_N, SMALL_B, d) for d in DIMS]
    out += [Case(f"rows{n}", n, SMALL_B, SMALL_DIM) for n in ROWS if n != SMALL_N]
    out += [Case(f"batch{b}", SMALL_N, b, SMALL_DIM) for b in BATCHES if b != SMALL_B]
    out += [
        Case("same_sign_dim32_one_slab", SMALL_N, SMALL_B, 32, "same_sign_rows", "same_sign_queries"),
        Case("same_sign_dim64_two_query_tiles", SMALL_N, 257, 64, "same_sign_rows", "same_sign_queries"),
        Case("same_sign_dim160_rows1003", 1003, 129, 160, "same_sign_rows", "same_sign_queries"),
        Case("spread_rows_dim288", 129, 129, 288, "spread", "uniform"),
        Case("spread_rows_dim32", 257, 97, 32, "spread", "uniform"),
        Case("scaled_queries_dim96", SMALL_N, 300, 96, "uniform", "scaled"),
        Case("scaled_queries_dim1024", 127, 130, 1024, "uniform", "scaled"),
        Case("corner_rows1003_batch300_dim1024", 1003, 300, 1024),
        Case("corner_row1_batch1_dim32", 1, 1, 32),
    ]
    return tuple(out)


def probe_cases():
    """One-hot rows at dim 96 and 1024 (every k position is some row's product), two query tiles of either kernel."""
    return (Case("probe_dim96", 130, 257, 96, "one_hot", "uniform"), Case("probe_dim1024", 1027, 130, 1024, "one_hot", "uniform"))


WALK_SHAPES = ((700, 300), (1100, 130))  # (rows, queries): 8 x 3 and 16 x 2 tiles of 128 x 128 (row tiles are padded to a multiple of 8)
WALK_DIMS = (32, 96, 160, 1024)          # 1, 3, 5 slabs: tile boundaries fall on both register sets; 32: the ring wraps 8 times a tile
WALK_GRIDS = (1, 2, 3, 8)
IMAGE_GRIDS = (1, 3, 7)


def walk_cases():
    return tuple(Case(f"walk_rows{n}_batch{b}_dim{d}", n, b, d) for n, b in WALK_SHAPES for d in WALK_DIMS)


@functools.lru_cache(maxsize=None)
def references(case, s):
    """(float64 dot, sum |e q|, d_split or None, dot bound, accumulation bound) of a case at split scale s (0: exact fp32), computed once."""
    E, Q = case.data()  # noqa: N806
    d, S = d_exact(E, Q), abs_dot(E, Q)  # noqa: N806
    return d, S, (d_split(E, Q, s) if s else None), dot_bound(E, Q, s), acc_bound(E, Q, bool(s))
