"""The row scan of scan.hip / scan16.hip stated in float64, NumPy only: reference, derived error bound, comparator, input makers.

Reference (`finish_score` as written): with dot = sum e_i q_i, |e| = sqrt(sum e_i^2), d2 = sum (e_i - q_i)^2,
    raw     dot                          (SCAN_RAW_DOT: the query-adapter matvec)
    dot     1 + dot
    l2      1 - sqrt(d2)
    cosine  1 - (1 - dot / (|e| |q|))    (a zero row or a zero query: 0 / 0 = NaN)
fp16-stored rows widen to float64 exactly, so the same statements cover them.

Bound.  Derived from the kernels' operations, never fitted to device output; u = 2^-24 is the unit roundoff of fp32 round-to-nearest.
A lane sums its T = NV * VEC elements (NV * 8 for fp16 storage) in one fma chain: one rounding per term.  The butterfly `wave_sum` adds
six more roundings on the way to lane 0.  With gamma(m) = m u / (1 - m u) (Higham, Accuracy and Stability, lemma 3.1 / eq. 3.4, any
order of summation) the reduced accumulator satisfies
    |acc - dot| <= gamma(T + 6) * sum |e_i q_i|
    |acc - d2|  <= gamma(T + 8) * d2            (l2: each difference is rounded, then squared inside the fma: two more factors 1 + u)
and the norms, whose terms are all positive, |ss - sum x^2| <= gamma(Tn + 6) sum x^2 with the chain Tn of the kernel that summed them
(`row_norms_kernel` / `row_norms16_kernel` for the rows, the scan kernel itself for the query).  A correctly rounded square root of
ss (1 + t) is sqrt(ss) (1 + t)^(1/2) (1 + u): relative error rho(g) = (1 + g / (2 (1 - g))) (1 + u) - 1.  The finishing operations:
    raw     nothing more
    dot     one addition:                                   + u |result|
    l2      the root, one subtraction:                      sqrt(d2) rho(gamma(T + 8)), + u |result|
    cosine  the two norms, their product, the division:     c = dot / (|e| |q|) moves by |c| R + gamma(T + 6) sum|e q| / (|e| |q|) (1 + R),
            R = (1 + u) / ((1 - rho_e)(1 - rho_q)(1 - u)) - 1; then the two subtractions, + u |1 - c| and + u |c|.
The chain lengths are a function of the kernel instantiation (`instantiation`), which restates the dispatchers of the two files: the
16-byte family (dim % 4 == 0 and 16-byte aligned rows AND queries), the scalar family otherwise, fp16 storage.  Integer-valued data in
{-3..3} has exact dots, norms and squared distances up to dim 4096 (|sum| <= 9 * 4096 < 2^24): `tests.util.sim_fp32_exact` gives the bits.
"""

import functools

import numpy as np

from oracle import oracle

U = 2.0 ** -24
METRICS = ("cosine", "dot", "l2")
DIM_MAX = 4096
SCALAR_DIM_MAX = 2048  # the scalar family (dim % 4 != 0, or rows / queries not 16-byte aligned) stops here

# ---- the cases of tests/test_gpu_scan.py (the host test shows the discriminating condition for each) ------------------------------
VEC4_DIMS = (4, 256, 260, 512, 516, 768, 772, 1024, 1028, 1536, 1540, 2048, 2052, 4096)  # both ends of NV = 1, 2, 3, 4, 6, 8, 16
SCALAR_DIMS = (1, 63, 65, 127, 129, 255, 257, 511, 513, 1023, 1025, 2047)                # both ends of NV = 1, 2, 4, 8, 16, 32
MISALIGNED_DIMS = (64, 128, 256, 512, 1024, 2048)                                       # the scalar family with a full last slot
F16_L2_DIMS = (128, 512, 768, 1024)                                                      # scan_rows16_kernel<1>, <2> (640 cannot be created)
F16_WIDE_DIMS = (1152, 2048, 2176, 3072, 3200, 4096)                                     # scan_rows16_wide_kernel<4>, <6>, <8>
STREAM_DIMS = (128, 256, 384, 512, 768, 1024)                                            # the MFMA stream kernels' widths


def gamma(m):
    return m * U / (1.0 - m * U)


def rho(g):
    """Relative error of sqrtf of a sum with relative error g."""
    return (1.0 + g / (2.0 * (1.0 - g))) * (1.0 + U) - 1.0


def _first(classes, nv):
    for c in classes:
        if nv <= c:
            return c
    raise ValueError("width outside every class")


def instantiation(dim, storage="f32", aligned=True):
    """The kernels a (dim, storage, alignment) runs -> dict: family ('vec4' / 'scalar' / 'f16'), vec (elements per load), nv (the scan's
    vector slots), terms (the scan's chain, also the query norm's), norm_nv / norm_terms (the row-norm kernel's), live (the last live
    slot), slot_cols (columns per slot)."""
    dim = int(dim)
    if not 1 <= dim <= DIM_MAX:
        raise ValueError("dim must be 1 .. 4096")
    if storage == "f16":
        if dim % 8:
            raise ValueError("fp16 storage: dim % 8 == 0")
        vec, family = 8, "f16"
        nv = 1 if dim <= 512 else 2 if dim <= 1024 else 4 if dim <= 2048 else 6 if dim <= 3072 else 8
        norm_nv = 8 if dim > 1024 else 1 if dim <= 512 else 2
    elif dim % 4 == 0 and aligned:
        vec, family = 4, "vec4"
        nv = _first((1, 2, 3, 4, 6, 8, 16), -(-dim // 256))
        norm_nv = _first((1, 2, 4, 8, 16), -(-dim // 256))
    else:
        if dim > SCALAR_DIM_MAX:
            raise ValueError("the scalar family stops at dim 2048")
        vec, family = 1, "scalar"
        nv = _first((1, 2, 4, 8, 16, 32), -(-dim // 64))
        norm_nv = _first((4, 16, 32), -(-dim // 64))
    slot_cols = 64 * vec
    return {"family": family, "vec": vec, "nv": nv, "terms": nv * vec, "norm_nv": norm_nv, "norm_terms": norm_nv * vec,
            "live": (dim - 1) // slot_cols, "slot_cols": slot_cols}


def dropped_columns(dim, storage="f32", aligned=True):
    """The columns a kernel is most likely to lose: the first, the last, the first of the last live vector slot (distinct ones)."""
    k = instantiation(dim, storage, aligned)
    return sorted({0, dim - 1, k["live"] * k["slot_cols"]})


# ---- reference ---------------------------------------------------------------------------------------------------------------------
def row_norms(E):
    """(|e|, |e|^2) per row, float64."""
    E = np.asarray(E, dtype=np.float64)
    ss = np.sum(E * E, axis=1)
    return np.sqrt(ss), ss


def reference(E, Q, metric, drop_dot=None, drop_norm=None):
    """float64 scores [B, n] of queries Q [B, dim] (or one [dim] -> [n]) over rows E [n, dim]; metric: cosine / dot / l2 / raw.
    `drop_dot` / `drop_norm`: a column left out of the dot (of the squared distance for l2) / of the ROW norm -- what a kernel that loses
    that column would compute (tests/test_scan_ref_host.py: the discriminating condition)."""
    E = np.asarray(E, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    single = Q.ndim == 1
    Q2 = Q[None, :] if single else Q
    Ed, Qd = E, Q2
    if drop_dot is not None:
        keep = np.arange(E.shape[1]) != drop_dot
        Ed, Qd = E[:, keep], Q2[:, keep]
    if metric == "l2":
        d2 = np.stack([np.sum((Ed - q[None, :]) ** 2, axis=1) for q in Qd])
        out = 1.0 - np.sqrt(d2)
    else:
        dot = Qd @ Ed.T
        if metric == "raw":
            out = dot
        elif metric == "dot":
            out = 1.0 + dot
        elif metric == "cosine":
            En = E if drop_norm is None else E[:, np.arange(E.shape[1]) != drop_norm]
            ne = row_norms(En)[0]
            nq = row_norms(Q2)[0]
            with np.errstate(invalid="ignore", divide="ignore"):
                out = 1.0 - (1.0 - dot / (nq[:, None] * ne[None, :]))
        else:
            raise ValueError(f"Unsupported metric: {metric}")
    return out[0] if single else out


# ---- bound -------------------------------------------------------------------------------------------------------------------------
def norm_bound(E, storage="f32", aligned=True):
    """Bounds (on |e|, on |e|^2) of the row-norm kernel's outputs, float64 [n]."""
    k = instantiation(np.shape(E)[1], storage, aligned)
    ne, ss = row_norms(E)
    g = gamma(k["norm_terms"] + 6)
    return ne * rho(g), ss * g


def bound(E, Q, metric, storage="f32", aligned=True, norms_aligned=None):
    """Per-row, per-query bound [B, n] (or [n]) on |device score - reference| for finite data.  `aligned`: rows AND queries of the scan are
    16-byte aligned; `norms_aligned`: the rows were when the index measured their norms (default: the same)."""
    E = np.asarray(E, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    single = Q.ndim == 1
    Q2 = Q[None, :] if single else Q
    dim = E.shape[1]
    k = instantiation(dim, storage, aligned)
    T = k["terms"]
    if metric == "l2":
        d2 = np.stack([np.sum((E - q[None, :]) ** 2, axis=1) for q in Q2])
        root = np.sqrt(d2)
        ds = root * rho(gamma(T + 8))
        out = ds + U * (np.abs(1.0 - root) + ds)
    else:
        dot = Q2 @ E.T
        S = np.abs(Q2) @ np.abs(E).T
        bd = gamma(T + 6) * S
        if metric == "raw":
            out = bd
        elif metric == "dot":
            out = bd + U * (np.abs(1.0 + dot) + bd)
        elif metric == "cosine":
            kn = instantiation(dim, storage, aligned if norms_aligned is None else norms_aligned)
            ne, nq = row_norms(E)[0], row_norms(Q2)[0]
            rho_e, rho_q = rho(gamma(kn["norm_terms"] + 6)), rho(gamma(T + 6))
            R = (1.0 + U) / ((1.0 - rho_e) * (1.0 - rho_q) * (1.0 - U)) - 1.0
            with np.errstate(invalid="ignore", divide="ignore"):
                den = nq[:, None] * ne[None, :]
                c = dot / den
                dc = np.abs(c) * R + bd / den * (1.0 + R)
            e1 = dc + U * (np.abs(1.0 - c) + dc)
            out = e1 + U * (np.abs(c) + e1)
        else:
            raise ValueError(f"Unsupported metric: {metric}")
    return out[0] if single else out


# ---- comparator --------------------------------------------------------------------------------------------------------------------
def ordered(scores, rows):
    """The returned order is consistent with the returned scores: (NaN last, score descending, row ascending), strictly."""
    s = np.asarray(scores, dtype=np.float64)
    r = np.asarray(rows, dtype=np.int64)
    nan = np.isnan(s)
    key = np.where(nan, -np.inf, s)
    later_class = nan[:-1] < nan[1:]
    same_class = nan[:-1] == nan[1:]
    return bool(np.all(later_class | (same_class & ((key[:-1] > key[1:]) | ((key[:-1] == key[1:]) & (r[:-1] < r[1:]))))))


def scatter(S, R, n):
    """(B, k >= n) search result -> scores [B, n] by row; asserts that every row of every query came back once, in an order consistent
    with the scores, and that the padding is (-inf, -1)."""
    S, R = np.atleast_2d(np.asarray(S)), np.atleast_2d(np.asarray(R))
    assert S.shape == R.shape and S.shape[1] >= n, (S.shape, R.shape, n)
    out = np.empty((len(S), n), dtype=S.dtype)
    for b in range(len(S)):
        assert np.array_equal(np.sort(R[b, :n]), np.arange(n)), f"query {b}: the returned rows are not every row once"
        assert np.all(R[b, n:] == -1) and np.all(np.isneginf(S[b, n:])), f"query {b}: padding is not (-inf, -1)"
        if not ordered(S[b, :n], R[b, :n]):
            i = next(i for i in range(n - 1) if not ordered(S[b, i:i + 2], R[b, i:i + 2]))
            raise AssertionError(f"query {b}: order inconsistent with the scores at place {i}: scores {S[b, i]!r}, {S[b, i + 1]!r}, rows {R[b, i]}, {R[b, i + 1]}")
        out[b, R[b, :n]] = S[b, :n]
    return out


def assert_within(got, ref64, bnd, what=""):
    """Every element within its bound of the reference; no element is excepted.  Returns the largest error / bound."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref64.shape == bnd.shape, (got.shape, ref64.shape, bnd.shape)
    assert np.all(np.isfinite(ref64)) and np.all(np.isfinite(bnd)), f"{what}: the comparator takes finite references"
    err = np.abs(got - ref64)
    bad = ~(err <= bnd)  # (a NaN output is bad)
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(np.isnan(err), np.inf, err / np.maximum(bnd, 1e-300)))), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} scores outside the bound; worst at {i}: got {got[i]!r}, reference "
                             f"{ref64[i]!r}, error {err[i]:.3e}, bound {bnd[i]:.3e}")
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(np.where(bnd > 0, err / bnd, 0.0))) if err.size else 0.0


def assert_search(S, R, E, Q, metric, storage="f32", aligned=True, norms_aligned=None, what="", known=None):
    """The comparator of every float-data GPU test: a k >= n search result against reference and bound.  Returns scores by row, ratio.
    `known`: (reference, bound) of a batch these queries are the first of, computed once by the caller."""
    E = np.asarray(E)
    Q2 = np.atleast_2d(np.asarray(Q))
    got = scatter(S, R, len(E))
    full, bnd = known if known is not None else (reference(E, Q2, metric), bound(E, Q2, metric, storage, aligned, norms_aligned))
    ratio = assert_within(got, full[:len(Q2)], bnd[:len(Q2)], what)
    return got, ratio


def exact_ranked(E, Q, metric):
    """Integer data: per query the oracle's (scores, rows) of every row, best first."""
    from tests.util import sim_fp32_exact

    E = np.asarray(E, dtype=np.float32)
    return [oracle.topk_desc(sim_fp32_exact(E, q, metric), len(E)) for q in np.atleast_2d(np.asarray(Q))]


def assert_exact(S, R, E, Q, metric, what="", known=None):
    """Integer data: scores bit for bit `sim_fp32_exact`, rows in the oracle's order (ties to the lowest row), padding (-inf, -1).
    `known`: `exact_ranked` of a batch these queries are the first of."""
    S, R = np.atleast_2d(np.asarray(S)), np.atleast_2d(np.asarray(R))
    Q2 = np.atleast_2d(np.asarray(Q))
    n = len(E)
    ranked = known if known is not None else exact_ranked(E, Q2, metric)
    assert S.shape == R.shape and S.shape[0] == len(Q2) and S.shape[1] >= n, (S.shape, R.shape, n)
    for b in range(len(Q2)):
        es, ei = ranked[b]
        assert np.array_equal(R[b, :n], ei), f"{what} query {b}: rows differ (ties resolve to the lowest row)"
        got, want = np.ascontiguousarray(S[b, :n], dtype=np.float32), es.astype(np.float32)
        nan = np.isnan(want)  # (a zero row or query under cosine: 0 / 0, whose NaN carries no agreed sign or payload)
        assert np.array_equal(np.isnan(got), nan), f"{what} query {b}: NaN scores differ"
        assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)), f"{what} query {b}: scores not bit-exact"
        assert np.all(R[b, n:] == -1) and np.all(np.isneginf(S[b, n:])), f"{what} query {b}: padding is not (-inf, -1)"


# ---- input makers ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _int_data(seed, n, dim):
    E = oracle.synth_matrix(seed, n, dim, "small_int")
    E.setflags(write=False)
    return E


def int_data(seed, n, dim):
    """Integers in {-3..3} as float32 [n, dim] (read-only, shared): exact in fp16 too."""
    return _int_data(int(seed), int(n), int(dim))


@functools.lru_cache(maxsize=None)
def _same_sign(seed, n, dim, negative, f16):
    x = np.float32(0.75) + np.float32(0.25) * oracle.synth_matrix(seed, n, dim)  # [0.5, 1): exact in fp32
    if f16:
        x = x.astype(np.float16).astype(np.float32)  # still [0.5, 1]
    x = -x if negative else x
    x.setflags(write=False)
    return x


def same_sign_rows(seed, n, dim, f16=False):
    """Rows with e_j in [0.5, 1] (read-only, shared); `f16`: rounded to fp16 first."""
    return _same_sign(int(seed), int(n), int(dim), False, bool(f16))


def same_sign_queries(seed, B, dim, f16=False):
    """Queries with q_j in [-1, -0.5]: no term of a dot cancels, every column adds >= 0.25 to |dot| and >= 1 to a squared distance."""
    return _same_sign(int(seed), int(B), int(dim), True, bool(f16))


# ---- the float-data cases ----------------------------------------------------------------------------------------------------------
N_ROWS = 203          # 26 blocks of 8 rows: 25 full trips of a block and a last one of three rows
N_ROWS_F16_WIDE = 1500
ADAPTER_DIMS = (5, 63, 257, 1023, 2047)
TILE_PERIOD = 509     # big corpora repeat this many base rows (prime: no alignment with waves, blocks or trips)


def float_case(dim, storage="f32", n=N_ROWS, B=7):
    """The same-sign rows and queries of a width -> (E [n, dim], Q [B, dim]), float32 values (fp16 values for fp16 storage).  Fewer rows
    or queries are a prefix of more (counter-based generator)."""
    return same_sign_rows(7000 + dim, n, dim, storage == "f16"), same_sign_queries(9000 + dim, B, dim, False)


def int_case(dim, n=N_ROWS, B=7):
    return int_data(3000 + dim, n, dim), int_data(5000 + dim, B, dim)


def tiled(base, n, shift=0):
    """n rows that repeat the base rows: row r is base[(r + shift) % len(base)]."""
    return np.ascontiguousarray(base[(np.arange(n) + shift) % len(base)])


def float_cases():
    """Every (dim, storage, aligned, metrics, n, B) tests/test_gpu_scan.py runs on same-sign data: the rows are `float_case(dim, storage,
    n, B)` (big corpora tile their first TILE_PERIOD rows; the adapter's matrix is the [dim, dim] case)."""
    out = []
    out += [(d, "f32", True, METRICS, N_ROWS, 7) for d in VEC4_DIMS]
    out += [(d, "f32", True, METRICS, TILE_PERIOD, 7) for d in (8, 260)]          # rows counts, trips, position independence
    out += [(d, "f32", False, METRICS, N_ROWS, 33) for d in SCALAR_DIMS]
    out += [(d, "f32", False, METRICS, TILE_PERIOD, 7) for d in (5, 63)]
    out += [(d, "f32", False, METRICS, N_ROWS, 7) for d in MISALIGNED_DIMS]
    out += [(d, "f16", True, ("l2",), N_ROWS, 4) for d in F16_L2_DIMS]
    out += [(d, "f16", True, METRICS, N_ROWS_F16_WIDE, 7) for d in F16_WIDE_DIMS]
    out += [(d, "f32", False, ("raw",), d, 7) for d in ADAPTER_DIMS]
    return out
