"""The exact MaxSim kernels (maxsim_stream.hip: `maxsim_stream_kernel` mode 0, `maxsim_stream2_kernel`; maxsim_generic.hip: the three pairs
kernels, `maxsim_cand_kernel`, `maxsim_generic_kernel`) stated in float64, NumPy only: reference, the split they use restated, derived
error bounds, planted defects, the launchers' choices restated, and the cases of tests/test_gpu_maxsim_float.py as data.  `gamma`, the
comparator and the same-sign makers are tests/scan_ref.py's; the fp16 split rules and their residuals are tests/score_gemm_ref.py's.

Reference.  d[i, j] = Q[i] . D[j] in float64, m[i, c] = max over the rows of chunk c, score[c] = sum_i m[i, c]; an empty chunk and a
candidate < 0 score -inf.

Per-dot bounds -- derived from each kernel's code, never fitted to device output.  S = sum_k |e_k q_k|, u = 2^-24, g23(m) = m 2^-23 / (1 - m
2^-23): Higham's gamma with the unit of a truncating adder, which the matrix pipe is charged with because its internal order and rounding
are not stated by the code (tests/score_gemm_ref.py, "accumulation"); it covers round-to-nearest fp32 additions too.
  (Every chain below counts only the k positions where both operands are non-zero: a zero product leaves an accumulator as it is.)
  generic   `maxsim_generic_kernel<NV, VEC>`: a lane runs ONE fma chain over its NV * VEC slots (slots past dim are skipped, which only
            shortens it), then `wave_sum`'s six butterfly additions:  gamma(NV VEC + 6) S.  The instantiation is `generic_instantiation`.
  pairs     `maxsim_pairs_kernel`, `maxsim_pairs_packed_kernel`, `maxsim_pairs_wide_kernel`, fp32 or fp16-stored rows (widened on the way
            in: exact): v_mfma_f32_16x16x4_f32 over ascending k into ONE accumulator per (row, query vector) -- `acc0` / `acc1` live across
            the k blocks (and across the wide kernel's windows) and are cleared only when the tile is complete, so NO addition merges K
            partials: a chain of dim products (the zero products of a partial last block add nothing):  g23(dim) S.
  cand      exact: one chain of 128 products, g23(128) S.  SPLIT: eh.qh into `acc` (128 products), el.qh and eh.ql into `acl` (256), one
            addition, one exact power of two: every product passes through at most 256 + 1 additions:  g23(3 * 128 + 1) S' + rep, with S'
            the halves' products, S' <= (1 + 2^-9) S.  fp16 rows: eh.qh then eh.ql into the same accumulator:  g23(256) S' + rep.
  stream    `maxsim_stream_kernel` / `maxsim_stream2_kernel`: compute wave w owns K quarter w (KW = dim / 4 columns).  Exact: a chain of KW
            products, then `kreduce`'s (p0 + p1) + (p2 + p3): two more additions on every partial:  g23(KW + 2) S.  SPLIT: `acc` KW
            products, `acl` 2 KW, acc + acl, times q_unscale (exact), the two merges:  g23(3 KW + 3) S' + rep.  fp16 rows: acc KW, acl KW,
            one addition, two merges:  g23(2 KW + 3) S' + rep.
  rep       what the (hi, lo) split itself drops, `rep_bound`: tests/score_gemm_ref.py's "representation" with the scales THIS code uses.
            Rows: x = fp32(e s), s the index's `e_scale` = 2^(14 - ex) of the corpus' largest |e| (`row_scale`; api.hip: update_split_scale
            from `row_range_kernel`'s maximum), hi / lo by truncation (`cvt_pkrtz`).  fp16-stored rows are exact: no residual, s = 1.
            Queries: y = fp32(q t), hi / lo rounded to nearest, where t = 2^(14 - ex) of the largest |q| of a SPAN: in
            `maxsim_stream_kernel` and `query_split_kernel` one K quarter of ALL the pass's vectors (the wave's `mx` runs over both query
            tiles and all four kq groups, then a 64-lane maximum), in `maxsim_cand_kernel` the whole query (nq x 128), over fp32 and
            over fp16-stored rows (until these tests it did not scale over fp16 rows: profiles/maxsim_float_error.txt).  The residuals are absolute in the scaled domain -- |y - qh - ql| <=
            max(2^-22 |y|, 2^-25) -- so an element far below its span's largest loses bits: once |y| < 2^-3 (2^-17 of the span's
            largest) its lo half is subnormal and the bound charges 2^-25 / t instead of 2^-22 |q|; below 2^-14 the hi half is too.
            `rep_bound` follows that: it is computed per span with the span's own scale, never per vector.
Score bound.  max is 1-Lipschitz: m[i, c] moves by at most max_j bound[i, j].  The sum over the query vectors: the generic kernel adds
ceil(nq / 64) values per lane and six butterfly steps; the MFMA kernels run a DPP / shuffle tree over 16 or 32 columns of which only nq hold
a value (x + 0 is exact), so a value passes through fewer than nq roundings:  gamma(adds) (sum_i |m_i| + sum_i b_i), adds = ceil(nq / 64) + 6
or nq.  `maxsim_scores` with more than 32 vectors runs the stream kernel in passes of 32 -- each with its own query scales -- and adds a
pass to what `out` holds: one more rounding, u |running sum|, per pass after the first (`stream_scores_bound`).

One-hot probes.  One-hot rows against dense queries (and one-hot query vectors against dense rows) leave ONE product in every dot: the
accumulation terms vanish next to the per-product residual, and every k position of every width is some row's only product.  The bound is
still the derived one above (S is that one product); tests/test_maxsim_ref_host.py shows that a dropped lo term exceeds it at dim 1024.
"""

import functools
from dataclasses import dataclass

import numpy as np

from tests import scan_ref
from tests.scan_ref import U, gamma
from tests.score_gemm_ref import U23, _f16_rn, pow2_scale, split_rows

STREAM_DIMS = scan_ref.STREAM_DIMS
NEG_INF = -np.inf


def g23(m):
    return m * U23 / (1.0 - m * U23)


# ---- the launchers' choices, restated (tests/test_maxsim_ref_host.py holds them to the source) -------------------------------------------
def generic_instantiation(dim, aligned=True):
    """(NV, VEC) of `launch_maxsim_generic`: the 16-byte family where dim % 4 == 0 and rows, queries and the query stride are 16-byte
    aligned, scalar loads otherwise."""
    dim = int(dim)
    if dim % 4 == 0 and aligned:
        nv = -(-dim // 256)
        for c in (1, 2, 4, 8, 16):
            if nv <= c:
                return c, 4
    else:
        nv = -(-dim // 64)
        for c in (2, 8, 32):
            if nv <= c:
                return c, 1
    raise ValueError("dim too large for the generic kernel")


def pairs_choice(dim, packed_mode, rows16=False):
    """The kernel `launch_maxsim_pairs` starts, as the template's name."""
    if dim % 16 or dim < 16 or dim > 4096:
        raise ValueError("unsupported")
    r = "true" if rows16 else "false"
    if dim > 1024:
        if dim % 128:
            raise ValueError("unsupported")
        return f"maxsim_pairs_wide_kernel<{r}>"
    full = dim % 128 == 0
    packed = packed_mode != 0 and full
    if packed and packed_mode == 2 and not rows16:
        return "maxsim_pairs_packed_kernel<128, false, 0, 16>"
    if packed:
        return f"maxsim_pairs_packed_kernel<{256 if dim % 256 == 0 else 128}, {r}>"
    if dim % 256 == 0:
        return f"maxsim_pairs_kernel<true, 256, {r}>"
    if full:
        return f"maxsim_pairs_kernel<true, 128, {r}>"
    return f"maxsim_pairs_kernel<false, 128, {r}>"


def nqt(nq):
    """Query tiles of 16 of the MFMA kernels (`launch_kw`, `launch_cand_any`)."""
    if not 1 <= nq <= 32:
        raise ValueError("nq must be 1 .. 32")
    return 1 if nq <= 16 else 2


def row_scale(E):
    """The index's `e_scale` (api.hip: update_split_scale): 2^(14 - max(ex, -100)) of the largest |element|; 1 for an all-zero corpus."""
    return pow2_scale(E) if np.any(E) else 1.0


def split_eligible(E):
    """The index keeps the split only while the largest elements of all non-zero rows lie within 2^10 of each other and all is finite."""
    mx = np.max(np.abs(np.asarray(E, dtype=np.float64)), axis=1)
    nz = mx[mx > 0]
    return bool(np.all(np.isfinite(mx)) and np.shape(E)[1] % 4 == 0 and (nz.size == 0 or nz.max() / nz.min() <= 1024.0))


def spans(kernel, dim):
    """The K ranges that share one query scale and one accumulator chain."""
    if kernel in ("stream", "stream2"):
        kw = dim // 4
        return tuple(slice(w * kw, (w + 1) * kw) for w in range(4))
    return (slice(0, dim),)


# ---- reference -----------------------------------------------------------------------------------------------------------------------
def dots(E, Q):
    """float64 [nq, n]."""
    return np.asarray(Q, dtype=np.float64) @ np.asarray(E, dtype=np.float64).T


def abs_dots(E, Q):
    return np.abs(np.asarray(Q, dtype=np.float64)) @ np.abs(np.asarray(E, dtype=np.float64)).T


def chunk_max(V, off, fill=NEG_INF):
    """[nq, n] -> [nq, n_chunks]: the maximum over each chunk's rows; `fill` for an empty chunk."""
    off = np.asarray(off, dtype=np.int64)
    assert off[0] == 0 and off[-1] == V.shape[1]
    out = np.full((V.shape[0], len(off) - 1), fill, dtype=np.float64)
    ne = off[1:] > off[:-1]
    if ne.any():
        out[:, ne] = np.maximum.reduceat(V, off[:-1][ne], axis=1)
    return out


def scores_from(V, off):
    """Chunk scores of per-dot values V [nq, n]: sum over the vectors of the chunk maxima; empty chunks -inf."""
    return chunk_max(V, off).sum(axis=0)


def scores(E, off, Q):
    return scores_from(dots(E, Q), off)


def take(chunk_scores, cand):
    """Scores of a candidate list: -inf for an ordinal outside [0, n_chunks)."""
    cand = np.asarray(cand, dtype=np.int64)
    ok = (cand >= 0) & (cand < len(chunk_scores))
    return np.where(ok, chunk_scores[np.where(ok, cand, 0)], NEG_INF)


# ---- the split, restated with this code's scales ------------------------------------------------------------------------------------------
def split_q(Q, kernel, arith):
    """(qh, ql, y, t): the query's halves in the scaled domain, float64 [nq, dim], and the scale t per column, [dim]."""
    Q32 = np.atleast_2d(np.asarray(Q, dtype=np.float32))  # noqa: N806
    t = np.ones(Q32.shape[1])
    for sl in spans(kernel, Q32.shape[1]):
        t[sl] = pow2_scale(Q32[:, sl])
    y = Q32 * t.astype(np.float32)[None, :]
    hi = _f16_rn(y)
    lo = _f16_rn((y - hi.astype(np.float32)).astype(np.float32))
    return hi, lo, y.astype(np.float64), t


def _rows(E, s, arith):
    if arith == "f16_stored":
        E64 = np.asarray(E, dtype=np.float64)  # noqa: N806
        assert np.array_equal(E64, E64.astype(np.float16).astype(np.float64)), "fp16-stored rows hold fp16 values"
        return E64, np.zeros_like(E64), E64, 1.0
    eh, el, x = split_rows(E, s)
    return eh, el, x, float(s)


def d_restated(E, Q, s, kernel, arith, terms=("hh", "lh", "hl"), unscale_by=None):
    """What a split kernel computes in exact arithmetic, float64 [nq, n].  `terms`: the products kept.  `unscale_by`: a permutation of the
    spans -- span w is unscaled by span unscale_by[w]'s scale (a planted defect)."""
    eh, el, _, s = _rows(E, s, arith)
    qh, ql, _, t = split_q(Q, kernel, arith)
    sp = spans(kernel, eh.shape[1])
    out = np.zeros((qh.shape[0], eh.shape[0]))
    for w, sl in enumerate(sp):
        part = np.zeros_like(out)
        if "hh" in terms:
            part += qh[:, sl] @ eh[:, sl].T
        if "lh" in terms:
            part += qh[:, sl] @ el[:, sl].T
        if "hl" in terms:
            part += ql[:, sl] @ eh[:, sl].T
        tw = t[sl][0] if unscale_by is None else t[sp[unscale_by[w]]][0]
        out += part / (s * tw)
    return out


def rep_bound(E, Q, s, kernel, arith):
    """|float64 dot - d_restated|, [nq, n]: X rq + re Y - re rq + el ql per product (tests/score_gemm_ref.py), per span with its scale."""
    _, _, X, s = _rows(E, s, arith)  # noqa: N806
    _, _, Y, t = split_q(Q, kernel, arith)  # noqa: N806
    aX, aY = np.abs(X), np.abs(Y)  # noqa: N806
    nzx, nzy = aX > 0, aY > 0
    if arith == "f16_stored":
        EL = RE = np.zeros_like(aX)  # noqa: N806
    else:
        EL = np.where(nzx, np.maximum(2.0 ** -10 * aX, 2.0 ** -24), 0.0)  # noqa: N806
        RE = np.where(nzx, np.maximum(2.0 ** -10 * EL, 2.0 ** -24), 0.0)  # noqa: N806
    DQ = np.where(nzy, np.maximum(2.0 ** -11 * aY, 2.0 ** -25), 0.0)  # noqa: N806
    QL = np.where(nzy, DQ * (1.0 + 2.0 ** -11) + 2.0 ** -25, 0.0)  # noqa: N806
    RQ = np.where(nzy, np.maximum(2.0 ** -11 * DQ, 2.0 ** -25), 0.0)  # noqa: N806
    u = 1.0 / (s * t)[None, :]
    return (RQ * u) @ aX.T + (aY * u) @ RE.T + (RQ * u) @ RE.T + (QL * u) @ EL.T


# ---- bounds ------------------------------------------------------------------------------------------------------------------------------
def chain(kernel, arith, dim, aligned=True):
    """(products, extra, per, halves): the longest chain of accumulated products a dot passes through, the additions behind it (butterfly,
    acc + acl, K merges), the products per k position, and whether they are products of halves."""
    if kernel == "generic":
        nv, vec = generic_instantiation(dim, aligned)
        return nv * vec, 6, 1, False
    if kernel == "pairs":
        return dim, 0, 1, False
    kw, merges = (dim // 4, 2) if kernel in ("stream", "stream2") else (dim, 0)
    if arith == "fp32_exact":
        return kw, merges, 1, False
    if arith == "f16_split":
        return 3 * kw, 1 + merges, 3, True
    if arith == "f16_stored":
        return 2 * kw, (1 if merges else 0) + merges, 2, True
    raise ValueError(arith)


def dot_bound(E, Q, s, kernel, arith, aligned=True):
    """|device dot - float64 dot|, [nq, n], for ONE pass's vectors Q (nq <= 32 for the MFMA kernels).  A product that is exactly zero
    leaves its accumulator as it is (x + 0 = x in every rounding mode, fma(e, 0, x) = x), so the chain counts only the k positions where
    both operands are non-zero -- on one-hot probes that is ONE, and the bound is the per-product one."""
    products, extra, per, halves = chain(kernel, arith, np.shape(E)[1], aligned)
    nz = (np.asarray(Q) != 0).astype(np.float64) @ (np.asarray(E) != 0).astype(np.float64).T
    T = np.minimum(products, per * nz) + extra  # noqa: N806
    g = (gamma if kernel == "generic" else g23)(T)
    S = abs_dots(E, Q)  # noqa: N806
    if not halves:
        return g * S
    return g * (1.0 + 2.0 ** -9) * S + rep_bound(E, Q, s, kernel, arith)


def sum_adds(kernel, nq):
    return -(-nq // 64) + 6 if kernel == "generic" else nq


def chunk_bound(D, B, off, kernel):
    """(score float64, bound) per chunk from dots D and per-dot bounds B [nq, n] of one pass; empty chunks: (-inf, 0)."""
    m, mb = chunk_max(D, off), chunk_max(B, off, 0.0)
    sc, sb = m.sum(axis=0), mb.sum(axis=0)
    with np.errstate(invalid="ignore"):
        bd = sb + gamma(sum_adds(kernel, D.shape[0])) * (np.abs(m).sum(axis=0) + sb)
    return sc, np.where(np.isfinite(sc), bd, 0.0)


def stream_scores_bound(E, off, Q, s, arith, kernel="stream"):
    """`DeviceIndex.maxsim_scores` over a stream width: passes of 32 vectors, each added to what the previous ones left."""
    total, bound = None, None
    for v0 in range(0, len(Q), 32):
        q = Q[v0:v0 + 32]
        sc, bd = chunk_bound(dots(E, q), dot_bound(E, q, s, kernel, arith), off, kernel)
        if total is None:
            total, bound = sc, bd
        else:
            total = total + sc
            with np.errstate(invalid="ignore"):
                bound = bound + bd
                bound = np.where(np.isfinite(total), bound + U * (np.abs(total) + bound), 0.0)
    return total, bound


def scores_bound(E, off, Q, s, kernel, arith, aligned=True):
    """(float64 chunk scores, bound) of one query through `kernel`."""
    if kernel in ("stream", "stream2"):
        return stream_scores_bound(E, off, Q, s, arith, kernel)
    return chunk_bound(dots(E, Q), dot_bound(E, Q, s, kernel, arith, aligned), off, kernel)


# ---- float32 restatements (tests/test_maxsim_ref_host.py: they stay inside the bounds) -------------------------------------------------------
def chain_f32(E, Q, kernel, dim_spans=None):
    """An fp32 chain in NumPy float32: per span an ordered multiply-add over ascending k (two roundings a step, which g23 covers), the spans
    merged (p0 + p1) + (p2 + p3)."""
    E32, Q32 = np.asarray(E, dtype=np.float32), np.asarray(Q, dtype=np.float32)  # noqa: N806
    parts = []
    for sl in dim_spans or spans(kernel, E32.shape[1]):
        acc = np.zeros((len(Q32), len(E32)), dtype=np.float32)
        for k in range(sl.start, sl.stop):
            acc = acc + Q32[:, k:k + 1] * E32[None, :, k]
        parts.append(acc)
    if len(parts) == 4:
        return ((parts[0] + parts[1]) + (parts[2] + parts[3])).astype(np.float64)
    return parts[0].astype(np.float64)


def sum_f32(V, off):
    """Chunk scores of float32 dots: the maxima summed in float32, vector by vector."""
    m = chunk_max(V, off).astype(np.float32)
    out = np.zeros(m.shape[1], dtype=np.float32)
    with np.errstate(invalid="ignore"):
        for i in range(m.shape[0]):
            out = out + m[i]
    return out.astype(np.float64)


# ---- planted defects: the chunk scores a defect would give ---------------------------------------------------------------------------------
def defect_dropped_lo(E, off, Q, s, kernel, arith, which):
    """`which` = 'lh' (el.qh never multiplied) or 'hl' (eh.ql: the `any_lo` shortcut taken when it must not be)."""
    keep = tuple(x for x in ("hh", "lh", "hl") if x != which)
    return scores_from(d_restated(E, Q, s, kernel, arith, keep), off)


def defect_neighbour_scale(E, off, Q, s, kernel, arith):
    """K quarter w is unscaled by quarter (w + 1) % 4's scale."""
    return scores_from(d_restated(E, Q, s, kernel, arith, unscale_by=(1, 2, 3, 0)), off)


def defect_row_past_end(E, off, Q):
    """The row behind a chunk's last one takes part in its maximum (the last chunk has none behind it)."""
    D = dots(E, Q)  # noqa: N806
    m = chunk_max(D, off)
    off = np.asarray(off)
    for c in range(len(off) - 1):
        if off[c + 1] > off[c] and off[c + 1] < D.shape[1]:
            m[:, c] = np.maximum(m[:, c], D[:, off[c + 1]])
    return m.sum(axis=0)


def defect_padded_vector(E, off, Q):
    """A padded query vector (index >= nq, the clamped load of vector nq - 1 not zeroed) adds its maximum."""
    m = chunk_max(dots(E, Q), off)
    pad = 16 * nqt(len(Q)) - len(Q)
    return m.sum(axis=0) + (m[-1] if pad else 0.0)


def defect_carried_max(E, off, Q):
    """The running maximum is not reset where a chunk ends."""
    m = chunk_max(dots(E, Q), off)
    out = m.copy()
    for c in range(1, m.shape[1]):
        if np.isfinite(m[0, c]) and np.isfinite(m[0, c - 1]):
            out[:, c] = np.maximum(m[:, c], m[:, c - 1])
    return out.sum(axis=0)


def defect_zero_max(E, off, Q):
    """The maximum starts from 0 instead of -inf."""
    m = chunk_max(dots(E, Q), off)
    return np.where(np.isfinite(m), np.maximum(m, 0.0), m).sum(axis=0)


def defect_skipped_tail(E, off, Q):
    """The last partial k block (dim % 128 != 0) is skipped."""
    dim = np.shape(E)[1]
    keep = dim - dim % 128
    return scores_from(dots(np.asarray(E)[:, :keep], np.asarray(Q)[:, :keep]), off)


# ---- input makers (deterministic; shared arrays are read-only) -----------------------------------------------------------------------------
def _ro(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x


def _f16(x):
    return x.astype(np.float16).astype(np.float32)


@functools.lru_cache(maxsize=None)
def make_rows(kind, seed, n, dim, f16=False, pow2=0):
    """normal: N(0, 1);  pos: [0.5, 1) (nothing cancels);  one_hot: row r holds U(0.25, 1) at k = r % dim.  `f16`: fp16 values (an
    fp16-stored index holds them exactly);  `pow2`: the corpus times 2^pow2."""
    rng = np.random.default_rng(seed)
    if kind == "normal":
        x = rng.standard_normal((n, dim)).astype(np.float32)
    elif kind == "pos":
        x = np.array(scan_ref.same_sign_rows(seed, n, dim))
    elif kind == "one_hot":
        x = np.zeros((n, dim), dtype=np.float32)
        x[np.arange(n), np.arange(n) % dim] = rng.uniform(0.25, 1.0, n).astype(np.float32)
    else:
        raise ValueError(kind)
    if f16:
        x = _f16(x)
    return _ro(x * np.float32(2.0 ** pow2))


@functools.lru_cache(maxsize=None)
def make_queries(kind, seed, n_queries, nq, dim):
    """[n_queries, nq, dim] float32.
    normal          N(0, 1)
    neg             [-1, -0.5]: against `pos` rows every dot is negative -- a masked row, a padded vector or a zero maximum would win
    spread          vector i scaled by 2^((5 i) % 17 - 8): 2^-8 .. 2^8 inside one query and inside every K quarter
    quarters        K quarter w scaled by 2^(12 (w % 2)): neighbouring quarters differ by 2^12
    f16             fp16 values: every lo half is zero (`any_lo` false)
    lo_one_quarter  fp16 values except K quarter 2 (a non-zero lo half in exactly one quarter)
    one_hot         vector i holds U(0.25, 1) at k = (37 i + 11 query) % dim, zero elsewhere: every dot is one product
    """
    rng = np.random.default_rng(seed)
    shape = (n_queries, nq, dim)
    if kind == "neg":
        x = np.array(scan_ref.same_sign_queries(seed, n_queries * nq, dim)).reshape(shape)
    elif kind == "one_hot":
        x = np.zeros(shape, dtype=np.float32)
        for b in range(n_queries):
            x[b, np.arange(nq), (37 * np.arange(nq) + 11 * b) % dim] = rng.uniform(0.25, 1.0, nq).astype(np.float32)
    else:
        x = rng.standard_normal(shape).astype(np.float32)
        w = (np.arange(dim) * 4) // max(dim, 4)
        if kind == "spread":
            x *= (2.0 ** ((5 * np.arange(nq)) % 17 - 8)).astype(np.float32)[None, :, None]
        elif kind == "quarters":
            x *= (2.0 ** (12 * (w % 2))).astype(np.float32)[None, None, :]
        elif kind == "f16":
            x = _f16(x)
        elif kind == "lo_one_quarter":
            x = np.where((w == 2)[None, None, :], x, _f16(x))
        elif kind != "normal":
            raise ValueError(kind)
    return _ro(x)


@functools.lru_cache(maxsize=None)
def make_offsets(layout, seed, n):
    """ragged: 1 .. 40 rows, every fifth chunk empty;  rows: every row its own chunk (rows_gaps: with empty chunks in between);  big: ragged around one chunk of 300 rows (it
    spans tiles and, in the stream kernels, would span workgroup shares: they cut at chunk ends)."""
    rng = np.random.default_rng(seed)
    if layout == "rows":
        off = np.arange(n + 1)
    elif layout == "rows_gaps":  # every row its own chunk, an empty chunk behind every fourth
        off = np.repeat(np.arange(n + 1), np.where(np.arange(n + 1) % 4 == 3, 2, 1))
    else:
        sizes, total = [], 0
        while total < n:
            sz = 0 if len(sizes) % 5 == 4 else int(rng.integers(1, 41))
            if layout == "big" and len(sizes) == 2:
                sz = 300
            sz = min(sz, n - total)
            sizes.append(sz)
            total += sz
        off = np.concatenate(([0], np.cumsum(sizes)))
    off = off.astype(np.int64)
    off.setflags(write=False)
    return off


@functools.lru_cache(maxsize=None)
def make_candidates(seed, n_queries, n_cand, n_chunks):
    """Random ordinals with a duplicate and -1 entries (the padding of a search result: -inf; the binding refuses any other ordinal outside
    [0, n_chunks) of a host list)."""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, n_chunks, (n_queries, n_cand)).astype(np.int32)
    if n_cand >= 4:
        c[:, 1] = c[:, 0]
        c[:, 2] = -1
        c[-1, 3] = -1
    c.setflags(write=False)
    return c


# ---- the cases of tests/test_gpu_maxsim_float.py ---------------------------------------------------------------------------------------------
N_ROWS = 203                    # not a multiple of 16: the last tile is ragged
WALK_ROWS = 256 * 16 * 5 + 37   # grid = min(CUs, tiles): every one of 256 workgroups walks at least five tiles
ARITHS = ("f16_split", "fp32_exact", "f16_stored")
NQS = (1, 15, 16, 17, 31, 32)   # both query-tile counts, padded vectors on either side
PASS_NQS = (33, 70)             # `maxsim_scores` accumulating passes: 32 + 1, 32 + 32 + 6
PAIRS_DIMS = (16, 48, 144, 256, 384, 1024)  # not FULL (16, 48, 144: one block, and two with a partial last); FULL at KB 128 (384), KB 256 (256, 1024)
#   (dim 128 belongs to `maxsim_cand_kernel` in `rl_maxsim_rerank`.  The pairs kernels see that width only behind the bound-filtered routes of
#   `maxsim_topk_batch`, which need the HI plane: a corpus of 64 Mi elements and more, half a million rows -- no quick test; its instantiation,
#   <true, 128>, and its packed ones run at dim 384)
WIDE_DIMS = (1152, 2048, 4096)  # nine windows (odd), sixteen, thirty-two
GENERIC_VEC4 = (4, 252, 260, 508, 516, 1020, 1028, 2048, 2052, 4096)  # both ends of NV = 1, 2, 4, 8, 16 outside the stream widths (a
#   stream width reaches the generic kernel through `maxsim_rerank` with more than 32 vectors: 256, 512, 1024 below)
GENERIC_SCALAR = (1, 127, 129, 511, 513, 2047)                          # both ends of NV = 2, 8, 32
GENERIC_RERANK = (256, 512, 1024, 100, 130)                             # NV = 1, 2, 4 with a full last slot; dims that are no multiple of 16


@dataclass(frozen=True)
class Case:
    name: str
    entry: str          # scores / rerank / topk
    kernel: str         # generic / pairs / cand / stream / stream2
    inst: str           # the template instantiation(s) it runs, for the reader
    dim: int
    nq: int
    n: int = N_ROWS
    layout: str = "ragged"
    rows: str = "normal"
    queries: str = "normal"
    storage: str = "f32"
    exact: bool = False       # set_exact_fp32()
    pow2: int = 0             # corpus scale
    n_queries: int = 1
    n_cand: int = 0
    packed: int = -1          # option pairs_packed (-1: not set)
    shift: str = ""           # "rows" / "queries": that tensor starts 4 bytes past 16-byte alignment

    @property
    def arith(self):
        """What `DeviceIndex.arithmetic` must say for this case."""
        if self.storage == "f16":
            return "f16_stored"
        return "f16_split" if not self.exact and self.dim % 4 == 0 else "fp32_exact"

    @property
    def aligned(self):
        return not self.shift

    def data(self):
        """(E [n, dim], off, Q [n_queries, nq, dim], cand [n_queries, n_cand] or None), read-only."""
        E = make_rows(self.rows, 1000 + self.dim, self.n, self.dim, self.storage == "f16", self.pow2)  # noqa: N806
        off = make_offsets(self.layout, 2000 + self.n, self.n)
        Q = make_queries(self.queries, 3000 + self.dim + self.nq, self.n_queries, self.nq, self.dim)  # noqa: N806
        cand = make_candidates(4000 + self.n_cand, self.n_queries, self.n_cand, len(off) - 1) if self.n_cand else None
        return E, off, Q, cand


@functools.lru_cache(maxsize=None)
def references(case):
    """Per query (float64 chunk scores, bound), computed once."""
    E, off, Q, _ = case.data()  # noqa: N806
    s = row_scale(E) if case.arith == "f16_split" else 0.0
    return tuple(scores_bound(E, off, q, s, case.kernel, case.arith, case.aligned) for q in Q)


def _stream_inst(dim, nq, arith):
    kw = dim // 4
    flags = {"f16_split": "false, true", "fp32_exact": "false, false", "f16_stored": "true, false"}[arith]
    return f"maxsim_stream_kernel<{kw}, {nqt(min(nq, 32))}, 0, false, 6, {flags}>"


def _variants(**kw):
    """The three arithmetics of one shape: (storage, exact).  A corpus at 2^+-40 has no fp16 form."""
    return [dict(kw), dict(kw, exact=True)] + ([] if kw.get("pow2") else [dict(kw, storage="f16")])


def stream_cases():
    out = []
    for dim in STREAM_DIMS:
        def add(tag, nq, **kw):
            for v in _variants(**kw):
                c = Case("", "scores", "stream", "", dim, nq, **v)
                out.append(Case(f"stream_dim{dim}_{tag}_{c.arith}", "scores", "stream", _stream_inst(dim, nq, c.arith), dim, nq, **v))
        for nq in NQS + PASS_NQS:
            add(f"nq{nq}", nq)
        add("rows_layout_all_negative", 17, layout="rows", rows="pos", queries="neg")    # every row a chunk; a zero maximum or a padded vector wins
        add("big_chunk_same_sign", 32, n=403, layout="big", rows="pos", queries="neg")   # a chunk across 19 tiles; the accumulation bound is tight
        add("spread_vectors", 32, queries="spread")                                      # 2^-8 .. 2^8 inside one K quarter's scale span
        add("spread_vectors_nq9", 9, queries="spread")
        add("quarters_2p12", 17, queries="quarters")                                     # a neighbour's q_unscale is 2^12 off
        add("f16_valued_queries", 32, queries="f16")                                     # any_lo false: the third product is skipped
        add("lo_in_one_quarter", 17, queries="lo_one_quarter")                           # any_lo differs between the compute waves
        add("corpus_2m40", 32, pow2=-40)
        add("corpus_2p40", 15, pow2=40)
        add("one_hot_rows", 32, n=dim + 19, layout="rows", rows="one_hot")               # every k position is some chunk's only product ...
        add("one_hot_rows_nq1", 1, n=dim + 19, layout="rows", rows="one_hot")            # ... and some score's
        add("one_hot_queries", 32, queries="one_hot")
    for dim in STREAM_DIMS:  # a workgroup walks five tiles and more: stages, ordinal ring and the epilogue pipeline wrap (split arithmetic;
        #                      the exact and fp16 kernels share the walk: one width each keeps the corpus uploads few)
        out.append(Case(f"stream_dim{dim}_walk_f16_split", "scores", "stream", _stream_inst(dim, 32, "f16_split"), dim, 32, n=WALK_ROWS))
    out.append(Case("stream_dim256_walk_fp32_exact", "scores", "stream", _stream_inst(256, 17, "fp32_exact"), 256, 17, n=WALK_ROWS, exact=True))
    out.append(Case("stream_dim512_walk_f16_stored", "scores", "stream", _stream_inst(512, 16, "f16_stored"), 512, 16, n=WALK_ROWS, storage="f16"))
    return tuple(out)


def _generic_inst(dim, aligned=True):
    return "maxsim_generic_kernel<%d, %d>" % generic_instantiation(dim, aligned)


def generic_cases():
    out = []
    for dim in GENERIC_VEC4 + GENERIC_SCALAR:  # `maxsim_scores`: the stream launcher declines the width
        nq = 65 if dim in (4, 127, 260, 2047) else 130 if dim in (129, 516) else 5  # more vectors than lanes: the lane-strided sum
        n = 67 if dim > 1024 else N_ROWS
        out.append(Case(f"generic_dim{dim}_nq{nq}", "scores", "generic", _generic_inst(dim), dim, nq, n=n))
    out.append(Case("generic_dim252_all_negative", "scores", "generic", _generic_inst(252), 252, 7, rows="pos", queries="neg", layout="rows"))
    out.append(Case("generic_dim129_all_negative", "scores", "generic", _generic_inst(129), 129, 3, rows="pos", queries="neg"))
    out.append(Case("generic_dim260_corpus_2m40", "scores", "generic", _generic_inst(260), 260, 5, pow2=-40))
    out.append(Case("generic_dim127_corpus_2p40", "scores", "generic", _generic_inst(127), 127, 5, pow2=40))
    out.append(Case("generic_dim516_one_hot_rows", "scores", "generic", _generic_inst(516), 516, 5, n=516 + 19, layout="rows", rows="one_hot"))
    out.append(Case("generic_dim513_one_hot_queries", "scores", "generic", _generic_inst(513), 513, 65, queries="one_hot"))
    out.append(Case("generic_dim64_misaligned_queries", "scores", "generic", _generic_inst(64, False), 64, 5, shift="queries"))
    out.append(Case("generic_dim2048_misaligned_rows", "scores", "generic", _generic_inst(2048, False), 2048, 3, n=67, shift="rows"))
    for dim in GENERIC_RERANK:  # `maxsim_rerank`: more than 32 vectors (cand and pairs decline), or a width that is no multiple of 16
        nq = 33 if dim % 16 == 0 else 6
        out.append(Case(f"generic_rerank_dim{dim}_nq{nq}", "rerank", "generic", _generic_inst(dim), dim, nq, n_queries=3, n_cand=21))
    out.append(Case("generic_rerank_dim128_misaligned_queries", "rerank", "generic", _generic_inst(128, False), 128, 9, n_queries=2, n_cand=21,
                    shift="queries"))
    return tuple(out)


CAND_LENGTHS = (1, 5, 13, 100, 300)  # one; fewer than a wave's eight; no multiple of 8; no multiple of 8 x 16 waves; a few hundred


def _cand_inst(nq, arith):
    flags = {"f16_split": "false, true", "fp32_exact": "false, false", "f16_stored": "true, false"}[arith]
    return f"maxsim_cand_kernel<{nqt(nq)}, {flags}>"


def cand_cases():
    out = []

    def add(tag, nq, **kw):
        for v in _variants(**kw):
            c = Case("", "rerank", "cand", "", 128, nq, **v)
            out.append(Case(f"cand_{tag}_{c.arith}", "rerank", "cand", _cand_inst(nq, c.arith), 128, nq, **v))
    for nq, n_cand in zip(NQS, CAND_LENGTHS + (37,)):
        add(f"nq{nq}_cand{n_cand}", nq, n_queries=3, n_cand=n_cand)
    add("all_negative", 17, n_queries=2, n_cand=60, rows="pos", queries="neg")
    add("big_chunk", 32, n=403, layout="big", n_queries=2, n_cand=30, rows="pos", queries="neg")
    add("spread_vectors", 32, n_queries=2, n_cand=60, queries="spread")  # ONE scale for the whole query: the small vectors lose bits
    add("quarters_2p12", 9, n_queries=2, n_cand=60, queries="quarters")
    add("f16_valued_queries", 32, n_queries=2, n_cand=60, queries="f16")
    add("corpus_2m40", 17, n_queries=2, n_cand=60, pow2=-40)
    add("corpus_2p40", 17, n_queries=2, n_cand=60, pow2=40)
    add("one_hot_rows", 32, n=147, layout="rows", n_queries=2, n_cand=300, rows="one_hot")
    add("one_hot_rows_nq1", 1, n=147, layout="rows", n_queries=2, n_cand=300, rows="one_hot")
    add("one_hot_queries", 32, n_queries=2, n_cand=60, queries="one_hot")
    return tuple(out)


def pairs_cases():
    out = []
    for dim in PAIRS_DIMS + WIDE_DIMS:
        for storage in ("f32", "f16"):
            if storage == "f16" and dim not in STREAM_DIMS and dim % 128:
                continue  # (such an fp16-stored index cannot be created: `maxsim_pairs_kernel<false, 128, true>` is out of the binding's reach)
            modes = (0, 1, 2) if dim <= 1024 else (2,)
            n = 67 if dim > 1024 else N_ROWS
            for mode in modes:
                inst = pairs_choice(dim, mode, storage == "f16")
                for nq, n_cand, kind in ((32, 300, "normal"), (17, 13, "spread"), (1, 5, "normal"), (16, 100, "normal"), (31, 37, "quarters")):
                    if mode != 2 and nq in (1, 16, 31):
                        continue
                    out.append(Case(f"pairs_dim{dim}_{storage}_packed{mode}_nq{nq}", "rerank", "pairs", inst, dim, nq, n=n, n_queries=3,
                                    n_cand=n_cand, queries=kind, storage=storage, packed=mode))
            out.append(Case(f"pairs_dim{dim}_{storage}_all_negative_big_chunk", "rerank", "pairs", pairs_choice(dim, 2, storage == "f16"), dim, 15,
                            n=403 if dim <= 1024 else 331, layout="big", n_queries=2, n_cand=40, rows="pos", queries="neg", storage=storage, packed=2))
    for dim in (48, 384, 1024, 1152):  # corpora far from unit scale (fp32 rows only: they have no fp16 form); one-hot query vectors
        for mode in ((0, 2) if dim <= 1024 else (2,)):
            inst = pairs_choice(dim, mode)
            n = 67 if dim > 1024 else N_ROWS
            out.append(Case(f"pairs_dim{dim}_packed{mode}_corpus_2m40", "rerank", "pairs", inst, dim, 17, n=n, n_queries=2, n_cand=60, pow2=-40, packed=mode))
            out.append(Case(f"pairs_dim{dim}_packed{mode}_corpus_2p40", "rerank", "pairs", inst, dim, 15, n=n, n_queries=2, n_cand=60, pow2=40, packed=mode))
            out.append(Case(f"pairs_dim{dim}_packed{mode}_one_hot_queries", "rerank", "pairs", inst, dim, 32, n=n, n_queries=2, n_cand=60, queries="one_hot",
                            packed=mode))
    for dim in (144, 1024, 2048):
        out.append(Case(f"pairs_dim{dim}_one_hot_rows", "rerank", "pairs", pairs_choice(dim, 0), dim, 32, n=dim + 19, layout="rows", n_queries=2,
                        n_cand=300, rows="one_hot", packed=0))
    for dim in WIDE_DIMS:  # `maxsim_scores` over a wide fp16-stored index: `launch_maxsim_pairs_all_wide` (candidates == nullptr)
        out.append(Case(f"pairs_all_wide_dim{dim}", "scores", "pairs", "maxsim_pairs_wide_kernel<true>", dim, 17, n=331, layout="big", storage="f16"))
    return tuple(out)


def topk_cases():
    """`maxsim_topk_batch` on two queries of 17 .. 32 vectors over an index with empty chunks (the half-width route declines them): one
    pass of `maxsim_stream2_kernel` over the rows, then the exact selection."""
    out = []
    for dim in STREAM_DIMS:
        for storage in ("f32", "f16"):
            for nq, kind in ((17, "normal"), (32, "spread")):
                arith = "f16_split" if storage == "f32" else "f16_stored"
                out.append(Case(f"stream2_dim{dim}_{arith}_nq{nq}", "topk", "stream2", f"maxsim_stream2_kernel<{dim // 4}, false, {str(storage == 'f16').lower()}>",
                                dim, nq, n=403, layout="big", n_queries=2, queries=kind, storage=storage))
            arith = "f16_split" if storage == "f32" else "f16_stored"
            inst = f"maxsim_stream2_kernel<{dim // 4}, false, {str(storage == 'f16').lower()}>"
            # every k position some chunk's only product; every dot negative; neighbouring quarters 2^12 apart; any_lo false
            for tag, nq, kw in (("one_hot_rows", 17, dict(n=dim + 19, layout="rows_gaps", rows="one_hot")),
                                ("all_negative", 25, dict(n=403, layout="big", rows="pos", queries="neg")),
                                ("quarters_2p12", 32, dict(queries="quarters")), ("f16_valued_queries", 31, dict(queries="f16"))):
                out.append(Case(f"stream2_dim{dim}_{arith}_{tag}", "topk", "stream2", inst, dim, nq, n_queries=2, storage=storage, **kw))
    out.append(Case("stream2_dim1024_walk", "topk", "stream2", "maxsim_stream2_kernel<256, false, false>", 1024, 25, n=WALK_ROWS, n_queries=2))
    return tuple(out)


def all_cases():
    return stream_cases() + generic_cases() + cand_cases() + pairs_cases() + topk_cases()
