"""What tests/test_gpu_pool_norm.py holds the kernels of pool_norm.hip (`rl_pool_norm`) against.  NumPy only, no GPU.

Reference.  `oracle.pool_norm_cast`: np.mean of float64 rows, `X /= ||X||` (or `/ max(||X||, eps)`), astype(float16); it is held
against the reference's own fixtures in tests/test_oracle_golden.py.  `reference` below only calls it.

`emulate` restates the kernels' own float64 arithmetic: rows added in order from +0.0, `* (1 / n)`, sum of squares, sqrt, fmax with
eps, `* (1 / norm)`.  It is used on the CPU only (tests/test_pool_norm_ref_host.py), to show that the committed batches meet the
comparator's condition before a GPU sees them; it is never the expected value of a GPU test.

`bound` is the per-element float64 distance a correct kernel may have from the reference, derived from the operations (its
docstring).  `assert_rounds_like` is the one comparator for fp32 and fp16 outputs: bit-equal to the reference rounded once, except
where the reference lies within the bound of a rounding boundary.  `CAP`: in every random batch the excepted elements are at most 1e-6
of the elements; the batches are seeded so that `emulate` has none.

The batches of the GPU tests are generated here (`registers_batch`, `stride_batch`, `dma_batch`, `capped_grid_batch`, `midpoints`), once
per process, with their references, so the CPU checks and the GPU tests use the same arrays.
"""

import functools

import numpy as np

from oracle import oracle

U = 2.0 ** -53  # unit roundoff of float64
CAP = 1e-6  # excepted elements / elements, at most, in a random batch
SENTINEL_F32 = np.float32(-7.0)
SENTINEL_F16_BITS = 0x5555
RING = {256: 8, 512: 8, 1024: 4}  # rows per wave in the LDS ring of pool_norm_dma_kernel<dim / 256>


def reference(tokens, begins, ends, normalize=True, eps=0.0):
    """-> (float64 [S, dim], its astype(float16)): `oracle.pool_norm_cast`, eps 0 meaning the unguarded divide."""
    with np.errstate(all="ignore"):
        return oracle.pool_norm_cast(tokens, begins, ends, normalize=normalize, eps=eps or None)


def emulate(tokens, begins, ends, normalize=True, eps=0.0):
    """The kernels' arithmetic in float64 -> float64 [S, dim].  (The sum of squares is np.sum's order here, a wave's on the device.)"""
    tokens = np.asarray(tokens, dtype=np.float64)
    out = np.empty((len(begins), tokens.shape[1]))
    with np.errstate(all="ignore"):
        for s, (b, e) in enumerate(zip(begins, ends)):
            b, e = int(b), int(e)
            acc = np.zeros(tokens.shape[1])
            if e > b:  # cumsum is sequential: ((0.0 + x_b) + x_b+1) + ...
                acc = np.cumsum(np.concatenate((acc[None], tokens[b:e])), axis=0)[-1]
            mean = acc * (np.float64(1.0) / np.float64(e - b))
            if normalize:
                norm = np.sqrt(np.sum(mean * mean))
                if eps > 0.0:
                    norm = np.fmax(norm, eps)
                mean = mean * (np.float64(1.0) / norm)
            out[s] = mean
    return out


def bound(tokens, begins, ends, normalize=True, eps=0.0):
    """Per-element bound float64 [S, dim] on |kernel - reference|, both in float64 (u = 2^-53).

    Mean.  Column c of a span of n rows, A_c = sum_j |x_jc| / n.  Any order of the n - 1 additions errs by at most (n - 1) u sum|x|
    (first order); the kernel then multiplies by fl(1 / n) (two roundings, 2 u |mean|), the reference divides (one).  With
    |mean| <= A_c:  kernel (n + 1) u A_c, reference n u A_c, together E_c = (2 n + 1) u A_c.  Stated from sum|x|, not |sum x|, so
    cancellation is covered.  A span of one row has E_c = 3 u A_c, an all-zero column E_c = 0.

    Norm.  N = max(||mean||, eps).  A side's own mean m' = m + d, |d_c| <= its share of E_c, has | ||m'|| - ||m|| | <= ||E||; the sum of dim
    squares of positive terms, the square root, the reciprocal and the product (kernel), or the division (reference), add a relative
    rho = (dim / 2 + 3) u to a side's scale factor, whatever the order of the sum.  Hence per side
        |out_c - m_c / N| <= (E_c + |m_c| ||E|| / N) / (N - ||E||) + rho |m_c| / N,
    and the bound is that with E the two sides' sum and 2 rho.  max(., eps) is 1-Lipschitz, so the guard changes nothing.

    Everything is evaluated in float64 from the reference's own mean and norm; the factor 1.01 covers that and the second-order terms
    (n u and dim u are below 1e-9 for any size a test uses).  Where the mean is not finite the bound is not either: the comparator then
    asks for equality."""
    tokens = np.asarray(tokens, dtype=np.float64)
    dim = tokens.shape[1]
    E = np.empty((len(begins), dim))
    mean = np.empty((len(begins), dim))
    with np.errstate(all="ignore"):
        for s, (b, e) in enumerate(zip(begins, ends)):
            n = int(e) - int(b)
            rows = tokens[int(b):int(e)]
            E[s] = (2 * n + 1) * U * (np.sum(np.abs(rows), axis=0) / n) if n else np.nan
            mean[s] = np.mean(rows, axis=0) if n else np.nan
        if not normalize:
            return 1.01 * E
        N = np.linalg.norm(mean, axis=1, keepdims=True)
        if eps > 0.0:
            N = np.maximum(N, eps)
        En = np.linalg.norm(E, axis=1, keepdims=True)
        rho = 2 * (dim / 2 + 3) * U
        out = 1.01 * ((E + np.abs(mean) * En / N) / (N - En) + rho * np.abs(mean) / N)
        out[np.broadcast_to(N - En <= 0, out.shape) & ~np.isnan(out)] = np.inf
        return out


def _as_float(out, dtype):
    out = np.asarray(out)
    if out.dtype.kind == "u":
        out = out.view({2: np.float16, 4: np.float32}[out.dtype.itemsize])
    assert out.dtype == dtype, (out.dtype, dtype)
    return out


def assert_rounds_like(out, ref64, bnd, dtype, what=""):
    """Every element of `out` (float16 / float32, or their bits as uint16 / uint32) is `ref64` rounded once to `dtype`, bit for bit;
    or `ref64` lies within `bnd` of the rounding boundary between that value and its neighbour in `dtype` (the midpoint of the two; past
    the largest finite value, the midpoint to 2^(emax + 1), which rounds to inf), and `out` is that neighbour.  NaN matches NaN, and
    zeros match whatever their sign (the kernels sum from +0.0, np.mean of -0.0 rows is -0.0).  -> the number of excepted elements."""
    dtype = np.dtype(dtype)
    out = _as_float(out, dtype)
    ref64 = np.asarray(ref64, dtype=np.float64)
    assert out.shape == ref64.shape, (out.shape, ref64.shape)
    bits = {2: np.uint16, 4: np.uint32}[dtype.itemsize]
    with np.errstate(all="ignore"):
        want = ref64.astype(dtype)
        same = (out.view(bits) == want.view(bits)) | (np.isnan(out) & np.isnan(want)) | ((out == 0) & (want == 0))
        bad = np.flatnonzero(~same.ravel())
        if len(bad) == 0:
            return 0
        o, w, r = out.ravel()[bad], want.ravel()[bad], ref64.ravel()[bad]
        b = np.broadcast_to(np.asarray(bnd, dtype=np.float64), ref64.shape).ravel()[bad]
        neighbour = np.nextafter(w, o)  # one step of `dtype` from the rounded reference towards the output
        is_neighbour = (neighbour.view(bits) == o.view(bits)) & ~np.isnan(o) & ~np.isnan(w)
        top = 2.0 ** (np.finfo(dtype).maxexp)  # 65536 / 2^128: where inf would be, were it a number
        w64, n64 = w.astype(np.float64), neighbour.astype(np.float64)
        w64 = np.where(np.isinf(w64), np.sign(w64) * top, w64)
        n64 = np.where(np.isinf(n64), np.sign(n64) * top, n64)
        boundary = 0.5 * w64 + 0.5 * n64  # exact: neighbours of a 24-bit format
        ok = is_neighbour & (np.abs(r - boundary) <= b)
    if not np.all(ok):
        i = int(bad[np.flatnonzero(~ok)[0]])
        idx = np.unravel_index(i, ref64.shape)
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ref64.size} {dtype.name} elements are not the reference rounded once; first at "
                             f"{tuple(int(k) for k in idx)}: got {out.ravel()[i]!r} ({int(out.view(bits).ravel()[i]):#x}), reference "
                             f"{ref64.ravel()[i]!r} -> {want.ravel()[i]!r}, bound {np.broadcast_to(bnd, ref64.shape).ravel()[i]!r}")
    return int(len(bad))


def cap(n_elements):
    """The largest number of excepted elements a random batch of `n_elements` may have."""
    return int(CAP * n_elements)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------

def edge_columns(dim):
    """The first and last column of every group of 64, without the last column of the row."""
    return sorted({c for g in range(0, dim, 64) for c in (g, min(g + 63, dim - 1))} - {dim - 1})


def make_tokens(rng, n, dim):
    """n token rows float32: a unit Gaussian row, extra weight (a quarter of the row's energy) on the first and last column of every group
    of 64, the last column set to 0.25 .. 0.35 of the rest of the row, each row scaled by 2^-2 .. 2^2.  A dropped, duplicated or shifted
    column or 1-KiB piece moves a pooled value by far more than rounding."""
    x = rng.standard_normal((n, dim))
    x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-300)
    edges = edge_columns(dim)
    if edges:
        x[:, edges] += rng.choice([-1.0, 1.0], size=(n, len(edges))) * np.sqrt(0.25 / len(edges))
    x[:, -1] = 0.0
    rest = np.linalg.norm(x, axis=1)
    x[:, -1] = rng.choice([-1.0, 1.0], size=n) * rng.uniform(0.25, 0.35, size=n) * np.where(rest > 0, rest, 1.0)
    return (x * np.exp2(rng.uniform(-2, 2, size=(n, 1)))).astype(np.float32)


class Batch:
    """tokens float32 [T, dim], begins / ends int64 [S]; the reference and the bound per (normalize, eps), computed once."""

    def __init__(self, tokens, begins, ends):
        self.tokens = tokens
        self.begins, self.ends = np.asarray(begins, np.int64), np.asarray(ends, np.int64)
        assert np.all(self.begins >= 0) and np.all(self.begins <= self.ends) and np.all(self.ends <= len(tokens))
        for a in (self.tokens, self.begins, self.ends):
            a.setflags(write=False)
        self.dim, self.n_spans = int(tokens.shape[1]), len(self.begins)
        self._ref = {}

    def ref(self, normalize, eps=0.0):
        """-> (ref64, ref16, bound); read-only, shared by every test that asks."""
        key = (bool(normalize), float(eps))
        if key not in self._ref:
            r64, r16 = reference(self.tokens, self.begins, self.ends, normalize, eps)
            bnd = bound(self.tokens, self.begins, self.ends, normalize, eps)
            for a in (r64, r16, bnd):
                a.setflags(write=False)
            self._ref[key] = (r64, r16, bnd)
        return self._ref[key]


VEC4_DIMS = [4, 256, 260, 512, 516, 768, 772, 1024, 1028, 1536, 1540, 2048, 2052, 4096]
SCALAR_DIMS = [1, 63, 65, 127, 129, 254, 257, 510, 513, 1022, 1025, 2047]


def instantiation(dim):
    """The `pool_norm_kernel<NV, VEC>` that `launch_pool_norm` dispatches for aligned buffers of this width."""
    if dim % 4 == 0:
        return next(nv for nv in (1, 2, 3, 4, 6, 8, 16) if (dim + 255) // 256 <= nv), 4
    return next(nv for nv in (1, 2, 4, 8, 16, 32) if (dim + 63) // 64 <= nv), 1


@functools.lru_cache(maxsize=None)
def registers_batch(dim):
    """Fewer than 64 spans (the register-staged kernel at any width): spans of 0, 1, 2, 3, 4, 5, 7, 8 and 9 rows laid end to end in a
    shuffled order, one span overlapping two others, one span listed twice, and the list then put out of order (reversed halves)."""
    rng = np.random.default_rng(7000 + dim)
    lengths = rng.permutation([0, 1, 2, 3, 4, 5, 7, 8, 9, 0, 3, 1])
    ends = np.cumsum(lengths)
    begins = ends - lengths
    tokens = make_tokens(rng, int(ends[-1]), dim)
    twice = int(np.flatnonzero(lengths == 9)[0])
    begins = np.concatenate((begins, [2, begins[twice]]))  # rows 2 .. 12 overlap their neighbours; the span of 9 rows twice
    ends = np.concatenate((ends, [13, ends[twice]]))
    order = np.concatenate((np.arange(7, 14), np.arange(0, 7)))
    return Batch(tokens, begins[order], ends[order])


STRIDE_SPANS = 70_000


@functools.lru_cache(maxsize=None)
def stride_batch():
    """dim 4, 70 000 spans of 0 .. 2 rows anywhere in 4 096 token rows: more spans than the widest launch of `pool_norm_kernel<1, 4>` has
    waves (tests/test_gpu_pool_norm.py::test_more_spans_than_waves says how many that is)."""
    rng = np.random.default_rng(7004)
    tokens = make_tokens(rng, 4096, 4)
    lengths = rng.integers(0, 3, size=STRIDE_SPANS)
    begins = rng.integers(0, 4096 - 2, size=STRIDE_SPANS)
    return Batch(tokens, begins, begins + lengths)


DMA_DIMS = [256, 512, 1024]
DMA_SPANS = [64, 65, 130, 448, 512, 577, 3001]
DMA_ROWS = 1200


def dma_lengths(dim):
    ring = RING[dim]
    return [0, 1, 2, ring - 1, ring, ring + 1, 2 * ring + 1, 37]


@functools.lru_cache(maxsize=None)
def dma_tokens(dim):
    tokens = make_tokens(np.random.default_rng(8000 + dim), DMA_ROWS, dim)
    tokens.setflags(write=False)
    return tokens


@functools.lru_cache(maxsize=None)
def dma_batch(dim, n_spans):
    """64 spans or more at a DMA width: lengths drawn from `dma_lengths` (around the ring depth), half of the spans starting where the
    previous one ended and half anywhere in the 1 200 token rows, plus one span of 300 rows and one that covers the whole matrix (both
    at seeded positions in the list)."""
    rng = np.random.default_rng(8000 + 10 * dim + n_spans)
    lengths = rng.choice(dma_lengths(dim), size=n_spans)
    begins = rng.integers(0, DMA_ROWS - 40, size=n_spans)
    follow = rng.random(n_spans) < 0.5
    for s in range(1, n_spans):
        if follow[s] and begins[s - 1] + lengths[s - 1] + lengths[s] <= DMA_ROWS:
            begins[s] = begins[s - 1] + lengths[s - 1]
    ends = begins + lengths
    long, whole = (int(v) for v in rng.choice(n_spans, size=2, replace=False))
    begins[long], ends[long] = 411, 711
    begins[whole], ends[whole] = 0, DMA_ROWS
    return Batch(dma_tokens(dim), begins, ends)


CAPPED_SPANS = 20_000


@functools.lru_cache(maxsize=None)
def capped_grid_batch():
    """dim 256, 20 000 spans of 0 .. 3 rows laid end to end: more than 64 spans per CU, so the DMA grid is capped at the CU count."""
    rng = np.random.default_rng(8256)
    lengths = rng.integers(0, 4, size=CAPPED_SPANS)
    ends = np.cumsum(lengths)
    return Batch(make_tokens(rng, int(ends[-1]), 256), ends - lengths, ends)


EMPTY_CASES = ["first", "last", "sixteen", "scattered", "last_queue", "all"]


@functools.lru_cache(maxsize=None)
def empties_batch(dim, case):
    """512 spans of 1, 2, 3 or 9 rows laid end to end, then the spans of `case` emptied."""
    rng = np.random.default_rng(9000 + dim)
    lengths = rng.choice([1, 2, 3, 9], size=512)
    ends = np.cumsum(lengths)
    begins = ends - lengths
    tokens = make_tokens(rng, int(ends[-1]), dim)
    emptied = {"first": [0], "last": [511], "sixteen": list(range(72, 88)), "scattered": [8, 11, 12, 15, 131, 133, 135, 200, 201, 202, 203, 204, 205, 206],
               "last_queue": list(range(448, 512)), "all": list(range(512))}[case]
    ends = ends.copy()
    ends[emptied] = begins[emptied]
    return Batch(tokens, begins, ends), np.asarray(emptied)


SPECIAL = {10: "nan", 40: "inf-inf", 41: "flt_max", 77: "inf"}


@functools.lru_cache(maxsize=None)
def isolation_batch(dim, healthy):
    """96 spans of 2, 3, 5 or 9 rows laid end to end; the rows of the spans in `SPECIAL` hold NaN, +-inf or FLT_MAX, or ones where `healthy`."""
    rng = np.random.default_rng(9500 + dim)
    lengths = rng.choice([2, 3, 5, 9], size=96)
    ends = np.cumsum(lengths)
    begins = ends - lengths
    tokens = make_tokens(rng, int(ends[-1]), dim)
    for s, kind in SPECIAL.items():
        rows = tokens[begins[s]:ends[s]]
        if healthy:
            rows[:] = 1.0
        elif kind == "nan":
            rows[1] = np.nan
        elif kind == "inf-inf":
            rows[0], rows[1] = np.inf, -np.inf
        elif kind == "inf":
            rows[-1] = np.inf
        else:
            rows[:] = np.finfo(np.float32).max
    return Batch(tokens, begins, ends)


@functools.lru_cache(maxsize=None)
def zero_rows_batch(n_spans):
    """dim 256, spans of 1, 2, 4 or 9 rows laid end to end; spans 0, 5, 6 and the last hold rows of zeros (one row of span 5: -0.0).
    -> (batch, those spans)"""
    rng = np.random.default_rng(9700 + n_spans)
    lengths = rng.choice([1, 2, 4, 9], size=n_spans)
    ends = np.cumsum(lengths)
    begins = ends - lengths
    tokens = make_tokens(rng, int(ends[-1]), 256)
    zero = np.asarray([0, 5, 6, n_spans - 1])
    for s in zero:
        tokens[begins[s]:ends[s]] = 0.0
    tokens[begins[5]] = -0.0
    return Batch(tokens, begins, ends), zero


# ---- the cast ----------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def midpoints():
    """All 31 744 positive float16 rounding midpoints m (between consecutive float16 values from +0 up, 65520 = the midpoint to
    overflow included), each as m - t/2, m, m + t/2 with t = 2^(floor(log2 m) - 30), both signs: 190 464 float64 values, every one the
    exact mean of the two float32 rows (2 m, +-t or 0).  -> (row0 float32, row1 float32, mean float64), flat."""
    h = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float64)  # +0 .. 65504
    m = 0.5 * (h + np.concatenate((h[1:], [65536.0])))  # exact
    t = np.exp2(np.floor(np.log2(m)) - 30)
    two_m = np.repeat(2.0 * m, 6)
    step = np.tile([-1.0, 0.0, 1.0, -1.0, 0.0, 1.0], len(m)) * np.repeat(t, 6)
    sign = np.tile([1.0, 1.0, 1.0, -1.0, -1.0, -1.0], len(m))
    row0, row1 = sign * two_m, sign * step
    mean = (row0 + row1) * 0.5
    assert len(mean) == 190_464
    for a in (row0, row1, mean):
        a.setflags(write=False)
    return row0, row1, mean


def midpoint_spans(dim):
    """The midpoint set laid out along the columns of two-row spans (186 at dim 1024, 372 at 512, 744 at 256, 47 at 4096) -> (tokens float32 [2 S, dim], begins, ends, mean float64 [S, dim])."""
    row0, row1, mean = midpoints()
    n = -(-len(mean) // dim)
    pad = np.zeros(n * dim - len(mean))  # (dim 4096: the last span's second half is zeros, whose mean is as exact)
    row0, row1, mean = (np.concatenate((a, pad)) for a in (row0, row1, mean))
    tokens = np.empty((2 * n, dim), np.float32)
    tokens[0::2] = row0.reshape(n, dim)
    tokens[1::2] = row1.reshape(n, dim)
    begins = np.arange(0, 2 * n, 2, dtype=np.int64)
    return tokens, begins, begins + 2, mean.reshape(n, dim)
