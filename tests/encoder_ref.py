"""References, bounds and inputs for the kernels of the native encoder forward (raglite_amd/csrc/encoder.hip), shared by
tests/test_encoder_ref_host.py (CPU) and tests/test_gpu_encoder_kernels.py: the skinny linear layer with its three epilogues, the layer
norm that closes a projection, and the embedding layer norm.

Per kernel there are three things over the same inputs:

* a float64 restatement from the 16-bit (or, for the layer norm's slices, f32) inputs -- the truth, with the sums of absolute values the
  bound is stated in;
* a bound, a function whose docstring carries its derivation.  `factor` is 2 for a kernel (the a-priori analysis doubled: the MFMA's
  internal order and the exact shape of the reduction trees are not part of the contract) and 1 for the emulations below;
* a float32 CPU emulation of the kernel's rounding points: f32 sums, one round-to-nearest-even per stored value.  The chunk-to-wave-to-
  slice order is not reproduced (torch's f32 sums have an order of their own), which is the point: the un-doubled bound has to hold for
  ANY f32 order.

Notation: u = 2^-24 (f32 unit roundoff); hu(t) half the spacing of the 16-bit format at |t| (`half_ulp`).

`linear_cases()`, `ln_cases()` and `embed_cases()` are the generators of inputs; everything they and the `*_f64` functions return is cached
and must be left unchanged."""

from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import torch

U = 2.0 ** -24
SIG_BITS = {"bfloat16": 8, "float16": 11}     # significand bits, the hidden one included
MIN_EXP = {"bfloat16": -126, "float16": -14}  # exponent of the smallest normal number: below it the spacing no longer shrinks
GELU_SLOPE = 1.13  # max |gelu'| = 1.1289.. (at v = sqrt(2) + ..): what an error of the pre-activation is multiplied by at most
DTYPES = ("bfloat16", "float16")
MAX_TOKENS = 256
KSPLIT_MAX = 8


def tdtype(name: str):
    return getattr(torch, name)


def half_ulp(t: torch.Tensor, dtype: str) -> torch.Tensor:
    """hu(t): half the spacing of `dtype` at |t| -- for 2^e <= |t| < 2^(e+1) the spacing is 2^(e + 1 - SIG_BITS); below the smallest normal
    number (fp16: 2^-14, so a spacing of 2^-24) it stays that of the subnormals.  A correctly rounded t is at most hu(t) from t."""
    _, ex = torch.frexp(t.abs().double())  # |t| = m 2^ex, m in [0.5, 1): e = ex - 1
    e = torch.clamp(ex.to(torch.int64) - 1, min=MIN_EXP[dtype])
    e = torch.where(t == 0, torch.full_like(e, MIN_EXP[dtype]), e)
    return torch.ldexp(torch.ones_like(t, dtype=torch.float64), (e - SIG_BITS[dtype]).to(torch.int32))


def one_ulp_off(t: torch.Tensor, dtype: str) -> torch.Tensor:
    """The correctly rounded t moved to the next representable value away from zero: what a bound that means something must refuse."""
    r = t.to(tdtype(dtype))
    bits = r.view(torch.int16).clone()
    return (bits + 1).view(tdtype(dtype))  # (sign-magnitude formats: + 1 on the bit pattern grows the magnitude, for either sign)


def gelu64(v: torch.Tensor) -> torch.Tensor:
    v = v.double()
    return 0.5 * v * (1.0 + torch.erf(v * (1.0 / math.sqrt(2.0))))


def gelu32(v32: torch.Tensor) -> torch.Tensor:
    """gelu_erf of the kernel, in float32 on v32's device: torch's erf, the kernel's formula."""
    assert v32.dtype == torch.float32
    return 0.5 * v32 * (1.0 + torch.erf(v32 * 0.70710678118654752440))


def gelu_c(v32: torch.Tensor, got32: torch.Tensor) -> float:
    """The worst error of a float32 erf-GELU `got32` at the float32 pre-activations v32, in units of u max(|v|, 1): the `c` of
    `gelu_bound`.  (Near v = -4 the factor 1 + erf cancels to a few u, and the product with 0.5 v carries that absolute error on: the
    error of a float32 GELU scales with |v|, not with |gelu(v)|.)"""
    v = v32.double().cpu()
    err = (got32.double().cpu() - gelu64(v)).abs()
    return float((err / (U * v.abs().clamp(min=1.0))).max())


# ---- the K slices of a projection -----------------------------------------------------------------------------------------------------
def ksplit(N: int, K: int) -> int:  # noqa: N803
    """encoder_ksplit (encoder.hip) restated: slabs x slices near 256, every wave of a slice with a 64-element chunk of its own, at most 8."""
    chunks = (K + 63) // 64
    want = 256 // max(1, N // 32)
    want = min(want, chunks // 4)
    want = max(1, min(want, KSPLIT_MAX))
    per = (chunks + want - 1) // want
    return (chunks + per - 1) // per


def slice_chunks(N: int, K: int) -> list:  # noqa: N803
    """The 64-element chunks [begin, end) of every K slice, as the launcher hands them out: ceil(chunks / slices) each."""
    chunks, s = (K + 63) // 64, ksplit(N, K)
    per = (chunks + s - 1) // s
    return [(i * per, min((i + 1) * per, chunks)) for i in range(s)]


def slice_ranges(N: int, K: int) -> list:  # noqa: N803
    """The k ranges [lo, hi) of the slices."""
    return [(64 * b, min(64 * e, K)) for b, e in slice_chunks(N, K)]


# ---- linear ----------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True, eq=False)  # (identity is the cache key of the references below)
class LinearCase:
    name: str
    dtype: str
    N: int
    K: int
    kind: str  # "exact": small integers times a power of two, every f32 sum exact in any order | "real": normal data
    Ms: tuple  # the row counts to run: rows 0 .. M - 1 of x (a row's bits do not depend on M)
    epilogues: tuple
    x: torch.Tensor     # (max(Ms), K), `dtype`, CPU
    W: torch.Tensor     # (N, K)
    bias: torch.Tensor  # (N,)


SMALL_SHAPES = [(32, 32), (96, 96), (64, 320), (32, 1056), (96, 1344), (64, 544), (64, 2080)]
ALL_MS = (1, 31, 32, 33, 64, 65, 128, 129, 255, 256)
FEW_MS = (1, 33, 129)
BGE_SHAPES = [(1024, 1024, "partial"), (1024, 4096, "partial"), (3072, 1024, "bias"), (4096, 1024, "gelu")]  # out, down, QKV, up
BGE_MS = (5, 33)
EPILOGUES = ("bias", "gelu", "partial")


def _make_linear(dtype: str, N: int, K: int, kind: str, Ms: tuple, epilogues: tuple, seed: int) -> LinearCase:  # noqa: N803
    g = torch.Generator().manual_seed(seed)
    M = max(Ms)  # noqa: N806
    if kind == "exact":
        # integers in [-4, 4]: x w sums to an integer of deviation 6.67 sqrt(K) (the variance of such an integer is 20 / 3); a power of two
        # brings that to about 2.5, so with the bias the pre-activations span about [-6, 6] (a few reach +- 10: both tails of erf).
        # |sum| <= 16 K <= 2^16 units of the power of two: exact in f32 whatever the order.
        scale = 2.0 ** -round(math.log2(6.67 * math.sqrt(K) / 2.5))
        x = torch.randint(-4, 5, (M, K), generator=g).float()
        w = torch.randint(-4, 5, (N, K), generator=g).float() * scale
        b = torch.randint(-4, 5, (N,), generator=g).float()
    else:
        x = torch.randn((M, K), generator=g)
        w = torch.randn((N, K), generator=g) * K ** -0.5
        b = torch.randn((N,), generator=g)
    dt = tdtype(dtype)
    return LinearCase(f"{dtype}-N{N}-K{K}-{kind}", dtype, N, K, kind, tuple(Ms), tuple(epilogues), x.to(dt), w.to(dt), b.to(dt))


@functools.lru_cache(maxsize=None)
def linear_cases() -> tuple:
    out, seed = [], 2000
    for dtype in DTYPES:
        for kind in ("exact", "real"):
            for N, K in SMALL_SHAPES:  # noqa: N806
                seed += 1
                out.append(_make_linear(dtype, N, K, kind, ALL_MS if (N, K) in ((96, 96), (32, 1056)) else FEW_MS, EPILOGUES, seed))
            for N, K, epi in BGE_SHAPES:  # noqa: N806
                seed += 1
                out.append(_make_linear(dtype, N, K, kind, BGE_MS, (epi,), seed))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def linear_f64(case: LinearCase):
    """(v, S): v = x W^T + bias and S = |x| |W|^T + |bias| in float64 from the 16-bit inputs, (max(Ms), N)."""
    x, w, b = case.x.double(), case.W.double(), case.bias.double()
    return x @ w.T + b, x.abs() @ w.abs().T + b.abs()


@functools.lru_cache(maxsize=None)
def linear_slices_f64(case: LinearCase):
    """Per K slice (lo, hi, p, S): p = x[:, lo:hi] W[:, lo:hi]^T, S the same of the absolute values -- no bias: the partial epilogue reads none."""
    x, w = case.x.double(), case.W.double()
    return tuple((lo, hi, x[:, lo:hi] @ w[:, lo:hi].T, x[:, lo:hi].abs() @ w[:, lo:hi].abs().T) for lo, hi in slice_ranges(case.N, case.K))


def sum_bound(K: int, S: torch.Tensor, factor: float = 2.0) -> torch.Tensor:  # noqa: N803
    """factor (K + 8) u S: the f32 error of a sum of K products (exact in f32: 16-bit x 16-bit) and a bias, in ANY order.  A sum of n
    terms in any order is off by at most gamma_(n-1) sum|terms| ~ (n - 1) u sum|terms|; K products, the waves' four partial tiles and the
    bias are fewer than K + 8 additions deep.  The factor 2 over that covers the MFMA's undocumented internal order (and whatever
    it does between its sixteen products)."""
    return factor * (K + 8) * U * S


def bias_bound(case: LinearCase, factor: float = 2.0) -> torch.Tensor:
    """|got - v| <= hu(v) + factor (K + 8) u S: the f32 sum's error, then ONE rounding to the 16-bit format."""
    v, S = linear_f64(case)  # noqa: N806
    return half_ulp(v, case.dtype) + sum_bound(case.K, S, factor)


def gelu_bound(case: LinearCase, c: float, factor: float = 2.0) -> torch.Tensor:
    """|got - gelu64(v)| <= hu(gelu64(v)) + 1.13 factor (K + 8) u S + c u max(|v|, 1): the pre-activation's f32 error through the largest
    slope of GELU, the float32 erf-GELU's own error (`gelu_c`: measured, never taken from the code under test), one rounding."""
    v, S = linear_f64(case)  # noqa: N806
    return half_ulp(gelu64(v), case.dtype) + GELU_SLOPE * sum_bound(case.K, S, factor) + c * U * v.abs().clamp(min=1.0)


def exact_gelu_bound(v: torch.Tensor, dtype: str, c: float) -> torch.Tensor:
    """Where the f32 pre-activation v is known exactly: hu(gelu64(v)) + c u max(|v|, 1)."""
    v = v.double()
    return half_ulp(gelu64(v), dtype) + c * U * v.abs().clamp(min=1.0)


def partial_bounds(case: LinearCase, factor: float = 2.0):
    """Per slice |part[s] - p_s| <= factor (K_s + 8) u S_s with the slice's own k range, and for the in-order f32 sum of the slices
    factor (K + 8) u sum_s S_s (the slices' errors, and fewer than 8 more additions)."""
    per = [sum_bound(hi - lo, S, factor) for lo, hi, _, S in linear_slices_f64(case)]
    total = sum_bound(case.K, sum(S for _, _, _, S in linear_slices_f64(case)), factor)
    return per, total


def linear_emulated(case: LinearCase, epilogue: str) -> torch.Tensor:
    """The kernel's rounding points in float32 on the CPU.  bias / gelu: (rows, N) in the case's dtype; partial: (slices, rows, N) f32."""
    x, w, b = case.x.float(), case.W.float(), case.bias.float()
    if epilogue == "partial":
        return torch.stack([x[:, lo:hi] @ w[:, lo:hi].T for lo, hi in slice_ranges(case.N, case.K)])
    y = x @ w.T + b
    return (gelu32(y) if epilogue == "gelu" else y).to(tdtype(case.dtype))


# ---- layer norm and embedding layer norm ----------------------------------------------------------------------------------------------
@dataclass(frozen=True, eq=False)
class LnCase:
    name: str
    dtype: str
    hidden: int
    slices: int
    M: int
    kind: str  # "normal" | "mean100" (rows of mean 100, spread 0.01) | "const" (constant rows)
    eps: float
    part: torch.Tensor   # (slices, M, hidden) f32
    bias: torch.Tensor   # (hidden,) `dtype`
    resid: torch.Tensor  # (M, hidden)
    ln_w: torch.Tensor
    ln_b: torch.Tensor

    def terms64(self) -> list:
        """The addends of a row in the kernel's order, float64 (M, hidden) each."""
        return [*self.part.double().unbind(0), self.bias.double().expand(self.M, -1), self.resid.double()]


LN_HIDDEN = (32, 192, 1024, 1056, 4096, 8192)  # 8, 48 and all 256 threads with data; one partly filled second pass; 4 and 8 full passes
LN_SLICES = (1, 4, 8)


def _affine(hidden: int, dt, g) -> tuple:
    return (1.0 + 0.25 * torch.randn(hidden, generator=g)).to(dt), (0.25 * torch.randn(hidden, generator=g)).to(dt)


def _make_ln(dtype: str, hidden: int, slices: int, M: int, kind: str, eps: float, seed: int) -> LnCase:  # noqa: N803
    g, dt = torch.Generator().manual_seed(seed), tdtype(dtype)
    if kind == "normal":
        part = torch.randn((slices, M, hidden), generator=g) / math.sqrt(slices)
        bias, resid = torch.randn(hidden, generator=g), torch.randn((M, hidden), generator=g)
    elif kind == "mean100":
        # the slices (f32) carry the mean and the spread -- no 16-bit format holds 100 +- 0.01 --, bias and residual a little more of it.
        # var = 1e-4 against a mean square of 1e4: E[v^2] - mean^2 in f32 is off by several times the variance itself
        part = (100.0 + 0.01 * torch.randn((slices, M, hidden), generator=g)) / slices
        bias, resid = 0.003 * torch.randn(hidden, generator=g), 0.003 * torch.randn((M, hidden), generator=g)
    else:
        # every addend constant along the row: the truth is ln_b.  The f32 mean of 0.7, 1.4, .. need not be the value itself, and a
        # variance that went negative would be a NaN
        rows = 0.7 * torch.arange(1, M + 1, dtype=torch.float32)[None, :, None]
        part = (rows / slices).expand(slices, M, hidden).contiguous()
        bias, resid = torch.full((hidden,), 0.3), (0.11 * torch.arange(1, M + 1, dtype=torch.float32))[:, None].expand(M, hidden).contiguous()
    w, b = _affine(hidden, dt, g)
    return LnCase(f"{dtype}-h{hidden}-s{slices}-M{M}-{kind}-eps{eps:g}", dtype, hidden, slices, M, kind, eps, part.float().contiguous(),
                  bias.to(dt), resid.to(dt).contiguous(), w, b)


@functools.lru_cache(maxsize=None)
def ln_cases() -> tuple:
    out, seed = [], 3000
    for dtype in DTYPES:
        for hidden in LN_HIDDEN:
            for slices in LN_SLICES:
                for kind, eps in (("normal", 1e-5), ("normal", 1e-12), ("mean100", 1e-5), ("const", 1e-5)):
                    seed += 1
                    out.append(_make_ln(dtype, hidden, slices, 3, kind, eps, seed))
        for M in (1, MAX_TOKENS):  # noqa: N806
            seed += 1
            out.append(_make_ln(dtype, 1024, 4, M, "normal", 1e-5, seed))
    return tuple(out)


def _ln_truth_and_bound(terms: list, w: torch.Tensor, b: torch.Tensor, eps: float, dtype: str, factor: float):
    """A first-order forward analysis of the order the kernel states (encoder.hip: the addends in order; the thread's elements, the
    wave's butterfly, the four waves; mean, then the variance of the centred values), times `factor`.

    v = the in-order sum of `terms`, A = the sum of their absolute values, D = 4 ceil(hidden / 1024) + 12 the depth of a row sum (a
    thread adds 4 elements per pass, then 6 butterfly steps, 3 additions over the waves, and the division and a spare):
        dv    = (terms - 1) u A                            the f32 sum of the addends
        dmean = mean(dv) + (D + 1) u mean|v|               the inputs' error through the mean, the row sum's own, the division
        dd    = dv + dmean + u |d|                         d = v - mean, one subtraction
        dvar  = 2 mean(|d| dd) + (D + 3) u var             d^2 to first order, the squares' roundings and their row sum
        rho   = dvar / (2 (var + eps)) + 3 u               relative error of rstd = 1 / sqrt(var + eps): the add, the root, the division
    and  |got - truth| <= hu(truth) + factor [ rstd |w| dd + |d rstd w| (rho + 3 u) + u |truth| ]: d's error scaled, the product's
    relative error (rstd's and three roundings), the last addition, then ONE rounding to the 16-bit format."""
    v = sum(terms)
    A = sum(t.abs() for t in terms)  # noqa: N806
    hidden = v.shape[-1]
    D = 4 * math.ceil(hidden / 1024) + 12  # noqa: N806
    w, b = w.double(), b.double()
    dv = (len(terms) - 1) * U * A
    mean = v.mean(-1, keepdim=True)
    dmean = dv.mean(-1, keepdim=True) + (D + 1) * U * v.abs().mean(-1, keepdim=True)
    d = v - mean
    dd = dv + dmean + U * d.abs()
    var = (d * d).mean(-1, keepdim=True)
    dvar = 2.0 * (d.abs() * dd).mean(-1, keepdim=True) + (D + 3) * U * var
    rho = 0.5 * dvar / (var + eps) + 3 * U
    rstd = 1.0 / torch.sqrt(var + eps)
    truth = d * rstd * w + b
    bound = half_ulp(truth, dtype) + factor * (rstd * w.abs() * dd + (d * rstd * w).abs() * (rho + 3 * U) + U * truth.abs())
    return truth, bound


def _ln_emulated(terms32: list, w: torch.Tensor, b: torch.Tensor, eps: float, dtype: str) -> torch.Tensor:
    v = terms32[0]
    for t in terms32[1:]:
        v = v + t  # f32, in order
    hidden = v.shape[-1]
    mean = v.sum(-1, keepdim=True) / hidden
    d = v - mean
    rstd = 1.0 / torch.sqrt((d * d).sum(-1, keepdim=True) / hidden + torch.tensor(eps, dtype=torch.float32))
    return (d * rstd * w.float() + b.float()).to(tdtype(dtype))


@functools.lru_cache(maxsize=None)
def ln_f64(case: LnCase):
    """(truth, kernel bound, un-doubled bound), float64 (M, hidden)."""
    truth, b2 = _ln_truth_and_bound(case.terms64(), case.ln_w, case.ln_b, case.eps, case.dtype, 2.0)
    _, b1 = _ln_truth_and_bound(case.terms64(), case.ln_w, case.ln_b, case.eps, case.dtype, 1.0)
    return truth, b2, b1


def ln_emulated(case: LnCase) -> torch.Tensor:
    return _ln_emulated([t.float() for t in case.terms64()], case.ln_w, case.ln_b, case.eps, case.dtype)


@dataclass(frozen=True, eq=False)
class EmbedCase:
    name: str
    dtype: str
    hidden: int
    n_tokens: int
    type_vocab: int
    ids: torch.Tensor        # int32 (n_tokens,), with entries outside their table
    positions: torch.Tensor
    type_ids: torch.Tensor | None
    tok: torch.Tensor        # (VOCAB, hidden) `dtype`
    pos: torch.Tensor        # (POSITIONS, hidden)
    typ: torch.Tensor        # (type_vocab, hidden)
    ln_w: torch.Tensor
    ln_b: torch.Tensor
    eps: float

    def terms64(self) -> list:
        """The three table rows of every token, indices clamped into their tables as the kernel clamps them."""
        def rows(table, idx):
            return table.double()[idx.long().clamp(0, table.shape[0] - 1)]

        typ_idx = self.type_ids if self.type_ids is not None else torch.zeros(self.n_tokens, dtype=torch.int32)
        return [rows(self.tok, self.ids), rows(self.pos, self.positions), rows(self.typ, typ_idx)]


VOCAB, POSITIONS, BIG = 50, 20, 2 ** 31 - 1
EMBED_HIDDEN = (32, 1024, 2080)  # 2080 = 2 x 1024 + 32: a third pass that only eight threads take
_IDS = {7: [-1, VOCAB, BIG, 3, VOCAB - 1, 0, 17], 1: [BIG]}
_POSITIONS = {7: [5, -1, POSITIONS, BIG, POSITIONS - 1, 0, 7], 1: [-1]}
_TYPES = {7: [0, 1, -1, 2, BIG, 1, 0], 1: [2]}  # (2 is the table size where there are two types, and past it where there is one)


@functools.lru_cache(maxsize=None)
def embed_cases() -> tuple:
    out, seed = [], 4000
    for dtype in DTYPES:
        dt = tdtype(dtype)
        for hidden in EMBED_HIDDEN:
            for n in (1, 7):
                for type_vocab, given in ((1, False), (1, True), (2, False), (2, True)):
                    seed += 1
                    g = torch.Generator().manual_seed(seed)
                    tok, pos = torch.randn((VOCAB, hidden), generator=g), 0.5 * torch.randn((POSITIONS, hidden), generator=g)
                    typ = 0.5 * torch.randn((type_vocab, hidden), generator=g)
                    w, b = _affine(hidden, dt, g)
                    i32 = lambda v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
                    out.append(EmbedCase(f"{dtype}-h{hidden}-n{n}-types{type_vocab}-{'given' if given else 'null'}", dtype, hidden, n, type_vocab,
                                         i32(_IDS[n]), i32(_POSITIONS[n]), i32(_TYPES[n]) if given else None, tok.to(dt), pos.to(dt), typ.to(dt),
                                         w, b, 1e-5))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def embed_f64(case: EmbedCase):
    """(truth, kernel bound, un-doubled bound): `_ln_truth_and_bound` with the three table rows as the addends."""
    truth, b2 = _ln_truth_and_bound(case.terms64(), case.ln_w, case.ln_b, case.eps, case.dtype, 2.0)
    _, b1 = _ln_truth_and_bound(case.terms64(), case.ln_w, case.ln_b, case.eps, case.dtype, 1.0)
    return truth, b2, b1


def embed_emulated(case: EmbedCase) -> torch.Tensor:
    return _ln_emulated([t.float() for t in case.terms64()], case.ln_w, case.ln_b, case.eps, case.dtype)


def worst_ratio(got: torch.Tensor, truth: torch.Tensor, bound: torch.Tensor) -> float:
    """max |got - truth| / bound; inf where got is not finite (a NaN must not pass as `not >`)."""
    err = (got.double().cpu() - truth).abs()
    if not bool(torch.isfinite(err).all()):
        return math.inf
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())  # (an exact zero is inside a bound of zero)
