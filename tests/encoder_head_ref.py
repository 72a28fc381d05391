"""References, bounds and inputs for the cross-encoder's head kernel (raglite_amd/csrc/encoder_head.hip), shared by
tests/test_cross_encoder_native_host.py (CPU) and tests/test_gpu_encoder_head.py, in the style of tests/encoder_ref.py, whose `U`,
`sum_bound` and `worst_ratio` are used as they are.

The kernel, per sequence, on the first token's row x (16-bit), every step in f32 and nothing rounded to 16 bits:
    a_j = sum_k Wp[j, k] x[k] + bp[j]      lane l: one fma chain over k = 4 l + 256 i + {0..3}, i ascending; the 64 chains through the
                                           butterfly xor 32, 16, 8, 4, 2, 1; then + bp[j]
    p_j = tanhf(a_j)
    logit = sum_j wh[j] p_j + bh           lane i < 8 of wave w: fma chain over j = 8 (4 t + w) + i, t ascending; then one thread adds the
                                           32 partials in the order (w, i) from 0; then + bh
The order is a function of `hidden` alone.

`head_cases()` makes the inputs; everything it and `head_f64` return is cached and must be left unchanged."""

from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import torch

from tests.encoder_ref import DTYPES, U, sum_bound, tdtype

HIDDEN = (32, 64, 96, 192, 384, 1024)  # one 32-wide chunk (8 lanes with data, one turn per wave); .. ; MiniLM's; four passes of a lane
KINDS = ("normal", "cancel", "saturate")
N_TOKENS = 300  # rows of x: more than one token block of 256, so that rows 255, 256 and n_tokens - 1 are three different places


@dataclass(frozen=True, eq=False)  # (identity is the cache key of `head_f64`)
class HeadCase:
    name: str
    dtype: str
    hidden: int
    kind: str
    x: torch.Tensor         # (N_TOKENS, hidden) `dtype`, CPU
    pooler_w: torch.Tensor  # (hidden, hidden)
    pooler_b: torch.Tensor  # (hidden,)
    head_w: torch.Tensor    # (1, hidden): nn.Linear(hidden, 1)'s own
    head_b: torch.Tensor    # (1,)


def _make(dtype: str, hidden: int, kind: str, seed: int) -> HeadCase:
    g, dt = torch.Generator().manual_seed(seed), tdtype(dtype)
    x = torch.randn((N_TOKENS, hidden), generator=g)
    w = torch.randn((hidden, hidden), generator=g) * hidden ** -0.5
    b = 0.5 * torch.randn(hidden, generator=g)
    wh = torch.randn((1, hidden), generator=g) * hidden ** -0.5
    bh = torch.randn(1, generator=g)
    if kind == "cancel":
        # x[2i + 1] = -x[2i] exactly (after the rounding to 16 bits, below) and Wp[j, 2i + 1] = Wp[j, 2i] (1 + 2^-6 n): a pre-activation is the
        # small difference of products whose absolute sum is about 4 sqrt(hidden) times larger; wh likewise pairs up against p's neighbours
        x = 4.0 * x
        x = x.to(dt).float()
        x[:, 1::2] = -x[:, 0::2]
        w[:, 1::2] = w[:, 0::2] * (1.0 + 2.0 ** -6 * torch.randn((hidden, hidden // 2), generator=g))
        wh = 4.0 * wh
        wh[:, 1::2] = -wh[:, 0::2] * (1.0 + 2.0 ** -6 * torch.randn((1, hidden // 2), generator=g))
        b = 0.05 * b
    elif kind == "saturate":
        w = 8.0 * w  # pre-activations of deviation 8: nearly every tanh is +-1 to the last bit, a few fall in between
        b = 4.0 * b
    return HeadCase(f"{dtype}-h{hidden}-{kind}", dtype, hidden, kind, x.to(dt), w.to(dt), b.to(dt), wh.to(dt), bh.to(dt))


@functools.lru_cache(maxsize=None)
def head_cases() -> tuple:
    out, seed = [], 5000
    for dtype in DTYPES:
        for hidden in HIDDEN:
            for kind in KINDS:
                seed += 1
                out.append(_make(dtype, hidden, kind, seed))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def head_f64(case: HeadCase):
    """(logit, a, S, T) in float64 from the 16-bit inputs, for EVERY row of x as the first token: a (rows, hidden) the pre-activations,
    S = |x| |Wp|^T + |bp| their sums of absolute values, logit (rows,) and T = sum_j |wh_j tanh(a_j)| + |bh| (rows,)."""
    x, w, b = case.x.double(), case.pooler_w.double(), case.pooler_b.double()
    wh, bh = case.head_w.double().reshape(-1), case.head_b.double().reshape(())
    a = x @ w.T + b
    S = x.abs() @ w.abs().T + b.abs()  # noqa: N806
    p = torch.tanh(a)
    return p @ wh + bh, a, S, (p * wh).abs().sum(-1) + bh.abs()


def tanh_c(v32: torch.Tensor, got32: torch.Tensor) -> float:
    """The worst error of a float32 tanh `got32` at the float32 arguments v32 against float64, in units of u = 2^-24 (|tanh| <= 1: an
    absolute unit is the right one): the `c` of `head_bound`.  Measured on a tanh that is NOT the kernel's, as `encoder_ref.gelu_c` is."""
    assert v32.dtype == torch.float32
    err = (got32.double().cpu() - torch.tanh(v32.double().cpu())).abs()
    return float((err / U).max())


def head_bound(case: HeadCase, c: float, factor: float = 2.0) -> torch.Tensor:
    """|got - logit| <= sum_j |wh_j| (factor (hidden + 8) u S_j + c u)  +  factor (hidden + 9) u T, per row:

    * a_j is a sum of `hidden` products and a bias in f32: off by at most `sum_bound(hidden, S_j)` = factor (hidden + 8) u S_j whatever the
      order (the kernel's chain, butterfly and bias are hidden / 64 * 4 + 7 additions deep; the fmas only remove roundings).  The 16-bit
      times 16-bit products are exact in f32.
    * tanh has slope <= 1, so that error reaches p_j undiminished at most, and the float32 tanhf adds its own c u (`tanh_c`: measured,
      never taken from the code under test).  p_j's error enters the logit times |wh_j|.
    * the logit is a sum of `hidden` products wh_j p_j and bh: `sum_bound(hidden + 1, T)` = factor (hidden + 9) u T covers the additions
      (hidden / 32 fmas, 32 additions and bh deep) and the products' own roundings.
    `factor` is 2 for the kernel, as everywhere in encoder_ref (the exact shape of the trees is not part of the contract), and 1 for the
    f32 emulation, which has an order of its own."""
    _, _, S, T = head_f64(case)  # noqa: N806
    wh = case.head_w.double().reshape(-1).abs()
    return (sum_bound(case.hidden, S, factor) + c * U) @ wh + sum_bound(case.hidden + 1, T, factor)


def head_emulated(case: HeadCase) -> torch.Tensor:
    """The kernel's rounding points in float32 on the CPU (torch's own order of summation): (rows,) float32."""
    x, w, b = case.x.float(), case.pooler_w.float(), case.pooler_b.float()
    return torch.tanh(x @ w.T + b) @ case.head_w.float().reshape(-1) + case.head_b.float().reshape(())


def moved_by_bound(got: torch.Tensor, truth: torch.Tensor, bound1: torch.Tensor) -> torch.Tensor:
    """`got` (float64) moved AWAY from the truth by the un-doubled bound's own size: its error is |got - truth| + bound1, which a bound
    that means something refuses wherever got != truth."""
    err = got - truth
    return got + torch.where(err >= 0, 1.0, -1.0) * bound1


def offsets_cases(n_tokens: int = N_TOKENS) -> dict:
    """name -> (seq_offsets as a list of n_seqs + 1 ints, the row each sequence reads or None for an empty one): n_seqs 1, 17 and 300;
    first tokens at 0, 255, 256 (a token-block edge) and n_tokens - 1; one empty sequence; offsets past n_tokens and below 0 (clamped)."""
    last = n_tokens - 1
    out = {}
    for r in (0, 255, 256, last):
        out[f"one-at-{r}"] = ([r, r + 1], [r])
    seventeen = [0, 3, 3, 40, 77, 100, 128, 200, 255, 256, 257, 270, 280, 290, 295, 298, last, n_tokens]  # sequence 1 is empty
    out["seventeen"] = (seventeen, [None if a == b else a for a, b in zip(seventeen, seventeen[1:])])
    out["three-hundred"] = (list(range(n_tokens + 1)), list(range(n_tokens)))
    # (ascending like real offsets, none equal to its neighbour: below 0 reads row 0, at or past n_tokens the last row)
    out["clamped"] = ([-5, n_tokens, n_tokens + 7, 2 ** 31 - 2, 2 ** 31 - 1], [0, last, last, last])
    return out


def bound_is_sane(case: HeadCase, c: float) -> bool:
    """The un-doubled bound stays an order below the scale a logit can have, sum_j |wh_j| + |bh| (|tanh| <= 1): a bound of the size of
    the values would accept everything.  (Not below T: where the pre-activations cancel, their error is large against a small tanh.)"""
    scale = float(case.head_w.double().abs().sum() + case.head_b.double().abs().sum())
    return bool((head_bound(case, c, 1.0) < 1e-1 * scale).all()) and math.isfinite(c)
