"""References and inputs for the variable-length attention kernel (raglite_amd/csrc/attention_varlen.hip), shared by
tests/test_attention_ref_host.py (CPU) and tests/test_gpu_attention_varlen.py.

Two functions over the same inputs:

* `attention_f64`: the float64 restatement -- per sequence and head, softmax(scale q k^T) v from the dtype-rounded inputs -- together with
  A[t, h, c] = sum_j w_j |v[j, h, c]|, the softmax-weighted mean of |v| that the error bound is stated in;
* `attention_emulated`: the kernel's roundings on the CPU -- f32 scores, the online softmax over key sub-tiles of 32 in f32 with the scale
  folded into the exp2 argument, P rounded to the dtype as the operand of P.V only (in bf16 as TWO operands, the rounded value and the
  rounded remainder: `P_SPLIT`), f32 accumulation of O and of the row sums, the output rounded to nearest even.

The bound: rounding P costs at most u A, rounding the output u |out| <= u A, the f32 score / exponent error about 2^-12 A for
|scaled score| <= 64; tests assert |out - truth| <= 2 (2 u + 2^-12) A elementwise (`bound`; the emulation is held to the un-doubled
bound), u = 2^-9 for bf16 and 2^-11 for fp16.  A bf16 rounding reaches 2^-8 relative, so in bf16 the output's rounding alone may use
up 2 u |out|, all but 2^-12 A of the un-doubled bound; that is why the kernel does not round P once there: with the remainder as a
second operand P's rounding costs 2^-16 A, and output rounding (< 2^-8 |out|) + 2^-16 A + the f32 terms stay inside (2^-8 + 2^-12) A.

`cases()` is the one generator of inputs; everything it returns is cached and must be left unchanged."""

from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

HEADS = 3
UNIT_ROUNDOFF = {"bfloat16": 2.0 ** -9, "float16": 2.0 ** -11}
P_SPLIT = {"bfloat16": True, "float16": False}  # P.V takes P as hi + rounded remainder (attention_varlen.hip, Mfma<T>::p_split)
LENGTH_LISTS = {
    "one": [1],
    "tiny": [1, 2, 3],
    "around32": [31, 32, 33],
    "around64": [63, 64, 65],
    "around128": [127, 128, 129],
    "mixed_with_empty": [300, 1, 0, 257],
    "forty_random": [int(x) for x in np.random.default_rng(40).integers(1, 91, size=40)],
}


@dataclass(frozen=True, eq=False)  # (identity is the cache key of the references below)
class Case:
    name: str
    dtype: str  # "bfloat16" | "float16"
    head_dim: int
    lengths: tuple
    max_len: int
    qkv: torch.Tensor  # (n_tokens, 3 * HEADS * head_dim), `dtype`, CPU
    scale: float

    @property
    def offsets(self) -> list:
        return [0, *np.cumsum(self.lengths).tolist()]


def bound(a64: torch.Tensor, dtype: str, factor: float = 2.0) -> torch.Tensor:
    """factor * (2 u + 2^-12) * A, elementwise."""
    return factor * (2.0 * UNIT_ROUNDOFF[dtype] + 2.0 ** -12) * a64


def _make(name: str, dtype: str, head_dim: int, lengths, seed: int, *, q_gain: float = 1.0, spike_at: int | None = None,
          extra_max_len: int = 0) -> Case:
    g = torch.Generator().manual_seed(seed)
    n = int(sum(lengths))
    x = torch.randn((n, 3, HEADS, head_dim), generator=g, dtype=torch.float32)
    x[:, 0] *= q_gain
    if spike_at is not None:
        # One key of the FIRST sequence that every query of it scores 8 +- 8 / sqrt(head_dim) above the mean of the rest (whose scores
        # have a deviation of 1.4): q gets a common component of 1 per channel, the key is 8 / sqrt(head_dim) on every channel.  The running
        # maximum jumps by 4 or more when the key arrives.  Not more than 8: the bound takes the rounding of P as RELATIVE, which holds
        # for P in the dtype's normal range -- exp(-8) = 3.4e-4 is inside fp16's (>= 2^-14 = 6.1e-5), exp(-17) would be a subnormal.
        x[: lengths[0], 0] += 1.0
        x[spike_at, 1] = 8.0 / math.sqrt(head_dim)
    qkv = x.to(getattr(torch, dtype)).reshape(n, 3 * HEADS * head_dim)
    return Case(name, dtype, head_dim, tuple(lengths), max(lengths) + extra_max_len, qkv, head_dim ** -0.5)


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    out = []
    seed = 1000
    for dtype in ("bfloat16", "float16"):
        for head_dim in (32, 64):
            tag = f"{dtype}-d{head_dim}"
            for lname, lengths in LENGTH_LISTS.items():  # standard-normal q, k, v
                seed += 1
                out.append(_make(f"{tag}-{lname}", dtype, head_dim, lengths, seed))
            for lname in ("around128", "mixed_with_empty"):  # q * 8: scores of tens, the running maximum keeps moving
                seed += 1
                out.append(_make(f"{tag}-{lname}-q8", dtype, head_dim, LENGTH_LISTS[lname], seed, q_gain=8.0))
            seed += 1  # a spiked key in the LAST key tile of a 300-token sequence: forces a late rescale of everything accumulated
            out.append(_make(f"{tag}-spike_last_tile", dtype, head_dim, [300, 40], seed, spike_at=290))
            seed += 1  # ... and in the FIRST key tile: the maximum is found at once and never moves again
            out.append(_make(f"{tag}-spike_first_tile", dtype, head_dim, [300, 40], seed, spike_at=3))
            seed += 1  # a max_len larger than needed: more workgroups that exit, the same bits
            out.append(_make(f"{tag}-long_max_len", dtype, head_dim, [70, 33, 5], seed, extra_max_len=200))
    return tuple(out)


def _split(case: Case, dtype):
    n = case.qkv.shape[0]
    x = case.qkv.to(dtype).view(n, 3, HEADS, case.head_dim)
    return x[:, 0], x[:, 1], x[:, 2]  # each (n, HEADS, head_dim)


@functools.lru_cache(maxsize=None)
def attention_f64(case: Case):
    """(out, A), float64 (n_tokens, HEADS, head_dim): exact arithmetic, to float64 rounding, on the dtype-rounded inputs."""
    q, k, v = _split(case, torch.float64)
    out, a = torch.zeros_like(q), torch.zeros_like(q)
    off = case.offsets
    for lo, hi in zip(off[:-1], off[1:]):
        if hi == lo:
            continue
        s = torch.einsum("qhd,khd->hqk", q[lo:hi], k[lo:hi]) * case.scale
        w = torch.softmax(s, dim=-1)
        out[lo:hi] = torch.einsum("hqk,khd->qhd", w, v[lo:hi])
        a[lo:hi] = torch.einsum("hqk,khd->qhd", w, v[lo:hi].abs())
    return out, a


def attention_emulated(case: Case, key_tile: int = 32) -> torch.Tensor:
    """The kernel's arithmetic on the CPU, (n_tokens, HEADS, head_dim) in the case's dtype."""
    dt = getattr(torch, case.dtype)
    q, k, v = _split(case, torch.float32)
    c2 = torch.tensor(case.scale, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    out = torch.zeros(q.shape, dtype=dt)
    off = case.offsets
    for lo, hi in zip(off[:-1], off[1:]):
        if hi == lo:
            continue
        n = hi - lo
        m = torch.full((HEADS, n), -math.inf, dtype=torch.float32)
        l = torch.zeros((HEADS, n), dtype=torch.float32)  # noqa: E741
        o = torch.zeros((HEADS, n, case.head_dim), dtype=torch.float32)
        for k0 in range(lo, hi, key_tile):
            k1 = min(k0 + key_tile, hi)
            t = torch.einsum("qhd,khd->hqk", q[lo:hi], k[k0:k1]) * c2  # f32 scores, scaled in f32
            mn = torch.maximum(m, t.max(dim=-1).values)
            alpha = torch.exp2(m - mn)
            p = torch.exp2(t - mn[..., None])
            l = l * alpha + p.sum(dim=-1)  # noqa: E741
            p_op = p.to(dt).float()
            if P_SPLIT[case.dtype]:
                p_op = p_op + (p - p_op).to(dt).float()  # (the two products accumulate in f32)
            o = o * alpha[..., None] + torch.einsum("hqk,khd->hqd", p_op, v[k0:k1])
            m = mn
        out[lo:hi] = (o * (1.0 / l)[..., None]).permute(1, 0, 2).to(dt)
    return out


def sdpa_per_sequence(case: Case, dtype=torch.float64, device="cpu") -> torch.Tensor:
    """torch's scaled_dot_product_attention, one call per sequence, in `dtype` on `device`: (n_tokens, HEADS, head_dim)."""
    from torch.nn import functional as F  # noqa: N812

    n = case.qkv.shape[0]
    x = case.qkv.to(device=device, dtype=dtype).view(n, 3, HEADS, case.head_dim)
    out = torch.zeros((n, HEADS, case.head_dim), dtype=dtype, device=device)
    off = case.offsets
    for lo, hi in zip(off[:-1], off[1:]):
        if hi > lo:
            q, k, v = (x[lo:hi, i].transpose(0, 1)[None] for i in range(3))
            out[lo:hi] = F.scaled_dot_product_attention(q, k, v, scale=case.scale)[0].transpose(0, 1)
    return out
