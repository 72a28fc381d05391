"""Variable-length attention forward through the C ABI (`rl_attention_varlen`, raglite_amd/csrc/attention_varlen.hip):
the attention of the packed encoder forward (`_torch_embedder.py`).  CUDA tensors only -- bf16 has no NumPy form -- so the wrapper lives
here, like those of `_comm.py`, and not among the `_ops*` wrappers that take either side."""

from __future__ import annotations

import math
from typing import Any

from raglite_amd._abi import ATTN_DTYPES, MEM_DEVICE, check, lib
from raglite_amd._ops_frame import _Args, _is_torch

HEAD_DIMS = (32, 64)


def attention_varlen_supports(dtype: Any, head_dim: int) -> bool:
    """Does the kernel cover this element type (a torch dtype) and head width?"""
    return str(dtype).split(".")[-1] in ATTN_DTYPES and head_dim in HEAD_DIMS


def attention_varlen(qkv: Any, seq_offsets: Any, max_len: int, heads: int, *, scale: float | None = None) -> Any:
    """Non-causal softmax attention over a packed batch, every token attending to its own sequence only.

    qkv: (n_tokens, 3 * heads * head_dim) CUDA tensor, bf16 or fp16 -- the fused QKV projection of `(n_tokens, hidden)`, read in place;
    seq_offsets: int32 CUDA tensor of n_seqs + 1 ascending offsets from 0 to n_tokens; max_len: a host integer >= every sequence length
    (it sizes the grid: nothing waits for the device); scale: default head_dim ** -0.5.  Returns (n_tokens, heads * head_dim) in qkv's
    dtype, enqueued on torch's current stream."""
    if not (_is_torch(qkv) and qkv.is_cuda and _is_torch(seq_offsets) and seq_offsets.is_cuda):
        raise ValueError("attention_varlen takes CUDA tensors only")
    import torch

    name = str(qkv.dtype).split(".")[-1]
    if name not in ATTN_DTYPES:
        raise ValueError("attention_varlen: qkv must be bfloat16 or float16")
    if qkv.dim() != 2 or heads < 1 or qkv.shape[1] % (3 * heads):
        raise ValueError("attention_varlen: qkv must be (n_tokens, 3 * heads * head_dim)")
    if seq_offsets.dtype != torch.int32 or seq_offsets.dim() != 1 or seq_offsets.numel() < 1:
        raise ValueError("attention_varlen: seq_offsets must be a 1-d int32 tensor of n_seqs + 1 offsets")
    n_tokens, head_dim = int(qkv.shape[0]), int(qkv.shape[1]) // (3 * heads)
    a = _Args.on(MEM_DEVICE, qkv.device)
    qkv = qkv.contiguous()
    if qkv.data_ptr() % 16:
        qkv = qkv.clone()
    seq_offsets = seq_offsets.to(qkv.device).contiguous()
    out = torch.empty((n_tokens, heads * head_dim), dtype=qkv.dtype, device=qkv.device)
    a.hold(qkv, seq_offsets, out)
    a.ensure_device()
    scale = float(scale) if scale is not None else 1.0 / math.sqrt(head_dim)
    check(lib().rl_attention_varlen(qkv.data_ptr(), seq_offsets.data_ptr(), int(seq_offsets.numel()) - 1, n_tokens, int(max_len), int(heads),
                                    head_dim, ATTN_DTYPES[name], scale, out.data_ptr(), MEM_DEVICE, a.stream))
    return out
