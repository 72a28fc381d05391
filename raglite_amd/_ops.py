"""Thin array-level wrappers over the C ABI.

Every function accepts either NumPy arrays (host pointers: the library stages them through HBM
and the call is synchronous) or `torch` CUDA tensors (device pointers: work is enqueued on torch's
current stream and results come back as CUDA tensors, no synchronisation).  PyTorch is only the
owner of device memory and streams here; no torch kernel runs on the hot path.

This module is the import surface.  The wrappers live beside it, split the way `csrc/api*.hip` is: `_ops_frame` (the per-call frame,
device initialisation, the handle base), `_ops_retrieval`, `_ops_keyword`, `_ops_index` and `_ops_ingestion`, each importing only
from those before it; what belongs to no object (options, `synth_fill`, `adapter_apply`, `topk`, `merge_topk`) is here.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from raglite_amd import _abi
from raglite_amd._abi import MEM_DEVICE, SYNTH_KINDS, check, lib
from raglite_amd._ops_frame import _Args, _current_device, _ensure_init, _is_half, _is_torch, _same_side, _torch, set_device  # noqa: F401
from raglite_amd._ops_index import DeviceIndex  # noqa: F401
from raglite_amd._ops_ingestion import (  # noqa: F401
    _partition_outputs,
    partition_chunklets,
    partition_chunks,
    partition_sentences,
    pool_norm,
    split_chunks_call,
)
from raglite_amd._ops_keyword import DeviceTermIds, KeywordAnalyzer, KeywordIndex, KeywordStore, _term_csr  # noqa: F401
from raglite_amd._ops_retrieval import (  # noqa: F401
    RERANK_MAX_ENTRIES,
    SPANS_MAX_ENTRIES,
    SPANS_MAX_OFFSETS,
    FilterSet,
    MetadataStore,
    SpanTable,
    _rank_limits,
    _span_offsets,
    filter_set,
    pack_bits,
    rerank_order,
    rrf_fuse,
    shard_hybrid_fuse,
)

K_MAX = 2048


# ----------------------------------------------------------------------------------------------
def set_default_option(name: str, value: int) -> None:
    """`rl_set_default_option`: the start value of a route option for every index created AFTERWARDS in this process."""
    check(lib().rl_set_default_option(_abi.option_key(name), int(value)))


def get_default_option(name: str) -> int:
    v = C.c_int64(0)
    check(lib().rl_get_default_option(_abi.option_key(name), C.byref(v)))
    return int(v.value)


def synth_fill(out, seed: int, start: int = 0, kind: str = "uniform"):
    """Fill a float32 CUDA tensor with the counter-based synthetic stream (oracle-identical bits)."""
    a = _Args()
    _, ptr = a.inp(out, np.float32)
    if a.mem != MEM_DEVICE or ptr != out.data_ptr():
        raise ValueError("synth_fill needs a contiguous float32 CUDA tensor")
    a.ensure_device()
    check(lib().rl_synth_fill(ptr, start, out.numel(), seed, SYNTH_KINDS[kind], a.stream))
    return out


def adapter_apply(A, queries, *, want_f16: bool = False, rows: bool = False):
    """a5: out[b] = A @ q[b] (`src/raglite/_search.py:62`).  Accepts a vector or a (B, dim) batch.  `rows`: `rl_adapter_apply_rows`,
    which gives every row of a batch the bits this call gives a single vector (the batched routes multiply with other kernels)."""
    if rows:
        from raglite_amd._adapter_rows import adapter_apply_rows  # (its `lib()` call is not one of this module's: see there)

        return adapter_apply_rows(A, queries, want_f16=want_f16)
    a = _Args()
    A, p_a = a.inp(A, np.float32)  # noqa: N806
    q = queries
    single = q.ndim == 1
    if single:
        q = q.reshape(1, -1)
    q, p_q = a.inp(q, np.float32)
    dim = int(A.shape[0])
    if tuple(A.shape) != (dim, dim) or int(q.shape[1]) != dim:
        raise ValueError("adapter must be (dim, dim) and queries (B, dim)")
    B = int(q.shape[0])
    out, p_o = a.out((B, dim), np.float16 if want_f16 else np.float32)
    a.ensure_device()
    check(lib().rl_adapter_apply(p_a, p_q, B, dim, None if want_f16 else p_o, p_o if want_f16 else None,
                                 a.mem, a.stream))
    return out[0] if single else out


def topk(scores, k: int):
    """Exact top-k per row of a (B, n) score matrix by (score desc, index asc)."""
    a = _Args()
    s2 = scores if scores.ndim == 2 else scores.reshape(1, -1)
    _, p_s = a.inp(s2, np.float32)
    B, n = int(s2.shape[0]), int(s2.shape[1])
    o_s, p_os = a.out((B, k), np.float32)
    o_i, p_oi = a.out((B, k), np.int32)
    a.ensure_device()
    check(lib().rl_topk(p_s, B, n, n, k, p_os, p_oi, a.mem, a.stream))
    return (o_s, o_i) if scores.ndim == 2 else (o_s[0], o_i[0])


def merge_topk(scores, ids, k: int):
    """Merge per-shard lists: scores/ids are (n_lists, B, k_in) -> (B, k)."""
    a = _Args()
    sv, p_s = a.inp(scores, np.float32)
    _, p_i = a.inp(ids, np.int32)
    n_lists, B, k_in = (int(v) for v in sv.shape)
    o_s, p_os = a.out((B, k), np.float32)
    o_i, p_oi = a.out((B, k), np.int32)
    a.ensure_device()
    check(lib().rl_merge_topk(p_s, p_i, n_lists, B, k_in, k, p_os, p_oi, a.mem, a.stream))
    return o_s, o_i
