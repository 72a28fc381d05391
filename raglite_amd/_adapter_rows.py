"""`rl_adapter_apply_rows` through the C ABI: the query adapter for a batch whose every row must equal the single call.

`rl_adapter_apply` picks its kernels by the number of queries, so a query's bits depend on the batch it arrives in; this entry runs the
single-query scan's arithmetic for every row in one launch.  The wrapper is reached as `_ops.adapter_apply(A, queries, rows=True)`; it
lives outside the `_ops*` modules because every `lib()` call spelled in those is part of the recorded host trace
(tests/test_ops_calls_host.py), which drives them with NumPy arguments on a machine without a device."""

from __future__ import annotations

import numpy as np

from raglite_amd._abi import check, lib
from raglite_amd._ops_frame import _Args


def adapter_apply_rows(A, queries, *, want_f16: bool = False):  # noqa: N803, ANN001, ANN201
    """out[b] = A @ q[b] with, for every b, the bits `_ops.adapter_apply(A, q[b])` gives: a vector or a (B, dim) batch, NumPy arrays
    or CUDA tensors (all on one side), float32 out -- float16 with `want_f16`."""
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
    B = int(q.shape[0])  # noqa: N806
    out, p_o = a.out((B, dim), np.float16 if want_f16 else np.float32)
    a.ensure_device()
    check(lib().rl_adapter_apply_rows(p_a, p_q, B, dim, None if want_f16 else p_o, p_o if want_f16 else None, a.mem, a.stream))
    return out[0] if single else out
