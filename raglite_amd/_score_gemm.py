"""Wrapper of `rl_score_gemm` (`csrc/api.hip`): the dense score GEMMs of `csrc/score_gemm.hip` and the row-score mode of
`csrc/maxsim_gemm.hip` on the caller's matrices, one named kernel per call."""

from __future__ import annotations

from typing import Any

import numpy as np

from raglite_amd._abi import MEM_DEVICE, SCORE_METRICS, check, lib
from raglite_amd._ops_frame import _Args, _is_torch

KERNELS = {"auto": 0, "128x128": 1, "128x256": 2, "image": 3}  # rl_score_gemm's `kernel`


def _row_stride(out: Any, n_rows: int) -> int:
    """`ld` of a (B, n_rows) float32 view whose rows are contiguous: the distance between two of them, in elements."""
    if _is_torch(out):
        s0, s1 = out.stride()
    else:
        s0, s1 = (int(s) // out.itemsize for s in out.strides)
    if out.shape[1] > 1 and s1 != 1:
        raise ValueError("score_gemm: the rows of out must be contiguous")
    return n_rows if out.shape[0] == 1 else int(s0)


def score_gemm(E: Any, Q: Any, metric: str = "raw", *, row_norm: Any | None = None, row_sumsq: Any | None = None,  # noqa: N803
               split_scale: float = 0.0, kernel: int | str = 0, max_workgroups: int = 0, out: Any | None = None,
               readback: bool = False) -> Any:
    """out[q, r] = metric(E[r] . Q[q]) of rows E (n_rows, dim) and queries Q (B, dim), float32 NumPy arrays or CUDA tensors (all on
    one side).  metric "raw" (the dot), "cosine" (reads `row_norm` = |e| per row), "dot", "l2" (reads `row_sumsq` = |e|^2 per row): the
    caller's norms, used as a search uses the index' own.  split_scale 0: exact fp32 MFMAs; a power of two: the fp16 split with the rows
    scaled by it.  kernel 0 / "auto": as a search over the stored rows chooses; 1 / "128x128", 2 / "128x256": that tile; 3 / "image":
    the GEMM over the pre-split image, built from E first.  max_workgroups: the persistent grid's size (0: the device's CUs).
    `out`, if given, is the (B, n_rows) float32 view written: its rows contiguous, any distance >= n_rows apart; nothing between them
    is touched.  readback: also return (|q|^2, q_scale) as the query-side kernels left them (q_scale None without a split scale)."""
    if metric not in SCORE_METRICS:
        raise ValueError(f"Unsupported metric: {metric}")
    k = KERNELS[kernel] if isinstance(kernel, str) else int(kernel)
    a = _Args()
    e, p_e = a.inp(E, np.float32)
    q, p_q = a.inp(Q, np.float32)
    if e.ndim != 2 or q.ndim != 2 or int(e.shape[1]) != int(q.shape[1]):
        raise ValueError("score_gemm: E must be (n_rows, dim) and Q (B, dim)")
    n, dim, B = int(e.shape[0]), int(e.shape[1]), int(q.shape[0])  # noqa: N806
    p_norm = None if row_norm is None else a.inp(row_norm, np.float32)[1]
    p_sumsq = None if row_sumsq is None else a.inp(row_sumsq, np.float32)[1]
    if out is None:
        out, p_out = a.out((B, n), np.float32)
        ld = n
    else:
        on_device = _is_torch(out)
        ok = (out.is_cuda and str(out.dtype) == "torch.float32") if on_device else (isinstance(out, np.ndarray) and out.dtype == np.float32)
        if not ok or on_device != (a.mem == MEM_DEVICE) or tuple(out.shape) != (B, n):
            raise ValueError(f"score_gemm: out must be a float32 view of shape {(B, n)} on the side of E and Q")
        ld = _row_stride(out, n)
        p_out = out.data_ptr() if on_device else out.ctypes.data
        a.hold(out)
    qss, p_qss = a.out((B,), np.float32) if readback else (None, None)
    qsc, p_qsc = a.out((B,), np.float32) if readback and split_scale != 0.0 else (None, None)
    a.ensure_device()
    check(lib().rl_score_gemm(p_e, n, dim, p_q, B, SCORE_METRICS[metric], p_norm, p_sumsq, float(split_scale), k, int(max_workgroups), p_out,
                              ld, p_qss, p_qsc, a.mem, a.stream))
    return (out, qss, qsc) if readback else out
