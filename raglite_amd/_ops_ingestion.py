"""Wrappers of `csrc/api_ingest.hip`: pooling and the document-batched splitter calls."""

from __future__ import annotations

from typing import Any

import numpy as np

from raglite_amd._abi import check, lib
from raglite_amd._ops_frame import _Args, _is_torch, _torch


def pool_norm(tokens, span_begin, span_end, *, normalize: bool = True, eps: float = 0.0,
              want_f32: bool = False, want_f16: bool = True):
    """a1+a2(+a3): mean-pool token rows [b, e) per span, L2-normalise, cast.  Returns (f32|None, f16|None).

    Mirrors `src/raglite/_embed.py:131-140` (eps == 0) and `:154-164` (eps > 0)."""
    a = _Args()
    tok, p_tok = a.inp(tokens, np.float32)
    begin, p_b = a.inp(span_begin, np.int64)
    end, p_e = a.inp(span_end, np.int64)
    if tok.ndim != 2:
        raise ValueError("tokens must be a (T, dim) matrix")
    n_rows, dim = int(tok.shape[0]), int(tok.shape[1])
    n_spans = int(begin.shape[0])
    if int(end.shape[0]) != n_spans:
        raise ValueError("span_begin and span_end must have the same length")
    o32, p32 = a.out((n_spans, dim), np.float32) if want_f32 else (None, None)
    o16, p16 = a.out((n_spans, dim), np.float16) if want_f16 else (None, None)
    a.ensure_device()
    check(lib().rl_pool_norm(p_tok, n_rows, dim, p_b, p_e, n_spans, int(normalize), float(eps), p32, p16,
                             a.mem, a.stream))
    return o32, o16


def _partition_outputs(a: _Args, n: int, n_docs: int, want_objective: bool = True) -> tuple[tuple[Any, Any, Any], tuple | None]:
    """The outputs of a document-batched partition call on the side of `a`: (cut uint8[n], objective float64[n_docs] or None, status
    int32[n_docs]) and their pointers.  The pointers are None when n == 0: the call would write nothing (every document is empty and
    has no cut), so the outputs are filled here and the caller returns them as they are."""
    cut, p_cut = a.out((n,), np.uint8)
    obj, p_obj = a.out((max(n_docs, 0),), np.float64) if want_objective else (None, None)
    status, p_status = a.out((max(n_docs, 0),), np.int32)
    if n == 0 and n_docs >= 0:
        if obj is not None:
            obj[...] = 0.0
        status[...] = 0
        return (cut, obj, status), None
    a.ensure_device()
    return (cut, obj, status), (p_cut, p_obj, p_status)


def partition_chunks(cost: Any, sizes: Any, doc_offsets: Any, max_size: int) -> tuple[Any, Any, Any]:
    """`rl_partition_chunks`: the optimal cuts of many documents in one call.  cost float32[n] (the layout `rl_partition_similarity`
    writes), sizes int64[n], doc_offsets int64[n_docs + 1] -> (cut uint8[n], objective float64[n_docs], status int32[n_docs]) on the
    side of `cost`."""
    a = _Args()
    cv, p_cost = a.inp(cost, np.float32)
    n = int(cv.shape[0])
    sv, p_sizes = a.same_side(sizes, np.int64)
    off, p_off = a.same_side(doc_offsets, np.int64)
    n_docs = int(off.shape[0]) - 1
    if int(sv.shape[0]) != n:
        raise ValueError("partition_chunks: cost and sizes differ in length")
    out, ptrs = _partition_outputs(a, n, n_docs)
    if ptrs is not None:
        check(lib().rl_partition_chunks(p_cost, p_sizes, p_off, n, n_docs, int(max_size), *ptrs, a.mem, a.stream))
    return out


def partition_chunklets(boundary: Any, statements: Any, lengths: Any, doc_offsets: Any, max_size: int,
                        want_objective: bool = True) -> tuple[Any, Any, Any]:
    """`rl_partition_chunklets`: the chunklet cuts of many documents in one call.  boundary / statements float64[n], lengths int64[n],
    doc_offsets int64[n_docs + 1] -> (cut uint8[n], objective float64[n_docs] or None, status int32[n_docs]) on the side of
    `boundary`."""
    a = _Args()
    bv, p_b = a.inp(boundary, np.float64)
    n = int(bv.shape[0])
    sv, p_s = a.same_side(statements, np.float64)
    lv, p_len = a.same_side(lengths, np.int64)
    if int(lv.shape[0]) != n or int(sv.shape[0]) != n:
        raise ValueError("partition_chunklets: boundary, statements and lengths differ in length")
    off, p_off = a.same_side(doc_offsets, np.int64)
    n_docs = int(off.shape[0]) - 1
    out, ptrs = _partition_outputs(a, n, n_docs, want_objective)
    if ptrs is not None:
        check(lib().rl_partition_chunklets(p_b, p_s, p_len, p_off, n, n_docs, int(max_size), *ptrs, a.mem, a.stream))
    return out


def partition_sentences(codepoints: Any, probas: Any, doc_offsets: Any, min_len: int = 4, max_len: int | None = None,
                        known: Any | None = None, want_objective: bool = True) -> tuple[Any, Any, Any]:
    """`rl_partition_sentences`: the sentence cuts of many documents in one call.  codepoints uint32[n] (a CUDA tensor: uint32 or
    int32, the same bits), probas float32[n] or float64[n] (other dtypes are widened to float64), doc_offsets int64[n_docs + 1],
    known float64[n] or None -> (cut uint8[n], objective float64[n_docs] or None, status int32[n_docs]) on the side of `probas`."""
    if min_len < 1 or (max_len is not None and max_len < 1):
        raise ValueError("partition_sentences: min_len >= 1 and max_len >= 1 (or None) are required")
    a = _Args()
    if _is_torch(probas):
        f64 = probas.dtype != _torch().float32
    else:
        probas = np.asarray(probas)
        f64 = probas.dtype != np.float32
    pv, p_p = a.inp(probas, np.float64 if f64 else np.float32)
    n = int(pv.shape[0])
    if _is_torch(codepoints):
        torch = _torch()
        if codepoints.dtype not in (torch.int32, torch.uint32):
            codepoints = codepoints.to(torch.int32)  # code points are below 2^21
        cp, p_cp = a.inp(codepoints.view(torch.int32), np.int32)
    else:
        cp, p_cp = a.same_side(np.ascontiguousarray(codepoints, dtype=np.uint32).view(np.int32), np.int32)
    kv, p_known = a.same_side(known, np.float64) if known is not None else (None, None)
    if int(cp.shape[0]) != n or (kv is not None and int(kv.shape[0]) != n):
        raise ValueError("partition_sentences: codepoints, probas and known differ in length")
    off, p_off = a.same_side(doc_offsets, np.int64)
    n_docs = int(off.shape[0]) - 1
    out, ptrs = _partition_outputs(a, n, n_docs, want_objective)
    if ptrs is not None:
        check(lib().rl_partition_sentences(p_cp, p_p, int(f64), p_known, p_off, n, n_docs, int(min_len), int(max_len or 0), *ptrs,
                                           a.mem, a.stream))
    return out


def split_chunks_call(embeddings: Any, doc_offsets: Any, nonoutlying: Any, is_heading: Any, sizes: Any, max_size: int,
                      want_cost: bool = False) -> tuple[Any, Any, Any, Any]:
    """`rl_split_chunks`: similarities -> heading adjustments -> partition for many documents in one call.  embeddings (n, dim);
    nonoutlying / is_heading uint8[n] or None -> (cut, cost or None, objective, status) on the side of `embeddings`."""
    a = _Args()
    x, p_x = a.inp(embeddings, np.float32)
    if x.ndim != 2:
        raise ValueError("split_chunks_call: embeddings must be (n, dim)")
    n, dim = int(x.shape[0]), int(x.shape[1])
    off, p_off = a.same_side(doc_offsets, np.int64)
    n_docs = int(off.shape[0]) - 1
    p_sel = a.same_side(nonoutlying, np.uint8)[1] if nonoutlying is not None else None
    p_head = a.same_side(is_heading, np.uint8)[1] if is_heading is not None else None
    sv, p_sizes = a.same_side(sizes, np.int64)
    if int(sv.shape[0]) != n or any(v is not None and len(v) != n for v in (nonoutlying, is_heading)):
        raise ValueError("split_chunks_call: sizes / flags do not match the embedding rows")
    cost, p_cost = a.out((n,), np.float32) if want_cost else (None, None)
    (cut, obj, status), ptrs = _partition_outputs(a, n, n_docs)
    if ptrs is not None:
        check(lib().rl_split_chunks(p_x, n, dim, p_off, n_docs, p_sel, p_head, p_sizes, int(max_size), ptrs[0], p_cost, *ptrs[1:],
                                    a.mem, a.stream))
    return cut, cost, obj, status
