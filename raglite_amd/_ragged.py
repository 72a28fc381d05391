"""Wrappers of the ragged MaxSim rerank (`rl_maxsim_rerank_ragged`, `rl_search_rerank_ragged`, `rl_search_rerank_spans_ragged`;
DESIGN.md 4.22): the calls of a `DeviceIndex` that take one (nq_b, dim) matrix of token vectors PER QUERY, of any length, where
`DeviceIndex.maxsim_rerank`, `search_rerank` and `search_rerank_spans` take one (B, nq, dim) block."""

from __future__ import annotations

from typing import Any, Sequence

import numpy as np

from raglite_amd._abi import check, lib
from raglite_amd._ops_frame import _Args, _is_torch, _torch
from raglite_amd._ops_index import DeviceIndex
from raglite_amd._ops_keyword import KeywordIndex, _term_csr_args
from raglite_amd._ops_retrieval import SPANS_MAX_ENTRIES, SpanTable, _span_offsets


def pack_vectors(vecs: Sequence[Any], dim: int | None = None) -> tuple[Any, np.ndarray]:
    """A list of (nq_b, dim) matrices -> (their rows in one (sum nq_b, dim) float32 matrix, offsets (B + 1,) int64): query b owns rows
    offsets[b] .. offsets[b + 1] - 1.  NumPy matrices give a NumPy matrix, CUDA tensors a CUDA tensor (one side per call); the offsets
    are NumPy either way (the library reads them on the host)."""
    vecs = list(vecs)
    for v in vecs:
        if getattr(v, "ndim", None) != 2:
            raise ValueError("every query's token vectors must be a 2-D (nq, dim) matrix")
    dims = {int(v.shape[1]) for v in vecs} | ({int(dim)} if dim is not None else set())
    if len(dims) > 1:
        raise ValueError(f"every query's token vectors must be (nq, dim) with the same dim, got dims {sorted(dims)}")
    offsets = np.zeros(len(vecs) + 1, dtype=np.int64)
    np.cumsum([int(v.shape[0]) for v in vecs], out=offsets[1:])
    if vecs and all(_is_torch(v) for v in vecs):
        torch = _torch()
        return torch.cat([v.to(torch.float32) for v in vecs]).contiguous(), offsets
    if any(_is_torch(v) for v in vecs):
        raise ValueError("all array arguments of one call must be NumPy arrays or all CUDA tensors")
    width = dims.pop() if dims else 0
    flat = np.concatenate([np.asarray(v, dtype=np.float32) for v in vecs]) if vecs else np.zeros((0, width), np.float32)
    return np.ascontiguousarray(flat, dtype=np.float32), offsets


def _flat_vectors(index: DeviceIndex, a: _Args, vecs: Sequence[Any], n_queries: int | None = None):
    """The packed vectors as the call's arguments: (pointer, offsets array, B)."""
    flat, offsets = pack_vectors(vecs, index.dim)
    B = int(offsets.size) - 1
    if n_queries is not None and B != n_queries:
        raise ValueError("one (nq, dim) matrix of token vectors per query is required")
    if B and int(np.diff(offsets).min()) < 1:
        raise ValueError("every query needs at least one token vector")
    _, p_v = a.inp(flat, np.float32)
    a.hold(offsets)
    return p_v, offsets, B


def maxsim_rerank_ragged(device_index: DeviceIndex, vecs: Sequence[Any], cand):
    """`rl_maxsim_rerank_ragged`: vecs[b] (nq_b, dim), candidates (B, n_cand) int32 -> scores (B, n_cand) float32.  Row b equals
    `device_index.maxsim_rerank(vecs[b][None], cand[b][None])[0]` bit for bit where nq_b <= 32, and the float32 sum, in order, of that
    call over the slabs of 32 of vecs[b] beyond."""
    a = _Args()
    p_v, offsets, B = _flat_vectors(device_index, a, vecs)
    cv, p_c = a.inp(cand, np.int32)
    if cv.ndim != 2 or int(cv.shape[0]) != B:
        raise ValueError("candidates must be (n_queries, n_cand)")
    n_cand = int(cv.shape[1])
    o_s, p_s = a.out((B, n_cand), np.float32)
    device_index._prep(a)  # noqa: SLF001
    check(lib().rl_maxsim_rerank_ragged(device_index._handle, p_v, offsets.ctypes.data, B, p_c, n_cand, p_s, a.mem, a.stream))  # noqa: SLF001
    return o_s


def _search_rerank_args(device_index: DeviceIndex, a: _Args, queries, vecs, keyword, query_term_ids, weights, chunk_filter, rank_limit,
                        query_filters):
    """`DeviceIndex._search_rerank_args` with the packed vectors and their offsets in place of the (B, nq, dim) block."""
    p_q, B, single = device_index._queries(a, queries)  # noqa: SLF001
    if single:
        raise ValueError("queries must be (n_queries, dim)")
    p_v, offsets, _ = _flat_vectors(device_index, a, vecs, B)
    if query_filters is None and (rank_limit is None or np.ndim(rank_limit) == 0):  # (one filter for the batch: every query maps to it)
        query_filters = None if chunk_filter is None else [chunk_filter] * B
        chunk_filter = None
        if query_filters is None and rank_limit:
            query_filters = [None] * B
    if query_filters is None:
        args = (None, 0, None, None)
    else:
        _, args = device_index._per_query(a, B, chunk_filter, query_filters, rank_limit)  # noqa: SLF001
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).ravel()[: 2 if keyword is not None else 1])
    p_off, p_terms = (None, None) if keyword is None else _term_csr_args(a, query_term_ids, B)
    return p_q, B, p_v, offsets, p_off, p_terms, args, w


def search_rerank_ragged(device_index: DeviceIndex, queries, num_hits: int, n_each: int, n_cand: int, vecs: Sequence[Any], k: int, *,
                         keyword: "KeywordIndex | None" = None, query_term_ids=None, weights=(0.75, 0.25), rrf_k: int = 60,
                         chunk_filter=None, rank_limit=None, query_filters=None):
    """`rl_search_rerank_ragged`: `DeviceIndex.search_rerank` with vecs[b] (nq_b, dim) per query: the hybrid search, then
    `maxsim_rerank_ragged` of each query's fused candidates, then `rerank_order`'s first k, on one stream.  Returns (MaxSim scores
    (B, k) float32, chunk ordinals (B, k) int32 best first, counts (B,) int32)."""
    a = _Args()
    p_q, B, p_v, offsets, p_off, p_terms, args, w = _search_rerank_args(device_index, a, queries, vecs, keyword, query_term_ids, weights,
                                                                        chunk_filter, rank_limit, query_filters)
    o_s, p_s = a.out((B, int(k)), np.float32)
    o_c, p_c = a.out((B, int(k)), np.int32)
    o_n, p_n = a.out((B,), np.int32)
    device_index._prep(a)  # noqa: SLF001
    check(lib().rl_search_rerank_ragged(device_index._handle, None if keyword is None else keyword._handle, p_q, B, int(num_hits),  # noqa: SLF001
                                        int(n_each), p_off, p_terms, *args, w.ctypes.data, int(rrf_k), int(n_cand), p_v, offsets.ctypes.data,
                                        int(k), p_s, p_c, p_n, a.call_mem, a.stream))
    return o_s, o_c, o_n


def search_rerank_spans_ragged(device_index: DeviceIndex, queries, num_hits: int, n_each: int, n_cand: int, vecs: Sequence[Any], k: int,
                               spans: "SpanTable", neighbors=(-1, 1), *, keyword: "KeywordIndex | None" = None, query_term_ids=None,
                               weights=(0.75, 0.25), rrf_k: int = 60, chunk_filter=None, rank_limit=None, query_filters=None):
    """`rl_search_rerank_spans_ragged`: `search_rerank_ragged`'s pipeline, then `spans.chunk_spans` of each query's reranked first k on
    the same stream.  Returns what `DeviceIndex.search_rerank_spans` returns."""
    offs = _span_offsets(neighbors)
    E = int(k) * (1 + int(offs.size))
    if int(k) < 1 or E > SPANS_MAX_ENTRIES:
        raise ValueError(f"search_rerank_spans_ragged: need k >= 1 and k * (1 + len(neighbors)) <= {SPANS_MAX_ENTRIES}")
    a = _Args()
    p_q, B, p_v, offsets, p_off, p_terms, args, w = _search_rerank_args(device_index, a, queries, vecs, keyword, query_term_ids, weights,
                                                                        chunk_filter, rank_limit, query_filters)
    o_tc, p_tc = a.out((B, int(k)), np.int32)
    o_tn, p_tn = a.out((B,), np.int32)
    o_c, p_oc = a.out((B, E), np.int32)
    o_l, p_ol = a.out((B, E), np.int32)
    o_s, p_os = a.out((B, E), np.float64)
    o_ns, p_ns = a.out((B,), np.int32)
    o_nc, p_nc = a.out((B,), np.int32)
    device_index._prep(a)  # noqa: SLF001
    check(lib().rl_search_rerank_spans_ragged(device_index._handle, None if keyword is None else keyword._handle, p_q, B,  # noqa: SLF001
                                              int(num_hits), int(n_each), p_off, p_terms, *args, w.ctypes.data, int(rrf_k), int(n_cand),
                                              p_v, offsets.ctypes.data, int(k), spans._handle,  # noqa: SLF001
                                              offs.ctypes.data if offs.size else None, int(offs.size), p_tc, p_tn, p_oc, p_ol, p_os, p_ns,
                                              p_nc, a.call_mem, a.stream))
    return o_tc, o_tn, o_c, o_l, o_s, o_ns, o_nc
