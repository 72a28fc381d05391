"""Thin array-level wrappers over the C ABI.

Every function accepts either NumPy arrays (host pointers: the library stages them through HBM
and the call is synchronous) or `torch` CUDA tensors (device pointers: work is enqueued on torch's
current stream and results come back as CUDA tensors, no synchronisation).  PyTorch is only the
owner of device memory and streams here; no torch kernel runs on the hot path.
"""

from __future__ import annotations

import ctypes as C
import threading
from typing import Any

import numpy as np

from raglite_amd import _abi
from raglite_amd._abi import MEM_DEVICE, MEM_FILTERS_DEVICE, MEM_HOST, METRICS, SYNTH_KINDS, check, lib

K_MAX = 2048


def _is_torch(x: Any) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


def _torch():
    import torch

    return torch


def _is_half(x: Any) -> bool:
    """IEEE fp16 data (NumPy float16 or torch.float16)?"""
    if _is_torch(x):
        return x.dtype == _torch().float16
    return getattr(x, "dtype", None) == np.float16


class _Args:
    """Collects the pointers of one call and enforces that they all live on the same side."""

    def __init__(self) -> None:
        self.mem: int | None = None
        self.device = None
        self.keep: list[Any] = []
        self.filters_flag = 0  # MEM_FILTERS_DEVICE once the call's filter table is a `FilterSet` (device memory whatever the rest is)

    @property
    def call_mem(self) -> int:
        """`mem` of a call that takes filters."""
        return self.mem | self.filters_flag

    def _side(self, mem: int, device=None) -> None:
        if self.mem is None:
            self.mem, self.device = mem, device
        elif self.mem != mem:
            raise ValueError("all array arguments of one call must be NumPy arrays or all CUDA tensors")

    def inp(self, x: Any, dtype: np.dtype) -> int:
        if _is_torch(x):
            torch = _torch()
            if not x.is_cuda:
                raise ValueError("torch tensors passed to raglite_amd must live on a CUDA (HIP) device")
            t = x.to(getattr(torch, np.dtype(dtype).name)).contiguous()
            self._side(MEM_DEVICE, t.device)
            self.keep.append(t)
            return t.data_ptr()
        a = np.ascontiguousarray(x, dtype=dtype)
        self._side(MEM_HOST)
        self.keep.append(a)
        return a.ctypes.data

    def out(self, shape: tuple[int, ...], dtype: np.dtype) -> tuple[Any, int]:
        if self.mem == MEM_DEVICE:
            torch = _torch()
            t = torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device=self.device)
            self.keep.append(t)
            return t, t.data_ptr()
        a = np.empty(shape, dtype=dtype)
        self.keep.append(a)
        return a, a.ctypes.data

    @property
    def stream(self) -> int:
        if self.mem == MEM_DEVICE:
            return _torch().cuda.current_stream(self.device).cuda_stream
        return 0

    def ensure_device(self) -> None:
        """Make the HIP device current for this thread (ctypes calls run on the caller's thread)."""
        dev = self.device.index if (self.mem == MEM_DEVICE and self.device.index is not None) else _current_device()
        _ensure_init(dev)


_tls = threading.local()


def _current_device() -> int:
    return getattr(_tls, "device", 0)


def _ensure_init(device: int) -> None:
    if getattr(_tls, "initialised", None) != device:
        _abi.init(device)
        _tls.initialised = device
        _tls.device = device


def set_device(device: int) -> None:
    """Select the GPU used by host-array calls made from this thread."""
    _tls.device = device
    _ensure_init(device)


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
    ptr = a.inp(out, np.float32)
    if a.mem != MEM_DEVICE or a.keep[0].data_ptr() != out.data_ptr():
        raise ValueError("synth_fill needs a contiguous float32 CUDA tensor")
    a.ensure_device()
    check(lib().rl_synth_fill(ptr, start, out.numel(), seed, SYNTH_KINDS[kind], a.stream))
    return out


def pool_norm(tokens, span_begin, span_end, *, normalize: bool = True, eps: float = 0.0,
              want_f32: bool = False, want_f16: bool = True):
    """a1+a2(+a3): mean-pool token rows [b, e) per span, L2-normalise, cast.  Returns (f32|None, f16|None).

    Mirrors `src/raglite/_embed.py:131-140` (eps == 0) and `:154-164` (eps > 0)."""
    a = _Args()
    p_tok = a.inp(tokens, np.float32)
    p_b = a.inp(span_begin, np.int64)
    p_e = a.inp(span_end, np.int64)
    tok = a.keep[0]
    if tok.ndim != 2:
        raise ValueError("tokens must be a (T, dim) matrix")
    n_rows, dim = int(tok.shape[0]), int(tok.shape[1])
    n_spans = int(a.keep[1].shape[0])
    if int(a.keep[2].shape[0]) != n_spans:
        raise ValueError("span_begin and span_end must have the same length")
    o32, p32 = a.out((n_spans, dim), np.float32) if want_f32 else (None, None)
    o16, p16 = a.out((n_spans, dim), np.float16) if want_f16 else (None, None)
    a.ensure_device()
    check(lib().rl_pool_norm(p_tok, n_rows, dim, p_b, p_e, n_spans, int(normalize), float(eps), p32, p16,
                             a.mem, a.stream))
    return o32, o16


def adapter_apply(A, queries, *, want_f16: bool = False):
    """a5: out[b] = A @ q[b] (`src/raglite/_search.py:62`).  Accepts a vector or a (B, dim) batch."""
    a = _Args()
    p_a = a.inp(A, np.float32)
    q = queries
    single = q.ndim == 1
    if single:
        q = q.reshape(1, -1)
    p_q = a.inp(q, np.float32)
    dim = int(a.keep[0].shape[0])
    if tuple(a.keep[0].shape) != (dim, dim) or int(a.keep[1].shape[1]) != dim:
        raise ValueError("adapter must be (dim, dim) and queries (B, dim)")
    B = int(a.keep[1].shape[0])
    out, p_o = a.out((B, dim), np.float16 if want_f16 else np.float32)
    a.ensure_device()
    check(lib().rl_adapter_apply(p_a, p_q, B, dim, None if want_f16 else p_o, p_o if want_f16 else None,
                                 a.mem, a.stream))
    return out[0] if single else out


def topk(scores, k: int):
    """Exact top-k per row of a (B, n) score matrix by (score desc, index asc)."""
    a = _Args()
    s2 = scores if scores.ndim == 2 else scores.reshape(1, -1)
    p_s = a.inp(s2, np.float32)
    B, n = int(s2.shape[0]), int(s2.shape[1])
    o_s, p_os = a.out((B, k), np.float32)
    o_i, p_oi = a.out((B, k), np.int32)
    a.ensure_device()
    check(lib().rl_topk(p_s, B, n, n, k, p_os, p_oi, a.mem, a.stream))
    return (o_s, o_i) if scores.ndim == 2 else (o_s[0], o_i[0])


def merge_topk(scores, ids, k: int):
    """Merge per-shard lists: scores/ids are (n_lists, B, k_in) -> (B, k)."""
    a = _Args()
    p_s = a.inp(scores, np.float32)
    p_i = a.inp(ids, np.int32)
    n_lists, B, k_in = (int(v) for v in a.keep[0].shape)
    o_s, p_os = a.out((B, k), np.float32)
    o_i, p_oi = a.out((B, k), np.int32)
    a.ensure_device()
    check(lib().rl_merge_topk(p_s, p_i, n_lists, B, k_in, k, p_os, p_oi, a.mem, a.stream))
    return o_s, o_i


def rrf_fuse(lists, weights, *, rrf_k: int = 60, k: int):
    """Weighted Reciprocal Rank Fusion (`rl_rrf_fuse`): the reference's `reciprocal_rank_fusion` (`src/raglite/_search.py:233-252`)
    for a batch, bit for bit.  `lists`: (R, B, len) chunk ordinals, or a sequence of R (B, len) arrays, R <= 4, R * len <= 4096,
    padded with entries < 0; `weights`: R finite floats.  Returns (scores (B, k) float64, ordinals (B, k) int32, counts (B,) int32),
    by score descending, ties by first occurrence; unfilled slots are (-inf, -1)."""
    if isinstance(lists, (list, tuple)):
        lists = _torch().stack(list(lists)) if lists and _is_torch(lists[0]) else np.stack([np.asarray(x) for x in lists])
    a = _Args()
    p_l = a.inp(lists, np.int32)
    if a.keep[0].ndim != 3:
        raise ValueError("lists must be (n_lists, n_queries, len)")
    R, B, L = (int(v) for v in a.keep[0].shape)
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).ravel())  # (host memory, whatever side the lists are on)
    if w.size != R:
        raise ValueError("one weight per list is required")
    if not (-(1 << 31) <= int(rrf_k) < (1 << 31)) or not (-(1 << 31) <= int(k) < (1 << 31)):
        raise ValueError("rrf_k and k must fit in int32")
    o_s, p_s = a.out((B, k), np.float64)
    o_i, p_i = a.out((B, k), np.int32)
    o_n, p_n = a.out((B,), np.int32)
    a.ensure_device()
    check(lib().rl_rrf_fuse(p_l, R, B, L, w.ctypes.data, int(rrf_k), int(k), p_s, p_i, p_n, a.mem, a.stream))
    return o_s, o_i, o_n


RERANK_MAX_ENTRIES = 4096  # candidates per query that rl_rerank_order sorts (one workgroup's LDS)


def rerank_order(scores, candidates, k: int):
    """`rl_rerank_order`: `MaxSimRanker.rank`'s order for a batch.  `scores` (B, n_cand) float32 and `candidates` (B, n_cand) int32, an
    entry < 0 being padding; per query the real candidates by score descending, NaN as -inf, -0.0 equal to +0.0, equal scores by
    position, padding last.  Returns (scores (B, k) float32 -- the input's bits --, candidates (B, k) int32, positions (B, k) int32 in
    the input list, counts (B,) int32); unfilled slots are (-inf, -1, -1).  1 <= k <= n_cand <= 4096."""
    a = _Args()
    p_s = a.inp(scores, np.float32)
    sv = a.keep[-1]
    p_c = a.inp(candidates, np.int32)
    cv = a.keep[-1]
    if sv.ndim != 2 or cv.ndim != 2 or tuple(sv.shape) != tuple(cv.shape):
        raise ValueError("scores and candidates must both be (n_queries, n_cand)")
    B, n_cand = int(sv.shape[0]), int(sv.shape[1])
    if not 1 <= int(k) <= n_cand <= RERANK_MAX_ENTRIES:
        raise ValueError(f"rerank_order: need 1 <= k <= n_cand <= {RERANK_MAX_ENTRIES} (k={k}, n_cand={n_cand})")
    o_s, p_os = a.out((B, int(k)), np.float32)
    o_c, p_oc = a.out((B, int(k)), np.int32)
    o_p, p_op = a.out((B, int(k)), np.int32)
    o_n, p_on = a.out((B,), np.int32)
    a.ensure_device()
    check(lib().rl_rerank_order(p_s, p_c, B, n_cand, int(k), p_os, p_oc, p_op, p_on, a.mem, a.stream))
    return o_s, o_c, o_p, o_n


SPANS_MAX_ENTRIES = 4096  # n_in * (1 + n_off) per query that rl_chunk_spans handles (one workgroup's LDS)
SPANS_MAX_OFFSETS = 64


def _span_offsets(neighbors) -> np.ndarray:
    offs = np.ascontiguousarray(np.asarray(() if neighbors is None else tuple(neighbors), dtype=np.int64).ravel())
    if offs.size > SPANS_MAX_OFFSETS:
        raise ValueError(f"at most {SPANS_MAX_OFFSETS} neighbour offsets are supported")
    if offs.size and (offs.min() < -(1 << 31) or offs.max() >= (1 << 31)):
        raise ValueError("neighbour offsets must fit in int32")
    return offs.astype(np.int32)


class SpanTable:
    """Where every chunk sits in its document (`rl_span_table`): `doc` and `pos` int32 per chunk ordinal of the `DeviceIndex` it sits
    beside, `doc` the dense number of the chunk's document id in sorted order (< 0: the chunk has no position), `pos` its
    `Chunk.index`."""

    def __init__(self, doc, pos) -> None:
        doc = np.ascontiguousarray(doc, dtype=np.int32).ravel()
        pos = np.ascontiguousarray(pos, dtype=np.int32).ravel()
        if doc.size != pos.size:
            raise ValueError("one (doc, pos) per chunk is required")
        self.n_chunks = int(doc.size)
        _ensure_init(_current_device())
        handle = C.c_void_p()
        check(lib().rl_span_table_create(C.byref(handle), doc.ctypes.data, pos.ctypes.data, self.n_chunks))
        self._handle = handle

    def info(self) -> tuple[int, int, int]:
        """(chunks covered, chunks with a position, device bytes held)."""
        n, live, nbytes = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(lib().rl_span_table_info(self._handle, C.byref(n), C.byref(live), C.byref(nbytes)))
        return int(n.value), int(live.value), int(nbytes.value)

    def close(self) -> None:
        h, self._handle = getattr(self, "_handle", None), None
        if h:
            lib().rl_span_table_destroy(h)

    def __del__(self) -> None:  # noqa: D105
        try:
            self.close()
        except Exception:  # noqa: BLE001,S110 - interpreter shutdown
            pass

    def chunk_spans(self, chunks, neighbors=(-1, 1)):
        """`rl_chunk_spans`: the reference's `retrieve_chunk_spans` (`src/raglite/_search.py:323-361`) on ordinals for a batch.  `chunks`
        (B, n_in) int32, each query's chunks best first; entries < 0, out of range or without a position are skipped and take no rank.
        `neighbors`: the offsets (None or () for none).  With E = n_in * (1 + len(neighbors)) <= 4096, returns (chunks (B, E) int32 --
        the distinct chunks span after span, best span first, ascending index within a span, padded with -1 --, span lengths (B, E)
        int32, span scores (B, E) float64, number of spans (B,) int32, number of chunks (B,) int32)."""
        offs = _span_offsets(neighbors)
        a = _Args()
        p_c = a.inp(chunks, np.int32)
        cv = a.keep[-1]
        if cv.ndim != 2:
            raise ValueError("chunks must be (n_queries, n_in)")
        B, n_in = int(cv.shape[0]), int(cv.shape[1])
        E = n_in * (1 + int(offs.size))
        if n_in < 1 or E > SPANS_MAX_ENTRIES:
            raise ValueError(f"chunk_spans: need n_in >= 1 and n_in * (1 + len(neighbors)) <= {SPANS_MAX_ENTRIES} (n_in={n_in}, "
                             f"{offs.size} offsets)")
        o_c, p_oc = a.out((B, E), np.int32)
        o_l, p_ol = a.out((B, E), np.int32)
        o_s, p_os = a.out((B, E), np.float64)
        o_ns, p_ns = a.out((B,), np.int32)
        o_nc, p_nc = a.out((B,), np.int32)
        a.ensure_device()
        check(lib().rl_chunk_spans(self._handle, p_c, B, n_in, offs.ctypes.data if offs.size else None, int(offs.size), p_oc, p_ol, p_os,
                                   p_ns, p_nc, a.mem, a.stream))
        return o_c, o_l, o_s, o_ns, o_nc


def shard_hybrid_fuse(gathered, *, num_hits: int, n_each: int, keywords: bool, weights, rrf_k: int = 60, k: int):
    """`rl_shard_hybrid_fuse`: the step after the one all-gather of a sharded hybrid batch.  `gathered`: (world, B, W) int32, what every
    rank packed -- num_hits row records (score bits, global row, global chunk), then with `keywords` n_each keyword records (score bits,
    global chunk): W = 3 num_hits (+ 2 n_each).  Returns (scores (B, k) float64, chunk ordinals (B, k) int32, counts (B,) int32) as
    `DeviceIndex.hybrid_search` does; a query with a SHARD_MISSING record comes back poisoned (NaN, -1, 0).  `UnsupportedError` past
    world * num_hits or world * n_each > 4096."""
    a = _Args()
    p_g = a.inp(gathered, np.int32)
    if a.keep[0].ndim != 3:
        raise ValueError("gathered must be (world, n_queries, W)")
    world, B, W = (int(v) for v in a.keep[0].shape)
    R = 2 if keywords else 1
    if W != 3 * int(num_hits) + (2 * int(n_each) if keywords else 0):
        raise ValueError("gathered: W must be 3 num_hits (+ 2 n_each with keywords)")
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).ravel()[:R])  # (host memory, whatever side the records are on)
    if w.size != R:
        raise ValueError("one weight per list is required")
    o_s, p_s = a.out((B, k), np.float64)
    o_c, p_c = a.out((B, k), np.int32)
    o_n, p_n = a.out((B,), np.int32)
    a.ensure_device()
    check(lib().rl_shard_hybrid_fuse(p_g, world, B, int(num_hits), int(n_each), R, w.ctypes.data, int(rrf_k), int(k), p_s, p_c, p_n, a.mem,
                                     a.stream))
    return o_s, o_c, o_n


def _term_csr(query_term_ids) -> tuple[np.ndarray, np.ndarray]:
    """One sequence of term ids per query -> (q_off int64 [B + 1], q_terms int32), each query's ids ascending and distinct."""
    qs = [np.unique(np.asarray(q, dtype=np.int32)) for q in query_term_ids]
    q_off = np.concatenate(([0], np.cumsum([q.size for q in qs]))).astype(np.int64)
    q_terms = np.ascontiguousarray(np.concatenate(qs) if qs else np.zeros(0, np.int32), dtype=np.int32)
    return q_off, q_terms


def pack_bits(mask) -> np.ndarray:
    """Boolean mask (NumPy / torch, any device) -> little-endian uint32 bitset (bit i of word i // 32)."""
    if _is_torch(mask):
        mask = mask.detach().cpu().numpy()
    m = np.asarray(mask)
    if m.dtype == np.uint32 and m.ndim == 1:
        return np.ascontiguousarray(m)
    b = np.packbits(m.astype(bool).ravel(), bitorder="little")
    pad = (-b.size) % 4
    if pad:
        b = np.concatenate([b, np.zeros(pad, np.uint8)])
    return np.ascontiguousarray(b).view(np.uint32)


def filter_set(query_filters, n_chunks: int, B: int) -> tuple[np.ndarray, np.ndarray]:
    """Per-query filters (B entries, each None or a bool mask over chunks / packed uint32 bitset) -> (bitsets uint32 [F, words], one per
    distinct filter -- identical masks are sent once, deduplicated by their packed bits -- and query_filter int32 [B], -1 = no filter)."""
    filters = list(query_filters)
    if len(filters) != B:
        raise ValueError(f"query_filters must have one entry per query ({len(filters)} for {B} queries)")
    words = (n_chunks + 31) // 32
    rows: list[np.ndarray] = []
    seen: dict[tuple, list[int]] = {}  # a cheap fingerprint -> the rows that have it (equal bits are then compared in full)
    query_filter = np.full(B, -1, np.int32)
    by_object: dict[int, int] = {}  # (a mask object shared by many queries is packed once)
    for b, f in enumerate(filters):
        if f is None:
            continue
        if id(f) in by_object:
            query_filter[b] = by_object[id(f)]
            continue
        bits = pack_bits(f)
        if bits.size != words:
            raise ValueError("chunk_filter must have one entry per chunk")
        key = (int(bits.sum(dtype=np.uint64)), int(bits[0]) if words else 0, int(bits[-1]) if words else 0)
        same = [j for j in seen.get(key, ()) if np.array_equal(rows[j], bits)]
        if same:
            j = same[0]
        else:
            j = len(rows)
            seen.setdefault(key, []).append(j)
            rows.append(bits)
        query_filter[b] = by_object[id(f)] = j
    table = np.empty((len(rows), words), np.uint32)
    for j, r in enumerate(rows):
        table[j] = r
    return table, query_filter


def _rank_limits(rank_limit, B: int) -> np.ndarray | None:
    """rank_limit as an int (or None) for every query, or a length-B sequence -> int64 [B] for the *_per_query calls (None: no array)."""
    if rank_limit is None or np.ndim(rank_limit) == 0:
        return None if not rank_limit else np.full(B, int(rank_limit), np.int64)
    lim = np.asarray([0 if r is None else int(r) for r in rank_limit], dtype=np.int64)
    if lim.size != B:
        raise ValueError(f"rank_limit must be an int or have one entry per query ({lim.size} for {B} queries)")
    return lim


class FilterSet:
    """Chunk bitsets on the device (`rl_filter_set`): what `MetadataStore.filters` writes and the *_per_query searches read in place
    (RL_MEM_FILTERS_DEVICE).  `n_filters` rows of `words` uint32 in the layout of `chunk_filters`.  `query_filter` (int32 per query,
    -1: none) maps a batch's queries to rows: `select` gives the set with a map, which `DeviceIndex.search_chunks(query_filters=)` and
    its kin and `KeywordIndex.search(query_filters=)` take in place of a list of masks.  Reused across calls it grows and never
    shrinks, so a warm call allocates nothing."""

    def __init__(self) -> None:
        self._handle = C.c_void_p()  # (null until the first `MetadataStore.filters`)
        self._owner: FilterSet | None = None
        self.n_filters, self.words = 0, 0
        self.query_filter: np.ndarray | None = None

    def select(self, query_filter) -> "FilterSet":
        """This set (not a copy: the same device table) with `query_filter` as its map."""
        view = FilterSet()
        view._owner = self._owner or self  # (the handle stays the owner's: a view of a closed set is an error, not a stale pointer)
        view.n_filters, view.words = self.n_filters, self.words
        view.query_filter = np.ascontiguousarray(query_filter, dtype=np.int32).ravel()
        return view

    def _bits(self) -> int | None:
        p, n, w = C.c_void_p(), C.c_int32(0), C.c_int64(0)
        check(lib().rl_filter_set_bits((self._owner or self)._handle, C.byref(p), C.byref(n), C.byref(w)))
        if (int(n.value), int(w.value)) != (self.n_filters, self.words):
            raise ValueError("FilterSet: the set was written again after this view of it was taken")
        return p.value

    def call_args(self, n_chunks: int, B: int):
        """(device pointer of the table, n_filters, query_filter int32 [B]) for a *_per_query call over `n_chunks` chunks."""
        qf = self.query_filter
        if qf is None or qf.size != B:
            raise ValueError(f"FilterSet.query_filter must have one entry per query ({0 if qf is None else qf.size} for {B} queries)")
        if self.n_filters and self.words != (n_chunks + 31) // 32:
            raise ValueError("chunk_filter must have one entry per chunk")
        if qf.size and (qf.min() < -1 or qf.max() >= self.n_filters):
            raise ValueError("FilterSet.query_filter entries must be -1 or a row of the set")
        return (self._bits() if self.n_filters else None), self.n_filters, qf

    def read(self) -> np.ndarray:
        """A host copy of the table, uint32 [n_filters x words]."""
        out = np.zeros((self.n_filters, self.words), np.uint32)
        if out.size:
            check(lib().rl_filter_set_read((self._owner or self)._handle, out.ctypes.data, MEM_HOST, None))
        return out

    def close(self) -> None:
        h, self._handle = getattr(self, "_handle", None), C.c_void_p()
        if h and getattr(self, "_owner", None) is None:
            lib().rl_filter_set_destroy(h)
        self.n_filters = self.words = 0

    def __del__(self) -> None:  # noqa: D105
        try:
            self.close()
        except Exception:  # noqa: BLE001,S110 - interpreter shutdown
            pass


class MetadataStore:
    """Every chunk's metadata tags on the device (`rl_metadata_store`), beside the `DeviceIndex` whose chunk ordinals it follows:
    `tag_off` int64 [n_chunks + 1] and `tags` int32, each chunk's ids ascending and free of duplicates
    (`raglite_amd._metadata.TagVocabulary.encode_chunks`).  Deleting chunks needs no call; after a compaction the store is made anew."""

    def __init__(self, tag_off, tags) -> None:
        tag_off, tags = self._csr(tag_off, tags)
        _ensure_init(_current_device())
        handle = C.c_void_p()
        check(lib().rl_metadata_store_create(C.byref(handle), tag_off.ctypes.data, tags.ctypes.data, int(tag_off.size - 1), MEM_HOST, None))
        self._handle = handle
        self.n_chunks = int(tag_off.size - 1)

    @staticmethod
    def _csr(tag_off, tags) -> tuple[np.ndarray, np.ndarray]:
        tag_off = np.ascontiguousarray(tag_off, dtype=np.int64)
        tags = np.ascontiguousarray(tags, dtype=np.int32)
        if tag_off.ndim != 1 or tag_off.size < 1 or tags.ndim != 1 or int(tag_off[-1]) != tags.size:
            raise ValueError("MetadataStore: tag_off must hold one entry per chunk plus one and end at len(tags)")
        return tag_off, tags

    def append(self, tag_off, tags) -> None:
        """New chunks at the end (`tag_off` from 0)."""
        tag_off, tags = self._csr(tag_off, tags)
        _ensure_init(_current_device())
        check(lib().rl_metadata_store_append(self._handle, tag_off.ctypes.data, tags.ctypes.data, int(tag_off.size - 1), MEM_HOST, None))
        self.n_chunks += int(tag_off.size - 1)

    def memory(self) -> tuple[int, int]:
        """(device bytes used, device bytes reserved)."""
        out = (C.c_int64 * 2)()
        check(lib().rl_metadata_store_memory(self._handle, out))
        return int(out[0]), int(out[1])

    def filters(self, index: "DeviceIndex", f_off, f_tags, filter_set: FilterSet | None = None):
        """`rl_metadata_filters`: filter j wants the tags f_tags[f_off[j] : f_off[j + 1]].  Returns (the `FilterSet` holding the F
        bitsets -- `filter_set` reused, or a new one --, matching chunks int64 [F], their embedding rows int64 [F]); tombstoned chunks
        count like any other.  One launch and one read-back of 16 bytes per filter."""
        f_off, f_tags = self._csr(f_off, f_tags)
        F = int(f_off.size - 1)
        fs = filter_set if filter_set is not None else FilterSet()
        if fs._owner is not None:  # noqa: SLF001
            raise ValueError("MetadataStore.filters writes a FilterSet itself, not a view of one")
        chunks, rows = np.zeros(F, np.int64), np.zeros(F, np.int64)
        _ensure_init(_current_device())
        check(lib().rl_metadata_filters(self._handle, index._handle, f_off.ctypes.data, f_tags.ctypes.data, F, C.byref(fs._handle),  # noqa: SLF001
                                        chunks.ctypes.data, rows.ctypes.data, MEM_HOST, None))
        fs.n_filters, fs.words = F, (self.n_chunks + 31) // 32
        return fs, chunks, rows

    def close(self) -> None:
        h, self._handle = getattr(self, "_handle", None), None
        if h:
            lib().rl_metadata_store_destroy(h)

    def __del__(self) -> None:  # noqa: D105
        try:
            self.close()
        except Exception:  # noqa: BLE001,S110 - interpreter shutdown
            pass


class DeviceIndex:
    """Device-resident chunk-embedding matrix + chunk CSR: the GPU image of the reference's
    `chunk_embedding` table (`src/raglite/_database.py:403-430`).

    `embeddings`: (n_rows, dim) float32 NumPy array (copied to HBM) or CUDA tensor (borrowed, kept
    alive by this object).  `chunk_offsets`: ascending int64 CSR of length n_chunks+1 (rows of a chunk
    contiguous, `src/raglite/_split_chunks.py:116-122`); None = one row per chunk."""

    def __init__(self, embeddings, chunk_offsets=None, *, metric: str = "cosine", storage: str = "f32") -> None:
        """storage="f16": keep the corpus as IEEE fp16 in HBM (lossless for the reference's data,
        `src/raglite/_embed.py:140`).  float16 input is taken as is, float32 input is rounded to nearest even."""
        if metric not in METRICS:
            raise ValueError(f"Unsupported metric: {metric}")  # wording of src/raglite/_query_adapter.py:207
        if storage not in ("f32", "f16"):
            raise ValueError("storage must be 'f32' or 'f16'")
        self.storage = storage
        a = _Args()
        if storage == "f16":
            if _is_torch(embeddings):
                t = embeddings.to(_torch().float16).contiguous()
                if not t.is_cuda:
                    raise ValueError("torch tensors passed to raglite_amd must live on a CUDA (HIP) device")
                a._side(MEM_DEVICE, t.device)  # noqa: SLF001
                a.keep.append(t)
                p_e = t.data_ptr()
            else:
                h = np.ascontiguousarray(np.asarray(embeddings).astype(np.float16, copy=False))
                a._side(MEM_HOST)  # noqa: SLF001
                a.keep.append(h)
                p_e = h.ctypes.data
        else:
            p_e = a.inp(embeddings, np.float32)
        emb = a.keep[0]
        if emb.ndim != 2:
            raise ValueError("embeddings must be a (n_rows, dim) matrix")
        self.n_rows, self.dim = int(emb.shape[0]), int(emb.shape[1])
        self.metric = metric
        self.mem = a.mem
        self.device = a.device
        self._keep = emb if a.mem == MEM_DEVICE else None
        if chunk_offsets is None:
            off_ptr, n_chunks = None, self.n_rows
            self.chunk_offsets = None
        else:
            off = np.ascontiguousarray(np.asarray(chunk_offsets.cpu() if _is_torch(chunk_offsets) else chunk_offsets),
                                       dtype=np.int64)
            if off.ndim != 1 or off.size < 1:
                raise ValueError("chunk_offsets must be a 1-D array of length n_chunks + 1")
            off_ptr, n_chunks = off.ctypes.data, int(off.size - 1)
            self.chunk_offsets = off
        self.n_chunks = n_chunks
        a.ensure_device()
        handle = C.c_void_p()
        create = lib().rl_index_create_f16 if storage == "f16" else lib().rl_index_create
        check(create(C.byref(handle), p_e, self.n_rows, self.dim, off_ptr, n_chunks, METRICS[metric], a.mem, a.stream))
        self._handle = handle

    def close(self) -> None:
        h, self._handle = getattr(self, "_handle", None), None
        if h:
            lib().rl_index_destroy(h)
        self._keep = None

    def __del__(self) -> None:  # noqa: D105
        try:
            self.close()
        except Exception:  # noqa: BLE001,S110 - interpreter shutdown
            pass

    # -- helpers -------------------------------------------------------------------------------
    def _queries(self, a: _Args, q) -> tuple[int, int, bool]:
        single = q.ndim == 1
        q2 = q.reshape(1, -1) if single else q
        ptr = a.inp(q2, np.float32)
        if int(a.keep[-1].shape[1]) != self.dim:
            raise ValueError(f"query dimension {int(a.keep[-1].shape[1])} != index dimension {self.dim}")
        return ptr, int(a.keep[-1].shape[0]), single

    def _prep(self, a: _Args) -> None:
        if a.mem == MEM_HOST and self.mem == MEM_DEVICE:
            _ensure_init(self.device.index or 0)
        else:
            a.ensure_device()

    def _filter(self, a: _Args, chunk_filter):
        """chunk_filter (bool mask over chunks, or a packed uint32 bitset) -> pointer on the call's side, or None."""
        if chunk_filter is None:
            return None
        bits = pack_bits(chunk_filter)
        if bits.size != (self.n_chunks + 31) // 32:
            raise ValueError("chunk_filter must have one entry per chunk")
        if a.mem == MEM_DEVICE:
            t = _torch().from_numpy(bits.view(np.int32)).to(a.device)
            a.keep.append(t)
            return t.data_ptr()
        a.keep.append(bits)
        return bits.ctypes.data

    def _per_query(self, a: _Args, B: int, chunk_filter, query_filters, rank_limit):
        """The filter arguments of a call that takes per-query filters or limits -> (per_query, args): per_query False keeps the
        single-filter entry point with args (chunk filter pointer, rank limit); True gives (bitsets pointer, n_filters, query_filter
        pointer, rank_limits pointer) for the *_per_query one."""
        if query_filters is None and (rank_limit is None or np.ndim(rank_limit) == 0):
            return False, (self._filter(a, chunk_filter), int(rank_limit or 0))
        if query_filters is not None and chunk_filter is not None:
            raise ValueError("pass chunk_filter (one for the batch) or query_filters (one per query), not both")
        if isinstance(query_filters, FilterSet):  # the table is on the device already: its pointer goes in as it is, with the flag
            p_f, n_filters, qf = query_filters.call_args(self.n_chunks, B)
            lim = _rank_limits(rank_limit, B)
            a.keep += [query_filters, qf, lim]
            a.filters_flag = MEM_FILTERS_DEVICE
            return True, (p_f, n_filters, qf.ctypes.data, None if lim is None else lim.ctypes.data)
        table, qf = filter_set([chunk_filter] * B if query_filters is None else query_filters, self.n_chunks, B)
        lim = _rank_limits(rank_limit, B)
        a.keep += [qf, lim]
        p_f = None
        if len(table):
            if a.mem == MEM_DEVICE:
                t = _torch().from_numpy(table.view(np.int32)).to(a.device)
                a.keep.append(t)
                p_f = t.data_ptr()
            else:
                a.keep.append(table)
                p_f = table.ctypes.data
        return True, (p_f, len(table), qf.ctypes.data, None if lim is None else lim.ctypes.data)

    # -- lifecycle ---------------------------------------------------------------
    def append(self, rows, chunk_sizes=None) -> None:
        """Append embedding rows as new chunks (`insert_documents`, `src/raglite/_insert.py:247-272`): existing
        row / chunk ordinals never change.  chunk_sizes: rows per new chunk (None = one chunk per row)."""
        a = _Args()
        p_r = a.inp(rows, np.float32)
        r = a.keep[0]
        if r.ndim != 2 or int(r.shape[1]) != self.dim:
            raise ValueError("rows must be (n_new_rows, dim)")
        n_new = int(r.shape[0])
        if chunk_sizes is None:
            sizes, p_sz, n_new_chunks = None, None, n_new
        else:
            sizes = np.ascontiguousarray(np.asarray(chunk_sizes), dtype=np.int64)
            p_sz, n_new_chunks = sizes.ctypes.data, int(sizes.size)
        self._prep(a)
        check(lib().rl_index_append(self._handle, p_r, n_new, p_sz, n_new_chunks, a.mem, a.stream))
        if self.chunk_offsets is not None or sizes is not None:
            old = self.chunk_offsets if self.chunk_offsets is not None else np.arange(self.n_rows + 1, dtype=np.int64)
            add = sizes if sizes is not None else np.ones(n_new, np.int64)
            self.chunk_offsets = np.concatenate([old, old[-1] + np.cumsum(add)]).astype(np.int64)
        self.n_rows += n_new
        self.n_chunks += n_new_chunks
        self._keep = None  # the index owns its storage after the first append

    def delete_chunks(self, chunk_ordinals) -> None:
        """Tombstone chunks (`delete_documents`, `src/raglite/_delete.py:148-176`): they never match again."""
        c = np.ascontiguousarray(np.asarray(chunk_ordinals), dtype=np.int64).ravel()
        _ensure_init(self.device.index or 0) if self.mem == MEM_DEVICE else _ensure_init(_current_device())
        check(lib().rl_index_delete_chunks(self._handle, c.ctypes.data, int(c.size), None))

    def compact(self) -> np.ndarray:
        """Reclaim tombstoned chunks (`rl_index_compact`): survivors keep their order and are renumbered 0..live-1.
        Returns remap (old n_chunks,) int64: new ordinal of every old chunk, -1 for a deleted one."""
        _ensure_init(self.device.index or 0) if self.mem == MEM_DEVICE else _ensure_init(_current_device())
        remap = np.empty(self.n_chunks, dtype=np.int64)
        n_rows, n_chunks = C.c_int64(0), C.c_int64(0)
        check(lib().rl_index_compact(self._handle, remap.ctypes.data, C.byref(n_rows), C.byref(n_chunks), None))
        if int(n_chunks.value) != self.n_chunks:
            if self.chunk_offsets is not None:
                sizes = np.diff(self.chunk_offsets)[remap >= 0]
                self.chunk_offsets = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
            self.n_rows, self.n_chunks = int(n_rows.value), int(n_chunks.value)
            self._keep = None  # the index owns its (rewritten) storage
        return remap

    def set_option(self, name: str, value: int) -> None:
        """`rl_index_set_option`: choose a route of this index (`_abi.OPTIONS` names the keys; include/raglite_hip.h "options" says what
        each one does).  Results never depend on an option; speed and memory do."""
        check(lib().rl_index_set_option(self._handle, _abi.option_key(name), int(value)))

    def get_option(self, name: str) -> int:
        v = C.c_int64(0)
        check(lib().rl_index_get_option(self._handle, _abi.option_key(name), C.byref(v)))
        return int(v.value)

    def options(self, **kv: int):
        """Context manager: set the options, run the block, restore the previous values (what the A/B tests use)."""
        index = self

        class _Ctx:
            def __enter__(self):
                self.old = {k: index.get_option(k) for k in kv}
                for k, v in kv.items():
                    index.set_option(k, v)
                return index

            def __exit__(self, *exc):
                for k, v in self.old.items():
                    index.set_option(k, v)

        return _Ctx()

    def set_exact_fp32(self, exact: bool = True) -> None:
        """Make the MFMA streaming kernel use exact fp32 MFMAs (an ordered fmaf chain) instead of the default fp16
        (hi, lo) split of its fp32 operands (`rl_index_set_arithmetic`, include/raglite_hip.h)."""
        check(lib().rl_index_set_arithmetic(self._handle, 1 if exact else 0))

    @property
    def arithmetic(self) -> str:
        """What the streaming kernel multiplies with: 'fp32_exact', 'f16_split' or 'f16_stored'."""
        m = C.c_int(0)
        check(lib().rl_index_arithmetic(self._handle, C.byref(m)))
        return {1: "fp32_exact", 2: "f16_split", 3: "f16_stored"}[int(m.value)]

    def live(self) -> tuple[int, int]:
        """(live rows, live chunks)."""
        r, c = C.c_int64(0), C.c_int64(0)
        check(lib().rl_index_live(self._handle, C.byref(r), C.byref(c), None))
        return int(r.value), int(c.value)

    def filter_stats(self) -> dict:
        """What the last bound-filtered search on this index did (`rl_index_filter_stats`): kind, queries, candidates per query
        (mean / max), list capacity, and whether the guarded full-precision fallback ran.  Synchronises."""
        out = (C.c_int64 * 6)()
        st = _Args()
        st._side(self.mem, self.device)  # noqa: SLF001
        self._prep(st)
        check(lib().rl_index_filter_stats(self._handle, out, st.stream))
        kind = {0: "none", 1: "maxsim_batch_hi", 2: "rows_hi", 3: "rows_fused", 4: "rows_fused_hi", 5: "maxsim_batch_f16_exact"}[int(out[0])]
        n = int(out[1])
        return {"kind": kind, "queries": n, "candidates_per_query_mean": (int(out[2]) / n if n else 0.0),
                "candidates_per_query_max": int(out[3]), "list_capacity": int(out[4]), "fallback": bool(out[5])}

    def memory(self) -> dict:
        """Device memory of this index in bytes (`rl_index_memory`): the stored rows, the three optional images (0 = not built: the
        device was too full, the index too small for them to pay, or a switch), the scratch grown so far, free / total device memory
        and the headroom an image must leave free to be built."""
        out = (C.c_int64 * 8)()
        check(lib().rl_index_memory(self._handle, out))
        keys = ("rows", "presplit_image", "hi_image", "hi_plane", "scratch", "device_free", "device_total", "image_headroom")
        return {k: int(v) for k, v in zip(keys, out)}

    IMAGES = {"presplit": 1, "hi_image": 2, "hi_plane": 4}  # include/raglite_hip.h: RL_IMAGE_*

    def prepare(self, *images: str) -> tuple[str, ...]:
        """`rl_index_prepare`: build the named lazy images ("presplit", "hi_image", "hi_plane"; none named = all three) NOW, outside the
        hot path, instead of inside the first search whose route reads them (device allocation + one pass over the rows + one stream
        synchronisation in that call).  Returns the images the index holds afterwards -- one that the options, the shape or the free
        memory do not allow is simply absent (the routes over the stored rows answer, same results)."""
        bits = 0
        for name in images or tuple(self.IMAGES):
            if name not in self.IMAGES:
                raise ValueError(f"unknown image {name!r}: one of {sorted(self.IMAGES)}")
            bits |= self.IMAGES[name]
        built = C.c_uint32(0)
        if self.mem == MEM_DEVICE:
            _ensure_init(self.device.index or 0)
            stream = _torch().cuda.current_stream(self.device).cuda_stream
        else:
            _ensure_init(_current_device())
            stream = 0
        check(lib().rl_index_prepare(self._handle, bits, C.byref(built), stream))
        return tuple(name for name, bit in self.IMAGES.items() if built.value & bit)

    # -- a6 + a7 -------------------------------------------------------------------------------
    def search_rows(self, queries, k: int, chunk_filter=None, rank_limit: int | None = None):
        """Exact top-k rows: (scores (B,k) desc, rows (B,k) int32); padding = (-inf, -1).
        chunk_filter: optional bool mask over chunks (the reference's filter-first branch, `_search.py:105-119`).
        rank_limit: the order-first-then-filter branch (`_search.py:120-141`): only the `rank_limit` nearest live rows of
        each query are eligible, the filter applies to those (None / 0: no cut)."""
        a = _Args()
        p_q, B, single = self._queries(a, queries)
        o_s, p_s = a.out((B, k), np.float32)
        o_r, p_r = a.out((B, k), np.int32)
        p_f = self._filter(a, chunk_filter)
        self._prep(a)
        check(lib().rl_search_rows_ranked(self._handle, p_q, B, k, p_f, int(rank_limit or 0), p_s, p_r, a.mem, a.stream))
        return (o_s[0], o_r[0]) if single else (o_s, o_r)

    # -- the order-first cut of a SHARDED corpus, in stages (rl_rank_cut_*; driven by ShardedIndex.search_rows) -------------------
    def rank_cut_begin(self, queries) -> int:
        """Similarities of every live row for `queries` (B, dim), kept by the index until `rank_cut_finish`.  Returns B."""
        a = _Args()
        p_q, B, _ = self._queries(a, queries)
        self._prep(a)
        check(lib().rl_rank_cut_begin(self._handle, p_q, B, a.mem, a.stream))
        self._rank_side = (a.mem, a.device, B)
        return B

    def _rank_args(self) -> tuple[_Args, int]:
        mem, device, B = self._rank_side
        a = _Args()
        a._side(mem, device)  # noqa: SLF001
        self._prep(a)
        return a, B

    def rank_cut_level(self, level: int, rank_limit: int):
        """This shard's histogram of radix level 0..2 (B, 2048) int32 under the prefix the summed previous levels define."""
        a, B = self._rank_args()
        o, p = a.out((B, 2048), np.int32)
        check(lib().rl_rank_cut_level(self._handle, int(level), int(rank_limit), p, a.mem, a.stream))
        return o

    def rank_cut_level_done(self, level: int, hist_sum) -> None:
        """The level's histogram summed over all shards."""
        a, B = self._rank_args()
        p = a.inp(hist_sum, np.int32)
        if tuple(a.keep[-1].shape) != (B, 2048):
            raise ValueError("hist_sum must be (n_queries, 2048)")
        check(lib().rl_rank_cut_level_done(self._handle, int(level), p, a.mem, a.stream))

    def rank_cut_ties(self, rank_limit: int):
        """(B,) int32: this shard's rows whose key is the global threshold key."""
        a, B = self._rank_args()
        o, p = a.out((B,), np.int32)
        check(lib().rl_rank_cut_ties(self._handle, int(rank_limit), p, a.mem, a.stream))
        return o

    def rank_cut_finish(self, rank_limit: int, ties_before, k: int, chunk_filter=None):
        """This shard's top-k inside the global cut: (scores (B, k), rows (B, k) int32, padding (-inf, -1))."""
        a, B = self._rank_args()
        p_t = a.inp(ties_before, np.int32)
        o_s, p_s = a.out((B, k), np.float32)
        o_r, p_r = a.out((B, k), np.int32)
        p_f = self._filter(a, chunk_filter)
        check(lib().rl_rank_cut_finish(self._handle, int(rank_limit), p_t, p_f, int(k), p_s, p_r, a.mem, a.stream))
        return o_s, o_r

    # -- a6 + a7 + a8 ----------------------------------------------------------------------------
    def search_chunks(self, queries, num_hits: int, k: int, chunk_filter=None, rank_limit=None, *, query_filters=None):
        """Reference two-stage semantics (`src/raglite/_search.py:66-79,143-149`; with chunk_filter the
        filter-first branch `:105-119`, with rank_limit the order-first-then-filter branch `:120-141`): returns
        (scores (B,k), chunk ordinals (B,k), counts (B,)).  Per query (`rl_search_chunks_per_query`): `query_filters` holds one entry
        per query, None or a mask / packed bitset, and `rank_limit` may be a length-B sequence (0 or None: no cut); row b is then
        what the call for query b alone with its own filter and limit returns."""
        a = _Args()
        p_q, B, single = self._queries(a, queries)
        o_s, p_s = a.out((B, k), np.float32)
        o_c, p_c = a.out((B, k), np.int32)
        o_n, p_n = a.out((B,), np.int32)
        per_query, args = self._per_query(a, B, chunk_filter, query_filters, rank_limit)
        self._prep(a)
        if per_query:
            check(lib().rl_search_chunks_per_query(self._handle, p_q, B, num_hits, k, *args, p_s, p_c, p_n, a.call_mem, a.stream))
        else:
            check(lib().rl_search_chunks_ranked(self._handle, p_q, B, num_hits, k, *args, p_s, p_c, p_n, a.mem, a.stream))
        return (o_s[0], o_c[0], o_n[0]) if single else (o_s, o_c, o_n)

    def hybrid_search(self, queries, num_hits: int, n_each: int, k: int, *, keyword: "KeywordIndex | None" = None, query_term_ids=None,
                      weights=(0.75, 0.25), rrf_k: int = 60, chunk_filter=None, rank_limit=None, query_filters=None):
        """`rl_hybrid_search`: per query the n_each best chunks of the two-stage vector search (as `search_chunks`) and, with `keyword`,
        the n_each best of BM25 over `query_term_ids` (one sequence per query), fused by weighted RRF on the device; `weights` are
        (vector,) or (vector, keyword).  Returns (scores (B, k) float64, chunk ordinals (B, k) int32, counts (B,) int32).
        `query_filters` / a sequence `rank_limit`: per query, as in `search_chunks` (`rl_hybrid_search_per_query`); the keyword half
        takes the same filters."""
        a = _Args()
        p_q, B, single = self._queries(a, queries)
        o_s, p_s = a.out((B, k), np.float64)
        o_c, p_c = a.out((B, k), np.int32)
        o_n, p_n = a.out((B,), np.int32)
        per_query, args = self._per_query(a, B, chunk_filter, query_filters, rank_limit)
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).ravel()[: 2 if keyword is not None else 1])
        p_off = p_terms = None
        if keyword is not None:
            if query_term_ids is None or len(query_term_ids) != B:
                raise ValueError("one sequence of term ids per query is required")
            q_off, q_terms = _term_csr(query_term_ids)
            if a.mem == MEM_DEVICE:
                torch = _torch()
                q_off = torch.from_numpy(q_off).to(a.device)
                q_terms = torch.from_numpy(q_terms if q_terms.size else np.zeros(1, np.int32)).to(a.device)
                p_off, p_terms = q_off.data_ptr(), q_terms.data_ptr()
            else:
                p_off, p_terms = q_off.ctypes.data, q_terms.ctypes.data
            a.keep += [q_off, q_terms]
        self._prep(a)
        fn = lib().rl_hybrid_search_per_query if per_query else lib().rl_hybrid_search
        check(fn(self._handle, None if keyword is None else keyword._handle, p_q, B, int(num_hits), int(n_each), p_off, p_terms, *args,
                 w.ctypes.data, int(rrf_k), int(k), p_s, p_c, p_n, a.call_mem if per_query else a.mem, a.stream))
        return (o_s[0], o_c[0], o_n[0]) if single else (o_s, o_c, o_n)

    def _search_rerank_args(self, a, queries, query_vecs, keyword, query_term_ids, weights, chunk_filter, rank_limit, query_filters):
        """The arguments `rl_search_rerank_per_query` and `rl_search_rerank_spans_per_query` share, up to `weights`: (B, nq, the pointers
        in call order after `n_each`, the weights array)."""
        p_q, B, single = self._queries(a, queries)
        if single:
            raise ValueError("queries must be (n_queries, dim)")
        p_v = a.inp(query_vecs, np.float32)
        qv = a.keep[-1]
        if qv.ndim != 3 or int(qv.shape[0]) != B or int(qv.shape[2]) != self.dim:
            raise ValueError("query_vecs must be (n_queries, nq, dim)")
        nq = int(qv.shape[1])
        if query_filters is None and (rank_limit is None or np.ndim(rank_limit) == 0):  # (one filter for the batch: every query maps to it)
            query_filters = None if chunk_filter is None else [chunk_filter] * B
            chunk_filter = None
            if query_filters is None and rank_limit:
                query_filters = [None] * B
        if query_filters is None:
            args = (None, 0, None, None)
        else:
            _, args = self._per_query(a, B, chunk_filter, query_filters, rank_limit)
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).ravel()[: 2 if keyword is not None else 1])
        p_off = p_terms = None
        if keyword is not None:
            if query_term_ids is None or len(query_term_ids) != B:
                raise ValueError("one sequence of term ids per query is required")
            q_off, q_terms = _term_csr(query_term_ids)
            if a.mem == MEM_DEVICE:
                torch = _torch()
                q_off = torch.from_numpy(q_off).to(a.device)
                q_terms = torch.from_numpy(q_terms if q_terms.size else np.zeros(1, np.int32)).to(a.device)
                p_off, p_terms = q_off.data_ptr(), q_terms.data_ptr()
            else:
                p_off, p_terms = q_off.ctypes.data, q_terms.ctypes.data
            a.keep += [q_off, q_terms]
        return p_q, B, p_v, nq, p_off, p_terms, args, w

    def search_rerank(self, queries, num_hits: int, n_each: int, n_cand: int, query_vecs, k: int, *,
                      keyword: "KeywordIndex | None" = None, query_term_ids=None, weights=(0.75, 0.25), rrf_k: int = 60, chunk_filter=None,
                      rank_limit=None, query_filters=None):
        """`rl_search_rerank_per_query`: `hybrid_search(queries, num_hits, n_each, k=n_cand, ...)`, then `maxsim_rerank` of each query's
        fused candidates against `query_vecs` (B, nq, dim), then `rerank_order`'s first k, all on one stream with nothing read back in
        between.  Returns (MaxSim scores (B, k) float32, chunk ordinals (B, k) int32 best first, counts (B,) int32).  Without
        `keyword` the candidates are the vector search's list alone.  The filter arguments are `hybrid_search`'s."""
        a = _Args()
        p_q, B, p_v, nq, p_off, p_terms, args, w = self._search_rerank_args(a, queries, query_vecs, keyword, query_term_ids, weights,
                                                                            chunk_filter, rank_limit, query_filters)
        o_s, p_s = a.out((B, int(k)), np.float32)
        o_c, p_c = a.out((B, int(k)), np.int32)
        o_n, p_n = a.out((B,), np.int32)
        self._prep(a)
        check(lib().rl_search_rerank_per_query(self._handle, None if keyword is None else keyword._handle, p_q, B, int(num_hits), int(n_each),
                                               p_off, p_terms, *args, w.ctypes.data, int(rrf_k), int(n_cand), p_v, nq, int(k), p_s, p_c,
                                               p_n, a.call_mem, a.stream))
        return o_s, o_c, o_n

    def search_rerank_spans(self, queries, num_hits: int, n_each: int, n_cand: int, query_vecs, k: int, spans: "SpanTable",
                            neighbors=(-1, 1), *, keyword: "KeywordIndex | None" = None, query_term_ids=None, weights=(0.75, 0.25),
                            rrf_k: int = 60, chunk_filter=None, rank_limit=None, query_filters=None):
        """`rl_search_rerank_spans_per_query`: `search_rerank`'s pipeline, then `spans.chunk_spans` of each query's reranked first k on
        the same stream, nothing read back in between.  Returns (top chunk ordinals (B, k) int32, their counts (B,) int32) followed by
        `SpanTable.chunk_spans`'s five results with n_in = k."""
        offs = _span_offsets(neighbors)
        E = int(k) * (1 + int(offs.size))
        if int(k) < 1 or E > SPANS_MAX_ENTRIES:
            raise ValueError(f"search_rerank_spans: need k >= 1 and k * (1 + len(neighbors)) <= {SPANS_MAX_ENTRIES}")
        a = _Args()
        p_q, B, p_v, nq, p_off, p_terms, args, w = self._search_rerank_args(a, queries, query_vecs, keyword, query_term_ids, weights,
                                                                            chunk_filter, rank_limit, query_filters)
        o_tc, p_tc = a.out((B, int(k)), np.int32)
        o_tn, p_tn = a.out((B,), np.int32)
        o_c, p_oc = a.out((B, E), np.int32)
        o_l, p_ol = a.out((B, E), np.int32)
        o_s, p_os = a.out((B, E), np.float64)
        o_ns, p_ns = a.out((B,), np.int32)
        o_nc, p_nc = a.out((B,), np.int32)
        self._prep(a)
        check(lib().rl_search_rerank_spans_per_query(self._handle, None if keyword is None else keyword._handle, p_q, B, int(num_hits),
                                                     int(n_each), p_off, p_terms, *args, w.ctypes.data, int(rrf_k), int(n_cand), p_v, nq,
                                                     int(k), spans._handle, offs.ctypes.data if offs.size else None, int(offs.size), p_tc,
                                                     p_tn, p_oc, p_ol, p_os, p_ns, p_nc, a.call_mem, a.stream))
        return o_tc, o_tn, o_c, o_l, o_s, o_ns, o_nc

    # -- a9 ----------------------------------------------------------------------------------------
    def maxsim_scores(self, query_vecs):
        a = _Args()
        p_q, nq, _ = self._queries(a, query_vecs)
        o_s, p_s = a.out((self.n_chunks,), np.float32)
        self._prep(a)
        check(lib().rl_maxsim_scores(self._handle, p_q, nq, p_s, a.mem, a.stream))
        return o_s

    def maxsim_topk(self, query_vecs, k: int, chunk_filter=None):
        a = _Args()
        p_q, nq, _ = self._queries(a, query_vecs)
        o_s, p_s = a.out((k,), np.float32)
        o_c, p_c = a.out((k,), np.int32)
        p_f = self._filter(a, chunk_filter)
        self._prep(a)
        check(lib().rl_maxsim_topk_filtered(self._handle, p_q, nq, k, p_f, p_s, p_c, a.mem, a.stream))
        return o_s, o_c

    def maxsim_topk_batch(self, query_batch, k: int):
        """query_batch (n_queries, nq, dim) -> (scores (n_queries, k), chunk ordinals (n_queries, k)); one corpus
        pass per query and one batched selection launch."""
        a = _Args()
        # fp16 queries -- what the reference's embed_strings / query adapter hand over (`_embed.py:140`, `_search.py:62`) -- go in as fp16
        # (`rl_maxsim_topk_batch_f16`): over an fp16-stored index the one-product pass is then exact and its top-k is the result
        half = _is_half(query_batch)
        p_q = a.inp(query_batch, np.float16 if half else np.float32)
        qv = a.keep[-1]
        if qv.ndim != 3 or int(qv.shape[2]) != self.dim:
            raise ValueError("query_batch must be (n_queries, nq, dim)")
        n_queries, nq = int(qv.shape[0]), int(qv.shape[1])
        o_s, p_s = a.out((n_queries, k), np.float32)
        o_c, p_c = a.out((n_queries, k), np.int32)
        self._prep(a)
        fn = lib().rl_maxsim_topk_batch_f16 if half else lib().rl_maxsim_topk_batch
        check(fn(self._handle, p_q, n_queries, nq, k, p_s, p_c, a.mem, a.stream))
        return o_s, o_c

    def maxsim_approx_scores(self, query_batch, kernel: int = 0):
        """The first stage of `maxsim_topk_batch`'s bound-filtered pipeline alone (`rl_maxsim_approx_scores`): approximate scores
        (n_queries, n_chunks) from the hi halves of corpus and queries, and per query the rigorous bound m with
        |approximate - exact| <= m for every chunk.  kernel 0: sixteen queries per pass (maxsim_pp.hip), 1: eight (maxsim_gemm.hip)."""
        a = _Args()
        p_q = a.inp(query_batch, np.float32)
        qv = a.keep[-1]
        if qv.ndim != 3 or int(qv.shape[2]) != self.dim:
            raise ValueError("query_batch must be (n_queries, nq, dim)")
        n_queries, nq = int(qv.shape[0]), int(qv.shape[1])
        o_s, p_s = a.out((n_queries, self.n_chunks), np.float32)
        o_b, p_b = a.out((n_queries,), np.float32)
        self._prep(a)
        check(lib().rl_maxsim_approx_scores(self._handle, p_q, n_queries, nq, int(kernel), p_s, p_b, a.mem, a.stream))
        return o_s, o_b

    def maxsim_batch_begin(self, query_batch, k: int):
        """First half of `maxsim_topk_batch` over one shard of a SHARDED corpus (`rl_maxsim_batch_begin`): the approximate passes; returns
        (n_queries, k + 1) float32 -- this shard's k best approximate scores per query (descending) and its error bound -- for the
        all-gather in front of `maxsim_batch_finish`.  Raises RaglitHipError(UNSUPPORTED) where the bound-filtered pipeline does not cover
        the batch: use `maxsim_topk_batch` then."""
        a = _Args()
        p_q = a.inp(query_batch, np.float32)
        qv = a.keep[-1]
        if qv.ndim != 3 or int(qv.shape[2]) != self.dim:
            raise ValueError("query_batch must be (n_queries, nq, dim)")
        n_queries, nq = int(qv.shape[0]), int(qv.shape[1])
        o, p_o = a.out((n_queries, int(k) + 1), np.float32)
        self._prep(a)
        check(lib().rl_maxsim_batch_begin(self._handle, p_q, n_queries, nq, int(k), p_o, a.mem, a.stream))
        return o

    def maxsim_batch_finish(self, query_batch, all_approx, rank: int, k: int):
        """Second half (`rl_maxsim_batch_finish`): all_approx (world, n_queries, k + 1) = every shard's `maxsim_batch_begin` result;
        returns (scores (n_queries, k), LOCAL chunk ordinals (n_queries, k)) of this shard's chunks that could be in the global top-k,
        ranked by exact score, padded with (-inf, -1)."""
        a = _Args()
        p_q = a.inp(query_batch, np.float32)
        qv = a.keep[-1]
        n_queries = int(qv.shape[0])
        p_a = a.inp(all_approx, np.float32)
        av = a.keep[-1]
        if av.ndim != 3 or int(av.shape[1]) != n_queries or int(av.shape[2]) != int(k) + 1:
            raise ValueError("all_approx must be (world, n_queries, k + 1)")
        world = int(av.shape[0])
        o_s, p_s = a.out((n_queries, int(k)), np.float32)
        o_c, p_c = a.out((n_queries, int(k)), np.int32)
        self._prep(a)
        check(lib().rl_maxsim_batch_finish(self._handle, p_q, p_a, world, int(rank), p_s, p_c, a.mem, a.stream))
        return o_s, o_c

    def maxsim_rerank(self, query_vecs, candidates):
        """query_vecs (n_queries, nq, dim), candidates (n_queries, n_cand) int32 -> scores (n_queries, n_cand)."""
        a = _Args()
        p_q = a.inp(query_vecs, np.float32)
        qv = a.keep[-1]
        if qv.ndim != 3 or int(qv.shape[2]) != self.dim:
            raise ValueError("query_vecs must be (n_queries, nq, dim)")
        p_c = a.inp(candidates, np.int32)
        cv = a.keep[-1]
        n_queries, nq = int(qv.shape[0]), int(qv.shape[1])
        if cv.ndim != 2 or int(cv.shape[0]) != n_queries:
            raise ValueError("candidates must be (n_queries, n_cand)")
        n_cand = int(cv.shape[1])
        o_s, p_s = a.out((n_queries, n_cand), np.float32)
        self._prep(a)
        check(lib().rl_maxsim_rerank(self._handle, p_q, n_queries, nq, p_c, n_cand, p_s, a.mem, a.stream))
        return o_s

    # -- 8f-3: device half of update_query_adapter ---------------------------------------------------
    def chunk_best_rows(self, queries, candidates):
        """For every (query b, chunk candidates[b][j]): the row ordinal maximising q . row, i.e.
        `np.argmax(chunk.embedding_matrix @ q)` (`src/raglite/_query_adapter.py:174,180`); -1 for candidate -1."""
        a = _Args()
        p_q, B, single = self._queries(a, queries)
        c2 = candidates.reshape(1, -1) if candidates.ndim == 1 else candidates
        p_c = a.inp(c2, np.int32)
        if int(a.keep[-1].shape[0]) != B:
            raise ValueError("candidates must have one row per query")
        n_cand = int(a.keep[-1].shape[1])
        o_r, p_r = a.out((B, n_cand), np.int32)
        self._prep(a)
        check(lib().rl_chunk_best_rows(self._handle, p_q, B, p_c, n_cand, p_r, a.mem, a.stream))
        return o_r[0] if single else o_r

    def gather_rows(self, rows):
        """Embedding rows as float32 (whatever the storage precision)."""
        a = _Args()
        p_r = a.inp(rows, np.int32)
        n = int(a.keep[0].shape[0])
        o, p_o = a.out((n, self.dim), np.float32)
        self._prep(a)
        check(lib().rl_gather_rows(self._handle, p_r, n, p_o, a.mem, a.stream))
        return o

    def query_targets(self, queries, rows, relevant, gap: float = 0.05):
        """`rl_query_targets`: the exact NNLS target of every eval in one call.  queries (B, dim), rows (B, n_examples) int32 row ordinals
        (-1 = none), relevant (B, n_examples) nonzero = positive -> (targets float64 (B, dim), weights float64 (B, n_examples),
        objective float64 (B,), status int32 (B,), iterations int32 (B,)) on the side of `queries`."""
        a = _Args()
        p_q, B, _ = self._queries(a, queries)
        p_r = _same_side(a, rows, np.int32)
        r = a.keep[-1]
        p_rel = _same_side(a, relevant, np.uint8)
        if r.ndim != 2 or int(r.shape[0]) != B or tuple(a.keep[-1].shape) != tuple(r.shape):
            raise ValueError("query_targets: rows and relevant must be (n_queries, n_examples)")
        k = int(r.shape[1])
        T, p_t = a.out((B, self.dim), np.float64)  # noqa: N806
        w, p_w = a.out((B, k), np.float64)
        obj, p_o = a.out((B,), np.float64)
        status, p_s = a.out((B,), np.int32)
        iters, p_i = a.out((B,), np.int32)
        self._prep(a)
        check(lib().rl_query_targets(self._handle, p_q, B, p_r, p_rel, k, float(gap), p_t, p_w, p_o, p_s, p_i, a.mem, a.stream))
        return T, w, obj, status, iters

    def time_kernel(self, kind: int, query_vecs_cuda, iters: int) -> float:
        """Milliseconds (HIP events on the launch stream) for `iters` launches of the dominant kernel."""
        a = _Args()
        p_q, nq, _ = self._queries(a, query_vecs_cuda)
        if a.mem != MEM_DEVICE:
            raise ValueError("time_kernel needs CUDA tensors")
        ms = C.c_float(0.0)
        self._prep(a)
        check(lib().rl_time_kernel(self._handle, kind, p_q, nq, iters, C.byref(ms), a.stream))
        return float(ms.value)


class KeywordIndex:
    """BM25 postings on the device (`rl_keyword_index`): the keyword half of hybrid search, over the chunk ordinals of the
    `DeviceIndex` it sits beside.  Built from a `raglite_amd._keyword.Postings` (host arrays; the impacts are computed on the device)."""

    def __init__(self, postings) -> None:
        p = postings
        arrs = [np.ascontiguousarray(p.term_off, dtype=np.int64), np.ascontiguousarray(p.post_chunk, dtype=np.int32),
                np.ascontiguousarray(p.post_tf, dtype=np.int32), np.ascontiguousarray(p.post_term, dtype=np.int32),
                np.ascontiguousarray(p.idf, dtype=np.float32), np.ascontiguousarray(p.nrm, dtype=np.float32)]
        term_off, post_chunk, post_tf, post_term, idf, nrm = arrs
        self.n_terms, self.n_postings, self.n_chunks = int(term_off.size - 1), int(post_chunk.size), int(nrm.size)
        _ensure_init(_current_device())
        handle = C.c_void_p()
        check(lib().rl_keyword_index_create(C.byref(handle), term_off.ctypes.data, self.n_terms, post_chunk.ctypes.data,
                                            post_tf.ctypes.data, post_term.ctypes.data, self.n_postings, idf.ctypes.data,
                                            nrm.ctypes.data, self.n_chunks, MEM_HOST, None))
        self._handle = handle

    @classmethod
    def _from_handle(cls, handle) -> "KeywordIndex":
        """Wraps an `rl_keyword_index` the library built (`KeywordStore.build`); the object owns it."""
        self = cls.__new__(cls)
        n_terms, n_postings, n_chunks = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        self._handle = handle
        check(lib().rl_keyword_index_info(handle, C.byref(n_terms), C.byref(n_postings), C.byref(n_chunks)))
        self.n_terms, self.n_postings, self.n_chunks = n_terms.value, n_postings.value, n_chunks.value
        return self

    def read(self):
        """(term_off int64 [n_terms + 1], post_chunk int32 [n_postings], post_impact float32 [n_postings]): the arrays the device holds."""
        term_off = np.empty(self.n_terms + 1, np.int64)
        post_chunk = np.empty(self.n_postings, np.int32)
        post_impact = np.empty(self.n_postings, np.float32)
        _ensure_init(_current_device())
        check(lib().rl_keyword_index_read(self._handle, term_off.ctypes.data, post_chunk.ctypes.data, post_impact.ctypes.data, MEM_HOST, None))
        return term_off, post_chunk, post_impact

    def close(self) -> None:
        h, self._handle = getattr(self, "_handle", None), None
        if h:
            lib().rl_keyword_index_destroy(h)

    def __del__(self) -> None:  # noqa: D105
        try:
            self.close()
        except Exception:  # noqa: BLE001,S110 - interpreter shutdown
            pass

    def search(self, query_term_ids, k: int, chunk_filter=None, *, query_filters=None):
        """BM25 top-k of a batch: `query_term_ids` holds one sequence of term ids per query (duplicates are dropped, order does not
        matter).  Returns (scores (B,k) float32, chunk ordinals (B,k) int32, counts (B,) int32); unfilled slots are (-inf, -1).
        `query_filters`: one entry per query, None or a mask / packed bitset (`rl_keyword_search_per_query`)."""
        q_off, q_terms = _term_csr(query_term_ids)
        B = int(q_off.size - 1)
        scores = np.empty((B, k), np.float32)
        chunks = np.empty((B, k), np.int32)
        counts = np.empty(B, np.int32)
        _ensure_init(_current_device())
        if query_filters is not None:
            if chunk_filter is not None:
                raise ValueError("pass chunk_filter (one for the batch) or query_filters (one per query), not both")
            if isinstance(query_filters, FilterSet):
                p_f, n_filters, qf = query_filters.call_args(self.n_chunks, B)
                mem = MEM_HOST | MEM_FILTERS_DEVICE
            else:
                table, qf = filter_set(query_filters, self.n_chunks, B)
                p_f, n_filters, mem = table.ctypes.data if len(table) else None, len(table), MEM_HOST
            check(lib().rl_keyword_search_per_query(self._handle, q_off.ctypes.data, q_terms.ctypes.data, B, k, p_f, n_filters,
                                                    qf.ctypes.data, scores.ctypes.data, chunks.ctypes.data, counts.ctypes.data, mem, None))
            return scores, chunks, counts
        p_f = None
        if chunk_filter is not None:
            bits = pack_bits(chunk_filter)
            if bits.size != (self.n_chunks + 31) // 32:
                raise ValueError("chunk_filter must have one entry per chunk")
            p_f = bits.ctypes.data
        check(lib().rl_keyword_search(self._handle, q_off.ctypes.data, q_terms.ctypes.data, B, k, p_f, scores.ctypes.data,
                                      chunks.ctypes.data, counts.ctypes.data, MEM_HOST, None))
        return scores, chunks, counts


class DeviceTermIds:
    """The result of one analyzer call, in device memory the analyzer owns: term ids int32 [n_tokens] and offsets int64 [n_chunks + 1].
    It is valid until the analyzer's next `begin` (or its `close`); `KeywordStore.append` takes it, `read` copies it out."""

    def __init__(self, analyzer: "KeywordAnalyzer", serial: int, p_ids: int, p_off: int, n_chunks: int, n_tokens: int) -> None:
        self._analyzer, self._serial, self._p_ids, self._p_off = analyzer, serial, p_ids, p_off
        self.n_chunks, self.n_tokens = n_chunks, n_tokens

    def _check(self) -> None:
        if self._analyzer._handle is None or self._analyzer._serial != self._serial:  # noqa: SLF001
            raise ValueError("DeviceTermIds: the analyzer has moved on to another call (or was closed); this result is gone")

    def pointers(self) -> tuple[int | None, int]:
        self._check()
        return self._p_ids or None, self._p_off

    def read(self) -> tuple[np.ndarray, np.ndarray]:
        """(flat int32 [n_tokens], offsets int64 [n_chunks + 1]) on the host."""
        self._check()
        flat = np.empty(self.n_tokens, dtype=np.int32)
        offsets = np.empty(self.n_chunks + 1, dtype=np.int64)
        check(lib().rl_keyword_analyze_result(self._analyzer._handle, flat.ctypes.data, offsets.ctypes.data, MEM_HOST, None))  # noqa: SLF001
        return flat, offsets


class KeywordAnalyzer:
    """The BM25 index analyzer on the device (`rl_keyword_analyzer`): fold, tokenize, drop stopwords, Porter-stem and number the stems
    of many chunk bodies in one call, with the results `raglite_amd._keyword.index_stems` + `stems_to_store_ids` give.
    fold_table: uint32 [0x110000] (`_keyword.fold_table()`); stopwords: the words; hash_bits: 0, or the low bits of the stem hash to keep
    (tests force collisions with it).  One call is `begin` (the distinct stems come back, in order of first appearance), the caller's
    vocabulary step, then `finish` (one id per distinct stem goes in, the term ids stay on the device)."""

    def __init__(self, fold_table, stopwords, hash_bits: int = 0) -> None:
        _ensure_init(_current_device())
        table = np.ascontiguousarray(fold_table, dtype=np.uint32)
        words = [w.encode("utf-8") for w in stopwords]
        blob = b"".join(words)
        stop_off = np.concatenate(([0], np.cumsum([len(w) for w in words], dtype=np.int64))).astype(np.int64)
        handle = C.c_void_p()
        self._handle = None
        check(lib().rl_keyword_analyzer_create(C.byref(handle), table.ctypes.data, int(table.size), blob, stop_off.ctypes.data, len(words),
                                               int(hash_bits)))
        self._handle = handle
        self._serial = 0
        self._counts = None

    def close(self) -> None:
        h, self._handle = getattr(self, "_handle", None), None
        if h:
            lib().rl_keyword_analyzer_destroy(h)

    def __del__(self) -> None:  # noqa: D105
        try:
            self.close()
        except Exception:  # noqa: BLE001,S110 - interpreter shutdown
            pass

    def begin(self, codepoints, text_off) -> tuple[int, list[str], np.ndarray]:
        """Step one over codepoints uint32 [n] (UTF-32) and text_off int64 [n_texts + 1]: (n_tokens, the distinct stems in order of
        first appearance, first_pos int64: the index of each stem's first token among the call's non-stopword tokens)."""
        cp = np.ascontiguousarray(codepoints, dtype=np.uint32)
        off = np.ascontiguousarray(text_off, dtype=np.int64)
        if cp.ndim != 1 or off.ndim != 1 or off.size < 1:
            raise ValueError("KeywordAnalyzer.begin: codepoints [n] and text_off [n_texts + 1] are required")
        _ensure_init(_current_device())
        counts = np.zeros(5, dtype=np.int64)
        self._serial += 1
        self._counts = None
        check(lib().rl_keyword_analyze_begin(self._handle, cp.ctypes.data if cp.size else None, off.ctypes.data, int(cp.size), int(off.size - 1),
                                             counts.ctypes.data, MEM_HOST, None))
        n_tokens, n_distinct, n_bytes = int(counts[0]), int(counts[1]), int(counts[2])
        blob = np.empty(n_bytes, dtype=np.uint8)
        stem_off = np.zeros(n_distinct + 1, dtype=np.int64)
        first_pos = np.empty(n_distinct, dtype=np.int64)
        check(lib().rl_keyword_analyze_stems(self._handle, blob.ctypes.data if n_bytes else None, stem_off.ctypes.data,
                                             first_pos.ctypes.data if n_distinct else None, MEM_HOST, None))
        text = blob.tobytes().decode("ascii")
        bounds = stem_off.tolist()
        stems = [text[bounds[i] : bounds[i + 1]] for i in range(n_distinct)]
        self._counts = (int(off.size - 1), n_tokens, n_distinct, int(counts[3]))
        self.last_sizes = {"code_points": int(cp.size), "texts": int(off.size - 1), "symbols": int(counts[3]), "all_tokens": int(counts[4]),
                           "tokens": n_tokens, "distinct": n_distinct, "stem_bytes": n_bytes}  # (of the last begin: what the benchmark sizes its bounds by)
        return n_tokens, stems, first_pos

    def finish(self, ids) -> DeviceTermIds:
        """Step two: ids int32 [n_distinct], one per distinct stem of `begin` in its order -> the term ids and offsets on the device."""
        if self._counts is None:
            raise ValueError("KeywordAnalyzer.finish: no begin before it")
        n_texts, n_tokens, n_distinct, _ = self._counts
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        if ids.shape != (n_distinct,):
            raise ValueError("KeywordAnalyzer.finish: one id per distinct stem is required")
        p_ids, p_off = C.c_void_p(), C.c_void_p()
        check(lib().rl_keyword_analyze_finish(self._handle, ids.ctypes.data if n_distinct else None, MEM_HOST, C.byref(p_ids), C.byref(p_off),
                                              None))
        return DeviceTermIds(self, self._serial, p_ids.value or 0, p_off.value or 0, n_texts, n_tokens)


class KeywordStore:
    """Each chunk's term ids on the device (`rl_keyword_store`), beside the `DeviceIndex` whose chunk ordinals it follows: the BM25
    postings are built from it on the device (`count`, then `build`), so an insert or a delete uploads only what is new.  Term ids are
    stable (`raglite_amd._keyword.Vocabulary`); `count` takes the permutation that turns them into ranks in the sorted vocabulary."""

    def __init__(self) -> None:
        _ensure_init(_current_device())
        handle = C.c_void_p()
        check(lib().rl_keyword_store_create(C.byref(handle)))
        self._handle = handle

    def close(self) -> None:
        h, self._handle = getattr(self, "_handle", None), None
        if h:
            lib().rl_keyword_store_destroy(h)

    def __del__(self) -> None:  # noqa: D105
        try:
            self.close()
        except Exception:  # noqa: BLE001,S110 - interpreter shutdown
            pass

    def info(self) -> dict:
        vals = [C.c_int64(0) for _ in range(4)]
        check(lib().rl_keyword_store_info(self._handle, *(C.byref(v) for v in vals)))
        return dict(zip(("n_chunks", "n_live", "n_tokens", "device_bytes"), (v.value for v in vals)))

    def append(self, flat_ids, offsets=None) -> None:
        """New chunks at the end: chunk i holds term ids flat_ids[offsets[i] : offsets[i + 1]] (any order, repeats = tf).  A
        `DeviceTermIds` (what `KeywordAnalyzer.finish` left on the device) is appended device to device, `offsets` then stays None."""
        if isinstance(flat_ids, DeviceTermIds):
            if offsets is not None:
                raise ValueError("KeywordStore.append: a DeviceTermIds carries its own offsets")
            p_ids, p_off = flat_ids.pointers()
            _ensure_init(_current_device())
            check(lib().rl_keyword_store_append(self._handle, p_ids, p_off, flat_ids.n_chunks, MEM_DEVICE, None))
            if flat_ids.n_chunks:
                self._counted = None
            return
        if offsets is None:
            raise ValueError("KeywordStore.append: offsets are required with host term ids")
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        flat = np.asarray(flat_ids)
        if flat.size and (flat.min() < 0 or flat.max() > np.iinfo(np.int32).max):
            raise ValueError("KeywordStore.append: term ids must be in [0, 2^31)")
        flat = np.ascontiguousarray(flat, dtype=np.int32)
        if offsets.ndim != 1 or offsets.size < 1 or flat.ndim != 1 or int(offsets[-1]) != flat.size:
            raise ValueError("KeywordStore.append: offsets must hold one entry per chunk plus one and end at len(flat_ids)")
        _ensure_init(_current_device())
        check(lib().rl_keyword_store_append(self._handle, flat.ctypes.data, offsets.ctypes.data, int(offsets.size - 1), MEM_HOST, None))
        if offsets.size > 1:
            self._counted = None

    def delete(self, ordinals) -> None:
        """The chunks never count again (their tokens stay until the store is rebuilt); an ordinal that is dead already is skipped."""
        ords = np.ascontiguousarray(ordinals, dtype=np.int64).reshape(-1)
        _ensure_init(_current_device())
        check(lib().rl_keyword_store_delete(self._handle, ords.ctypes.data, int(ords.size), None))
        if ords.size:
            self._counted = None

    def count(self, n_terms: int, term_rank=None):
        """Builds the postings of the live chunks on the device; term t of them is term_rank[id] (None: the ids themselves).  Returns
        (df int64 [n_terms], length int64 [n_chunks], n_live, total_length, n_postings): what `_keyword.bm25_weights` takes."""
        n_chunks = self.info()["n_chunks"]
        p_rank = None
        if term_rank is not None:
            rank = np.ascontiguousarray(term_rank, dtype=np.int32)
            if rank.shape != (n_terms,):
                raise ValueError("KeywordStore.count: term_rank must hold one rank per term")
            p_rank = rank.ctypes.data
        df = np.zeros(n_terms, np.int64)
        length = np.zeros(n_chunks, np.int64)
        totals = np.zeros(3, np.int64)
        self._counted = None
        check(lib().rl_keyword_store_count(self._handle, p_rank, n_terms, df.ctypes.data, length.ctypes.data, totals.ctypes.data, MEM_HOST, None))
        self._counted = (n_terms, n_chunks)
        return df, length, int(totals[0]), int(totals[1]), int(totals[2])

    def build(self, idf, nrm) -> "KeywordIndex":
        """The `KeywordIndex` of the counted postings with these weights (float32 [n_terms], [n_chunks]); needs a `count` since the last
        change, and uses it up."""
        idf = np.ascontiguousarray(idf, dtype=np.float32)
        nrm = np.ascontiguousarray(nrm, dtype=np.float32)
        counted = getattr(self, "_counted", None)  # (n_terms, n_chunks) of the last count; the library refuses a build without one
        if counted is not None and counted != (idf.size, nrm.size):
            raise ValueError("KeywordStore.build: idf / nrm must hold one weight per counted term / chunk")
        handle = C.c_void_p()
        check(lib().rl_keyword_store_build(self._handle, idf.ctypes.data if counted else None, nrm.ctypes.data if counted else None,
                                           C.byref(handle), MEM_HOST, None))
        self._counted = None
        return KeywordIndex._from_handle(handle)  # noqa: SLF001


# ----------------------------------------------------------------------------------------------
def _same_side(a: _Args, x: Any, dtype: np.dtype) -> int:
    """`a.inp` for the small host-derived arrays of a call (offsets, sizes, flags): NumPy input follows the call to the device."""
    if a.mem == MEM_DEVICE and not _is_torch(x):
        x = _torch().from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(a.device)
    return a.inp(x, dtype)


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
    p_cost = a.inp(cost, np.float32)
    n = int(a.keep[0].shape[0])
    p_sizes = _same_side(a, sizes, np.int64)
    p_off = _same_side(a, doc_offsets, np.int64)
    n_docs = int(a.keep[-1].shape[0]) - 1
    if int(a.keep[-2].shape[0]) != n:
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
    p_b = a.inp(boundary, np.float64)
    n = int(a.keep[0].shape[0])
    p_s = _same_side(a, statements, np.float64)
    p_len = _same_side(a, lengths, np.int64)
    if int(a.keep[-1].shape[0]) != n or int(a.keep[-2].shape[0]) != n:
        raise ValueError("partition_chunklets: boundary, statements and lengths differ in length")
    p_off = _same_side(a, doc_offsets, np.int64)
    n_docs = int(a.keep[-1].shape[0]) - 1
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
    p_p = a.inp(probas, np.float64 if f64 else np.float32)
    n = int(a.keep[0].shape[0])
    if _is_torch(codepoints):
        torch = _torch()
        if codepoints.dtype not in (torch.int32, torch.uint32):
            codepoints = codepoints.to(torch.int32)  # code points are below 2^21
        p_cp = a.inp(codepoints.view(torch.int32), np.int32)
    else:
        p_cp = _same_side(a, np.ascontiguousarray(codepoints, dtype=np.uint32).view(np.int32), np.int32)
    p_known = _same_side(a, known, np.float64) if known is not None else None
    if any(int(x.shape[0]) != n for x in a.keep[1:]):
        raise ValueError("partition_sentences: codepoints, probas and known differ in length")
    p_off = _same_side(a, doc_offsets, np.int64)
    n_docs = int(a.keep[-1].shape[0]) - 1
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
    p_x = a.inp(embeddings, np.float32)
    x = a.keep[0]
    if x.ndim != 2:
        raise ValueError("split_chunks_call: embeddings must be (n, dim)")
    n, dim = int(x.shape[0]), int(x.shape[1])
    p_off = _same_side(a, doc_offsets, np.int64)
    n_docs = int(a.keep[-1].shape[0]) - 1
    p_sel = _same_side(a, nonoutlying, np.uint8) if nonoutlying is not None else None
    p_head = _same_side(a, is_heading, np.uint8) if is_heading is not None else None
    p_sizes = _same_side(a, sizes, np.int64)
    if int(a.keep[-1].shape[0]) != n or any(v is not None and len(v) != n for v in (nonoutlying, is_heading)):
        raise ValueError("split_chunks_call: sizes / flags do not match the embedding rows")
    cost, p_cost = a.out((n,), np.float32) if want_cost else (None, None)
    (cut, obj, status), ptrs = _partition_outputs(a, n, n_docs)
    if ptrs is not None:
        check(lib().rl_split_chunks(p_x, n, dim, p_off, n_docs, p_sel, p_head, p_sizes, int(max_size), ptrs[0], p_cost, *ptrs[1:],
                                    a.mem, a.stream))
    return cut, cost, obj, status
