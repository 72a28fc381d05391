"""Wrappers of `csrc/api_retrieval.hip`: fusion, rerank order, span tables, metadata filters, and the filter arguments the searches share."""

from __future__ import annotations

import ctypes as C

import numpy as np

from raglite_amd._abi import MEM_FILTERS_DEVICE, MEM_HOST, check, lib
from raglite_amd._ops_frame import _Args, _Handle, _ensure_thread, _is_torch, _torch


def rrf_fuse(lists, weights, *, rrf_k: int = 60, k: int):
    """Weighted Reciprocal Rank Fusion (`rl_rrf_fuse`): the reference's `reciprocal_rank_fusion` (`src/raglite/_search.py:233-252`)
    for a batch, bit for bit.  `lists`: (R, B, len) chunk ordinals, or a sequence of R (B, len) arrays, R <= 4, R * len <= 4096,
    padded with entries < 0; `weights`: R finite floats.  Returns (scores (B, k) float64, ordinals (B, k) int32, counts (B,) int32),
    by score descending, ties by first occurrence; unfilled slots are (-inf, -1)."""
    if isinstance(lists, (list, tuple)):
        lists = _torch().stack(list(lists)) if lists and _is_torch(lists[0]) else np.stack([np.asarray(x) for x in lists])
    a = _Args()
    lv, p_l = a.inp(lists, np.int32)
    if lv.ndim != 3:
        raise ValueError("lists must be (n_lists, n_queries, len)")
    R, B, L = (int(v) for v in lv.shape)
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
    sv, p_s = a.inp(scores, np.float32)
    cv, p_c = a.inp(candidates, np.int32)
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


class SpanTable(_Handle):
    """Where every chunk sits in its document (`rl_span_table`): `doc` and `pos` int32 per chunk ordinal of the `DeviceIndex` it sits
    beside, `doc` the dense number of the chunk's document id in sorted order (< 0: the chunk has no position), `pos` its
    `Chunk.index`."""

    _destroy = "rl_span_table_destroy"

    def __init__(self, doc, pos) -> None:
        doc = np.ascontiguousarray(doc, dtype=np.int32).ravel()
        pos = np.ascontiguousarray(pos, dtype=np.int32).ravel()
        if doc.size != pos.size:
            raise ValueError("one (doc, pos) per chunk is required")
        self.n_chunks = int(doc.size)
        _ensure_thread()
        handle = C.c_void_p()
        check(lib().rl_span_table_create(C.byref(handle), doc.ctypes.data, pos.ctypes.data, self.n_chunks))
        self._handle = handle

    def info(self) -> tuple[int, int, int]:
        """(chunks covered, chunks with a position, device bytes held)."""
        n, live, nbytes = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(lib().rl_span_table_info(self._handle, C.byref(n), C.byref(live), C.byref(nbytes)))
        return int(n.value), int(live.value), int(nbytes.value)

    def chunk_spans(self, chunks, neighbors=(-1, 1)):
        """`rl_chunk_spans`: the reference's `retrieve_chunk_spans` (`src/raglite/_search.py:323-361`) on ordinals for a batch.  `chunks`
        (B, n_in) int32, each query's chunks best first; entries < 0, out of range or without a position are skipped and take no rank.
        `neighbors`: the offsets (None or () for none).  With E = n_in * (1 + len(neighbors)) <= 4096, returns (chunks (B, E) int32 --
        the distinct chunks span after span, best span first, ascending index within a span, padded with -1 --, span lengths (B, E)
        int32, span scores (B, E) float64, number of spans (B,) int32, number of chunks (B,) int32)."""
        offs = _span_offsets(neighbors)
        a = _Args()
        cv, p_c = a.inp(chunks, np.int32)
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
    gv, p_g = a.inp(gathered, np.int32)
    if gv.ndim != 3:
        raise ValueError("gathered must be (world, n_queries, W)")
    world, B, W = (int(v) for v in gv.shape)
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


def _filter_bits(chunk_filter, n_chunks: int) -> np.ndarray:
    """chunk_filter (bool mask over chunks, or a packed uint32 bitset) -> the packed bitset, checked against `n_chunks`."""
    bits = pack_bits(chunk_filter)
    if bits.size != (n_chunks + 31) // 32:
        raise ValueError("chunk_filter must have one entry per chunk")
    return bits


def _bitset_ptr(a: _Args, bits: np.ndarray) -> int:
    """A uint32 bitset or table of bitsets -> its pointer on the call's side (on the device as int32, the same bits)."""
    return a.same_side(bits.view(np.int32), np.int32)[1]


class FilterSet(_Handle):
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

    def close(self) -> None:  # (its own: a view does not own the handle, and a closed set is an empty one, not a dead one)
        h, self._handle = self._handle, C.c_void_p()
        if h and getattr(self, "_owner", None) is None:
            lib().rl_filter_set_destroy(h)
        self.n_filters = self.words = 0


class MetadataStore(_Handle):
    """Every chunk's metadata tags on the device (`rl_metadata_store`), beside the `DeviceIndex` whose chunk ordinals it follows:
    `tag_off` int64 [n_chunks + 1] and `tags` int32, each chunk's ids ascending and free of duplicates
    (`raglite_amd._metadata.TagVocabulary.encode_chunks`).  Deleting chunks needs no call; after a compaction the store is made anew."""

    _destroy = "rl_metadata_store_destroy"

    def __init__(self, tag_off, tags) -> None:
        tag_off, tags = self._csr(tag_off, tags)
        _ensure_thread()
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
        _ensure_thread()
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
        _ensure_thread()
        check(lib().rl_metadata_filters(self._handle, index._handle, f_off.ctypes.data, f_tags.ctypes.data, F, C.byref(fs._handle),  # noqa: SLF001
                                        chunks.ctypes.data, rows.ctypes.data, MEM_HOST, None))
        fs.n_filters, fs.words = F, (self.n_chunks + 31) // 32
        return fs, chunks, rows


def _query_filter_args(a: _Args, n_chunks: int, B: int, query_filters, rank_limit=None) -> tuple:  # noqa: N803
    """The filter arguments of a *_per_query call over `n_chunks` chunks: (bitsets pointer, n_filters, query_filter pointer,
    rank_limits pointer).  `query_filters`: one mask / bitset / None per query (the table goes to the call's side), or a `FilterSet`
    (its table is on the device already: the pointer goes in as it is, with the flag in `a.call_mem`)."""
    if isinstance(query_filters, FilterSet):
        p_f, n_filters, qf = query_filters.call_args(n_chunks, B)
        a.hold(query_filters)
        a.filters_flag = MEM_FILTERS_DEVICE
        table = None
    else:
        table, qf = filter_set(query_filters, n_chunks, B)
        n_filters = len(table)
    lim = _rank_limits(rank_limit, B)
    a.hold(qf, lim)
    if table is not None:
        p_f = _bitset_ptr(a, table) if n_filters else None
    return p_f, n_filters, qf.ctypes.data, None if lim is None else lim.ctypes.data
