"""Wrappers of `csrc/api.hip`: the device index and its searches; as methods of the index, also the hybrid, search-rerank and span calls
of `csrc/api_retrieval.hip`."""

from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

from raglite_amd import _abi
from raglite_amd._abi import MEM_DEVICE, MEM_HOST, METRICS, check, lib
from raglite_amd._ops_frame import _Args, _Handle, _ensure_init, _is_half, _is_torch
from raglite_amd._ops_keyword import KeywordIndex, _term_csr_args
from raglite_amd._ops_retrieval import SPANS_MAX_ENTRIES, SpanTable, _bitset_ptr, _filter_bits, _query_filter_args, _span_offsets


class DeviceIndex(_Handle):
    """Device-resident chunk-embedding matrix + chunk CSR: the GPU image of the reference's
    `chunk_embedding` table (`src/raglite/_database.py:403-430`).

    `embeddings`: (n_rows, dim) float32 NumPy array (copied to HBM) or CUDA tensor (borrowed, kept
    alive by this object).  `chunk_offsets`: ascending int64 CSR of length n_chunks+1 (rows of a chunk
    contiguous, `src/raglite/_split_chunks.py:116-122`); None = one row per chunk."""

    _destroy = "rl_index_destroy"

    def __init__(self, embeddings, chunk_offsets=None, *, metric: str = "cosine", storage: str = "f32") -> None:
        """storage="f16": keep the corpus as IEEE fp16 in HBM (lossless for the reference's data,
        `src/raglite/_embed.py:140`).  float16 input is taken as is, float32 input is rounded to nearest even."""
        if metric not in METRICS:
            raise ValueError(f"Unsupported metric: {metric}")  # wording of src/raglite/_query_adapter.py:207
        if storage not in ("f32", "f16"):
            raise ValueError("storage must be 'f32' or 'f16'")
        self.storage = storage
        a = _Args()
        emb, p_e = a.inp(embeddings, np.float16 if storage == "f16" else np.float32)
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
        super().close()
        self._keep = None

    # -- helpers -------------------------------------------------------------------------------
    def _queries(self, a: _Args, q) -> tuple[int, int, bool]:
        single = q.ndim == 1
        q2 = q.reshape(1, -1) if single else q
        qv, ptr = a.inp(q2, np.float32)
        if int(qv.shape[1]) != self.dim:
            raise ValueError(f"query dimension {int(qv.shape[1])} != index dimension {self.dim}")
        return ptr, int(qv.shape[0]), single

    def _query_batch(self, a: _Args, x, name: str, dtype=np.float32, n_queries: int | None = None) -> tuple[int, int, int]:
        """A (n_queries, nq, dim) batch of query vectors -> (pointer, n_queries, nq)."""
        qv, ptr = a.inp(x, dtype)
        if qv.ndim != 3 or int(qv.shape[2]) != self.dim or n_queries not in (None, int(qv.shape[0])):
            raise ValueError(f"{name} must be (n_queries, nq, dim)")
        return ptr, int(qv.shape[0]), int(qv.shape[1])

    def _prep(self, a: _Args) -> None:
        if a.mem == MEM_HOST and self.mem == MEM_DEVICE:
            _ensure_init(self.device.index or 0)
        else:
            a.ensure_device()

    def _frame(self, mem: int | None = None, device=None) -> _Args:
        """The frame of a call on this index that takes no array, with the device made current: the index's own side, device and
        stream, or the side a staged call began on (`_rank_args`)."""
        a = _Args.on(self.mem, self.device) if mem is None else _Args.on(mem, device)
        self._prep(a)
        return a

    def _filter(self, a: _Args, chunk_filter):
        """chunk_filter (bool mask over chunks, or a packed uint32 bitset) -> pointer on the call's side, or None."""
        return None if chunk_filter is None else _bitset_ptr(a, _filter_bits(chunk_filter, self.n_chunks))

    def _per_query(self, a: _Args, B: int, chunk_filter, query_filters, rank_limit):
        """The filter arguments of a call that takes per-query filters or limits -> (per_query, args): per_query False keeps the
        single-filter entry point with args (chunk filter pointer, rank limit); True gives (bitsets pointer, n_filters, query_filter
        pointer, rank_limits pointer) for the *_per_query one."""
        if query_filters is None and (rank_limit is None or np.ndim(rank_limit) == 0):
            return False, (self._filter(a, chunk_filter), int(rank_limit or 0))
        if query_filters is not None and chunk_filter is not None:
            raise ValueError("pass chunk_filter (one for the batch) or query_filters (one per query), not both")
        return True, _query_filter_args(a, self.n_chunks, B, [chunk_filter] * B if query_filters is None else query_filters, rank_limit)

    # -- lifecycle ---------------------------------------------------------------
    def append(self, rows, chunk_sizes=None) -> None:
        """Append embedding rows as new chunks (`insert_documents`, `src/raglite/_insert.py:247-272`): existing
        row / chunk ordinals never change.  chunk_sizes: rows per new chunk (None = one chunk per row)."""
        a = _Args()
        r, p_r = a.inp(rows, np.float32)
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
        self._frame()  # (the index's device made current; the call takes host memory and the null stream)
        check(lib().rl_index_delete_chunks(self._handle, c.ctypes.data, int(c.size), None))

    def compact(self) -> np.ndarray:
        """Reclaim tombstoned chunks (`rl_index_compact`): survivors keep their order and are renumbered 0..live-1.
        Returns remap (old n_chunks,) int64: new ordinal of every old chunk, -1 for a deleted one."""
        self._frame()  # (the index's device made current; the call takes host memory and the null stream)
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

    @contextlib.contextmanager
    def options(self, **kv: int):
        """Context manager: set the options, run the block, restore the previous values (what the A/B tests use)."""
        old = {k: self.get_option(k) for k in kv}
        for k, v in kv.items():
            self.set_option(k, v)
        try:
            yield self
        finally:
            for k, v in old.items():
                self.set_option(k, v)

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
        check(lib().rl_index_filter_stats(self._handle, out, self._frame().stream))
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
        check(lib().rl_index_prepare(self._handle, bits, C.byref(built), self._frame().stream))
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
        return self._frame(mem, device), B

    def rank_cut_level(self, level: int, rank_limit: int):
        """This shard's histogram of radix level 0..2 (B, 2048) int32 under the prefix the summed previous levels define."""
        a, B = self._rank_args()
        o, p = a.out((B, 2048), np.int32)
        check(lib().rl_rank_cut_level(self._handle, int(level), int(rank_limit), p, a.mem, a.stream))
        return o

    def rank_cut_level_done(self, level: int, hist_sum) -> None:
        """The level's histogram summed over all shards."""
        a, B = self._rank_args()
        hv, p = a.inp(hist_sum, np.int32)
        if tuple(hv.shape) != (B, 2048):
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
        _, p_t = a.inp(ties_before, np.int32)
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
        p_off, p_terms = (None, None) if keyword is None else _term_csr_args(a, query_term_ids, B)
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
        p_v, _, nq = self._query_batch(a, query_vecs, "query_vecs", n_queries=B)
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
        p_off, p_terms = (None, None) if keyword is None else _term_csr_args(a, query_term_ids, B)
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
        p_q, n_queries, nq = self._query_batch(a, query_batch, "query_batch", np.float16 if half else np.float32)
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
        p_q, n_queries, nq = self._query_batch(a, query_batch, "query_batch")
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
        p_q, n_queries, nq = self._query_batch(a, query_batch, "query_batch")
        o, p_o = a.out((n_queries, int(k) + 1), np.float32)
        self._prep(a)
        check(lib().rl_maxsim_batch_begin(self._handle, p_q, n_queries, nq, int(k), p_o, a.mem, a.stream))
        return o

    def maxsim_batch_finish(self, query_batch, all_approx, rank: int, k: int):
        """Second half (`rl_maxsim_batch_finish`): all_approx (world, n_queries, k + 1) = every shard's `maxsim_batch_begin` result;
        returns (scores (n_queries, k), LOCAL chunk ordinals (n_queries, k)) of this shard's chunks that could be in the global top-k,
        ranked by exact score, padded with (-inf, -1)."""
        a = _Args()
        qv, p_q = a.inp(query_batch, np.float32)
        n_queries = int(qv.shape[0])
        av, p_a = a.inp(all_approx, np.float32)
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
        p_q, n_queries, nq = self._query_batch(a, query_vecs, "query_vecs")
        cv, p_c = a.inp(candidates, np.int32)
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
        cv, p_c = a.inp(c2, np.int32)
        if int(cv.shape[0]) != B:
            raise ValueError("candidates must have one row per query")
        n_cand = int(cv.shape[1])
        o_r, p_r = a.out((B, n_cand), np.int32)
        self._prep(a)
        check(lib().rl_chunk_best_rows(self._handle, p_q, B, p_c, n_cand, p_r, a.mem, a.stream))
        return o_r[0] if single else o_r

    def gather_rows(self, rows):
        """Embedding rows as float32 (whatever the storage precision)."""
        a = _Args()
        rv, p_r = a.inp(rows, np.int32)
        n = int(rv.shape[0])
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
        r, p_r = a.same_side(rows, np.int32)
        rel, p_rel = a.same_side(relevant, np.uint8)
        if r.ndim != 2 or int(r.shape[0]) != B or tuple(rel.shape) != tuple(r.shape):
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
