"""Wrappers of `csrc/api_keyword.hip`: the BM25 index, the analyzer and the token store."""

from __future__ import annotations

import ctypes as C

import numpy as np

from raglite_amd._abi import MEM_DEVICE, MEM_HOST, check, lib
from raglite_amd._ops_frame import _Args, _Handle, _ensure_thread
from raglite_amd._ops_retrieval import _filter_bits, _query_filter_args


def _term_csr(query_term_ids) -> tuple[np.ndarray, np.ndarray]:
    """One sequence of term ids per query -> (q_off int64 [B + 1], q_terms int32), each query's ids ascending and distinct."""
    qs = [np.unique(np.asarray(q, dtype=np.int32)) for q in query_term_ids]
    q_off = np.concatenate(([0], np.cumsum([q.size for q in qs]))).astype(np.int64)
    q_terms = np.ascontiguousarray(np.concatenate(qs) if qs else np.zeros(0, np.int32), dtype=np.int32)
    return q_off, q_terms


def _term_csr_args(a: _Args, query_term_ids, B: int) -> tuple[int, int]:  # noqa: N803
    """The term CSR of a batch of B queries on the call's side -> (q_off pointer, q_terms pointer).  On the device an empty term list
    is a one-element placeholder: torch gives an empty tensor no address."""
    if query_term_ids is None or len(query_term_ids) != B:
        raise ValueError("one sequence of term ids per query is required")
    q_off, q_terms = _term_csr(query_term_ids)
    if a.mem == MEM_DEVICE and not q_terms.size:
        q_terms = np.zeros(1, np.int32)
    return a.same_side(q_off, np.int64)[1], a.same_side(q_terms, np.int32)[1]


class KeywordIndex(_Handle):
    """BM25 postings on the device (`rl_keyword_index`): the keyword half of hybrid search, over the chunk ordinals of the
    `DeviceIndex` it sits beside.  Built from a `raglite_amd._keyword.Postings` (host arrays; the impacts are computed on the device)."""

    _destroy = "rl_keyword_index_destroy"

    def __init__(self, postings) -> None:
        p = postings
        arrs = [np.ascontiguousarray(p.term_off, dtype=np.int64), np.ascontiguousarray(p.post_chunk, dtype=np.int32),
                np.ascontiguousarray(p.post_tf, dtype=np.int32), np.ascontiguousarray(p.post_term, dtype=np.int32),
                np.ascontiguousarray(p.idf, dtype=np.float32), np.ascontiguousarray(p.nrm, dtype=np.float32)]
        term_off, post_chunk, post_tf, post_term, idf, nrm = arrs
        self.n_terms, self.n_postings, self.n_chunks = int(term_off.size - 1), int(post_chunk.size), int(nrm.size)
        _ensure_thread()
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
        _ensure_thread()
        check(lib().rl_keyword_index_read(self._handle, term_off.ctypes.data, post_chunk.ctypes.data, post_impact.ctypes.data, MEM_HOST, None))
        return term_off, post_chunk, post_impact

    def search(self, query_term_ids, k: int, chunk_filter=None, *, query_filters=None):
        """BM25 top-k of a batch: `query_term_ids` holds one sequence of term ids per query (duplicates are dropped, order does not
        matter).  Returns (scores (B,k) float32, chunk ordinals (B,k) int32, counts (B,) int32); unfilled slots are (-inf, -1).
        `query_filters`: one entry per query, None or a mask / packed bitset (`rl_keyword_search_per_query`)."""
        q_off, q_terms = _term_csr(query_term_ids)
        B = int(q_off.size - 1)
        scores = np.empty((B, k), np.float32)
        chunks = np.empty((B, k), np.int32)
        counts = np.empty(B, np.int32)
        _ensure_thread()
        if query_filters is not None:
            if chunk_filter is not None:
                raise ValueError("pass chunk_filter (one for the batch) or query_filters (one per query), not both")
            a = _Args.on(MEM_HOST)
            p_f, n_filters, p_qf, _ = _query_filter_args(a, self.n_chunks, B, query_filters)
            check(lib().rl_keyword_search_per_query(self._handle, q_off.ctypes.data, q_terms.ctypes.data, B, k, p_f, n_filters, p_qf,
                                                    scores.ctypes.data, chunks.ctypes.data, counts.ctypes.data, a.call_mem, None))
            return scores, chunks, counts
        bits = None if chunk_filter is None else _filter_bits(chunk_filter, self.n_chunks)
        check(lib().rl_keyword_search(self._handle, q_off.ctypes.data, q_terms.ctypes.data, B, k, None if bits is None else bits.ctypes.data,
                                      scores.ctypes.data, chunks.ctypes.data, counts.ctypes.data, MEM_HOST, None))
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


class KeywordAnalyzer(_Handle):
    """The BM25 index analyzer on the device (`rl_keyword_analyzer`): fold, tokenize, drop stopwords, Porter-stem and number the stems
    of many chunk bodies in one call, with the results `raglite_amd._keyword.index_stems` + `stems_to_store_ids` give.
    fold_table: uint32 [0x110000] (`_keyword.fold_table()`); stopwords: the words; hash_bits: 0, or the low bits of the stem hash to keep
    (tests force collisions with it).  One call is `begin` (the distinct stems come back, in order of first appearance), the caller's
    vocabulary step, then `finish` (one id per distinct stem goes in, the term ids stay on the device)."""

    _destroy = "rl_keyword_analyzer_destroy"

    def __init__(self, fold_table, stopwords, hash_bits: int = 0) -> None:
        _ensure_thread()
        table = np.ascontiguousarray(fold_table, dtype=np.uint32)
        words = [w.encode("utf-8") for w in stopwords]
        blob = b"".join(words)
        stop_off = np.concatenate(([0], np.cumsum([len(w) for w in words], dtype=np.int64))).astype(np.int64)
        handle = C.c_void_p()
        check(lib().rl_keyword_analyzer_create(C.byref(handle), table.ctypes.data, int(table.size), blob, stop_off.ctypes.data, len(words),
                                               int(hash_bits)))
        self._handle = handle
        self._serial = 0
        self._counts = None

    def begin(self, codepoints, text_off) -> tuple[int, list[str], np.ndarray]:
        """Step one over codepoints uint32 [n] (UTF-32) and text_off int64 [n_texts + 1]: (n_tokens, the distinct stems in order of
        first appearance, first_pos int64: the index of each stem's first token among the call's non-stopword tokens)."""
        cp = np.ascontiguousarray(codepoints, dtype=np.uint32)
        off = np.ascontiguousarray(text_off, dtype=np.int64)
        if cp.ndim != 1 or off.ndim != 1 or off.size < 1:
            raise ValueError("KeywordAnalyzer.begin: codepoints [n] and text_off [n_texts + 1] are required")
        _ensure_thread()
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


class KeywordStore(_Handle):
    """Each chunk's term ids on the device (`rl_keyword_store`), beside the `DeviceIndex` whose chunk ordinals it follows: the BM25
    postings are built from it on the device (`count`, then `build`), so an insert or a delete uploads only what is new.  Term ids are
    stable (`raglite_amd._keyword.Vocabulary`); `count` takes the permutation that turns them into ranks in the sorted vocabulary."""

    _destroy = "rl_keyword_store_destroy"

    def __init__(self) -> None:
        _ensure_thread()
        handle = C.c_void_p()
        check(lib().rl_keyword_store_create(C.byref(handle)))
        self._handle = handle

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
            _ensure_thread()
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
        _ensure_thread()
        check(lib().rl_keyword_store_append(self._handle, flat.ctypes.data, offsets.ctypes.data, int(offsets.size - 1), MEM_HOST, None))
        if offsets.size > 1:
            self._counted = None

    def delete(self, ordinals) -> None:
        """The chunks never count again (their tokens stay until the store is rebuilt); an ordinal that is dead already is skipped."""
        ords = np.ascontiguousarray(ordinals, dtype=np.int64).reshape(-1)
        _ensure_thread()
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
