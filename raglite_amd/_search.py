"""Host mirror of the retrieval half of `src/raglite/_search.py` over a device-resident index.

    vector_search(query, *, num_results=3, oversample=4, metadata_filter=None, config=None)
        -> (list[ChunkId], list[float])                                   (`_search.py:36-153`)
    keyword_search(query, *, num_results=3, metadata_filter=None, config=None)
        -> (list[ChunkId], list[float])   BM25 on the device               (`_search.py:156-230`)
    hybrid_search(...)                                                    (`_search.py:255-279`)
    hybrid_search_batch(queries, ...) -> list of hybrid_search's results, one device round trip for the batch
    vector_search_batch / keyword_search_batch(queries, ...) -> the same for vector_search / keyword_search
                                                            (the batched searches take one metadata filter per query)
    rerank_chunks(query, chunk_ids, *, config=None) -> list[chunk]        (`_search.py:364-397`)
    search_and_rerank_chunks(...)                                         (`_search.py:400-414`)
    search_and_rerank_chunks_batch(queries, ...) -> list of search_and_rerank_chunks's results: search, fusion, MaxSim rerank and
                                                    ordering of the whole batch in one device call
    rerank_chunks_batch(queries, chunk_ids_per_query, ...) -> the MaxSim rerank of given lists, one launch whatever the queries' lengths
    retrieve_chunk_spans(chunk_ids, *, neighbors=(-1, 1), config=None) -> list[ChunkSpan]      (`_search.py:302-361`)
    retrieve_chunk_spans_batch(chunk_ids_per_query, ...) -> the same for ragged lists, one device call
    search_and_rerank_chunk_spans(...)                                    (`_search.py:417-433`)
    search_and_rerank_chunk_spans_batch(queries, ...) -> search, fusion, MaxSim rerank, ordering and spans of the whole batch in one
                                                        device call
    retrieve_context(query, *, config=None) -> list[ChunkSpan]            (`_rag.py:43-64`)
    GpuVectorSearch   -- a `BasicSearchMethod` (`_typing.py:35-43`) for `RAGLiteConfig.search_method`
    MaxSimRanker      -- a duck-typed `rerankers.BaseRanker` for `RAGLiteConfig.reranker`
                         (`.rank(query=, docs=)` -> `.results[*].doc_id`, `_search.py:394-396`)

The reference evaluates distance + ORDER BY/LIMIT + GROUP BY inside DuckDB/pgvector; here the
`chunk_embedding` table lives in HBM (`GpuIndex`) and the same three steps run as HIP kernels.  The
store, ORM and HNSW index are out of scope.
"""

from __future__ import annotations

import threading
from dataclasses import dataclass, field
from functools import partial
from typing import Any, Callable, Sequence

import numpy as np

from raglite_amd import _embed, _keyword, _metadata, _ops, _ragged
from raglite_amd._config import DEFAULT_CHUNK_MAX_SIZE, HotPathConfig
from raglite_amd._embed import embed_strings

ChunkId = str


class GpuIndex:
    """Device image of the `chunk` / `chunk_embedding` tables for one database.

    chunk_ids        list[str] -- `Chunk.id` per chunk ordinal (`_database.py:233`)
    chunk_embeddings list of (n_i, dim) matrices -- `Chunk.embedding_matrix` (`_database.py:279-283`),
                     or a single (N, dim) matrix together with `chunk_offsets`
    query_adapter    optional (dim, dim) matrix -- `IndexMetadata.get("default")["query_adapter"]`
                     (`_search.py:58-62`, fitted by `_query_adapter.py:141-219`, out of scope)
    docs             optional list[str] -- `str(chunk)` per chunk, lets `MaxSimRanker` map the strings the
                     reranker plugin receives back to chunk ordinals
    metadata         optional list[dict] per chunk for `metadata_filter`
    storage          "f32", or "f16" (the reference's own storage precision)
    exact_fp32       multiply with exact fp32 MFMAs instead of the default fp16 (hi, lo) split of fp32 operands
    keyword_texts    optional list[str] -- `Chunk.body` per chunk: builds the BM25 keyword side (`keyword_search`, the keyword
                     half of `hybrid_search`; DESIGN.md "Keyword search"), rebuilt from the live chunks after every change
    keyword_build    "device" (the default): the chunks' term ids stay on the device (`KeywordStore`) and every rebuild of the postings
                     runs there; "host": the postings are rebuilt on the host and uploaded (the oracle of the device
                     build, and its A/B path).  Every result is the same either way.
    keyword_analyzer "host" (the default): every chunk body is analyzed by `_keyword.index_stems` in Python; "device" (needs
                     keyword_build="device"): the bodies of a build, an insert or a sync are folded, tokenized, Porter-stemmed and
                     numbered on the device in one call per batch (`_keyword.analyze_texts_device`) and appended to
                     the `KeywordStore` device to device; the index then keeps each chunk's int32 term ids on the host instead of
                     its stems.  Queries are analyzed on the host either way, and every result is the same either way.
    metadata_filters "device" (the default): the chunks' metadata stays on the device as tag lists (`MetadataStore`) and every
                     `metadata_filter` is evaluated there, its bitset handed to the search without a trip through the host (DESIGN.md
                     4.13); "host": the filters are evaluated by a Python loop over `metadata` (the oracle of the device evaluation,
                     and its A/B path).  Every result is the same either way.
    positions        optional list of (document_id: str, index: int) -- `Chunk.document_id` / `Chunk.index` per chunk
                     (`_database.py:207-224`; None: the chunk has no position): builds the span table (`retrieve_chunk_spans`;
                     DESIGN.md 4.11), rebuilt from the live chunks after every change
    """

    # keyword side (class defaults: an index without one): each chunk's index stems (None once deleted), the vocabulary and the device
    # postings built from them
    keyword: _ops.KeywordIndex | None = None
    _kw_stems: list | None = None  # per chunk: its stems, or (keyword_analyzer="device") its int32 term ids; None once deleted
    _kw_vocab: dict[str, int] = {}
    # keyword_build="device": the stable term ids (host) and the chunks' ids on the device; the postings are built from them there
    keyword_build: str = "device"
    keyword_analyzer: str = "host"
    _kw_vocabulary: _keyword.Vocabulary | None = None
    _kw_store: _ops.KeywordStore | None = None
    _kw_built_ranks: np.ndarray | None = None  # `_kw_vocabulary.ranks()` as of the build of `keyword`
    # span side (class defaults: an index without one): each chunk's (document_id, index) (None once deleted) and the device table
    positions: list | None = None
    spans: _ops.SpanTable | None = None
    # metadata_filters="device": the stable tag ids (host) and the chunks' tag lists on the device
    metadata_filters: str = "device"
    _meta_vocab: _metadata.TagVocabulary | None = None
    _meta_store: _ops.MetadataStore | None = None

    def __init__(self, chunk_ids: Sequence[ChunkId], chunk_embeddings, *, chunk_offsets=None,
                 metric: str = "cosine", query_adapter=None, docs: Sequence[str] | None = None,
                 metadata: Sequence[dict] | None = None, storage: str = "f32", exact_fp32: bool = False,
                 keyword_texts: Sequence[str] | None = None, positions: Sequence[tuple[str, int] | None] | None = None,
                 keyword_build: str = "device", metadata_filters: str = "device", keyword_analyzer: str = "host") -> None:
        if keyword_build not in ("device", "host"):
            raise ValueError('keyword_build must be "device" or "host"')
        if keyword_analyzer not in ("device", "host"):
            raise ValueError('keyword_analyzer must be "device" or "host"')
        if keyword_analyzer == "device" and keyword_build != "device":
            raise ValueError('keyword_analyzer="device" needs keyword_build="device": the term ids it makes stay on the device')
        self.keyword_analyzer = keyword_analyzer
        if metadata_filters not in ("device", "host"):
            raise ValueError('metadata_filters must be "device" or "host"')
        self.keyword_build = keyword_build
        self.metadata_filters = metadata_filters
        if chunk_offsets is None:
            mats = [np.asarray(m, dtype=np.float32).reshape(len(m), -1) for m in chunk_embeddings]
            sizes = np.asarray([len(m) for m in mats], dtype=np.int64)
            chunk_offsets = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
            dim = mats[0].shape[1] if mats else 0
            matrix = np.vstack(mats) if mats else np.zeros((0, max(dim, 1)), dtype=np.float32)
        else:
            matrix = chunk_embeddings
        if len(chunk_ids) != len(chunk_offsets) - 1:
            raise ValueError("one chunk id per chunk is required")
        self.chunk_ids = list(chunk_ids)
        self.index = _ops.DeviceIndex(matrix, chunk_offsets, metric=metric, storage=storage)
        if exact_fp32:  # ordered fp32 MFMA chain instead of the fp16 (hi, lo) split (include/raglite_hip.h, rl_index_set_arithmetic)
            self.index.set_exact_fp32()
        self.metric = metric
        self.query_adapter = None if query_adapter is None else np.asarray(query_adapter, dtype=np.float32)
        self.docs = None if docs is None else list(docs)
        self._doc_to_ordinal = None if docs is None else {d: i for i, d in enumerate(self.docs)}
        self.metadata = None if metadata is None else list(metadata)
        self._id_to_ordinal = {cid: i for i, cid in enumerate(self.chunk_ids)}
        self._reset_metadata_store()
        if keyword_texts is not None:
            if len(keyword_texts) != len(self.chunk_ids):
                raise ValueError("one keyword text per chunk is required")
            if keyword_analyzer == "device":
                self._reset_keyword_store(list(keyword_texts))
            elif keyword_build == "device":
                self._kw_stems = [_keyword.index_stems(t) for t in keyword_texts]
                self._reset_keyword_store()
            else:
                self._kw_stems = [_keyword.index_stems(t) for t in keyword_texts]
                self._rebuild_keywords()
        if positions is not None:
            if len(positions) != len(self.chunk_ids):
                raise ValueError("one (document_id, index) position per chunk is required")
            self._rebuild_spans(list(positions))

    @property
    def has_keywords(self) -> bool:
        return self._kw_stems is not None

    @property
    def has_positions(self) -> bool:
        return self.positions is not None

    def _reset_metadata_store(self) -> None:
        """metadata_filters="device": a fresh tag vocabulary and store from `metadata`, by one upload of every chunk's tags (the
        constructor, and `compact`, which renumbers the chunks).  Metadata that does not cover the chunks one to one has no store: the
        host path answers, as before."""
        old = self._meta_store
        self._meta_vocab = self._meta_store = None
        if self.metadata_filters == "device" and self.metadata is not None and len(self.metadata) == len(self.chunk_ids):
            vocab = _metadata.TagVocabulary()
            store = _ops.MetadataStore(*vocab.encode_chunks(self.metadata))
            self._meta_vocab, self._meta_store = vocab, store
        if old is not None:
            old.close()

    def _rebuild_spans(self, positions: list) -> None:
        """The span table of `positions` (one per chunk ordinal; None: no position): documents are numbered in sorted(document_id)
        order, Python's string comparison, which is what the reference's `sorted(..., key=(document_id, index))` compares
        (`_search.py:342`).  Built before the old table goes, and `self.positions` changes only then: a failure leaves the index as
        it was."""
        self._check_positions(positions)
        doc_no = {d: i for i, d in enumerate(sorted({p[0] for p in positions if p is not None}))}
        doc = np.full(len(positions), -1, dtype=np.int32)
        pos = np.zeros(len(positions), dtype=np.int32)
        for o, p in enumerate(positions):
            if p is not None:
                doc[o], pos[o] = doc_no[p[0]], int(p[1])
        new = _ops.SpanTable(doc, pos)
        if self.spans is not None:
            self.spans.close()
        self.spans, self.positions = new, positions

    def span_table(self) -> "_ops.SpanTable":
        if self.spans is None:
            raise ValueError("GpuIndex was built without `positions`: pass positions= (one (document_id, index) per chunk) or use "
                             "from_store(); chunk spans need them")
        return self.spans

    def _rebuild_keywords(self) -> None:
        """The reference rebuilds its FTS index after every insert and delete (`_insert.py:268`, `_delete.py:173`): N, avgdl and df
        change, so the postings are rebuilt from the live chunks' cached stems (no text is analysed again)."""
        vocab, postings = _keyword.build_from_stems(self._kw_stems)
        new = _ops.KeywordIndex(postings)  # (built before the old one goes: a failure leaves the index as it was)
        if self.keyword is not None:
            self.keyword.close()
        self.keyword, self._kw_vocab = new, {s: i for i, s in enumerate(vocab)}

    @staticmethod
    def _analyze_into_store(texts: Sequence[str | None], vocab: "_keyword.Vocabulary", store: "_ops.KeywordStore") -> list:
        """keyword_analyzer="device": the bodies analyzed on the device and appended to `store` device to device; returns each chunk's
        int32 term ids (a host copy: what `compact` uploads again), None for a dead chunk."""
        first = store.info()["n_chunks"]
        ids: list = []
        for result in _keyword.analyze_texts_device(texts, vocab):
            store.append(result)
            flat, offsets = result.read()
            ids.extend(np.split(flat, offsets[1:-1]))
        dead = [i for i, t in enumerate(texts) if t is None]
        for i in dead:
            ids[i] = None
        store.delete(np.asarray(dead, dtype=np.int64) + first)
        return ids

    def _reset_keyword_store(self, texts: list | None = None) -> None:
        """keyword_build="device": a fresh vocabulary and token store from `_kw_stems`, by one upload of every chunk's ids (the
        constructor, and `compact` -- a rare operation, which renumbers the chunks), then the postings.  keyword_analyzer="device":
        the constructor hands in the bodies (`texts`) and they are analyzed on the device; `compact` uploads the kept chunks' ids
        under the SAME vocabulary -- stable ids stay valid, and a stem that lived only in dropped chunks keeps its rank with df = 0."""
        on_device = self.keyword_analyzer == "device"
        vocab = self._kw_vocabulary if on_device and texts is None else _keyword.Vocabulary()
        store = _ops.KeywordStore()
        old = (self._kw_vocabulary, self._kw_store, self._kw_built_ranks)
        try:
            if on_device and texts is not None:
                self._kw_stems = self._analyze_into_store(texts, vocab, store)
            elif on_device:
                sizes = np.fromiter((0 if ids is None else len(ids) for ids in self._kw_stems), dtype=np.int64, count=len(self._kw_stems))
                kept = [ids for ids in self._kw_stems if ids is not None and len(ids)]
                store.append(np.concatenate(kept) if kept else np.zeros(0, dtype=np.int32), np.concatenate(([0], np.cumsum(sizes))))
                store.delete(np.asarray([i for i, ids in enumerate(self._kw_stems) if ids is None], dtype=np.int64))
            else:
                flat, offsets, dead = _keyword.stems_to_store_ids(self._kw_stems, vocab)
                store.append(flat, offsets)
                store.delete(dead)
            self._kw_vocabulary, self._kw_store = vocab, store
            self._build_keywords_on_device()
        except Exception:
            self._kw_vocabulary, self._kw_store, self._kw_built_ranks = old
            store.close()
            raise
        if old[1] is not None:
            old[1].close()

    def _build_keywords_on_device(self) -> None:
        """What `_rebuild_keywords` does, without the host touching a token: the store counts the postings of the live chunks
        (`rl_keyword_store_count`), `_keyword.bm25_weights` turns the statistics into idf and nrm, the store builds the index."""
        vocab, store = self._kw_vocabulary, self._kw_store
        ranks = vocab.ranks()
        df, length, n_live, total_length, _ = store.count(len(vocab), ranks)
        idf, nrm, _ = _keyword.bm25_weights(df, length, n_live, total_length)
        new = store.build(idf, nrm)  # (built before the old one goes: a failure leaves the keyword index as it was)
        if self.keyword is not None:
            self.keyword.close()
        # queries are numbered by the ranks the index was BUILT with: the vocabulary may grow before a later build succeeds
        self.keyword, self._kw_built_ranks = new, ranks

    def keyword_query_ids(self, query: str) -> list[int]:
        """Term ids of the query's distinct stems that are in the vocabulary, ascending."""
        if self._kw_vocabulary is not None:  # (the device build's terms are ranks over every stem ever stored)
            return self._kw_vocabulary.query_ranks(_keyword.query_stems(query), self._kw_built_ranks)
        return sorted(self._kw_vocab[s] for s in _keyword.query_stems(query) if s in self._kw_vocab)

    def ordinal_of(self, chunk_id: ChunkId) -> int:
        return self._id_to_ordinal[chunk_id]

    def ordinal_of_doc(self, doc: str) -> int:
        if self._doc_to_ordinal is None:
            raise ValueError("GpuIndex was built without `docs`; MaxSimRanker cannot map strings to chunks")
        return self._doc_to_ordinal[doc]

    # -- lifecycle -------------------------------------------------------------------------
    def insert_chunks(self, chunk_ids: Sequence[ChunkId], chunk_embeddings, *, docs: Sequence[str] | None = None,
                      metadata: Sequence[dict] | None = None, keyword_texts: Sequence[str] | None = None,
                      positions: Sequence[tuple[str, int] | None] | None = None) -> None:
        """`insert_documents` on the device image (`src/raglite/_insert.py:247-272`): append the chunks'
        embedding matrices; existing ordinals keep their meaning.  `keyword_texts` (the chunks' bodies) iff the index has a
        keyword side; `positions` iff it was built with them."""
        mats = [np.asarray(m, dtype=np.float32).reshape(len(m), -1) for m in chunk_embeddings]
        if len(mats) != len(chunk_ids):
            raise ValueError("one embedding matrix per chunk id is required")
        if any(cid in self._id_to_ordinal for cid in chunk_ids):
            raise ValueError("chunk id already present")  # the reference skips existing documents (`_insert.py:184-186`)
        if (self.docs is None) != (docs is None) or (self.metadata is None) != (metadata is None):
            raise ValueError("docs / metadata must be given iff the index was built with them")
        if self.has_keywords != (keyword_texts is not None):
            raise ValueError("keyword_texts must be given iff the index was built with them")
        if keyword_texts is not None and len(keyword_texts) != len(chunk_ids):
            raise ValueError("one keyword text per chunk id is required")
        if self.has_positions != (positions is not None):
            raise ValueError("positions must be given iff the index was built with them")
        if positions is not None and len(positions) != len(chunk_ids):
            raise ValueError("one (document_id, index) position per chunk id is required")
        if not mats:
            return
        if positions is not None:  # (checked before the index changes: two live chunks at one position raise here)
            self._check_positions(self.positions + list(positions))
        self.index.append(np.vstack(mats), np.asarray([len(m) for m in mats], dtype=np.int64))
        base = len(self.chunk_ids)
        self.chunk_ids.extend(chunk_ids)
        self._id_to_ordinal.update({cid: base + i for i, cid in enumerate(chunk_ids)})
        if docs is not None:
            self.docs.extend(docs)
            self._doc_to_ordinal.update({d: base + i for i, d in enumerate(docs)})
        if metadata is not None:
            self.metadata.extend(metadata)
            if self._meta_store is not None:  # only the new chunks' tags go to the device
                if len(metadata) == len(mats):
                    self._meta_store.append(*self._meta_vocab.encode_chunks(metadata))
                else:
                    self._reset_metadata_store()
        if keyword_texts is not None and self.keyword_analyzer == "device":  # the new bodies are analyzed where their ids stay
            self._kw_stems.extend(self._analyze_into_store(list(keyword_texts), self._kw_vocabulary, self._kw_store))
            self._build_keywords_on_device()
        elif keyword_texts is not None:
            stems = [_keyword.index_stems(t) for t in keyword_texts]
            self._kw_stems.extend(stems)
            if self._kw_store is not None:  # only the new chunks' ids go to the device
                flat, offsets, _ = _keyword.stems_to_store_ids(stems, self._kw_vocabulary)
                self._kw_store.append(flat, offsets)
                self._build_keywords_on_device()
            else:
                self._rebuild_keywords()
        if positions is not None:
            self._rebuild_spans(self.positions + list(positions))

    @staticmethod
    def _check_positions(positions: list) -> None:
        """Every position is None or (document_id: str, index: int in [0, 2^31)), and no two live chunks share one."""
        live = [(p[0], int(p[1])) for p in positions if p is not None]
        if any(not isinstance(d, str) or not 0 <= i < (1 << 31) for d, i in live):
            raise ValueError("positions: document_id must be a str and index an int in [0, 2^31)")
        if len(set(live)) != len(live):
            seen: set = set()
            dup = next(p for p in live if p in seen or seen.add(p))
            raise ValueError(f"positions: two live chunks are at (document_id={dup[0]!r}, index={dup[1]})")

    def delete_chunks(self, chunk_ids: Sequence[ChunkId]) -> int:
        """`delete_documents` on the device image (`src/raglite/_delete.py:148-176`): the chunks never match
        again; unknown ids are ignored like the reference's `WHERE id IN (...)`.  Returns the number deleted."""
        ords = [self._id_to_ordinal.pop(cid) for cid in chunk_ids if cid in self._id_to_ordinal]
        if ords:
            self.index.delete_chunks(np.asarray(ords, dtype=np.int64))
            if self.has_keywords:
                for o in ords:
                    self._kw_stems[o] = None
                if self._kw_store is not None:
                    self._kw_store.delete(np.asarray(ords, dtype=np.int64))
                    self._build_keywords_on_device()
                else:
                    self._rebuild_keywords()
            if self.has_positions:
                gone = set(ords)
                self._rebuild_spans([None if o in gone else p for o, p in enumerate(self.positions)])
        return len(ords)

    # -- the real store ----------------------------------------------------------------------
    @classmethod
    def from_store(cls, bind: Any, *, metric: str = "cosine", storage: str = "f32", exact_fp32: bool = False,
                   keywords: bool = False, keyword_build: str = "device", metadata_filters: str = "device",
                   keyword_analyzer: str = "host") -> "GpuIndex":
        """Build the device index from a RAGLite database: `chunk_embedding` rows ordered by (chunk_id, id)
        (`src/raglite/_database.py:403-430`), the chunks' `str(chunk)` text and metadata, and the stored query adapter
        (`:450-462`).  `bind`: SQLAlchemy Engine / Connection / Session or a database URL.  `metric` is the store's
        `vector_search_distance_metric` (`_config.py:69`).  `keywords`: also build the BM25 keyword side from `chunk.body`
        (`keyword_build` and `keyword_analyzer` as in the constructor).  `metadata_filters` as in the constructor.
        The index remembers `bind` for `sync()`."""
        from raglite_amd import _store

        conn, owned = _store._connection(bind)  # noqa: SLF001
        try:
            img = _store.read_chunks(conn)
            adapter = _store.read_query_adapter(conn)
        finally:
            if owned:
                conn.close()
        if not img.rows:
            raise ValueError("First run `insert_documents()` to insert documents.")  # the reference's wording for an empty store
        off = np.concatenate(([0], np.cumsum(np.asarray(img.sizes, dtype=np.int64)))).astype(np.int64)
        gi = cls(img.chunk_ids, img.matrix(), chunk_offsets=off, metric=metric, query_adapter=adapter, docs=img.docs,
                 metadata=img.metadata, storage=storage, exact_fp32=exact_fp32, keyword_texts=img.bodies if keywords else None,
                 positions=img.positions, keyword_build=keyword_build, metadata_filters=metadata_filters,
                 keyword_analyzer=keyword_analyzer)
        gi._bind = bind  # noqa: SLF001
        return gi

    def sync(self, bind: Any = None, *, compact_above: float = 0.25) -> tuple[int, int]:
        """Bring the device image up to date with the store after `insert_documents` / `delete_documents`
        (`src/raglite/_insert.py:247-272`, `src/raglite/_delete.py:148-176`): chunk ids that appeared are appended
        (rows ordered by `id` within a chunk), ids that vanished are tombstoned, the query adapter is re-read; when
        more than `compact_above` of the rows are dead the index is compacted.  Returns (appended, deleted)."""
        from raglite_amd import _store

        bind = bind if bind is not None else getattr(self, "_bind", None)
        if bind is None:
            raise ValueError("sync() needs the store: build the index with GpuIndex.from_store() or pass `bind`")
        conn, owned = _store._connection(bind)  # noqa: SLF001
        try:
            in_store = set(_store.list_embedded_chunk_ids(conn))
            gone = [cid for cid in self._id_to_ordinal if cid not in in_store]
            new = sorted(in_store.difference(self._id_to_ordinal))
            img = _store.read_chunks(conn, new) if new else None
            self.query_adapter = _store.read_query_adapter(conn)
        finally:
            if owned:
                conn.close()
        n_deleted = self.delete_chunks(gone)
        if img is not None and img.rows:
            mats, at = [], 0
            for size in img.sizes:
                mats.append(np.vstack(img.rows[at : at + size]))
                at += size
            self.insert_chunks(img.chunk_ids, mats, docs=img.docs if self.docs is not None else None,
                               metadata=img.metadata if self.metadata is not None else None,
                               keyword_texts=img.bodies if self.has_keywords else None,
                               positions=img.positions if self.has_positions else None)
        live_rows, _ = self.index.live()
        if self.index.n_rows and 1.0 - live_rows / self.index.n_rows > compact_above:
            self.compact()
        return (len(img.chunk_ids) if img is not None else 0), n_deleted

    def compact(self) -> None:
        """Drop the tombstoned chunks for good (`rl_index_compact`) and renumber the host-side tables accordingly."""
        remap = self.index.compact()
        keep = np.nonzero(remap >= 0)[0]
        if len(keep) == len(remap):
            return
        self.chunk_ids = [self.chunk_ids[i] for i in keep]
        self._id_to_ordinal = {cid: i for i, cid in enumerate(self.chunk_ids)}
        if self.docs is not None:
            self.docs = [self.docs[i] for i in keep]
            self._doc_to_ordinal = {d: i for i, d in enumerate(self.docs)}
        if self.metadata is not None:
            self.metadata = [self.metadata[i] for i in keep]
            self._reset_metadata_store()  # (the ordinals changed: one upload of the kept chunks' tags)
        if self.has_keywords:
            self._kw_stems = [self._kw_stems[i] for i in keep]
            if self._kw_store is not None:  # (the ordinals changed: one upload of the kept chunks' ids)
                self._reset_keyword_store()
            else:
                self._rebuild_keywords()
        if self.has_positions:
            self._rebuild_spans([self.positions[i] for i in keep])

    def close(self) -> None:
        self.index.close()
        if self.keyword is not None:
            self.keyword.close()
        if self._kw_store is not None:
            self._kw_store.close()
        if self.spans is not None:
            self.spans.close()
        if self._meta_store is not None:
            self._meta_store.close()
            self._meta_store = None


# config (hashable, like the reference's lru_cache keys) -> GpuIndex
_attached: dict[Any, GpuIndex] = {}
_DEFAULT_KEY = "default"


def attach_index(index: GpuIndex, config: Any | None = None) -> None:
    """Make `index` the one `vector_search(..., config=config)` searches."""
    _attached[_DEFAULT_KEY if config is None else config] = index


def detach_index(config: Any | None = None) -> None:
    _attached.pop(_DEFAULT_KEY if config is None else config, None)


def _index_for(config: Any | None) -> GpuIndex:
    idx = _attached.get(_DEFAULT_KEY if config is None else config) or _attached.get(_DEFAULT_KEY)
    if idx is None:
        raise ValueError("No GpuIndex attached: call raglite_amd.attach_index(index, config) first.")
    return idx


def _adapt_metadata(metadata_filter: dict | None) -> dict | None:
    """Normalise filter values to lists (`src/raglite/_database.py` `_adapt_metadata`)."""
    if not metadata_filter:
        return None
    return {k: (list(v) if isinstance(v, (list, tuple, set)) else [v]) for k, v in metadata_filter.items()}


def _matches(meta: dict, flt: dict) -> bool:
    """JSON containment `metadata @> filter` (`_search.py:84-97`): every filter value must occur."""
    for key, wanted in flt.items():
        have = meta.get(key)
        have = list(have) if isinstance(have, (list, tuple, set)) else [have]
        if any(w not in have for w in wanted):
            return False
    return True


_filter_sets = threading.local()  # one `_ops.FilterSet` per thread, reused across calls: a warm evaluation allocates nothing


class _DeviceMask:
    """Stands where a filter's bool mask stands when its bitset is on the device: `n` chunks match (`any()` is what the searches'
    decisions ask of a mask)."""

    __slots__ = ("n",)

    def __init__(self, n: int) -> None:
        self.n = n

    def any(self) -> bool:
        return self.n > 0


def _filters_on_device(gi: GpuIndex, filters: Sequence[dict]):
    """Evaluate a call's distinct normalised filters on the device (`rl_metadata_filters`, one call): (the thread's `FilterSet` with
    filter j's bitset in row j, matching chunks [F], their embedding rows [F]).  None where the host path must answer: the index keeps
    no device metadata, or a filter is not encodable.  Tombstoned chunks count like any other, as in the loop over `gi.metadata`."""
    if gi._meta_store is None or not filters:  # noqa: SLF001
        return None
    encoded = gi._meta_vocab.encode_filters(filters)  # noqa: SLF001
    if encoded is None:
        return None
    fs, chunks, rows = gi._meta_store.filters(gi.index, *encoded, filter_set=getattr(_filter_sets, "set", None))  # noqa: SLF001
    _filter_sets.set = fs
    return fs, chunks, rows


VECTOR_SEARCH_OVERSAMPLE = 4  # vector_search's default `oversample`: what hybrid_search's vector half runs with (`_search.py:36-41`)


def vector_search(query: str | np.ndarray, *, num_results: int = 3, oversample: int = VECTOR_SEARCH_OVERSAMPLE,
                  metadata_filter: dict | None = None, config: Any | None = None,
                  index: GpuIndex | None = None) -> tuple[list[ChunkId], list[float]]:
    """Search chunks with an exact GPU scan (the reference's HNSW search is approximate)."""
    cfg = config or HotPathConfig()
    gi = index or _index_for(config)
    metadata_filter = _adapt_metadata(metadata_filter)
    if getattr(cfg, "self_query", False) and isinstance(query, str):
        raise NotImplementedError("self_query needs the LLM stack, which is outside this package")
    # Embed the query (`_search.py:54-56`).
    q = embed_strings([query], config=cfg)[0, :] if isinstance(query, str) else np.ravel(query)
    # Apply the query adapter (`_search.py:58-62`): result is cast back to the query dtype.
    if cfg.vector_search_query_adapter and gi.query_adapter is not None:
        q = _ops.adapter_apply(gi.query_adapter, np.asarray(q, dtype=np.float32)).astype(q.dtype)
    if gi.index.n_rows == 0:
        return [], []  # empty database (`tests/test_search.py:76-85`)
    # `_search.py:66-67`
    corrected_oversample = oversample * cfg.chunk_max_size / DEFAULT_CHUNK_MAX_SIZE
    num_hits = round(corrected_oversample) * max(num_results, 10)
    if num_hits < 1 or num_results < 1:
        return [], []
    if metadata_filter:
        return _filtered_search(gi, q, num_hits, num_results, metadata_filter)
    _check_limits(num_hits, num_results)
    scores, chunks, count = gi.index.search_chunks(np.asarray(q, dtype=np.float32), num_hits, num_results)
    n = int(count)
    return [gi.chunk_ids[c] for c in chunks[:n].tolist()], [float(s) for s in scores[:n]]


def _check_limits(num_hits: int, num_results: int) -> None:
    """The exact selection ranks at most K_MAX rows per query; asking for more is an error, not a silent truncation
    (the reference's `LIMIT num_hits` has no such bound: a documented limit of this implementation)."""
    if num_hits > _ops.K_MAX or num_results > _ops.K_MAX:
        raise ValueError(f"vector_search: num_results={num_results} needs the top {num_hits} rows, more than the "
                         f"{_ops.K_MAX} the exact top-k kernel ranks; lower num_results or oversample")


_NO_METADATA = "GpuIndex was built without `metadata`; metadata_filter cannot be applied"
_NO_KEYWORDS = "GpuIndex was built without keyword texts: pass keyword_texts= or from_store(..., keywords=True)"


def _keyword_limit_message(num_results: int) -> str:
    return (f"keyword_search: num_results={num_results} is more than the {_ops.K_MAX} the exact top-k kernel ranks; "
            "lower num_results")


FILTER_FIRST_MAX_ROWS = 100_000  # `metadata_count <= 100_000` (`src/raglite/_search.py:105`)
ORDER_FIRST_LIMIT = 1_000_000    # `.limit(1_000_000)` (`src/raglite/_search.py:124`)


def _filtered_search(gi: GpuIndex, q, num_hits: int, num_results: int, flt: dict):
    """The reference's filtered vector search (`_search.py:96-141`): evaluate the JSON containment on the host metadata and
    push the result down as a bitset over chunk ordinals.  Like the reference, count the matching embedding rows first
    (`:97-103`): up to 100 000 -> filter first, rank the matching rows (`:105-119`); more -> order first, i.e. only the
    1 000 000 rows nearest to the query are eligible, then the filter (`:120-141`).  Both branches rank exactly; they
    differ only on a corpus of more than 1 000 000 rows."""
    if gi.metadata is None:
        raise ValueError(_NO_METADATA)
    on_device = _filters_on_device(gi, [flt])
    if on_device is not None:  # the same decisions from the device's counts; the bitset goes to the search where it is
        fs, n_chunks, n_rows = on_device
        if n_chunks[0] == 0:
            return [], []
        _check_limits(num_hits, num_results)
        rank_limit = ORDER_FIRST_LIMIT if int(n_rows[0]) > FILTER_FIRST_MAX_ROWS else 0
        scores, chunks, count = gi.index.search_chunks(np.asarray(q, dtype=np.float32), num_hits, num_results,
                                                       query_filters=fs.select([0]), rank_limit=[rank_limit])
        n = int(count)
        return [gi.chunk_ids[c] for c in chunks[:n].tolist()], [float(s) for s in scores[:n]]
    allowed = np.fromiter((_matches(m, flt) for m in gi.metadata), dtype=bool, count=len(gi.metadata))
    if not allowed.any():
        return [], []
    _check_limits(num_hits, num_results)
    offsets = gi.index.chunk_offsets
    rows_per_chunk = np.diff(offsets) if offsets is not None else np.ones(len(allowed), dtype=np.int64)
    matching_rows = int(rows_per_chunk[allowed].sum())
    rank_limit = ORDER_FIRST_LIMIT if matching_rows > FILTER_FIRST_MAX_ROWS else None
    scores, chunks, count = gi.index.search_chunks(np.asarray(q, dtype=np.float32), num_hits, num_results,
                                                   chunk_filter=allowed, rank_limit=rank_limit)
    n = int(count)
    return [gi.chunk_ids[c] for c in chunks[:n].tolist()], [float(s) for s in scores[:n]]


def keyword_search(query: str, *, num_results: int = 3, metadata_filter: dict | None = None, config: Any | None = None,
                   index: GpuIndex | None = None) -> tuple[list[ChunkId], list[float]]:
    """Search chunks with BM25 (`src/raglite/_search.py:156-230`, DuckDB's `match_bm25` over `chunk.body`) on the device.  Chunks
    that contain no query stem are no result, so fewer than `num_results` may come back; equal scores rank by chunk ordinal."""
    cfg = config or HotPathConfig()
    gi = index or _index_for(config)
    metadata_filter = _adapt_metadata(metadata_filter)
    if getattr(cfg, "self_query", False) and isinstance(query, str):
        raise NotImplementedError("self_query needs the LLM stack, which is outside this package")
    if not gi.has_keywords:
        raise ValueError(_NO_KEYWORDS)
    if num_results < 1:
        return [], []
    if num_results > _ops.K_MAX:
        raise ValueError(_keyword_limit_message(num_results))
    ids = gi.keyword_query_ids(query)
    if not ids:
        return [], []
    allowed = None
    if metadata_filter:
        if gi.metadata is None:
            raise ValueError(_NO_METADATA)
        on_device = _filters_on_device(gi, [metadata_filter])
        if on_device is not None:
            if on_device[1][0] == 0:
                return [], []
            scores, chunks, counts = gi.keyword.search([ids], num_results, query_filters=on_device[0].select([0]))
            n = int(counts[0])
            return [gi.chunk_ids[c] for c in chunks[0, :n].tolist()], [float(x) for x in scores[0, :n]]
        allowed = np.fromiter((_matches(m, metadata_filter) for m in gi.metadata), dtype=bool, count=len(gi.metadata))
        if not allowed.any():
            return [], []
    scores, chunks, counts = gi.keyword.search([ids], num_results, chunk_filter=allowed)
    n = int(counts[0])
    return [gi.chunk_ids[c] for c in chunks[0, :n].tolist()], [float(x) for x in scores[0, :n]]


_device_keyword_search = keyword_search  # (hybrid_search's `keyword_search` argument shadows the name)


class GpuVectorSearch:
    """`BasicSearchMethod` for `RAGLiteConfig.search_method` (`src/raglite/_typing.py:35-43`,
    consumed at `src/raglite/_rag.py:53-63`)."""

    def __init__(self, index: GpuIndex, *, oversample: int = 4) -> None:
        self.index = index
        self.oversample = oversample

    def __call__(self, query: str | np.ndarray, *, num_results: int = 8, metadata_filter: dict | None = None,
                 config: Any | None = None) -> tuple[list[ChunkId], list[float]]:
        return vector_search(query, num_results=num_results, oversample=self.oversample,
                             metadata_filter=metadata_filter, config=config, index=self.index)


# ---- hybrid search ------------------------------------------------------------------------
def reciprocal_rank_fusion(rankings: Sequence[Sequence[ChunkId]], *, k: int = 60,
                           weights: Sequence[float] | None = None) -> tuple[list[ChunkId], list[float]]:
    """Reciprocal Rank Fusion (`src/raglite/_search.py:233-252`): score(id) = sum_r w_r / (k + rank_r(id)), ranked by
    descending score; ids with equal scores keep the order in which they were first seen (stable sort)."""
    if weights is None:
        weights = [1.0] * len(rankings)
    if len(weights) != len(rankings):
        raise ValueError("The number of weights must match the number of rankings.")
    score: dict[ChunkId, float] = {}
    for ranking, weight in zip(rankings, weights):
        for i, cid in enumerate(ranking):
            score[cid] = score.get(cid, 0.0) + weight / (k + i)
    if not score:
        return [], []
    ordered = sorted(score.items(), key=lambda kv: kv[1], reverse=True)
    return [cid for cid, _ in ordered], [s for _, s in ordered]


def hybrid_search(query: str | np.ndarray, *, num_results: int = 3, oversample: int = 2,
                  vector_search_weight: float = 0.75, keyword_search_weight: float = 0.25,
                  metadata_filter: dict | None = None, config: Any | None = None, index: GpuIndex | None = None,
                  keyword_search: Callable[..., tuple[list[ChunkId], list[float]]] | None = None,
                  ) -> tuple[list[ChunkId], list[float]]:
    """`src/raglite/_search.py:255-279`: GPU vector search fused with a BM25 keyword ranking by RRF.  The keyword ranking
    comes from `keyword_search=` when given (e.g. the reference's own SQL `keyword_search`), else from this package's
    `keyword_search` when the index has a keyword side; an index without one and no callable fuses the vector ranking alone."""
    vs_ids, _ = vector_search(query, num_results=oversample * num_results, metadata_filter=metadata_filter,
                              config=config, index=index)
    ks_ids: list[ChunkId] = []
    if keyword_search is not None:
        ks_ids, _ = keyword_search(query, num_results=oversample * num_results, metadata_filter=metadata_filter,
                                   config=config)
    elif isinstance(query, str) and (gi := index or _index_for(config)).has_keywords:
        ks_ids, _ = _device_keyword_search(query, num_results=oversample * num_results, metadata_filter=metadata_filter,
                                           config=config, index=gi)
    ids, scores = reciprocal_rank_fusion([vs_ids, ks_ids], weights=[vector_search_weight, keyword_search_weight])
    return ids[:num_results], scores[:num_results]


RRF_K = 60  # reciprocal_rank_fusion's `k` as hybrid_search calls it


def _embed_one_by_one(queries: Sequence[str], query_vectors, cfg: Any, gi: GpuIndex) -> np.ndarray:
    """The (B, dim) float32 query matrix vector_search would build query by query: each string embedded on its own (a list handed
    to embed_strings is one document's sentences under late chunking), then the query adapter applied per query (its batched route
    multiplies with other kernels than the single-query one) and cast back to the embedding's dtype."""
    if query_vectors is not None:
        if _ops._is_torch(query_vectors):  # noqa: SLF001
            query_vectors = query_vectors.detach().cpu().numpy()
        qv = np.asarray(query_vectors)
        if qv.ndim != 2 or qv.shape[0] != len(queries):
            raise ValueError("query_vectors must be (len(queries), dim)")
        rows = list(qv)
    else:
        rows = [embed_strings([q], config=cfg)[0, :] if isinstance(q, str) else np.ravel(q) for q in queries]
    if cfg.vector_search_query_adapter and gi.query_adapter is not None:
        rows = [_ops.adapter_apply(gi.query_adapter, np.asarray(q, dtype=np.float32)).astype(q.dtype) for q in rows]
    return np.stack([np.asarray(q, dtype=np.float32).ravel() for q in rows])


def _config_embedder(cfg: Any) -> Any | None:
    """`embedder_for(cfg)`, or None where no token-level embedder is installed (the loop then says so, if it gets that far)."""
    try:
        return _embed.embedder_for(cfg)
    except ModuleNotFoundError:
        return None


def _query_pack(queries: Sequence[Any], query_vectors, cfg: Any, embedder: Any | None = None):
    """The token matrices of a batch's text queries from ONE `embedder.embed_pack` call, as (indices of the string
    entries, their matrices, the embedder), or None where the batch embeds one by one: `query_vectors` given, no string entry, an
    embedder other than a late-chunking one with `embed_pack`, or a string whose single call would not be one whole segment (empty, or
    holding the sentinel: the loop raises for it, and so must the batch)."""
    if query_vectors is not None:
        return None
    at = [b for b, q in enumerate(queries) if isinstance(q, str)]
    if not at or _embed.embedding_type(config=cfg) != "late_chunking":
        return None
    texts = [queries[b] for b in at]
    if any(not t or _embed.SENTINEL in t for t in texts):
        return None
    embedder = embedder if embedder is not None else _config_embedder(cfg)
    embed_pack = getattr(embedder, "embed_pack", None)
    if embed_pack is None:
        return None
    mats = embed_pack(texts)
    if mats is None:
        return None
    if any(len(embedder.tokenize(t.encode(), add_bos=False)) == 0 for t in texts):  # (no token rows to apportion: the loop's business)
        return None
    if len(mats) != len(texts):
        raise ValueError("embed_pack must return one token matrix per text")
    return at, list(mats), embedder


def _pooled_pack(mats: Sequence[Any], cfg: Any, gi: GpuIndex) -> np.ndarray:
    """`_embed_one_by_one`'s rows for the strings whose token matrices are `mats`, as (B, dim) float32 with its bits: ONE `rl_pool_norm`
    over the B spans (a span's result does not depend on the other spans of a call; eps = 0 and the normalisation as
    `embed_strings_with_late_chunking` has them), the fp16 cast, the single-query adapter arithmetic for all rows in one launch
    (`rl_adapter_apply_rows`), the cast back to fp16 -- on the device where the matrices are, read back once."""
    lengths = np.asarray([len(m) for m in mats], dtype=np.int64)
    ends = np.cumsum(lengths)
    tokens = _embed._stack([_embed._token_matrix(m) for m in mats])  # noqa: SLF001
    adapt = cfg.vector_search_query_adapter and gi.query_adapter is not None
    if _embed._is_device_tensor(tokens):  # noqa: SLF001
        import torch

        b, e = torch.as_tensor(ends - lengths, device=tokens.device), torch.as_tensor(ends, device=tokens.device)
        _, pooled = _ops.pool_norm(tokens, b, e, normalize=bool(cfg.embedder_normalize), eps=0.0)
        if adapt:
            A = torch.as_tensor(np.ascontiguousarray(gi.query_adapter, dtype=np.float32)).to(tokens.device)  # noqa: N806
            pooled = _ops.adapter_apply(A, pooled.float(), rows=True)
        pooled = pooled.cpu().numpy()
    else:
        _, pooled = _ops.pool_norm(tokens, ends - lengths, ends, normalize=bool(cfg.embedder_normalize), eps=0.0)
        if adapt:
            pooled = _ops.adapter_apply(gi.query_adapter, pooled.astype(np.float32), rows=True)
    return pooled.astype(np.float16).astype(np.float32)  # (`.astype(q.dtype)`: the embedding's fp16; then the query matrix's float32)


def _embed_queries(queries: Sequence[Any], query_vectors, cfg: Any, gi: GpuIndex, pack=None) -> np.ndarray:
    """`_embed_one_by_one`'s matrix, bit for bit, with the batch's text queries through one packed native forward where the config's
    embedder offers one (`_query_pack`; `pack`: its result when the caller has made the call already, to share it).  Raw-vector
    entries, `query_vectors=`, every other embedder and a None from `embed_pack` go through `_embed_one_by_one` as before."""
    pack = pack if pack is not None else _query_pack(queries, query_vectors, cfg)
    if pack is None:
        return _embed_one_by_one(queries, query_vectors, cfg, gi)
    at, mats, _ = pack
    pooled = _pooled_pack(mats, cfg, gi)
    if len(at) == len(queries):
        return pooled
    rest = [b for b in range(len(queries)) if not isinstance(queries[b], str)]
    others = _embed_one_by_one([queries[b] for b in rest], None, cfg, gi)
    if others.shape[1] != pooled.shape[1]:
        raise ValueError("all input arrays must have the same shape")  # (np.stack's words in _embed_one_by_one)
    Q = np.empty((len(queries), pooled.shape[1]), dtype=np.float32)  # noqa: N806
    Q[at], Q[rest] = pooled, others
    return Q


# ---- batches with one metadata filter per query ------------------------------------------------------------------
def _batch_filters(metadata_filter, B: int) -> list[dict | None]:
    """A batch's metadata_filter -- None or one dict for every query, or a sequence of B entries, each None or a dict -- as the B
    normalised filters (`_adapt_metadata`)."""
    if metadata_filter is None or isinstance(metadata_filter, dict):
        return [_adapt_metadata(metadata_filter)] * B
    filters = list(metadata_filter)
    if len(filters) != B:
        raise ValueError(f"metadata_filter must be a dict or have one entry per query ({len(filters)} for {B} queries)")
    return [_adapt_metadata(f) for f in filters]


@dataclass
class FilterPlan:
    """The metadata filters of a batch: `allowed[j]` is distinct filter j's bool mask over chunks (None on an index without metadata,
    where applying a filter raises), `rank_limit[j]` its branch (ORDER_FIRST_LIMIT: order first; 0: filter first) and
    `query_filter[b]` the filter of query b (-1: none).  Evaluated on the device, `filter_set` holds filter j's bitset in row j and
    `allowed[j]` only says whether any chunk matches (`_DeviceMask`)."""

    allowed: list = field(default_factory=list)
    rank_limit: list = field(default_factory=list)
    query_filter: list = field(default_factory=list)
    filter_set: Any = None  # _ops.FilterSet

    def of(self, b: int):
        """(mask, rank limit) of query b: (None, 0) without a filter."""
        j = self.query_filter[b]
        return (None, 0) if j < 0 else (self.allowed[j], self.rank_limit[j])


def plan_filters(filters: Sequence[dict | None], metadata: Sequence[dict] | None, rows_per_chunk: np.ndarray,
                 index: GpuIndex | None = None) -> FilterPlan:
    """Evaluate each distinct normalised filter against the metadata once, take its filter-first / order-first decision once
    (`_search.py:97-141`: more than FILTER_FIRST_MAX_ROWS matching embedding rows -> order first) and map every query to its filter.
    With `index` (a GpuIndex that keeps its metadata on the device) all distinct filters are evaluated there by one call, unless one
    of them is not encodable; else by `_matches`, the JSON containment, chunk by chunk."""
    plan = FilterPlan()
    seen: dict[str, int] = {}
    distinct: list[dict] = []
    for flt in filters:
        if not flt:
            plan.query_filter.append(-1)
            continue
        key = repr(sorted(flt.items(), key=lambda kv: repr(kv[0])))
        if key not in seen:
            seen[key] = len(distinct)
            distinct.append(flt)
        plan.query_filter.append(seen[key])
    on_device = None if index is None or metadata is None else _filters_on_device(index, distinct)
    if on_device is not None:
        plan.filter_set, n_chunks, n_rows = on_device
        plan.allowed = [_DeviceMask(int(n)) for n in n_chunks]
        plan.rank_limit = [ORDER_FIRST_LIMIT if int(r) > FILTER_FIRST_MAX_ROWS else 0 for r in n_rows]
        return plan
    for flt in distinct:
        allowed = None
        if metadata is not None:
            allowed = np.fromiter((_matches(m, flt) for m in metadata), dtype=bool, count=len(metadata))
        plan.allowed.append(allowed)
        rows = 0 if allowed is None else int(rows_per_chunk[allowed].sum())
        plan.rank_limit.append(ORDER_FIRST_LIMIT if rows > FILTER_FIRST_MAX_ROWS else 0)
    return plan


def _rows_per_chunk(gi: GpuIndex) -> np.ndarray:
    offsets = gi.index.chunk_offsets
    return np.diff(offsets) if offsets is not None else np.ones(len(gi.chunk_ids), dtype=np.int64)


def _vector_searches(gi: GpuIndex, flt, allowed, num_hits: int, num_results: int) -> bool:
    """vector_search's decisions for one embedded query, in its order: True where it searches the device, False where it returns
    ([], []); raises where it raises."""
    if gi.index.n_rows == 0 or num_hits < 1 or num_results < 1:
        return False
    if flt:
        if gi.metadata is None:
            raise ValueError(_NO_METADATA)
        if not allowed.any():
            return False
    _check_limits(num_hits, num_results)
    return True


def _keyword_searches(gi: GpuIndex, flt, allowed, ids, num_results: int) -> bool:
    """keyword_search's decisions for one query, in its order (as _vector_searches)."""
    if not gi.has_keywords:
        raise ValueError(_NO_KEYWORDS)
    if num_results < 1:
        return False
    if num_results > _ops.K_MAX:
        raise ValueError(_keyword_limit_message(num_results))
    if not ids:
        return False
    if flt:
        if gi.metadata is None:
            raise ValueError(_NO_METADATA)
        if not allowed.any():
            return False
    return True


def _device_filters(plan: FilterPlan, queries: Sequence[int]):
    """(query_filters, rank_limit) of one batched device call over `queries`: (None, None) where none of them has a filter, which is
    the unfiltered call.  A query whose filter matches nothing keeps it: its lists come back empty, as the loop's do."""
    if all(plan.query_filter[b] < 0 for b in queries):
        return None, None
    if plan.filter_set is not None:  # the bitsets are on the device: the set with these queries' rows, no mask goes through the host
        return plan.filter_set.select([plan.query_filter[b] for b in queries]), [plan.of(b)[1] for b in queries]
    pairs = [plan.of(b) for b in queries]
    return [a for a, _ in pairs], [r for _, r in pairs]


def _self_query(cfg: Any, queries: Sequence[Any]) -> None:
    if getattr(cfg, "self_query", False) and any(isinstance(q, str) for q in queries):
        raise NotImplementedError("self_query needs the LLM stack, which is outside this package")


def _collect(gi: GpuIndex, out: list, active: Sequence[int], scores, chunks, counts) -> list:
    for i, b in enumerate(active):
        n = int(counts[i])
        out[b] = ([gi.chunk_ids[c] for c in chunks[i, :n].tolist()], [float(x) for x in scores[i, :n]])
    return out


def _plan_vector_batch(gi: GpuIndex, cfg: Any, queries: list, num_results: int, oversample: int, metadata_filter, query_vectors,
                       pack=None):
    """The host decisions of a batch of vector searches (B >= 1), in vector_search's order: (query matrix, num_hits, filter plan, the
    queries that search the device -- the others return ([], [])); raises where the loop would raise."""
    B = len(queries)
    filters = _batch_filters(metadata_filter, B)
    _self_query(cfg, queries)
    Q = _embed_queries(queries, query_vectors, cfg, gi, pack)
    num_hits = round(oversample * cfg.chunk_max_size / DEFAULT_CHUNK_MAX_SIZE) * max(num_results, 10)  # (`_search.py:66-67`)
    plan = plan_filters(filters, gi.metadata, _rows_per_chunk(gi), gi)
    active = [b for b in range(B) if _vector_searches(gi, filters[b], plan.of(b)[0], num_hits, num_results)]
    return Q, num_hits, plan, active


def vector_search_batch(queries: Sequence[str | np.ndarray], *, num_results: int = 3, oversample: int = VECTOR_SEARCH_OVERSAMPLE,
                        metadata_filter=None, config: Any | None = None, index: GpuIndex | None = None,
                        query_vectors=None) -> list[tuple[list[ChunkId], list[float]]]:
    """`vector_search` for a batch: element b is what `vector_search(queries[b], metadata_filter=<its filter>, ...)` returns with the
    same arguments (the same chunk ids, the same float scores), from one device call (`rl_search_chunks_per_query`).
    `metadata_filter`: None or one dict for every query, or one entry (None or a dict) per query; each distinct filter is evaluated
    once.  `query_vectors` ((B, dim)) skips the embedding.  Raises where the loop would raise for some element, with its message."""
    cfg = config or HotPathConfig()
    gi = index or _index_for(config)
    queries = list(queries)
    B = len(queries)
    if B == 0:
        return []
    Q, num_hits, plan, active = _plan_vector_batch(gi, cfg, queries, num_results, oversample, metadata_filter, query_vectors)
    out: list = [([], []) for _ in range(B)]
    if active:
        qf, lim = _device_filters(plan, active)
        scores, chunks, counts = gi.index.search_chunks(Q[active], num_hits, num_results, query_filters=qf, rank_limit=lim)
        _collect(gi, out, active, scores, chunks, counts)
    return out


def keyword_search_batch(queries: Sequence[str], *, num_results: int = 3, metadata_filter=None, config: Any | None = None,
                         index: GpuIndex | None = None) -> list[tuple[list[ChunkId], list[float]]]:
    """`keyword_search` for a batch: element b is what `keyword_search(queries[b], metadata_filter=<its filter>, ...)` returns, from
    one device call (`rl_keyword_search_per_query`); `metadata_filter` as in `vector_search_batch`."""
    cfg = config or HotPathConfig()
    gi = index or _index_for(config)
    queries = list(queries)
    B = len(queries)
    if B == 0:
        return []
    filters = _batch_filters(metadata_filter, B)
    _self_query(cfg, queries)
    plan = plan_filters(filters, gi.metadata, _rows_per_chunk(gi), gi)
    ids = [gi.keyword_query_ids(q) for q in queries] if gi.has_keywords else [[] for _ in queries]
    active = [b for b in range(B) if _keyword_searches(gi, filters[b], plan.of(b)[0], ids[b], num_results)]
    out: list = [([], []) for _ in range(B)]
    if active:
        qf, _ = _device_filters(plan, active)
        scores, chunks, counts = gi.keyword.search([ids[b] for b in active], num_results, query_filters=qf)
        _collect(gi, out, active, scores, chunks, counts)
    return out


@dataclass
class HybridPlan:
    """The host decisions of a batch of hybrid searches: what each half is asked for (`n_each`, `num_hits`), which halves run for at
    least one query (`vector`, `keyword`; R of them), the fused list's length `k`, the query matrix, term ids and filter plan."""

    Q: np.ndarray
    n_each: int
    num_hits: int
    plan: FilterPlan
    term_ids: list | None
    vector: bool
    keyword: bool
    R: int
    k: int


def _plan_hybrid_batch(gi: GpuIndex, cfg: Any, queries: list, num_results: int, oversample: int, metadata_filter,
                       query_vectors, pack=None) -> HybridPlan:
    """hybrid_search's decisions for every query of a batch (B >= 1), in its order; raises where the loop would raise."""
    B = len(queries)
    if getattr(cfg, "self_query", False):
        raise NotImplementedError("self_query needs the LLM stack, which is outside this package")
    filters = _batch_filters(metadata_filter, B)
    n_each = oversample * num_results  # what hybrid_search asks of each half
    Q = _embed_queries(queries, query_vectors, cfg, gi, pack)
    num_hits = round(VECTOR_SEARCH_OVERSAMPLE * cfg.chunk_max_size / DEFAULT_CHUNK_MAX_SIZE) * max(n_each, 10)
    plan = plan_filters(filters, gi.metadata, _rows_per_chunk(gi), gi)
    # (hybrid_search runs the keyword half for query strings only; a query given as a vector has none)
    term_ids = [gi.keyword_query_ids(q) if isinstance(q, str) else [] for q in queries] if gi.has_keywords else None
    vector = keyword = False
    for b in range(B):  # hybrid_search's decisions for each query, in its order: its vector half, then its keyword half
        allowed = plan.of(b)[0]
        vector = _vector_searches(gi, filters[b], allowed, num_hits, n_each) or vector
        if gi.has_keywords and isinstance(queries[b], str):
            keyword = _keyword_searches(gi, filters[b], allowed, term_ids[b], n_each) or keyword
    R = int(vector) + int(keyword)
    k = R * n_each if num_results < 1 else min(num_results, R * n_each)  # (hybrid_search slices the fused list [:num_results])
    return HybridPlan(Q, n_each, num_hits, plan, term_ids, vector, keyword, R, k)


def hybrid_search_batch(queries: Sequence[str], *, num_results: int = 3, oversample: int = 2,
                        vector_search_weight: float = 0.75, keyword_search_weight: float = 0.25,
                        metadata_filter=None, config: Any | None = None, index: GpuIndex | None = None,
                        query_vectors=None) -> list[tuple[list[ChunkId], list[float]]]:
    """`hybrid_search` for a batch of query strings: element b is what `hybrid_search(queries[b], ...)` returns with the same
    arguments (the same chunk ids, the same float scores).  The vector half, the keyword half and the RRF fusion of all queries run
    on one stream (`rl_hybrid_search`, `rl_hybrid_search_per_query`) and the results are read back once.  `metadata_filter`: None or
    one dict for every query, or one entry (None or a dict) per query -- element b is then `hybrid_search(queries[b],
    metadata_filter=<its entry>, ...)`; each distinct filter is evaluated once.  `query_vectors` ((B, dim), e.g. embeddings computed
    elsewhere) skips the embedding; the strings still give the keyword half.  An external `keyword_search=` callable is not part of
    the batched call (use `hybrid_search`)."""
    cfg = config or HotPathConfig()
    gi = index or _index_for(config)
    queries = list(queries)
    B = len(queries)
    if B == 0:
        return []
    hp = _plan_hybrid_batch(gi, cfg, queries, num_results, oversample, metadata_filter, query_vectors)
    if hp.R == 0:
        return [([], []) for _ in range(B)]
    qf, lim = _device_filters(hp.plan, range(B))
    if hp.vector:
        scores, chunks, counts = gi.index.hybrid_search(hp.Q, hp.num_hits, hp.n_each, hp.k, keyword=gi.keyword if hp.keyword else None,
                                                        query_term_ids=hp.term_ids, weights=(vector_search_weight, keyword_search_weight),
                                                        rrf_k=RRF_K, query_filters=qf, rank_limit=lim)
    else:  # no vector results for any query (an empty index, num_hits < 1): RRF of the keyword list alone is the same fusion
        _, kw_chunks, _ = gi.keyword.search(hp.term_ids, hp.n_each, query_filters=qf)
        scores, chunks, counts = _ops.rrf_fuse(kw_chunks[None], [keyword_search_weight], rrf_k=RRF_K, k=hp.k)
    out = []
    for b in range(B):
        n = int(counts[b])
        ids = [gi.chunk_ids[c] for c in chunks[b, :n].tolist()]
        out.append((ids[:num_results], [float(x) for x in scores[b, :n]][:num_results]))
    return out


# ---- reranking -------------------------------------------------------------------------------------------
@dataclass
class Result:
    """Shape of `rerankers.results.Result` that `_search.py:396` reads (`.doc_id`), plus score and rank."""

    doc_id: int
    score: float
    rank: int
    text: str = ""


@dataclass
class RankedResults:
    results: list[Result] = field(default_factory=list)
    query: str = ""

    def top_k(self, k: int) -> list[Result]:
        return self.results[:k]


def _groups_by_nq(vecs: Sequence[np.ndarray]) -> list[list[int]]:
    """The queries grouped by their number of token vectors, each group in query order: the calls of a ranker that takes no ragged
    route (`MaxSimRanker._routes`), one per group."""
    groups: dict[int, list[int]] = {}
    for b, v in enumerate(vecs):
        groups.setdefault(int(v.shape[0]), []).append(b)
    return list(groups.values())


class MaxSimRanker:
    """ColBERT-style late-interaction reranker behind the reference's reranker plugin boundary.

    `rank(query=, docs=)` scores every doc as  sum_i max_j q_i . d_j  over the query's token vectors
    q_i and the doc's chunklet vectors d_j (GPU: `rl_maxsim_rerank`) and returns them best-first.
    `query_encoder(query: str) -> (nq, dim)` supplies the query's multi-vector representation.

    `ragged`: a batch of queries of several lengths is ONE device call (`rl_maxsim_rerank_ragged`,
    `rl_search_rerank_ragged`) instead of one per distinct length, and a query of more than 32 vectors is scored on an fp16-stored
    index instead of raising.  Every query's score bits are those of the call for that query alone.  False: one call per length.
    """

    ragged = True

    def __init__(self, index: GpuIndex, query_encoder: Callable[[str], np.ndarray]) -> None:
        self.index = index
        self.query_encoder = query_encoder
        # set by `from_embedder`: the token-level embedder, and `(queries, mats=None) -> list of (nq, dim) | None`, every query's
        # `query_encoder` result from one `embedder.embed_pack` call (`mats`: that call's result where the caller made it already)
        self.embedder: Any | None = None
        self.query_batch_encoder: Callable[..., list | None] | None = None

    @classmethod
    def from_embedder(cls, index: GpuIndex, embedder: Any, *, normalize: bool = True, max_vectors: int | None = 32) -> "MaxSimRanker":
        """Query side from a token-level embedder (`raglite_amd.TorchTokenEmbedder`, or llama.cpp with pooling NONE):
        the query's token embeddings, L2-normalised like the stored chunklet vectors, at most `max_vectors` of them
        (the first tokens are kept; None: all of them -- nothing is padded, a query keeps its own length)."""

        def finish(m: np.ndarray) -> np.ndarray:
            m = m[:max_vectors]
            if normalize:
                m = m / np.maximum(np.linalg.norm(m, axis=1, keepdims=True), np.finfo(np.float32).eps)
            return m.astype(np.float32)

        def encode(query: str) -> np.ndarray:
            m = embedder.embed(query)
            return finish(m.float().cpu().numpy() if hasattr(m, "cpu") else np.asarray(m, dtype=np.float32))

        def encode_batch(queries: Sequence[str], mats: Sequence[Any] | None = None) -> list | None:
            """`encode` of every query from one `embed_pack` call: the same NumPy lines on the same token rows, so the same bits;
            None where the embedder has no pack route for these queries."""
            if mats is None:
                embed_pack = getattr(embedder, "embed_pack", None)
                mats = embed_pack(list(queries)) if embed_pack is not None else None
            if mats is None:
                return None
            if len(mats) and all(_ops._is_torch(m) for m in mats):  # noqa: SLF001 - one copy to the host, cut there
                import torch

                host = torch.cat([m.float() for m in mats]).cpu().numpy()
                mats = np.split(host, np.cumsum([len(m) for m in mats])[:-1])
            return [finish(np.asarray(m, dtype=np.float32)) for m in mats]

        ranker = cls(index, encode)
        ranker.embedder, ranker.query_batch_encoder = embedder, encode_batch
        return ranker

    def score(self, query: str, ordinals: Sequence[int]) -> np.ndarray:
        qv = np.asarray(self.query_encoder(query), dtype=np.float32)
        qv = qv.reshape(1, *qv.shape) if qv.ndim == 2 else qv.reshape(1, 1, -1)
        cand = np.asarray(ordinals, dtype=np.int32).reshape(1, -1)
        dev = self.index.index
        if self.ragged and isinstance(dev, _ops.DeviceIndex) and dev.storage == "f16" and qv.shape[1] > 32:
            return np.asarray(_ragged.maxsim_rerank_ragged(dev, [qv[0]], cand))[0]  # (`maxsim_rerank` stops at 32 vectors there)
        return np.asarray(dev.maxsim_rerank(qv, cand))[0]

    def _routes(self, vecs: Sequence[np.ndarray]) -> list[tuple[list[int], bool]]:
        """How a batch is scored: (queries in query order, ragged?) per device call.  Queries of one length, a ranker with `ragged`
        off and an index that is no `DeviceIndex`: one `maxsim_rerank` shape per distinct length, as ever.  Otherwise ONE ragged call
        for every query of at most 32 vectors and, on an fp16-stored index, the longer ones too; on an fp32-stored index those keep
        their per-length calls, whose kernel `score` takes for them as well (their last bits differ from a sum of slabs)."""
        groups = _groups_by_nq(vecs)
        dev = self.index.index
        if not self.ragged or not isinstance(dev, _ops.DeviceIndex):
            return [(g, False) for g in groups]
        f16 = dev.storage == "f16"
        if len(groups) == 1 and not (f16 and int(vecs[groups[0][0]].shape[0]) > 32):
            return [(groups[0], False)]
        ragged = [b for b, v in enumerate(vecs) if f16 or int(v.shape[0]) <= 32]
        taken = set(ragged)
        rest = [(g, False) for g in groups if g[0] not in taken]
        return rest + ([(ragged, True)] if ragged else [])

    def _token_vectors(self, queries: Sequence[Any], query_token_vectors=None, mats: Sequence[Any] | None = None) -> list[np.ndarray]:
        """Each query's (nq, dim) float32 token vectors: `query_token_vectors[b]` when given; else, for a ranker made by `from_embedder`
        whose embedder packs these queries, all of them from one forward (`query_batch_encoder`; `mats`: the token matrices of that
        forward where the caller has made it already); else `query_encoder(queries[b])`, one query at a time."""
        if query_token_vectors is not None and len(query_token_vectors) != len(queries):
            raise ValueError("query_token_vectors must have one (nq, dim) matrix per query")
        if query_token_vectors is None and self.query_batch_encoder is not None and len(queries) and all(isinstance(q, str) for q in queries):
            query_token_vectors = self.query_batch_encoder(queries, mats)
        out = []
        for b, q in enumerate(queries):
            v = query_token_vectors[b] if query_token_vectors is not None else self.query_encoder(q)
            if _ops._is_torch(v):  # noqa: SLF001
                v = v.detach().cpu().numpy()
            v = np.asarray(v, dtype=np.float32)
            out.append(v if v.ndim == 2 else v.reshape(1, -1))
        return out

    def _score_and_order(self, vecs: Sequence[np.ndarray], ordinals: Sequence[Sequence[int]]):
        """Per query (its candidates' scores in list order, their positions best first): one scoring call and one `rl_rerank_order`
        per route (`_routes`: one `rl_maxsim_rerank_ragged` for a batch of mixed lengths, one `rl_maxsim_rerank` for a uniform one).
        Short lists are padded with -1; short queries are NOT padded with zero vectors (that could change the summation order and so
        the score bits): each keeps its own length."""
        lists = [np.asarray(o, dtype=np.int32).ravel() for o in ordinals]
        if len(lists) != len(vecs):
            raise ValueError("one list of candidates per query is required")
        out: list = [(np.zeros(0, np.float32), np.zeros(0, np.int32)) for _ in lists]
        for group, ragged in self._routes(vecs):
            n_cand = max(len(lists[b]) for b in group)
            if n_cand == 0:
                continue
            if n_cand > _ops.RERANK_MAX_ENTRIES:
                raise ValueError(f"MaxSimRanker: at most {_ops.RERANK_MAX_ENTRIES} candidates per query can be ordered on the device")
            cand = np.full((len(group), n_cand), -1, dtype=np.int32)
            for i, b in enumerate(group):
                cand[i, : len(lists[b])] = lists[b]
            if ragged:
                scores = np.asarray(_ragged.maxsim_rerank_ragged(self.index.index, [vecs[b] for b in group], cand))
            else:
                scores = np.asarray(self.index.index.maxsim_rerank(np.stack([vecs[b] for b in group]), cand))
            _, _, pos, counts = _ops.rerank_order(scores, cand, n_cand)
            for i, b in enumerate(group):
                out[b] = (scores[i, : len(lists[b])], pos[i, : int(counts[i])])
        return out

    def score_batch(self, queries: Sequence[str], ordinals: Sequence[Sequence[int]], *, query_token_vectors=None) -> list[np.ndarray]:
        """`score(queries[b], ordinals[b])` for every b (ragged lists): one `rl_maxsim_rerank_ragged` for queries of mixed lengths,
        one `rl_maxsim_rerank` where they all have the same (`_routes`)."""
        return [s for s, _ in self._score_and_order(self._token_vectors(queries, query_token_vectors), ordinals)]

    def rank_batch(self, queries: Sequence[str], docs_per_query: Sequence[Sequence[Any]], *, query_token_vectors=None) -> list[RankedResults]:
        """`rank(query=queries[b], docs=docs_per_query[b])` for every b: the same `RankedResults`, from one scoring call and one
        `rl_rerank_order` for the batch, whatever the queries' lengths (`_routes`), instead of one call and one host sort per query."""
        queries, docs_per_query = list(queries), [list(d) for d in docs_per_query]
        if len(queries) != len(docs_per_query):
            raise ValueError("one list of docs per query is required")
        ordinals = [[self.index.ordinal_of_doc(d if isinstance(d, str) else str(d)) for d in docs] for docs in docs_per_query]
        ranked = self._score_and_order(self._token_vectors(queries, query_token_vectors), ordinals)
        return [RankedResults([Result(doc_id=int(i), score=float(scores[i]), rank=r + 1, text=str(docs[i])) for r, i in enumerate(order)], q)
                for q, docs, (scores, order) in zip(queries, docs_per_query, ranked)]

    def rank(self, query: str, docs: Sequence[Any], doc_ids: Sequence[int] | None = None, **_: Any) -> RankedResults:
        docs = list(docs)
        if not docs:
            return RankedResults([], query)
        ordinals = [self.index.ordinal_of_doc(d if isinstance(d, str) else str(d)) for d in docs]
        scores = self.score(query, ordinals)
        # best first; equal scores keep input order (stable), NaN last
        key = np.where(np.isnan(scores), -np.inf, scores)
        order = np.lexsort((np.arange(len(docs)), -key))
        ids = list(doc_ids) if doc_ids is not None else list(range(len(docs)))
        return RankedResults(
            [Result(doc_id=ids[i], score=float(scores[i]), rank=r + 1, text=str(docs[i])) for r, i in enumerate(order)],
            query,
        )


_language_detector: Callable[[str], str] | None = None
_language_detector_set = False


def set_language_detector(detect: Callable[[str], str] | None) -> None:
    """Install the callable `rerank_chunks` uses to pick a language-specific reranker from a `dict` of rerankers
    (`src/raglite/_search.py:379-392`).  The reference imports `langdetect.detect`; any `str -> language code` callable
    works (fastText, lingua, a customer's own).  None restores the default (langdetect if installed, else no detection)."""
    global _language_detector, _language_detector_set
    _language_detector, _language_detector_set = detect, detect is not None


def _default_language_detector() -> Callable[[str], str] | None:
    if _language_detector_set:
        return _language_detector
    try:
        from langdetect import detect  # the reference's dependency (`_search.py:13`); not in this image

        return detect
    except ImportError:
        return None


def select_reranker(reranker: Any, query: str, chunks: Sequence[Any], detect: Callable[[str], str] | None = None) -> Any:
    """The reference's reranker selection (`src/raglite/_search.py:378-392`): a `dict` maps language codes (and "other")
    to rankers; when every chunk and the query are detected as ONE language that has an entry, that ranker is used,
    otherwise the "other" entry.  A failing detector (the reference suppresses `LangDetectException`) or no detector at
    all falls back to "other"."""
    if not isinstance(reranker, dict):
        return reranker
    detect = detect or _default_language_detector()
    langs: set[str] = set()
    if detect is not None:
        try:
            langs = {detect(str(chunk)) for chunk in chunks}
            langs.add(detect(query))
        except Exception:  # noqa: BLE001 - e.g. langdetect's LangDetectException on text without letters
            langs = set()
    if len(langs) == 1 and (lang := next(iter(langs))) in reranker:
        return reranker[lang]
    return reranker.get("other")


def rerank_chunks(query: str, chunk_ids: Sequence[Any], *, config: Any | None = None,
                  chunk_lookup: Callable[[Sequence[ChunkId]], list[Any]] | None = None,
                  detect: Callable[[str], str] | None = None) -> list[Any]:
    """Rerank chunks according to their relevance to a query (`src/raglite/_search.py:364-397`).

    `chunk_ids` may be chunk ids or chunk objects (anything whose `str()` is the chunk text).  Ids are
    resolved through `chunk_lookup` (the reference uses `retrieve_chunks`, a SQL query, out of scope).
    `detect`: language detector for a `dict` of rerankers (default: `set_language_detector` / langdetect)."""
    cfg = config or HotPathConfig()
    chunks = list(chunk_ids)
    if chunks and all(isinstance(c, ChunkId) for c in chunks):
        if chunk_lookup is None:
            raise ValueError("chunk ids need a chunk_lookup callable (the reference's retrieve_chunks)")
        chunks = chunk_lookup(chunks)
    reranker = getattr(cfg, "reranker", None)
    if not reranker or not chunks:
        return chunks
    reranker = select_reranker(reranker, query, chunks, detect)
    if reranker:
        results = reranker.rank(query=query, docs=[str(chunk) for chunk in chunks])
        chunks = [chunks[result.doc_id] for result in results.results]
    return chunks


def search_and_rerank_chunks(query: str, *, num_results: int = 8, oversample: int = 4,
                             search: Callable[..., tuple[list[ChunkId], list[float]]] = vector_search,
                             config: Any | None = None, metadata_filter: dict | None = None,
                             chunk_lookup: Callable[[Sequence[ChunkId]], list[Any]] | None = None) -> list[Any]:
    """`src/raglite/_search.py:400-414` (the default `search` there is hybrid_search; pass `search=hybrid_search` over an index
    with a keyword side for the same pipeline on the device)."""
    chunk_ids, _ = search(query, num_results=oversample * num_results, metadata_filter=metadata_filter, config=config)
    return rerank_chunks(query, chunk_ids, config=config, chunk_lookup=chunk_lookup)[:num_results]


def _device_ranker(cfg: Any, gi: GpuIndex) -> "MaxSimRanker | None":
    """`cfg.reranker` when it is a MaxSimRanker over the searched index: the case the device pipeline covers."""
    reranker = getattr(cfg, "reranker", None)
    return reranker if isinstance(reranker, MaxSimRanker) and reranker.index is gi else None


def _native_cross_encoder(cfg: Any) -> Any | None:
    """`cfg.reranker` when it is ONE `TorchCrossEncoderRanker` with `forward == "native"` (not a dict by language): the case the
    batched cross-encoder path covers."""
    reranker = getattr(cfg, "reranker", None)
    if reranker is None or isinstance(reranker, (dict, MaxSimRanker)):
        return None
    from raglite_amd._cross_encoder import TorchCrossEncoderRanker

    return reranker if isinstance(reranker, TorchCrossEncoderRanker) and reranker.forward == "native" else None


def _cross_encoder_rerank_batch(ranker: Any, queries: Sequence[str], found: Sequence[Sequence[Any]],
                                chunk_lookup: Callable[[Sequence[ChunkId]], list[Any]] | None) -> tuple[list[list[Any]], list[RankedResults]]:
    """`rerank_chunks` for every query with ONE `rank_batch`: per query the ids are resolved through `chunk_lookup` (once, as there),
    `str(chunk)` is the doc, and the chunks come back best first; also the `RankedResults` (their `doc_id`s index the query's list)."""
    resolved = []
    for ids in found:
        chunks = list(ids)
        if chunks and all(isinstance(c, ChunkId) for c in chunks):
            if chunk_lookup is None:
                raise ValueError("chunk ids need a chunk_lookup callable (the reference's retrieve_chunks)")
            chunks = chunk_lookup(chunks)
        resolved.append(chunks)
    ranked = ranker.rank_batch(queries, [[str(chunk) for chunk in chunks] for chunks in resolved])
    return [[chunks[r.doc_id] for r in res.results] for chunks, res in zip(resolved, ranked)], ranked


def rerank_chunks_batch(queries: Sequence[str], chunk_ids_per_query: Sequence[Sequence[ChunkId]], *, config: Any,
                        index: GpuIndex | None = None, query_token_vectors=None,
                        chunk_lookup: Callable[[Sequence[ChunkId]], list[Any]] | None = None) -> list[tuple[list[ChunkId], list[float]]]:
    """MaxSim-rerank a batch of (ragged) chunk id lists: element b is (ids best first, their MaxSim scores), the order
    `config.reranker.rank(queries[b], <those chunks' docs>)` gives.  `config.reranker` must be a `MaxSimRanker` over `index`; one
    scoring call and one `rl_rerank_order` for the batch: `rl_maxsim_rerank_ragged` where the queries' lengths differ
    (`MaxSimRanker._routes`).  `query_token_vectors`: one (nq, dim) matrix per query, of any lengths, skips the ranker's query encoder.

    Or `config.reranker` is a `TorchCrossEncoderRanker(forward="native")`, with a `chunk_lookup` for the ids' texts: element b is (ids
    best first, their cross-encoder scores), from one `rank_batch` -- one native forward per pack of pairs, not per query (no index is
    needed or looked at)."""
    cross = _native_cross_encoder(config)
    if cross is not None:
        queries, id_lists = list(queries), [list(ids) for ids in chunk_ids_per_query]
        if len(queries) != len(id_lists):
            raise ValueError("one list of chunk ids per query is required")
        _, ranked = _cross_encoder_rerank_batch(cross, queries, id_lists, chunk_lookup)
        return [([ids[r.doc_id] for r in res.results], [r.score for r in res.results]) for ids, res in zip(id_lists, ranked)]
    gi = index or _index_for(config)
    ranker = _device_ranker(config, gi)
    if ranker is None:
        raise ValueError("rerank_chunks_batch needs config.reranker to be a MaxSimRanker over the index, or a native cross-encoder")
    queries, id_lists = list(queries), [list(ids) for ids in chunk_ids_per_query]
    if len(queries) != len(id_lists):
        raise ValueError("one list of chunk ids per query is required")
    ordinals = [[gi.ordinal_of(cid) for cid in ids] for ids in id_lists]
    ranked = ranker._score_and_order(ranker._token_vectors(queries, query_token_vectors), ordinals)  # noqa: SLF001
    return [([ids[i] for i in order.tolist()], [float(scores[i]) for i in order.tolist()]) for ids, (scores, order) in zip(id_lists, ranked)]


_SEARCHES = {"hybrid": "hybrid", "vector": "vector", hybrid_search: "hybrid", vector_search: "vector"}


def search_and_rerank_chunks_batch(queries: Sequence[str], *, num_results: int = 8, oversample: int = 4, search: Any = "hybrid",
                                   config: Any | None = None, metadata_filter=None, index: GpuIndex | None = None, query_vectors=None,
                                   query_token_vectors=None,
                                   chunk_lookup: Callable[[Sequence[ChunkId]], list[Any]] | None = None) -> list[list[Any]]:
    """`search_and_rerank_chunks` for a batch: element b is what `search_and_rerank_chunks(queries[b], search=hybrid_search |
    vector_search, metadata_filter=<its filter>, ...)` returns with the same arguments -- the same chunks in the same order -- as
    chunk ids, or as `chunk_lookup(ids)` per query when a lookup is given.  `search`: "hybrid" or "vector" (or those two functions).

    With `config.reranker` a `MaxSimRanker` over the searched index, the searches, the RRF fusion, the MaxSim scoring of every query's
    `oversample * num_results` candidates and their ordering run on one stream in one device call -- `rl_search_rerank_per_query`
    where every query has the same number of token vectors, `rl_search_rerank_ragged` where they differ (`MaxSimRanker._routes`;
    with `ranker.ragged` off, one call per distinct length) -- nothing is read back in between, and the best `num_results` are read
    back once.  Query token vectors come from the ranker's `query_encoder`, one query at a time, or from `query_token_vectors` (one
    (nq, dim) matrix per query, of any lengths).
    Without a reranker the batched search's results are returned truncated.  With `config.reranker` ONE
    `TorchCrossEncoderRanker(forward="native")` the batched search runs, then one `rank_batch` over all queries' found chunks: one native
    forward per pack of (query, chunk) pairs instead of one rerank per query.  Any other reranker (a dict by language, a
    cross-encoder with `forward="torch"`, anything with only `rank`) is outside the device path: the batched search runs, then
    `rerank_chunks` per query.  `metadata_filter` and `query_vectors` as in
    `hybrid_search_batch`.  Raises where the loop would raise for some element, with its message."""
    cfg = config or HotPathConfig()
    gi = index or _index_for(config)
    queries = list(queries)
    B = len(queries)
    if search not in _SEARCHES:
        raise ValueError("search must be 'hybrid' or 'vector'")
    kind = _SEARCHES[search]
    if B == 0:
        return []
    n_cand = oversample * num_results  # what search_and_rerank_chunks asks of its search
    ranker = _device_ranker(cfg, gi)
    found: list[list[ChunkId]]
    if ranker is None:
        batch = hybrid_search_batch if kind == "hybrid" else vector_search_batch
        found = [ids for ids, _ in batch(queries, num_results=n_cand, metadata_filter=metadata_filter, config=cfg, index=gi,
                                         query_vectors=query_vectors)]
        if getattr(cfg, "reranker", None) and any(found):
            cross = _native_cross_encoder(cfg)
            if cross is not None:  # one rank_batch for all queries' found chunks: one native forward per pack
                return [chunks[:num_results] for chunks in _cross_encoder_rerank_batch(cross, queries, found, chunk_lookup)[0]]
            return [rerank_chunks(q, ids, config=cfg, chunk_lookup=chunk_lookup)[:num_results] for q, ids in zip(queries, found)]
    elif kind == "hybrid":
        found = _hybrid_rerank_device(gi, cfg, ranker, queries, num_results, n_cand, metadata_filter, query_vectors, query_token_vectors)
    else:
        found = _vector_rerank_device(gi, cfg, ranker, queries, num_results, n_cand, metadata_filter, query_vectors, query_token_vectors)
    found = [ids[:num_results] for ids in found]
    return [chunk_lookup(ids) if chunk_lookup is not None and ids else ids for ids in found]


def _shared_pack(cfg: Any, ranker: "MaxSimRanker", queries: Sequence[Any], query_vectors, query_token_vectors):
    """One forward for both sides of a batched search-and-rerank: where the ranker was made `from_embedder` over the very embedder the
    config embeds queries with, every query is a string and neither side's vectors are given, (`_query_pack`'s result for the pooled
    query matrix, the same token matrices for the MaxSim vectors); else (None, None) and each side embeds for itself."""
    if query_vectors is not None or query_token_vectors is not None or ranker.query_batch_encoder is None:
        return None, None
    if not all(isinstance(q, str) for q in queries) or _embed.embedding_type(config=cfg) != "late_chunking":
        return None, None
    embedder = _config_embedder(cfg)
    if embedder is None or embedder is not ranker.embedder:
        return None, None
    pack = _query_pack(queries, None, cfg, embedder)
    return (pack, pack[1]) if pack is not None else (None, None)


def _ids_of(gi: GpuIndex, out: list, group: Sequence[int], chunks, counts) -> None:
    for i, b in enumerate(group):
        out[b] = [gi.chunk_ids[c] for c in chunks[i, : int(counts[i])].tolist()]


def _rerank_calls(device_index: Any, ragged: bool):
    """(search_rerank, search_rerank_spans, maxsim_rerank) of a route: the index's own calls, which take a (B, nq, dim) block, or the
    ragged ones, which take a list of (nq_b, dim) matrices (looked up when called: `_ragged`'s functions stay replaceable)."""
    if not ragged:
        return (lambda *a, **kw: device_index.search_rerank(*a, **kw), lambda *a, **kw: device_index.search_rerank_spans(*a, **kw),
                lambda *a, **kw: device_index.maxsim_rerank(*a, **kw))
    return (lambda *a, **kw: _ragged.search_rerank_ragged(device_index, *a, **kw),
            lambda *a, **kw: _ragged.search_rerank_spans_ragged(device_index, *a, **kw),
            lambda *a, **kw: _ragged.maxsim_rerank_ragged(device_index, *a, **kw))


def _hybrid_rerank_device(gi, cfg, ranker, queries, num_results, n_cand, metadata_filter, query_vectors, query_token_vectors,
                          spans: "_SpanRequest | None" = None) -> list:
    """The device path of search_and_rerank_chunks_batch over hybrid_search: its host decisions are hybrid_search_batch's.  With
    `spans` each group's call is the span pipeline and the result is every query's spans."""
    B = len(queries)
    pack, mats = _shared_pack(cfg, ranker, queries, query_vectors, query_token_vectors)
    hp = _plan_hybrid_batch(gi, cfg, queries, n_cand, 2, metadata_filter, query_vectors, pack)  # (hybrid_search's own oversample: 2)
    out: list = [[] for _ in range(B)]
    if hp.R == 0:
        return out
    k = min(num_results, hp.k)
    vecs = ranker._token_vectors(queries, query_token_vectors, mats)  # noqa: SLF001
    for group, ragged in ranker._routes(vecs):  # noqa: SLF001
        qf, lim = _device_filters(hp.plan, group)
        V = [vecs[b] for b in group] if ragged else np.stack([vecs[b] for b in group])
        pipeline, pipeline_spans, rerank = _rerank_calls(gi.index, ragged)
        terms = None if hp.term_ids is None else [hp.term_ids[b] for b in group]
        if hp.vector and spans is not None:
            res = pipeline_spans(hp.Q[group], hp.num_hits, hp.n_each, hp.k, V, k, spans.table, spans.neighbors,
                                 keyword=gi.keyword if hp.keyword else None, query_term_ids=terms, weights=(0.75, 0.25),
                                 rrf_k=RRF_K, query_filters=qf, rank_limit=lim)
            _spans_of(gi, out, group, *res[2:6])
            continue
        if hp.vector:
            _, chunks, counts = pipeline(hp.Q[group], hp.num_hits, hp.n_each, hp.k, V, k, keyword=gi.keyword if hp.keyword else None,
                                         query_term_ids=terms, weights=(0.75, 0.25), rrf_k=RRF_K, query_filters=qf,
                                         rank_limit=lim)
        else:  # no vector results for any query: the keyword list alone, fused, scored and ordered by separate calls
            _, kw_chunks, _ = gi.keyword.search(terms, hp.n_each, query_filters=qf)
            _, fused, _ = _ops.rrf_fuse(kw_chunks[None], [0.25], rrf_k=RRF_K, k=hp.k)
            _, chunks, _, counts = _ops.rerank_order(rerank(V, fused), fused, k)
        if spans is not None:  # (the ordered list is padded with -1 past its count)
            _spans_of(gi, out, group, *spans.table.chunk_spans(chunks, spans.neighbors)[:4])
        else:
            _ids_of(gi, out, group, chunks, counts)
    return out


def _vector_rerank_device(gi, cfg, ranker, queries, num_results, n_cand, metadata_filter, query_vectors, query_token_vectors,
                          spans: "_SpanRequest | None" = None) -> list:
    """The device path over vector_search: its host decisions are vector_search_batch's; the pipeline call without a keyword index
    fuses the vector list alone, which keeps its order.  `spans` as in _hybrid_rerank_device."""
    B = len(queries)
    pack, mats = _shared_pack(cfg, ranker, queries, query_vectors, query_token_vectors)
    Q, num_hits, plan, active = _plan_vector_batch(gi, cfg, queries, n_cand, VECTOR_SEARCH_OVERSAMPLE, metadata_filter, query_vectors,
                                                   pack)
    out: list = [[] for _ in range(B)]
    if not active:
        return out
    k = min(num_results, n_cand)
    vecs = ranker._token_vectors([queries[b] for b in active],  # noqa: SLF001
                                 None if query_token_vectors is None else [query_token_vectors[b] for b in active],
                                 None if mats is None else [mats[b] for b in active])
    for group, ragged in ranker._routes(vecs):  # noqa: SLF001
        members = [active[i] for i in group]
        qf, lim = _device_filters(plan, members)
        V = [vecs[i] for i in group] if ragged else np.stack([vecs[i] for i in group])
        pipeline, pipeline_spans, _ = _rerank_calls(gi.index, ragged)
        if spans is not None:
            res = pipeline_spans(Q[members], num_hits, n_cand, n_cand, V, k, spans.table, spans.neighbors, weights=(1.0,), rrf_k=RRF_K,
                                 query_filters=qf, rank_limit=lim)
            _spans_of(gi, out, members, *res[2:6])
            continue
        _, chunks, counts = pipeline(Q[members], num_hits, n_cand, n_cand, V, k, weights=(1.0,), rrf_k=RRF_K, query_filters=qf,
                                     rank_limit=lim)
        _ids_of(gi, out, members, chunks, counts)
    return out


# ---- chunk spans ---------------------------------------------------------------------------------------
@dataclass
class ChunkSpan:
    """A run of consecutive chunks of one document (the reference's `ChunkSpan`, `_database.py`, without its ORM objects):
    the chunks' ids in ascending `Chunk.index`, their document's id, and the span's score -- the sum of its chunks' reciprocal
    ranks, which is what `retrieve_chunk_spans` orders the spans by (`_search.py:355-360`)."""

    chunk_ids: list[ChunkId]
    document_id: str
    score: float


@dataclass
class _SpanRequest:
    table: Any      # _ops.SpanTable
    neighbors: Any  # the offsets as given: a tuple of ints, () or None


def _spans_of(gi: GpuIndex, out: list, group: Sequence[int], chunks, span_len, span_scores, n_spans) -> None:
    """The spans of each query of a device call, from rl_chunk_spans' outputs (host arrays; turned into lists once: per-row NumPy
    slicing would cost more than the device call)."""
    rows, lens, scores, counts = chunks.tolist(), span_len.tolist(), span_scores.tolist(), n_spans.tolist()
    ids, positions = gi.chunk_ids, gi.positions
    for i, b in enumerate(group):
        row, at, spans = rows[i], 0, []
        for s in range(counts[i]):
            ords = row[at : at + lens[i][s]]
            at += lens[i][s]
            spans.append(ChunkSpan([ids[c] for c in ords], positions[ords[0]][0], scores[i][s]))
        out[b] = spans


def retrieve_chunk_spans_batch(chunk_ids_per_query: Sequence[Sequence[Any]], *, neighbors: Sequence[int] | None = (-1, 1),
                               config: Any | None = None, index: GpuIndex | None = None) -> list[list[ChunkSpan]]:
    """`retrieve_chunk_spans` for a batch of (ragged) lists: element b is `retrieve_chunk_spans(chunk_ids_per_query[b], ...)`, from one
    device call (`rl_chunk_spans`; short lists are padded with -1, which takes no rank)."""
    gi = index or _index_for(config)
    lists = [list(ids) for ids in chunk_ids_per_query]
    out: list = [[] for _ in lists]
    if not any(lists):
        return out
    table = gi.span_table()
    ordinals = []
    for ids in lists:
        if all(isinstance(c, ChunkId) for c in ids):
            # ids: `retrieve_chunks` (`_search.py:282-299`) returns each stored chunk once, in the order of its first occurrence
            ordinals.append([gi._id_to_ordinal[c] for c in dict.fromkeys(ids) if c in gi._id_to_ordinal])  # noqa: SLF001
        else:
            # chunk objects are taken as they come (`:321`): of one that comes twice the last rank stands (`:324`)
            ordinals.append([gi._id_to_ordinal.get(getattr(c, "id", c), -1) for c in ids])  # noqa: SLF001
    n_in = max(len(o) for o in ordinals)
    if n_in == 0:
        return out
    chunks = np.full((len(lists), n_in), -1, dtype=np.int32)
    for b, o in enumerate(ordinals):
        chunks[b, : len(o)] = o
    _spans_of(gi, out, range(len(lists)), *table.chunk_spans(chunks, neighbors)[:4])
    return out


def retrieve_chunk_spans(chunk_ids: Sequence[Any], *, neighbors: Sequence[int] | None = (-1, 1), config: Any | None = None,
                         index: GpuIndex | None = None) -> list[ChunkSpan]:
    """Group chunks into spans of consecutive chunks and order the spans by the summed reciprocal ranks of their chunks
    (`src/raglite/_search.py:302-361`), on the device (`rl_chunk_spans`).  `chunk_ids`: chunk ids, best first -- de-duplicated to
    their first occurrence, unknown ids dropped, as the reference's `retrieve_chunks` does -- or chunk objects with an `.id`.
    `neighbors`: the offsets in `Chunk.index` of the chunks to add (None or (): none).  Chunks that have no embedding are not in the
    index and so are never neighbours here."""
    if not chunk_ids:
        return []
    return retrieve_chunk_spans_batch([chunk_ids], neighbors=neighbors, config=config, index=index)[0]


@dataclass
class _ChunkRef:
    """What a reranker outside the device path sees of a chunk: `str()` is its text; `.id` leads back to it."""

    id: ChunkId
    text: str

    def __str__(self) -> str:
        return self.text


def _ref_lookup(gi: GpuIndex) -> Callable[[Sequence[ChunkId]], list[Any]]:
    return lambda ids: [_ChunkRef(c, gi.docs[gi.ordinal_of(c)] if gi.docs is not None else c) for c in ids]


def search_and_rerank_chunk_spans(query: str, *, num_results: int = 8, oversample: int = 4, neighbors: Sequence[int] | None = (-1, 1),
                                  search: Callable[..., tuple[list[ChunkId], list[float]]] = hybrid_search, config: Any | None = None,
                                  metadata_filter: dict | None = None, index: GpuIndex | None = None) -> list[ChunkSpan]:
    """`src/raglite/_search.py:417-433`: search, rerank, keep the best `num_results`, collate them into chunk spans."""
    gi = index or _index_for(config)
    gi.span_table()
    if index is not None:  # (the search looks its index up by config unless told)
        search = partial(search, index=index)
    chunks = search_and_rerank_chunks(query, num_results=num_results, oversample=oversample, search=search, config=config,
                                      metadata_filter=metadata_filter, chunk_lookup=_ref_lookup(gi))
    return retrieve_chunk_spans(chunks, neighbors=neighbors, config=config, index=gi)


def search_and_rerank_chunk_spans_batch(queries: Sequence[str], *, num_results: int = 8, oversample: int = 4,
                                        neighbors: Sequence[int] | None = (-1, 1), search: Any = "hybrid", config: Any | None = None,
                                        metadata_filter=None, index: GpuIndex | None = None, query_vectors=None,
                                        query_token_vectors=None) -> list[list[ChunkSpan]]:
    """`search_and_rerank_chunk_spans` for a batch: element b is what `search_and_rerank_chunk_spans(queries[b], search=hybrid_search |
    vector_search, metadata_filter=<its filter>, ...)` returns with the same arguments.  The planning, the routes by query length,
    the filters and the fallbacks are `search_and_rerank_chunks_batch`'s.  With `config.reranker` a `MaxSimRanker` over the searched
    index, everything from the searches to the ordered spans runs on one stream in one device call (`rl_search_rerank_spans_per_query`
    for queries of one length, `rl_search_rerank_spans_ragged` for mixed lengths) and is read back once.  Otherwise the batched search
    runs, then the rerank path of `search_and_rerank_chunks_batch`, then one `rl_chunk_spans` for the batch."""
    cfg = config or HotPathConfig()
    gi = index or _index_for(config)
    queries = list(queries)
    if search not in _SEARCHES:
        raise ValueError("search must be 'hybrid' or 'vector'")
    if not queries:
        return []
    request = _SpanRequest(gi.span_table(), neighbors)
    ranker = _device_ranker(cfg, gi)
    if ranker is None:
        found = search_and_rerank_chunks_batch(queries, num_results=num_results, oversample=oversample, search=search, config=cfg,
                                               metadata_filter=metadata_filter, index=gi, query_vectors=query_vectors,
                                               chunk_lookup=_ref_lookup(gi))
        return retrieve_chunk_spans_batch([[c.id for c in chunks] for chunks in found], neighbors=neighbors, index=gi)
    device = _hybrid_rerank_device if _SEARCHES[search] == "hybrid" else _vector_rerank_device
    return device(gi, cfg, ranker, queries, num_results, oversample * num_results, metadata_filter, query_vectors, query_token_vectors,
                  spans=request)


def retrieve_context(query: str, *, num_chunks: int = 10, metadata_filter: dict | None = None, config: Any | None = None,
                     index: GpuIndex | None = None) -> list[ChunkSpan]:
    """Retrieve context for RAG (`src/raglite/_rag.py:43-64`): call `config.search_method` and turn what it returns into chunk spans
    as `:57-63` does -- an (ids, scores) tuple and a list of chunk ids (or of chunk objects with an `.id`) go through
    `retrieve_chunk_spans`, a list of `ChunkSpan` is returned as it is, anything else gives no spans."""
    cfg = config or HotPathConfig()
    search_method = getattr(cfg, "search_method", None)
    if search_method is None:
        raise ValueError("retrieve_context needs config.search_method (e.g. GpuVectorSearch, or a function returning chunk spans)")
    results = search_method(query, num_results=num_chunks, metadata_filter=metadata_filter, config=config)
    if isinstance(results, tuple):
        return retrieve_chunk_spans(results[0], config=config, index=index)
    results = list(results)
    if all(isinstance(r, ChunkSpan) for r in results):
        return results
    if all(isinstance(r, ChunkId) or hasattr(r, "id") for r in results):
        return retrieve_chunk_spans(results, config=config, index=index)
    return []
