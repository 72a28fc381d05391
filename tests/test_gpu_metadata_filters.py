"""Metadata filters evaluated on the device: `rl_metadata_filters` against its NumPy restatement
(`_metadata.filter_bits_host`) word for word and count for count; the *_per_query searches reading a device table in place under
RL_MEM_FILTERS_DEVICE against the same calls with the host table, bit for bit; and the public functions over two indexes of the same
data, `metadata_filters="host"` and `"device"`, returning equal ids and equal floats -- also once `_search._matches` raises, which is
what a "device" index never calls."""

import zlib

import numpy as np
import pytest

import raglite_amd
from oracle import oracle
from raglite_amd import _keyword, _metadata, _ops, _search
from tests import keyword_ref as ref

pytestmark = pytest.mark.gpu

STAGE, PIECE, GROUP = 4096, 1024, 64  # csrc/common.h: MF_STAGE_TAGS, MF_FILTER_TAGS, MF_GROUP
N_BIG = STAGE + 904                   # tags of the one chunk that does not fit the staging budget


# ---- 1. the kernel against filter_bits_host --------------------------------------------------------------------------------------
def _chunk_tags(rng, C):
    """Ragged ascending tag lists over ids < 40, a third of the chunks without a tag, and chunk (C - 1) // 2 with N_BIG tags: it and the
    chunks behind it in its workgroup read their lists from global memory."""
    lists = [np.sort(rng.choice(40, size=int(rng.integers(1, 7)), replace=False)) if rng.random() > 0.33 else np.zeros(0, np.int64)
             for _ in range(C)]
    lists[(C - 1) // 2] = np.arange(N_BIG)
    off = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.int64)
    return off, np.concatenate(lists).astype(np.int32)


def _filter_tags(rng, F):
    """Filters with no tag, the sentinel, one to three tags, more tags than an LDS piece holds (only the big chunk matches) and a few
    hundred tags each, so that a group's filters come through LDS in several pieces."""
    lists = []
    for j in range(F):
        kind = j % 7
        if kind == 0:
            lists.append(np.sort(rng.choice(40, size=int(rng.integers(1, 4)), replace=False)))
        elif kind == 1:
            lists.append(np.zeros(0, np.int64))
        elif kind == 2:
            lists.append(np.asarray([int(rng.integers(40)), _metadata.NO_TAG]))
        elif kind == 3:
            lists.append(rng.permutation(N_BIG)[: PIECE + 76])  # any order, read from global memory
        elif kind == 4:
            lists.append(np.arange(50, 50 + 300))
        elif kind == 5:
            lists.append(np.asarray([int(rng.integers(40))]))
        else:
            lists.append(np.asarray([N_BIG + 5]))  # a tag no chunk carries
    off = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.int64)
    return off, np.concatenate(lists).astype(np.int32)


def _tiny_index(rng, C):
    sizes = rng.integers(0, 5, size=C)  # ragged rows per chunk, some chunks without a row
    sizes[0] = max(int(sizes[0]), 1)
    off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    return _ops.DeviceIndex(rng.standard_normal((int(off[-1]), 8)).astype(np.float32), off), sizes


def _check(store, idx, tag_off, tags, sizes, f_off, f_tags, fs=None):
    fs, chunks, rows = store.filters(idx, f_off, f_tags, filter_set=fs)
    want = _metadata.filter_bits_host(tag_off, tags, f_off, f_tags)
    got = fs.read()
    assert got.shape == want.shape == (f_off.size - 1, (tag_off.size - 1 + 31) // 32)
    assert np.array_equal(got, want)  # word for word: the bits past C are zero in both
    want_chunks, want_rows = _metadata.filter_counts_host(want, sizes)
    assert np.array_equal(chunks, want_chunks) and np.array_equal(rows, want_rows)
    return fs, want_chunks


@pytest.mark.parametrize("F", [1, 3, GROUP + 1])
@pytest.mark.parametrize("C", [1, 31, 33, 64, 65, 257, 1000])
def test_kernel_equals_the_host_restatement(torch_cuda, C, F):
    rng = np.random.default_rng(1000 * F + C)
    tag_off, tags = _chunk_tags(rng, C)
    f_off, f_tags = _filter_tags(rng, F)
    idx, sizes = _tiny_index(rng, C)
    store = _ops.MetadataStore(tag_off, tags)
    try:
        fs, n = _check(store, idx, tag_off, tags, sizes, f_off, f_tags)
        if F > 3:
            assert n.max() == C and n.min() == 0 and (n == 1).any() and (C < 64 or ((n > 1) & (n < C)).any())
            used, reserved = store.memory()
            assert used == 8 * (C + 1) + 4 * tags.size <= reserved
        fs.close()
    finally:
        store.close()
        idx.close()


def test_append_across_a_word_boundary_and_a_filter_set_that_grows(torch_cuda):
    rng = np.random.default_rng(5)
    tag_off, tags = _chunk_tags(rng, 40)
    idx, sizes = _tiny_index(rng, 40)
    store = _ops.MetadataStore(tag_off, tags)
    try:
        fs, _ = _check(store, idx, tag_off, tags, sizes, *_filter_tags(rng, 1))  # a set of one filter over two words ...
        more_off, more_tags = _chunk_tags(rng, 30)  # ... then 70 chunks: the append ends inside the third word
        more_sizes = rng.integers(1, 4, size=30)
        with pytest.raises(ValueError, match="another number of chunks"):
            store.append(more_off, more_tags)
            store.filters(idx, *_filter_tags(rng, 1))
        idx.append(rng.standard_normal((int(more_sizes.sum()), 8)).astype(np.float32), more_sizes)
        tag_off = np.concatenate([tag_off, tag_off[-1] + more_off[1:]])
        tags, sizes = np.concatenate([tags, more_tags]), np.concatenate([sizes, more_sizes])
        for F in (3, GROUP + 1, 2):  # the same set, reused: it has to grow, then holds more than it needs
            again, _ = _check(store, idx, tag_off, tags, sizes, *_filter_tags(rng, F), fs=fs)
            assert again is fs and (fs.n_filters, fs.words) == (F, 3)
        store.append(np.zeros(1, np.int64), np.zeros(0, np.int32))  # no chunk: nothing changes
        _check(store, idx, tag_off, tags, sizes, *_filter_tags(rng, 2), fs=fs)
        # tombstoned chunks are evaluated like any other: the searches and-in the live rows
        idx.delete_chunks(np.arange(0, 70, 3, dtype=np.int64))
        _check(store, idx, tag_off, tags, sizes, *_filter_tags(rng, 5), fs=fs)
        fs.close()
    finally:
        store.close()
        idx.close()


# ---- 2. RL_MEM_FILTERS_DEVICE: a device table beside host queries ---------------------------------------------------------------------
def _same(got, want, what):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.asarray(g).tobytes() == np.asarray(w).tobytes(), what


def test_per_query_calls_read_a_device_table_in_place(torch_cuda):
    rng = np.random.default_rng(7)
    C, dim, B = 3000, 64, 40
    sizes = rng.integers(1, 4, size=C)
    off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    idx = _ops.DeviceIndex(oracle.synth_matrix(11, int(off[-1]), dim, "small_int"), off)  # integer-valued: every route is exact
    flat, koff = ref.zipf_corpus(rng, C, 500, 20)
    kw = _ops.KeywordIndex(_keyword.build_from_term_ids(flat, koff, 500))
    metadata = [{"tenant": f"t{int(rng.integers(6))}", "lang": ["en", "de"][i % 2]} for i in range(C)]
    vocab = _metadata.TagVocabulary()
    store = _ops.MetadataStore(*vocab.encode_chunks(metadata))
    try:
        filters = [{"tenant": ["t1"]}, {"lang": ["en"]}, {"tenant": ["nobody"]}, {"tenant": ["t2"], "lang": ["de"]}, {"lang": []}]
        fs, n, _ = store.filters(idx, *vocab.encode_filters(filters))
        assert n.tolist() == [sum(_search._matches(m, f) for m in metadata) for f in filters]  # noqa: SLF001
        table = fs.read()
        idx.delete_chunks(np.arange(5, C, 9, dtype=np.int64))  # (the table covers the tombstoned chunks; the searches drop them)
        Q = oracle.synth_matrix(12, B, dim, "small_int")
        terms = [sorted(set(int(x) for x in t)) for t in ref.zipf_queries(rng, B, 500)]
        qf = rng.integers(-1, len(filters), size=B).astype(np.int32)
        host = [None if j < 0 else table[j] for j in qf]
        limits = [[0, 2000, 10**9][b % 3] for b in range(B)]
        for lim in (None, limits):
            _same(idx.search_chunks(Q, 64, 10, query_filters=fs.select(qf), rank_limit=lim),
                  idx.search_chunks(Q, 64, 10, query_filters=host, rank_limit=lim), ("chunks", lim))
            for keyword in (kw, None):
                _same(idx.hybrid_search(Q, 64, 16, 16, keyword=keyword, query_term_ids=terms, query_filters=fs.select(qf), rank_limit=lim),
                      idx.hybrid_search(Q, 64, 16, 16, keyword=keyword, query_term_ids=terms, query_filters=host, rank_limit=lim),
                      ("hybrid", lim, keyword is None))
        _same(kw.search(terms, 10, query_filters=fs.select(qf)), kw.search(terms, 10, query_filters=host), "keyword")
        # one query, one filter: the single-filter call
        _same(idx.search_chunks(Q[0], 64, 10, query_filters=fs.select([1]), rank_limit=[2000]),
              idx.search_chunks(Q[0], 64, 10, chunk_filter=table[1], rank_limit=2000), "single")
        with pytest.raises(ValueError, match="one entry per query"):
            idx.search_chunks(Q, 64, 10, query_filters=fs.select(qf[:-1]))
        with pytest.raises(ValueError, match="a row of the set"):
            idx.search_chunks(Q, 64, 10, query_filters=fs.select(np.full(B, len(filters))))
        view = fs.select(qf)
        fs.close()  # a view of a closed set is an error, not a stale pointer
        with pytest.raises(ValueError, match="null filter set"):
            idx.search_chunks(Q, 64, 10, query_filters=view)
    finally:
        store.close()
        kw.close()
        idx.close()


# ---- 3. the public functions: metadata_filters="device" against "host" ----------------------------------------------------------------
DIM = 64
WORDS = ["gpu", "kernel", "memory", "bandwidth", "search", "vector", "keyword", "ranking", "fusion", "chunk", "document", "index",
         "query", "rerank", "embedding", "latency", "throughput", "cache", "tile", "wave", "matrix", "score", "token"]
FILTERS = [None, {"tenant": "t1"}, {"tenant": "nobody"}, {"lang": "en"}, {"tenant": ["t2"], "lang": "de"}, {}, {"tenant": "t1"},
           {"topics": ["a", "b"]}, {"level": 1.0}, {"level": [True], "lang": "en"}, {"topics": []}]


def _ints(rng, shape):
    return rng.integers(-3, 4, size=shape).astype(np.float32)


def _hash_ints(text, shape):
    return _ints(np.random.default_rng(zlib.crc32(text.encode())), shape)


def _meta(i):
    m = {"tenant": f"t{i % 5}", "lang": ["en", "de"][i % 2], "level": [1, 2.0, True, 3][i % 4]}
    if i % 3:
        m["topics"] = [["a", "b"], ["b"], ["a", "c", "b"]][i % 3]
    return m


def _chunks(rng, first, n):
    ids = [f"chunk-{i:06d}" for i in range(first, first + n)]
    mats = [_ints(rng, (int(rng.integers(1, 4)), DIM)) for _ in range(n)]
    bodies = [" ".join(rng.choice(WORDS, size=int(rng.integers(3, 25)))) for _ in range(n)]
    positions = [(f"doc-{i // 7:04d}", i % 7) for i in range(first, first + n)]
    return ids, mats, dict(metadata=[_meta(i) for i in range(first, first + n)], keyword_texts=bodies, positions=positions,
                           docs=[f"{i} {b}" for i, b in zip(ids, bodies)])


@pytest.fixture
def pair(torch_cuda, monkeypatch):
    """Two indexes over the same data, `metadata_filters="host"` and `"device"`, with integer-valued embeddings, and per index a
    config whose reranker is a MaxSimRanker over it."""
    monkeypatch.setattr(_search, "embed_strings", lambda strings, config=None: np.stack([_hash_ints(s, (DIM,)) for s in strings]))
    ids, mats, kw = _chunks(np.random.default_rng(61), 0, 3000)
    out = {}
    for mode in ("host", "device"):
        gi = raglite_amd.GpuIndex(ids, mats, metadata_filters=mode, **kw)
        ranker = raglite_amd.MaxSimRanker(gi, lambda q: _hash_ints("tokens " + q, (4 if q.endswith("y") else 8, DIM)))
        out[mode] = (gi, raglite_amd.HotPathConfig(vector_search_query_adapter=False, reranker=ranker))
    assert out["device"][0]._meta_store is not None and out["host"][0]._meta_store is None  # noqa: SLF001
    yield out
    for gi, _ in out.values():
        gi.close()


def _queries(rng, n):
    qs = [" ".join(rng.choice(WORDS, size=int(rng.integers(1, 5)))) for _ in range(n)]
    qs[-1] = "zebra unicorn"  # no known stem
    return qs


def _outcome(fn, *args, **kw):
    try:
        return fn(*args, **kw)
    except (ValueError, NotImplementedError) as e:
        return (type(e), str(e))


def _both(pair, fn, *args, **kw):
    """fn over the "host" index and over the "device" index: equal ids and equal floats (or the same error); returns the result."""
    want, got = (_outcome(fn, *args, index=pair[mode][0], config=pair[mode][1], **kw) for mode in ("host", "device"))
    assert got == want, (fn.__name__, kw)
    return got


BATCHES = [raglite_amd.vector_search_batch, raglite_amd.keyword_search_batch, raglite_amd.hybrid_search_batch]


def _compare_everything(pair, rng, monkeypatch):
    queries = _queries(rng, 23)
    filters = [FILTERS[i % len(FILTERS)] for i in range(len(queries))]
    _compare(pair, queries, filters)
    with monkeypatch.context() as m:  # a real cut at test scale: "lang en" matches ~3 000 rows > 500 -> order first, limit 800
        m.setattr(_search, "FILTER_FIRST_MAX_ROWS", 500)
        m.setattr(_search, "ORDER_FIRST_LIMIT", 800)
        assert pair["device"][0].index.n_rows > 800
        _compare(pair, queries, filters)
        device = pair["device"][0]
        plan = _search.plan_filters(_search._batch_filters(filters, len(filters)), device.metadata,  # noqa: SLF001
                                    _search._rows_per_chunk(device), device)  # noqa: SLF001
        assert plan.filter_set is not None and set(plan.rank_limit) == {0, 800}  # both branches, decided from the device's counts


def _compare(pair, queries, filters):
    for f in FILTERS[1:]:
        _both(pair, raglite_amd.vector_search, queries[0], metadata_filter=f, num_results=5)
        _both(pair, raglite_amd.keyword_search, queries[1], metadata_filter=f, num_results=5)
    _both(pair, raglite_amd.hybrid_search, queries[2], metadata_filter=FILTERS[3])
    for batch in BATCHES:
        got = _both(pair, batch, queries, metadata_filter=filters, num_results=5)
        assert any(g[0] for g in got) and any(g == ([], []) for g in got)
        _both(pair, batch, queries, metadata_filter={"lang": "de"})  # one dict for the batch
    for search in ("hybrid", "vector"):
        got = _both(pair, raglite_amd.search_and_rerank_chunks_batch, queries, search=search, metadata_filter=filters, num_results=4)
        assert any(got) and not all(got)
        got = _both(pair, raglite_amd.search_and_rerank_chunk_spans_batch, queries, search=search, metadata_filter=filters, num_results=4)
        assert any(got) and not all(got)


def test_public_functions_equal_the_host_path(pair, monkeypatch):
    rng = np.random.default_rng(62)
    _compare_everything(pair, rng, monkeypatch)
    # after an insert (70 chunks: the new tags end inside a word), a delete, and a compaction
    ids, mats, kw = _chunks(rng, 3000, 70)
    for gi, _ in pair.values():
        gi.insert_chunks(ids, mats, **kw)
        assert gi.delete_chunks([f"chunk-{i:06d}" for i in range(0, 3070, 3)]) == 1024
    _compare_everything(pair, rng, monkeypatch)
    for gi, _ in pair.values():
        gi.compact()
        assert len(gi.chunk_ids) == 3070 - 1024
    device = pair["device"][0]
    assert device._meta_store.n_chunks == len(device.chunk_ids) == device.index.n_chunks  # noqa: SLF001
    _compare_everything(pair, rng, monkeypatch)
    # the device evaluation against the loop over the metadata, after all that
    distinct = [_search._adapt_metadata(f) for f in FILTERS[1:] if f]  # noqa: SLF001
    fs, n, rows = _search._filters_on_device(device, distinct)  # noqa: SLF001
    bits = np.unpackbits(fs.read().view(np.uint8), axis=1, bitorder="little")[:, : len(device.chunk_ids)].astype(bool)
    sizes = np.diff(device.index.chunk_offsets)
    for j, f in enumerate(distinct):
        want = np.array([_search._matches(m, f) for m in device.metadata])  # noqa: SLF001
        assert np.array_equal(bits[j], want) and n[j] == want.sum() and rows[j] == sizes[want].sum()


def test_the_same_errors_are_raised(pair):
    queries = _queries(np.random.default_rng(63), 4)
    nothing = [{"tenant": "nobody"}] * 4
    for batch in BATCHES:
        assert isinstance(_both(pair, batch, queries, metadata_filter=[None] * 3)[1], str)
        for n in (1025, 2049):
            for filters in (nothing, nothing[:3] + [None], [{"lang": "en"}] * 4, None):
                _both(pair, batch, queries, metadata_filter=filters, num_results=n)
    for n in (1025, 2049):
        for f in (nothing[0], {"lang": "en"}):
            _both(pair, raglite_amd.vector_search, queries[0], metadata_filter=f, num_results=n)
            _both(pair, raglite_amd.keyword_search, queries[0], metadata_filter=f, num_results=n)
    # vector_search returns before its limit check where the filter matches nothing
    assert _both(pair, raglite_amd.vector_search_batch, queries, metadata_filter=nothing, num_results=1025) == [([], [])] * 4
    bare = raglite_amd.GpuIndex(["a", "b"], [_ints(np.random.default_rng(1), (2, DIM))] * 2, keyword_texts=["gpu kernel", "memory"])
    try:
        assert bare._meta_store is None  # noqa: SLF001
        for fn, q in ((raglite_amd.vector_search, queries[0]), (raglite_amd.keyword_search, "gpu"), (raglite_amd.vector_search_batch, queries)):
            with pytest.raises(ValueError, match="without `metadata`"):
                fn(q, metadata_filter={"tenant": "t1"}, index=bare, config=pair["device"][1])
    finally:
        bare.close()
    with pytest.raises(ValueError, match="metadata_filters"):
        raglite_amd.GpuIndex(["a"], [np.zeros((1, DIM), np.float32)], metadata_filters="gpu")


def test_a_filter_that_cannot_be_encoded_takes_the_host_path(pair, monkeypatch):
    queries = _queries(np.random.default_rng(64), 6)
    calls = []
    real = _search._matches  # noqa: SLF001
    monkeypatch.setattr(_search, "_matches", lambda m, f: calls.append(1) or real(m, f))
    filters = [{"tenant": "t1"}, {"tenant": None}, None, {"lang": "en"}, {"tenant": "t1"}, {"lang": ["en", float("nan")]}]
    for batch in BATCHES:
        _both(pair, batch, queries, metadata_filter=filters)
    n_host = len(calls)
    assert n_host == 2 * 3 * 4 * 3000  # both indexes looped: four distinct filters, three batches
    _both(pair, raglite_amd.vector_search, queries[0], metadata_filter={"tenant": None})
    assert len(calls) == n_host + 2 * 3000
    # a chunk value that cannot be a tag makes its key host-only from then on; the other keys stay on the device
    ids, mats, kw = _chunks(np.random.default_rng(65), 3000, 2)
    kw["metadata"][1]["level"] = None
    for gi, _ in pair.values():
        gi.insert_chunks(ids, mats, **kw)
    calls.clear()
    _both(pair, raglite_amd.vector_search, queries[0], metadata_filter={"level": 2})
    assert len(calls) == 2 * 3002
    _both(pair, raglite_amd.vector_search, queries[0], metadata_filter={"tenant": "t3"})
    assert len(calls) == 3 * 3002  # (the host index alone looped)


def test_a_device_index_never_calls_matches(pair, monkeypatch):
    """The test that fails without the device evaluation: every filtered search evaluated its filter by `_matches`."""
    queries = _queries(np.random.default_rng(66), 9)
    filters = [FILTERS[i % len(FILTERS)] for i in range(len(queries))]
    host, cfg_host = pair["host"]
    want_single = [raglite_amd.vector_search(queries[0], metadata_filter=f, index=host, config=cfg_host) for f in FILTERS[1:5]]
    want_kw = raglite_amd.keyword_search(queries[1], metadata_filter={"lang": "en"}, index=host, config=cfg_host)
    want_batches = [batch(queries, metadata_filter=filters, index=host, config=cfg_host) for batch in BATCHES]
    want_rerank = raglite_amd.search_and_rerank_chunks_batch(queries, metadata_filter=filters, index=host, config=cfg_host)
    want_hybrid = raglite_amd.hybrid_search(queries[2], metadata_filter={"tenant": "t2"}, index=host, config=cfg_host)

    def boom(meta, flt):
        raise AssertionError("_matches was called")

    monkeypatch.setattr(_search, "_matches", boom)
    gi, cfg = pair["device"]
    assert [raglite_amd.vector_search(queries[0], metadata_filter=f, index=gi, config=cfg) for f in FILTERS[1:5]] == want_single
    assert any(ids for ids, _ in want_single) and ([], []) in want_single
    assert raglite_amd.keyword_search(queries[1], metadata_filter={"lang": "en"}, index=gi, config=cfg) == want_kw
    assert [batch(queries, metadata_filter=filters, index=gi, config=cfg) for batch in BATCHES] == want_batches
    assert raglite_amd.search_and_rerank_chunks_batch(queries, metadata_filter=filters, index=gi, config=cfg) == want_rerank
    assert raglite_amd.hybrid_search(queries[2], metadata_filter={"tenant": "t2"}, index=gi, config=cfg) == want_hybrid
