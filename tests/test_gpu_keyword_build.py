"""The BM25 postings built on the device (raglite_amd/csrc/keyword_build.hip): a `KeywordStore` holds the chunks' term
ids, `count` + `build` make the `KeywordIndex`.  The reference everywhere is the host build, `_keyword.build_from_term_ids` over
`rank[flat]`, with the float32 impacts of tests/keyword_ref.py: term_off and post_chunk compare as integers, post_impact as uint32
bits, and df, length and the three totals of `count` equal the `Postings` fields."""

import ctypes as C

import numpy as np
import pytest

import raglite_amd
from oracle.fake_embedder import FakeLlama
from raglite_amd import _abi, _keyword, _ops
from tests import keyword_ref as ref

pytestmark = pytest.mark.gpu


def _count_and_build(store, n_terms, rank, corpus=None):
    """(KeywordIndex, what count returned); `corpus`: (df, n_live, total_length) to weight with instead of the store's own."""
    df, length, n_live, total_length, n_postings = store.count(n_terms, rank)
    w_df, w_live, w_total = corpus if corpus is not None else (df, n_live, total_length)
    idf, nrm, _ = _keyword.bm25_weights(w_df, length, w_live, w_total)
    return store.build(idf, nrm), (df, length, n_live, total_length, n_postings)


def _host(flat, off, n_terms, rank, live=None):
    keys = np.asarray(flat, dtype=np.int64) if rank is None else np.asarray(rank, dtype=np.int64)[flat]
    return _keyword.build_from_term_ids(keys, off, n_terms, live)


def _assert_equal(p, kw, counts=None, what=""):
    term_off, post_chunk, post_impact = kw.read()
    assert (kw.n_terms, kw.n_postings, kw.n_chunks) == (p.n_terms, p.post_chunk.size, p.n_chunks), what
    assert term_off.dtype == np.int64 and np.array_equal(term_off, p.term_off), what
    assert post_chunk.dtype == np.int32 and np.array_equal(post_chunk, p.post_chunk), what
    assert np.array_equal(post_impact.view(np.uint32), ref.impacts_f32(p).view(np.uint32)), what
    if counts is not None:
        df, length, n_live, total_length, n_postings = counts
        assert np.array_equal(df, p.df) and np.array_equal(length, p.length), what
        assert (n_live, total_length, n_postings) == (p.n_live, int(p.length.sum()), int(p.post_chunk.size)), what


def _build_and_check(flat, off, n_terms, rank, live=None, what=""):
    store = _ops.KeywordStore()
    try:
        store.append(flat, off)
        if live is not None:
            store.delete(np.nonzero(~live)[0])
        kw, counts = _count_and_build(store, n_terms, rank)
        try:
            _assert_equal(_host(flat, off, n_terms, rank, live), kw, counts, what)
        finally:
            kw.close()
    finally:
        store.close()


# ---- 1. Zipf corpora -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_chunks", [1, 37, 5000, 300_000])
def test_zipf_corpora_of_every_size(torch_cuda, n_chunks):
    rng = np.random.default_rng(2000 + n_chunks)
    n_terms = max(50, min(20_000, n_chunks * 2))
    flat, off = ref.zipf_corpus(rng, n_chunks, n_terms, mean_len=12)
    _build_and_check(flat, off, n_terms, rng.permutation(n_terms).astype(np.int32))


@pytest.mark.parametrize("n_terms", [1, 2, 256, 257, 65_536, 65_537])
def test_both_sides_of_every_digit_boundary(torch_cuda, n_terms):
    """One, two and three 8-bit passes.  Half of the tokens are drawn uniformly so that the top ids (the ones that need the last digit)
    occur; the top id itself is planted."""
    rng = np.random.default_rng(3000 + n_terms)
    flat, off = ref.zipf_corpus(rng, 5000, n_terms, mean_len=12)
    uniform = rng.random(flat.size) < 0.5
    flat[uniform] = rng.integers(0, n_terms, size=int(uniform.sum()))
    flat[-1] = n_terms - 1
    rank = rng.permutation(n_terms).astype(np.int32)
    _build_and_check(flat, off, n_terms, rank, what="permuted")
    _build_and_check(flat, off, n_terms, None, what="identity")


# ---- 2. planted shapes -----------------------------------------------------------------------------------------------------------
def test_planted_shapes(torch_cuda):
    rng = np.random.default_rng(17)
    n_chunks, n_terms = 5000, 3000
    everywhere, never = 1234, 2999
    chunks = []
    for c in range(n_chunks):
        if c in (0, n_chunks - 1) or 2000 <= c < 2100:  # first and last chunk empty, and a run of 100 empty chunks
            chunks.append(np.zeros(0, np.int64))
        elif c == 700:  # 10 000 tokens, all one term (tf = 10 000: the run crosses sort blocks); no other term, `everywhere` included
            chunks.append(np.full(10_000, 77, np.int64))
        elif c == 3100:  # 10 000 tokens over 50 terms
            chunks.append(np.concatenate(([everywhere], rng.integers(100, 150, size=9_999))))
        else:
            body = (rng.zipf(1.1, size=int(rng.integers(1, 24))) - 1) % (n_terms - 1)  # (never reaches `never`)
            chunks.append(np.concatenate(([everywhere], body)))
    flat = np.concatenate(chunks)
    assert not (flat == never).any()
    off = np.concatenate(([0], np.cumsum([len(c) for c in chunks]))).astype(np.int64)
    rank = rng.permutation(n_terms).astype(np.int32)
    # every chunk alive: the term present in every non-empty chunk has df = their number, and its chunks ascend over many blocks
    _build_and_check(flat, off, n_terms, rank, what="all live")
    p = _host(flat, off, n_terms, rank)
    t = int(rank[everywhere])
    assert p.df[t] == n_chunks - 102 - 1 and p.df[rank[never]] == 0 and p.post_tf.max() == 10_000
    live = rng.random(n_chunks) > 0.3  # 30 % dead chunks
    live[[700, 3100]] = True
    _build_and_check(flat, off, n_terms, rank, live, what="30 % dead")
    live[[700, 3100]] = False
    _build_and_check(flat, off, n_terms, rank, live, what="the long chunks dead")


# ---- 3. lifecycle ----------------------------------------------------------------------------------------------------------------
def test_lifecycle_appends_deletes_and_determinism(torch_cuda):
    rng = np.random.default_rng(23)
    n_chunks, n_terms = 6000, 900
    flat, off = ref.zipf_corpus(rng, n_chunks, n_terms, mean_len=12)
    rank = rng.permutation(n_terms).astype(np.int32)
    store = _ops.KeywordStore()
    try:
        assert store.info() == {"n_chunks": 0, "n_live": 0, "n_tokens": 0, "device_bytes": 0}
        for a, b in ((0, 1), (1, 2500), (2500, 2537), (2537, 6000), (6000, 6000)):  # five uneven pieces, the last with no chunk
            store.append(flat[off[a] : off[b]], off[a : b + 1] - off[a])
        info = store.info()
        assert (info["n_chunks"], info["n_live"], info["n_tokens"]) == (n_chunks, n_chunks, flat.size) and info["device_bytes"] > 0
        kw, counts = _count_and_build(store, n_terms, rank)
        _assert_equal(_host(flat, off, n_terms, rank), kw, counts, "appended in pieces")
        kw.close()
        live = np.ones(n_chunks, bool)
        gone = rng.choice(n_chunks, size=n_chunks // 3, replace=False)
        store.delete(gone)
        live[gone] = False
        kw, counts = _count_and_build(store, n_terms, rank)
        _assert_equal(_host(flat, off, n_terms, rank, live), kw, counts, "a third deleted")
        kw.close()
        again = np.concatenate((gone[:500], rng.choice(n_chunks, size=700, replace=False), gone[:3]))  # dead ones included, and repeats
        store.delete(again)
        live[again] = False
        assert store.info()["n_live"] == int(live.sum())
        first, counts = _count_and_build(store, n_terms, rank)
        second, counts2 = _count_and_build(store, n_terms, rank)  # the same store again: the build is deterministic
        p = _host(flat, off, n_terms, rank, live)
        _assert_equal(p, first, counts, "deleted again")
        _assert_equal(p, second, counts2, "built twice")
        for x, y in zip(first.read(), second.read()):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        first.close()
        second.close()
        store.append(flat[: off[40]], off[:41])  # and it still grows: the deleted ordinals stay dead
        flat2, off2 = np.concatenate((flat, flat[: off[40]])), np.concatenate((off, off[-1] + off[1:41]))
        kw, counts = _count_and_build(store, n_terms, rank)
        _assert_equal(_host(flat2, off2, n_terms, rank, np.concatenate((live, np.ones(40, bool)))), kw, counts, "appended after deletes")
        kw.close()
    finally:
        store.close()


def test_empty_stores(torch_cuda):
    store = _ops.KeywordStore()
    try:
        for n_terms in (0, 5):  # no chunks at all
            kw, counts = _count_and_build(store, n_terms, None)
            _assert_equal(_host(np.zeros(0, np.int64), np.zeros(1, np.int64), n_terms, None), kw, counts, "no chunks")
            assert counts[2:] == (0, 0, 0)
            kw.close()
        flat, off = np.array([3, 1, 3], np.int64), np.array([0, 0, 3, 3], np.int64)
        store.append(flat, off)
        store.delete([1])  # chunks, but no live token
        live = np.array([True, False, True])
        kw, counts = _count_and_build(store, 5, None)
        _assert_equal(_host(flat, off, 5, None, live), kw, counts, "no live token")
        assert counts[2:] == (2, 0, 0) and kw.search([[3, 1]], 4)[2].tolist() == [0]
        kw.close()
    finally:
        store.close()


# ---- 4. shard split --------------------------------------------------------------------------------------------------------------
def test_two_stores_hold_the_halves_of_one_corpus(torch_cuda):
    rng = np.random.default_rng(31)
    n_chunks, n_terms, cut = 4000, 700, 1700
    flat, off = ref.zipf_corpus(rng, n_chunks, n_terms, mean_len=12)
    live = rng.random(n_chunks) > 0.2
    parts = []
    for lo, hi in ((0, cut), (cut, n_chunks)):
        store = _ops.KeywordStore()
        store.append(flat[off[lo] : off[hi]], off[lo : hi + 1] - off[lo])
        store.delete(np.nonzero(~live[lo:hi])[0])
        parts.append((lo, hi, store, store.count(n_terms)))  # (global term ids: no permutation)
    corpus = _keyword.ShardCounts(sum(c[0] for *_, c in parts), sum(c[2] for *_, c in parts), sum(c[3] for *_, c in parts))
    whole = _keyword.build_from_term_ids(flat, off, n_terms, live)
    assert np.array_equal(corpus.df, whole.df) and (corpus.n_live, corpus.total_length) == (whole.n_live, int(whole.length.sum()))
    whole_imp = ref.impacts_f32(whole)
    seen = np.zeros(whole_imp.size, bool)
    try:
        for lo, hi, store, counts in parts:
            idf, nrm, _ = _keyword.bm25_weights(corpus.df, counts[1], corpus.n_live, corpus.total_length)
            kw = store.build(idf, nrm)
            f, o = flat[off[lo] : off[hi]], off[lo : hi + 1] - off[lo]
            p = _keyword.build_shard_from_term_ids(f, o, n_terms, live[lo:hi], corpus)
            _assert_equal(p, kw, None, f"shard {lo}:{hi}")
            assert np.array_equal(counts[0], p.df) and np.array_equal(counts[1], p.length)
            # ... and the shard's impacts are the slice of one build over everything
            _, post_chunk, post_impact = kw.read()
            inside = (whole.post_chunk >= lo) & (whole.post_chunk < hi)
            assert np.array_equal(post_chunk + lo, whole.post_chunk[inside])
            assert np.array_equal(post_impact.view(np.uint32), whole_imp[inside].view(np.uint32))
            seen |= inside
            kw.close()
        assert seen.all()
    finally:
        for _, _, store, _ in parts:
            store.close()


# ---- 5. search through the built index -------------------------------------------------------------------------------------------
def _check_search(p, kw, queries, k, allowed=None):
    """tests/test_gpu_keyword.py's check: the device's top k, bitwise the float32 restatement's."""
    imp = ref.impacts_f32(p)
    got_s, got_c, got_n = kw.search(queries, k, chunk_filter=allowed)
    assert got_s.shape == (len(queries), k) and got_c.shape == (len(queries), k) and got_n.shape == (len(queries),)
    for b, q in enumerate(queries):
        want_s, want_c = ref.topk_f32(ref.scores_f32(p, imp, q), k, allowed)
        n = len(want_c)
        assert int(got_n[b]) == n, (b, k)
        assert np.array_equal(got_c[b, :n], want_c), (b, k)
        assert np.array_equal(got_s[b, :n].view(np.uint32), want_s.view(np.uint32)), (b, k)
        assert np.all(got_c[b, n:] == -1) and np.all(got_s[b, n:] == -np.inf)


def test_search_through_the_built_index(torch_cuda):
    rng = np.random.default_rng(41)
    n_chunks, n_terms = 20_000, 4000
    flat, off = ref.zipf_corpus(rng, n_chunks, n_terms, mean_len=12)
    rank = rng.permutation(n_terms).astype(np.int32)
    live = rng.random(n_chunks) > 0.1
    store = _ops.KeywordStore()
    try:
        store.append(flat, off)
        store.delete(np.nonzero(~live)[0])
        kw, _ = _count_and_build(store, n_terms, rank)
        p = _host(flat, off, n_terms, rank, live)
        queries = ref.zipf_queries(rng, 12, n_terms) + [np.array([], np.int32), np.array([n_terms + 5, -3], np.int32)]
        allowed = rng.random(n_chunks) > 0.5
        for k in (1, 100, 2048):
            _check_search(p, kw, queries, k)
            _check_search(p, kw, queries, k, allowed)
        kw.close()
    finally:
        store.close()


# ---- 6. errors -------------------------------------------------------------------------------------------------------------------
def test_invalid_input_raises_and_leaves_the_store_usable(torch_cuda):
    rng = np.random.default_rng(53)
    n_terms = 40
    flat, off = ref.zipf_corpus(rng, 300, n_terms, mean_len=8)
    store = _ops.KeywordStore()
    lib = _abi.lib()
    try:
        store.append(flat, off)
        kw, _ = _count_and_build(store, n_terms, None)
        kw.close()
        ids = np.array([1, 2, 3], np.int32)
        with pytest.raises(ValueError, match="offsets must start at 0"):
            store.append(ids, np.array([1, 3], np.int64))
        with pytest.raises(ValueError, match="offsets must be ascending"):
            store.append(ids, np.array([0, 2, 1, 3], np.int64))
        with pytest.raises(ValueError, match="term ids"):
            store.append(np.array([1, -2, 3]), np.array([0, 3], np.int64))
        bad, bad_off = np.array([1, -2, 3], np.int32), np.array([0, 3], np.int64)  # ... and the library's own check of the same
        assert lib.rl_keyword_store_append(store._handle, bad.ctypes.data, bad_off.ctypes.data, 1, _abi.MEM_HOST, None) == _abi.RL_ERR_INVALID  # noqa: SLF001
        assert "negative term id" in _abi.last_error()
        with pytest.raises(ValueError, match="out of range"):
            store.delete([5, 300])
        with pytest.raises(ValueError, match="out of range"):
            store.delete([-1])
        assert store.info()["n_live"] == 300  # (a refused delete deletes nothing, the 5 included)
        with pytest.raises(ValueError, match=">= n_terms"):
            store.count(int(flat.max()))  # a stored id reaches n_terms
        with pytest.raises(ValueError, match="permutation"):
            store.count(n_terms, np.zeros(n_terms, np.int32))
        with pytest.raises(ValueError, match="permutation"):
            store.count(n_terms, np.arange(1, n_terms + 1, dtype=np.int32))
        idf, nrm = np.ones(n_terms, np.float32), np.ones(300, np.float32)
        with pytest.raises(ValueError, match="rl_keyword_store_count"):
            store.build(idf, nrm)  # no count since the last build
        store.count(n_terms)
        store.append(ids, np.array([0, 3], np.int64))
        with pytest.raises(ValueError, match="rl_keyword_store_count"):
            store.build(idf, np.ones(301, np.float32))  # an append in between
        store.count(n_terms)
        store.delete([300])
        with pytest.raises(ValueError, match="rl_keyword_store_count"):
            store.build(idf, np.ones(301, np.float32))  # a delete in between
        store.count(n_terms)
        with pytest.raises(ValueError, match="one weight per"):
            store.build(idf, nrm)  # 300 weights for 301 chunks
        # after all of that the store builds what the host builds
        flat2, off2 = np.concatenate((flat, ids)), np.concatenate((off, [off[-1] + 3]))
        live = np.ones(301, bool)
        live[300] = False
        rank = rng.permutation(n_terms).astype(np.int32)
        kw, counts = _count_and_build(store, n_terms, rank)
        _assert_equal(_host(flat2, off2, n_terms, rank, live), kw, counts, "after the errors")
        kw.close()
        h = C.c_void_p()
        assert lib.rl_keyword_store_build(None, None, None, C.byref(h), _abi.MEM_HOST, None) == _abi.RL_ERR_INVALID and not h.value
    finally:
        store.close()


# ---- 7. GpuIndex twins -----------------------------------------------------------------------------------------------------------
OLD_WORDS = ["gpu", "kernel", "memory", "bandwidth", "search", "vector", "keyword", "ranking", "fusion", "chunk", "document", "index",
             "query", "rerank", "embedding", "latency", "throughput", "cache", "tile", "wave", "matrix", "score", "token"]
NEW_WORDS = ["aardvark", "abacus", "banana", "cobalt", "dynamo"]  # every one sorts before most of the old stems


def _bodies(rng, n, words):
    return [" ".join(rng.choice(words, size=int(rng.integers(3, 25)))) for _ in range(n)]


def _twins_agree(dev, host, cfg, queries):
    for q in queries:
        assert raglite_amd.keyword_search(q, num_results=50, index=dev) == raglite_amd.keyword_search(q, num_results=50, index=host), q
    for fn, kw in ((raglite_amd.keyword_search_batch, {}), (raglite_amd.keyword_search_batch, {"metadata_filter": {"topic": "t1"}}),
                   (raglite_amd.hybrid_search_batch, {"config": cfg})):
        got = fn(queries, num_results=10, index=dev, **kw)
        want = fn(queries, num_results=10, index=host, **kw)
        assert len(got) == len(want) == len(queries)
        for b, (g, w) in enumerate(zip(got, want)):
            assert g[0] == w[0] and g[1] == w[1] and all(type(x) is float for x in g[1]), (fn.__name__, b)


def test_device_and_host_built_indexes_are_twins(torch_cuda):
    rng = np.random.default_rng(61)
    dim, n = 64, 400
    raglite_amd.set_embedder_factory(lambda config: FakeLlama(dim=dim))
    cfg = raglite_amd.HotPathConfig(embedder="llama-cpp-python/fake/keyword-build", vector_search_query_adapter=False)

    def chunks(prefix, count, words):
        mats = [rng.standard_normal((int(rng.integers(1, 4)), dim)).astype(np.float32) for _ in range(count)]
        return [f"{prefix}-{i:04d}" for i in range(count)], mats, [{"topic": [f"t{i % 3}"]} for i in range(count)], _bodies(rng, count, words)

    ids, mats, meta, texts = chunks("base", n, OLD_WORDS)
    texts[7] = "solitary zeppelin"  # stems that live in this chunk alone
    dev = raglite_amd.GpuIndex(ids, mats, metadata=meta, keyword_texts=texts)
    host = raglite_amd.GpuIndex(ids, mats, metadata=meta, keyword_texts=texts, keyword_build="host")
    assert dev.keyword_build == "device" and host.keyword_build == "host" and dev._kw_store is not None and host._kw_store is None  # noqa: SLF001
    queries = [" ".join(rng.choice(OLD_WORDS + NEW_WORDS, size=int(rng.integers(1, 5)))) for _ in range(17)]
    queries += ["zeppelin", "solitary zeppelin kernel", "zebra unicorn"]  # 20: one whose only stem will live in a deleted chunk alone
    try:
        _twins_agree(dev, host, cfg, queries)
        ids2, mats2, meta2, texts2 = chunks("new", 50, OLD_WORDS + NEW_WORDS)  # new stems that sort before old ones
        for gi in (dev, host):
            gi.insert_chunks(ids2, mats2, metadata=meta2, keyword_texts=texts2)
        _twins_agree(dev, host, cfg, queries)
        gone = [ids[7]] + [ids[int(i)] for i in rng.choice(np.arange(8, n), size=27, replace=False)] + ids2[:2]
        for gi in (dev, host):
            assert gi.delete_chunks(gone) == 30
        assert raglite_amd.keyword_search("zeppelin", index=dev) == ([], []) and dev.keyword_query_ids("zeppelin") and not host.keyword_query_ids("zeppelin")
        _twins_agree(dev, host, cfg, queries)
        ids3, mats3, meta3, texts3 = chunks("more", 20, OLD_WORDS + NEW_WORDS)
        for gi in (dev, host):
            gi.insert_chunks(ids3, mats3, metadata=meta3, keyword_texts=texts3)
        _twins_agree(dev, host, cfg, queries)
        for gi in (dev, host):
            gi.compact()
        assert dev.index.n_chunks == n + 50 + 20 - 30 and not dev.keyword_query_ids("zeppelin")  # (compact drops the dead stems)
        _twins_agree(dev, host, cfg, queries)
    finally:
        raglite_amd.set_embedder_factory(None)
        dev.close()
        host.close()
