"""BM25 keyword search on the device (raglite_amd/csrc/keyword.hip, DESIGN.md "Keyword search"): scores and chunk ordinals bitwise
equal to the float32 restatement (tests/keyword_ref.py), the store lifecycle, and keyword_search / hybrid_search through the
public interface."""

import numpy as np
import pytest

import raglite_amd
from oracle.fake_embedder import FakeLlama
from raglite_amd import _keyword, _ops
from tests import keyword_ref as ref
from tests import store_fixture as sf

pytestmark = pytest.mark.gpu

KS = (1, 10, 100, 2048)


def _check(p, kw, queries, k, allowed=None):
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


@pytest.mark.parametrize("n_chunks", [1, 37, 5000, 300_000])
@pytest.mark.parametrize("B", [1, 7, 64])
def test_bitwise_equal_to_the_restatement_on_zipf_corpora(torch_cuda, n_chunks, B):
    rng = np.random.default_rng(1000 + n_chunks + B)
    n_terms = max(50, min(20_000, n_chunks * 2))
    flat, off = ref.zipf_corpus(rng, n_chunks, n_terms, mean_len=12)
    p = _keyword.build_from_term_ids(flat, off, n_terms)
    queries = ref.zipf_queries(rng, B, n_terms)
    kw = _ops.KeywordIndex(p)
    try:
        for k in KS:
            _check(p, kw, queries, k)
    finally:
        kw.close()


def test_filter_dead_chunks_and_unknown_terms(torch_cuda):
    rng = np.random.default_rng(7)
    n_chunks, n_terms = 3000, 400
    flat, off = ref.zipf_corpus(rng, n_chunks, n_terms, mean_len=10)
    live = rng.random(n_chunks) > 0.3
    p = _keyword.build_from_term_ids(flat, off, n_terms, live)
    kw = _ops.KeywordIndex(p)
    try:
        queries = ref.zipf_queries(rng, 9, n_terms) + [np.array([], np.int32), np.array([n_terms + 5, -3], np.int32)]
        for k in (5, 300):
            _check(p, kw, queries, k)
            allowed = rng.random(n_chunks) > 0.5
            _check(p, kw, queries, k, allowed)
        s, c, n = kw.search(queries[-2:], 4)  # no term / only unknown ids: nothing
        assert n.tolist() == [0, 0] and np.all(c == -1) and np.all(s == -np.inf)
        # dead chunks have no postings: they never come back
        s, c, n = kw.search([np.arange(n_terms)], 2048)
        assert not np.isin(c[0, : n[0]], np.nonzero(~live)[0]).any()
        with pytest.raises(ValueError, match="k must be <= 2048"):
            kw.search(queries[:1], 2049)
    finally:
        kw.close()


def test_duplicate_bodies_come_back_in_ordinal_order(torch_cuda):
    texts = ["red apples and green pears"] * 5 + ["blue sky"] + ["red apples and green pears"] * 3 + ["an apple a day"]
    gi = raglite_amd.GpuIndex([f"c{i}" for i in range(len(texts))], [np.eye(1, 8, i % 8, dtype=np.float32) for i in range(len(texts))],
                              keyword_texts=texts)
    try:
        ids, scores = raglite_amd.keyword_search("red apple", num_results=20, index=gi)
        assert ids == [f"c{i}" for i in (0, 1, 2, 3, 4, 6, 7, 8)] + ["c9"]
        assert len(set(scores[:8])) == 1 and scores[8] < scores[0]
        assert raglite_amd.keyword_search("zebra", index=gi) == ([], [])
        assert raglite_amd.keyword_search("the of and", index=gi) == ([], [])  # stopwords: never indexed
        assert raglite_amd.keyword_search("...", index=gi) == ([], [])
    finally:
        gi.close()


def _bodies(rng, n):
    words = ["gpu", "kernel", "memory", "bandwidth", "search", "vector", "keyword", "ranking", "fusion", "chunk", "document",
             "index", "query", "rerank", "embedding", "latency", "throughput", "cache", "tile", "wave", "matrix", "score", "token"]
    return [" ".join(rng.choice(words, size=int(rng.integers(3, 25)))) for _ in range(n)]


def _store_docs(rng, n_docs, dim, prefix):
    docs = sf.synthetic_documents(rng, n_docs, dim, prefix)
    out = []
    for doc_id, chunks in docs:
        bodies = _bodies(rng, len(chunks))
        out.append((doc_id, [(cid, h, body, m) for (cid, h, _, m), body in zip(chunks, bodies)]))
    return out


def _same_keyword_results(a, b, queries):
    for q in queries:
        ia, sa_ = raglite_amd.keyword_search(q, num_results=2048, index=a)
        ib, sb = raglite_amd.keyword_search(q, num_results=2048, index=b)
        assert sa_ == sb and dict(zip(ia, sa_)) == dict(zip(ib, sb)) and len(ia) == len(ib)
        fa = raglite_amd.keyword_search(q, num_results=7, metadata_filter={"topic": "t1"}, index=a)
        fb = raglite_amd.keyword_search(q, num_results=7, metadata_filter={"topic": "t1"}, index=b)
        assert fa[1] == fb[1]


def test_store_lifecycle_matches_a_fresh_index(torch_cuda):
    rng = np.random.default_rng(21)
    dim = 32
    engine = sf.create_store()
    docs = _store_docs(rng, 30, dim, "doc")
    for doc_id, chunks in docs:
        sf.insert_document(engine, doc_id, chunks)
    gi = raglite_amd.GpuIndex.from_store(engine, keywords=True)
    queries = ["gpu kernel", "memory bandwidth latency", "vector search ranking fusion", "tile", "unknown words only"]
    try:
        fresh = raglite_amd.GpuIndex.from_store(engine, keywords=True)
        _same_keyword_results(gi, fresh, queries)
        fresh.close()
        # insert, delete (changes N, avgdl and df), sync, compact: always what a fresh index over the live chunks returns
        for doc_id, chunks in _store_docs(rng, 6, dim, "new"):
            sf.insert_document(engine, doc_id, chunks)
        for doc_id, _ in docs[:4]:
            sf.delete_document(engine, doc_id)
        added, deleted = gi.sync(compact_above=1.0)
        assert added > 0 and deleted > 0 and gi.index.live()[1] < gi.index.n_chunks
        fresh = raglite_amd.GpuIndex.from_store(engine, keywords=True)
        _same_keyword_results(gi, fresh, queries)
        gi.compact()
        assert gi.index.live()[1] == gi.index.n_chunks
        _same_keyword_results(gi, fresh, queries)
        fresh.close()
        # a store-built index without keywords keeps its old behaviour
        plain = raglite_amd.GpuIndex.from_store(engine)
        assert not plain.has_keywords
        with pytest.raises(ValueError, match="without keyword texts"):
            raglite_amd.keyword_search("gpu", index=plain)
        plain.close()
    finally:
        gi.close()


def test_keyword_search_through_attach_index_and_hybrid_search(torch_cuda):
    rng = np.random.default_rng(5)
    dim, n = 64, 200
    texts = _bodies(rng, n)
    mats = [rng.standard_normal((int(rng.integers(1, 4)), dim)).astype(np.float32) for _ in range(n)]
    ids = [f"chunk-{i:03d}" for i in range(n)]
    meta = [{"topic": [f"t{i % 3}"]} for i in range(n)]
    gi = raglite_amd.GpuIndex(ids, mats, metadata=meta, keyword_texts=texts)
    cfg = raglite_amd.HotPathConfig(embedder="llama-cpp-python/fake/keyword", vector_search_query_adapter=False)
    raglite_amd.attach_index(gi)
    raglite_amd.set_embedder_factory(lambda config: FakeLlama(dim=dim))
    try:
        got = raglite_amd.keyword_search("kernel tile wave", num_results=10)
        assert got == raglite_amd.keyword_search("kernel tile wave", num_results=10, index=gi)
        assert len(got[0]) == 10 and all(a >= b for a, b in zip(got[1], got[1][1:]))
        filtered, _ = raglite_amd.keyword_search("kernel tile wave", num_results=10, metadata_filter={"topic": "t2"})
        assert filtered and all(meta[ids.index(c)]["topic"] == ["t2"] for c in filtered)
        assert raglite_amd.keyword_search("kernel", metadata_filter={"topic": "none"}) == ([], [])
        with pytest.raises(ValueError, match="2048"):
            raglite_amd.keyword_search("kernel", num_results=2049)
        with pytest.raises(NotImplementedError):
            raglite_amd.keyword_search("kernel", config=raglite_amd.HotPathConfig(self_query=True))
        # hybrid search over a keyword-enabled index: RRF of the two rankings, each computed on its own
        for query, flt in (("memory bandwidth of the kernel", None), ("vector search ranking", {"topic": "t1"})):
            vs, _ = raglite_amd.vector_search(query, num_results=2 * 5, metadata_filter=flt, config=cfg)
            ks, _ = raglite_amd.keyword_search(query, num_results=2 * 5, metadata_filter=flt, config=cfg)
            assert ks and ks != vs
            want = raglite_amd.reciprocal_rank_fusion([vs, ks], weights=[0.75, 0.25])
            assert raglite_amd.hybrid_search(query, num_results=5, metadata_filter=flt, config=cfg) == (want[0][:5], want[1][:5])
            assert raglite_amd.hybrid_search(query, num_results=5, metadata_filter=flt, config=cfg, index=gi) == (want[0][:5], want[1][:5])
    finally:
        raglite_amd.set_embedder_factory(None)
        raglite_amd.detach_index()
        gi.close()
