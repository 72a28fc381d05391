"""Batched search-and-rerank on the device: the ordering kernel (rl_rerank_order) against its NumPy restatement,
the one-call pipeline (rl_search_rerank_per_query) against the composition of the existing calls, and the public batched functions
against a loop of the single-query ones, element by element.

Embeddings, query vectors and token vectors are integer-valued in [-3, 3] wherever two routes are compared: every product and sum is
then exact whatever kernel a route takes, so batch and loop agree bit for bit (DESIGN.md §4.9 uses the same rule), and MaxSim ties
are frequent, which exercises the stable order."""

import zlib

import numpy as np
import pytest
import torch

import raglite_amd
from raglite_amd import _ops, _search
from tests import rerank_ref as ref

pytestmark = pytest.mark.gpu

N_CANDS = [1, 2, 5, 8, 33, 64, 65, 100, 4096]  # the smallest sorts, non-powers of two, the wave boundary, the LDS limit


# ---- 1. rl_rerank_order ---------------------------------------------------------------------------------------------------------
def _check_order(got, want, k, device):
    if device:
        assert all(t.is_cuda for t in got)
        got = tuple(t.cpu().numpy() for t in got)
    s, c, p, n = got
    ws, wc, wp, wn = want
    assert s.dtype == np.float32 and c.dtype == p.dtype == n.dtype == np.int32
    assert np.array_equal(n, np.minimum(wn, k))
    assert np.array_equal(p, wp[:, :k]) and np.array_equal(c, wc[:, :k])
    assert np.array_equal(ref.bits(s), ref.bits(ws[:, :k]))  # the input's own bits: that NaN, that zero; the tail -inf


@pytest.mark.parametrize("B", [1, 7, 300])  # 300: more workgroups than compute units
def test_rerank_order_equals_the_restatement(torch_cuda, B):
    rng = np.random.default_rng(B)
    for n_cand in N_CANDS:
        for pad in (0.0, 0.3, 1.0):
            scores, cand = ref.adversarial(rng, B, n_cand, pad=pad)
            want = ref.order(scores, cand, n_cand)
            ks = sorted({1, min(5, n_cand), n_cand})
            for k in ks:
                _check_order(_ops.rerank_order(scores, cand, k), want, k, device=False)
            k = ks[len(ks) // 2]
            _check_order(_ops.rerank_order(torch.as_tensor(scores, device="cuda"), torch.as_tensor(cand, device="cuda"), k), want, k,
                         device=True)


# ---- shared corpus ----------------------------------------------------------------------------------------------------------------
WORDS = ["gpu", "kernel", "memory", "bandwidth", "search", "vector", "keyword", "ranking", "fusion", "chunk", "document", "index",
         "query", "rerank", "embedding", "latency", "throughput", "cache", "tile", "wave", "matrix", "score", "token"]
DIM = 64


def _ints(rng, shape):
    return rng.integers(-3, 4, size=shape).astype(np.float32)


def _bodies(rng, n):
    return [" ".join(rng.choice(WORDS, size=int(rng.integers(3, 25)))) for _ in range(n)]


def _queries(rng, n):
    qs = [" ".join(rng.choice(WORDS, size=int(rng.integers(1, 5)))) + f" q{i}" for i in range(n)]
    qs[-1] = "zebra unicorn"  # no known stem: an empty keyword list
    return qs


def _index(rng, n=3000, dim=DIM, storage="f32", keywords=True):
    mats = [_ints(rng, (int(rng.integers(1, 4)), dim)) for _ in range(n)]
    ids = [f"chunk-{i:06d}" for i in range(n)]
    return raglite_amd.GpuIndex(ids, mats, metric="dot", storage=storage, docs=[f"text of chunk {i}" for i in range(n)],
                                metadata=[{"topic": [f"t{i % 3}"]} for i in range(n)], keyword_texts=_bodies(rng, n) if keywords else None)


@pytest.fixture(scope="module")
def corpus(torch_cuda):
    rng = np.random.default_rng(2024)
    gi = _index(rng)
    gi.delete_chunks([f"chunk-{i:06d}" for i in range(0, 3000, 7)])  # tombstones
    yield gi
    gi.close()


# ---- 2. DeviceIndex.search_rerank against hybrid_search -> maxsim_rerank -> the restatement ------------------------------------------
def _check_pipeline(gi, Q, V, terms, keyword, k, n_each=12, num_hits=40, device=False, **filters):
    kw = {"keyword": gi.keyword if keyword else None, "query_term_ids": terms if keyword else None}
    n_cand = min(16, (2 if keyword else 1) * n_each)
    k = min(k, n_cand)
    _, fused, _ = gi.index.hybrid_search(Q, num_hits, n_each, n_cand, **kw, **filters)
    scores = gi.index.maxsim_rerank(V, fused)
    ws, wc, _, wn = ref.order(scores, fused, k)
    if device:
        Q, V = torch.as_tensor(Q, device="cuda"), torch.as_tensor(V, device="cuda")
    s, c, n = gi.index.search_rerank(Q, num_hits, n_each, n_cand, V, k, **kw, **filters)
    if device:
        assert s.is_cuda and c.is_cuda and n.is_cuda and s.dtype == torch.float32
        s, c, n = s.cpu().numpy(), c.cpu().numpy(), n.cpu().numpy()
    assert np.array_equal(c, wc) and np.array_equal(n, wn)
    assert np.array_equal(ref.bits(s), ref.bits(ws))
    return c, n, fused


@pytest.mark.parametrize("nq", [1, 4, 32])
@pytest.mark.parametrize("B", [1, 16, 130])
def test_search_rerank_equals_the_composition(corpus, B, nq):
    gi = corpus
    rng = np.random.default_rng(100 * B + nq)
    Q, V = _ints(rng, (B, DIM)), _ints(rng, (B, nq, DIM))
    terms = [gi.keyword_query_ids(q) for q in _queries(rng, B)]
    n_chunks = len(gi.chunk_ids)
    reordered = False
    for keyword in (True, False):
        c, n, fused = _check_pipeline(gi, Q, V, terms, keyword, 16)
        assert (n > 0).all()
        reordered = reordered or any(c[b, : n[b]].tolist() != fused[b, : n[b]].tolist() for b in range(B))
        _check_pipeline(gi, Q, V, terms, keyword, 5, device=True)
        # per-query filters: none, two masks, one that matches nothing
        masks = [None, np.arange(n_chunks) % 3 == 1, np.arange(n_chunks) % 5 != 0, np.zeros(n_chunks, bool)]
        qf = [masks[(b + 1) % 4] for b in range(B)]
        c, n, _ = _check_pipeline(gi, Q, V, terms, keyword, 8, query_filters=qf)
        assert all(n[b] == 0 for b in range(B) if (b + 1) % 4 == 3)
        _check_pipeline(gi, Q, V, terms, keyword, 8, query_filters=qf, device=True)
        _check_pipeline(gi, Q, V, terms, keyword, 1, chunk_filter=masks[1])
    assert reordered  # the rerank changed some query's order: the comparison shows something
    assert not set(range(0, 3000, 7)).intersection(c[c >= 0].tolist())  # no tombstoned chunk comes back


@pytest.mark.parametrize("keyword", [True, False])
def test_search_rerank_at_odd_sizes_equals_the_composition(corpus, keyword):
    """The scratch of search_rerank (csrc/scratch_layout.h: RerankScratch over HybridLists) at odd sizes: B = 3, nq = 3, n_each = 5, k = 3;
    n_cand = 5 from the vector search alone, 10 with the keyword list."""
    rng = np.random.default_rng(77)
    B, nq = 3, 3
    Q, V = _ints(rng, (B, DIM)), _ints(rng, (B, nq, DIM))
    terms = [corpus.keyword_query_ids(q) for q in _queries(rng, B)]
    c, n, _ = _check_pipeline(corpus, Q, V, terms, keyword, 3, n_each=5, num_hits=20)
    assert (n == 3).all() and c.shape == (B, 3)
    _check_pipeline(corpus, Q, V, terms, keyword, 3, n_each=5, num_hits=20, device=True)


def test_search_rerank_on_an_fp16_stored_index_of_dim_1024(torch_cuda):
    rng = np.random.default_rng(3)
    gi = _index(rng, n=400, dim=1024, storage="f16")
    try:
        B, nq = 16, 32
        Q, V = _ints(rng, (B, 1024)), _ints(rng, (B, nq, 1024))
        terms = [gi.keyword_query_ids(q) for q in _queries(rng, B)]
        c, n, fused = _check_pipeline(gi, Q, V, terms, True, 16)
        assert (n >= 12).all()
        _check_pipeline(gi, Q, V, terms, False, 4, device=True)
        with pytest.raises(ValueError, match="nq <= 32"):
            gi.index.search_rerank(Q, 40, 12, 16, _ints(rng, (B, 33, 1024)), 4)
    finally:
        gi.close()


def test_search_rerank_argument_errors(corpus):
    gi = corpus
    Q, V = np.zeros((2, DIM), np.float32), np.zeros((2, 4, DIM), np.float32)
    with pytest.raises(ValueError, match="n_cand"):
        gi.index.search_rerank(Q, 40, 12, 4097, V, 4)
    with pytest.raises(ValueError, match="k must be"):
        gi.index.search_rerank(Q, 40, 12, 13, V, 4)  # more candidates than one list holds
    with pytest.raises(ValueError, match="k must be"):
        gi.index.search_rerank(Q, 40, 12, 8, V, 9)
    with pytest.raises(ValueError, match="query_vecs"):
        gi.index.search_rerank(Q, 40, 12, 8, V[:1], 4)


# ---- 3. search_and_rerank_chunks_batch against the loop --------------------------------------------------------------------------
def _hash_ints(text, shape):
    return _ints(np.random.default_rng(zlib.crc32(text.encode())), shape)


def _encode(query):
    """Token vectors of a query: two query lengths in one batch."""
    return _hash_ints("tokens " + query, (4 if query.endswith(("3", "7")) else 32, DIM))


@pytest.fixture
def pipeline(corpus, monkeypatch):
    """The corpus attached, integer-valued query embeddings, and a config whose reranker is a MaxSimRanker over the corpus."""
    monkeypatch.setattr(_search, "embed_strings", lambda strings, config=None: np.stack([_hash_ints(s, (DIM,)) for s in strings]))
    raglite_amd.attach_index(corpus)
    yield raglite_amd.HotPathConfig(vector_search_query_adapter=False, reranker=raglite_amd.MaxSimRanker(corpus, _encode))
    raglite_amd.detach_index()


def _lookup(gi):
    return lambda ids: [gi.docs[gi.ordinal_of(cid)] for cid in ids]


def _same_as_loop(gi, cfg, queries, search, filters=None, **kw):
    fn = raglite_amd.hybrid_search if search == "hybrid" else raglite_amd.vector_search
    per_query = filters if isinstance(filters, list) else [filters] * len(queries)
    want = [raglite_amd.search_and_rerank_chunks(q, search=fn, config=cfg, metadata_filter=f, chunk_lookup=_lookup(gi), **kw)
            for q, f in zip(queries, per_query)]
    got = raglite_amd.search_and_rerank_chunks_batch(queries, search=search, config=cfg, index=gi, metadata_filter=filters,
                                                     chunk_lookup=_lookup(gi), **kw)
    assert got == want, (search, filters, kw)
    ids = raglite_amd.search_and_rerank_chunks_batch(queries, search=fn, config=cfg, index=gi, metadata_filter=filters, **kw)
    assert [_lookup(gi)(x) for x in ids] == want  # without a lookup: the chunk ids
    return ids


@pytest.mark.parametrize("search", ["hybrid", "vector"])
@pytest.mark.parametrize("B", [1, 16, 257])
def test_batch_equals_the_loop(corpus, pipeline, B, search):
    gi, cfg = corpus, pipeline
    rng = np.random.default_rng(B)
    queries = _queries(rng, B)
    ids = _same_as_loop(gi, cfg, queries, search)  # num_results 8, oversample 4
    assert all(len(x) == 8 for x in ids)
    # the rerank changed some query's order
    plain = raglite_amd.HotPathConfig(vector_search_query_adapter=False)
    searched = raglite_amd.search_and_rerank_chunks_batch(queries, search=search, config=plain, index=gi)
    assert any(a != b for a, b in zip(ids, searched))
    per_query = [[None, {"topic": "t1"}, {"topic": "none"}, {"topic": ["t2"]}][b % 4] for b in range(B)]
    out = _same_as_loop(gi, cfg, queries, search, filters=per_query)
    assert all(out[b] == [] for b in range(B) if b % 4 == 2)
    if B == 257:
        return
    for num_results, oversample in ((1, 1), (1, 4), (8, 1)):
        _same_as_loop(gi, cfg, queries, search, num_results=num_results, oversample=oversample)
    _same_as_loop(gi, cfg, queries, search, filters={"topic": "t1"})
    assert all(x == [] for x in _same_as_loop(gi, cfg, queries, search, filters={"topic": "none"}))
    # precomputed query vectors and token vectors: the same answers
    vecs = np.stack([_hash_ints(q, (DIM,)) for q in queries])
    assert raglite_amd.search_and_rerank_chunks_batch(queries, search=search, config=cfg, index=gi, query_vectors=vecs,
                                                      query_token_vectors=[_encode(q) for q in queries]) == ids
    # no reranker: the search results, truncated
    assert _same_as_loop(gi, plain, queries, search) == [x[:8] for x in searched]
    # the loop's errors
    for kw in ({"num_results": 300}, {"num_results": 8, "oversample": 300}):
        with pytest.raises(ValueError, match="2048"):
            raglite_amd.search_and_rerank_chunks_batch(queries, search=search, config=cfg, index=gi, **kw)
        with pytest.raises(ValueError, match="2048"):
            raglite_amd.search_and_rerank_chunks(queries[0], search=raglite_amd.hybrid_search if search == "hybrid" else raglite_amd.vector_search,
                                                 config=cfg, **kw)
    with pytest.raises(NotImplementedError):
        raglite_amd.search_and_rerank_chunks_batch(queries, search=search, index=gi,
                                                   config=raglite_amd.HotPathConfig(self_query=True, reranker=cfg.reranker))
    with pytest.raises(ValueError, match="one entry per query"):
        raglite_amd.search_and_rerank_chunks_batch(queries, search=search, config=cfg, index=gi, metadata_filter=[None] * (B + 1))


def test_another_reranker_runs_per_query(corpus, pipeline):
    class Reversed:  # any other reranker: outside the device path
        def rank(self, query, docs):
            return _search.RankedResults([_search.Result(doc_id=i, score=0.0, rank=0) for i in reversed(range(len(docs)))], query)

    cfg = raglite_amd.HotPathConfig(vector_search_query_adapter=False, reranker=Reversed())
    queries = _queries(np.random.default_rng(1), 5)
    got = raglite_amd.search_and_rerank_chunks_batch(queries, config=cfg, index=corpus, chunk_lookup=_lookup(corpus))
    want = [raglite_amd.search_and_rerank_chunks(q, search=raglite_amd.hybrid_search, config=cfg, chunk_lookup=_lookup(corpus)) for q in queries]
    assert got == want and all(len(x) == 8 for x in got)


# ---- 4. rank_batch and rerank_chunks_batch against rank per query -------------------------------------------------------------------
def test_rank_batch_equals_rank(corpus, pipeline):
    gi, cfg = corpus, pipeline
    ranker = cfg.reranker
    rng = np.random.default_rng(9)
    queries = _queries(rng, 12)
    live = [i for i in range(3000) if i % 7]
    lists = [rng.choice(live, size=int(rng.integers(1, 40))).tolist() for _ in queries]  # ragged, with duplicates
    lists[2] = []  # an empty list
    lists[3] = [5, 5, 5, 9, 5]
    lists[4] = [0, 7, 5]  # tombstoned chunks score -inf and rank by position
    docs = [[gi.docs[i] for i in ids] for ids in lists]
    want = [ranker.rank(query=q, docs=d) for q, d in zip(queries, docs)]
    got = ranker.rank_batch(queries, docs)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.query == w.query and [r.doc_id for r in g.results] == [r.doc_id for r in w.results]
        assert [(r.rank, r.text) for r in g.results] == [(r.rank, r.text) for r in w.results]
        assert np.array_equal(ref.bits([r.score for r in g.results]), ref.bits([r.score for r in w.results]))
    assert [r.doc_id for r in got[4].results][-2:] == [0, 1] and got[2].results == []
    for s, q, ids in zip(ranker.score_batch(queries, lists), queries, lists):
        assert np.array_equal(ref.bits(s), ref.bits(ranker.score(q, ids)) if ids else np.zeros(0, np.uint32))
    keep = [b for b in range(len(queries)) if b != 4]  # (a deleted chunk's id is no longer known to the index)
    queries, want, lists = [queries[b] for b in keep], [want[b] for b in keep], [lists[b] for b in keep]
    reranked = raglite_amd.rerank_chunks_batch(queries, [[gi.chunk_ids[i] for i in ids] for ids in lists], config=cfg, index=gi)
    for (ids, scores), w, src in zip(reranked, want, lists):
        assert ids == [gi.chunk_ids[src[r.doc_id]] for r in w.results]
        assert scores == [r.score for r in w.results] and all(type(x) is float for x in scores)
