"""Batched hybrid search (DESIGN.md "Batched hybrid search"): the RRF kernel (rl_rrf_fuse) against the reference's fusion bit for
bit, and hybrid_search_batch against a loop of hybrid_search, element by element."""

import numpy as np
import pytest
import torch

import raglite_amd
from oracle.fake_embedder import FakeLlama
from raglite_amd import _ops
from tests import rrf_ref as ref

pytestmark = pytest.mark.gpu


def _check_fuse(lists, weights, rrf_k, k, device=False):
    arg = torch.as_tensor(lists, device="cuda") if device else lists
    s, i, n = _ops.rrf_fuse(arg, weights, rrf_k=rrf_k, k=k)
    if device:
        assert s.is_cuda and i.is_cuda and n.is_cuda
        s, i, n = s.cpu().numpy(), i.cpu().numpy(), n.cpu().numpy()
    R, B, L = lists.shape
    for b in range(B):
        want_ids, want_scores = raglite_amd.reciprocal_rank_fusion([[int(x) for x in lists[r, b] if x >= 0] for r in range(R)], k=rrf_k,
                                                                   weights=list(weights))
        m = min(k, len(want_ids))
        assert int(n[b]) == m, (R, L, b)
        assert i[b, :m].tolist() == want_ids[:m], (R, L, b)
        assert np.array_equal(s[b, :m].view(np.uint64), np.asarray(want_scores[:m], np.float64).view(np.uint64)), (R, L, b)
        assert np.all(i[b, m:] == -1) and np.all(s[b, m:] == -np.inf)


@pytest.mark.parametrize("R", [1, 2, 3, 4])
@pytest.mark.parametrize("B", [1, 7, 300])
def test_rrf_fuse_bits_equal_the_reference(torch_cuda, R, B):
    rng = np.random.default_rng(100 * R + B)
    weights = [0.75, 0.25, -0.5, 1.0][:R]
    for L in (1, 6, 20, 2048 // R):
        lists = ref.random_lists(rng, R, B, L)
        for k in sorted({1, min(5, R * L), R * L}):
            _check_fuse(lists, weights, 60, k)
        _check_fuse(lists, weights, 1, R * L, device=True)


@pytest.mark.parametrize("weights", [(1.0, 1.0), (1.0, -0.5), (0.0, 1.0), (-0.0, 0.3), (-0.0, -0.0), (2.5, 0.0, -1.25)])
@pytest.mark.parametrize("rrf_k", [1, 60])
def test_rrf_fuse_edge_cases(torch_cuda, weights, rrf_k):
    rng = np.random.default_rng(7)
    R = len(weights)
    for L in (3, 40):
        _check_fuse(ref.random_lists(rng, R, 9, L, universe=L), weights, rrf_k, R * L)  # heavy overlap and repeats
        _check_fuse(ref.random_lists(rng, R, 9, L, pad=0.9), weights, rrf_k, R * L, device=True)
    if R == 2:
        _check_fuse(ref.tie_lists(4, 16), weights, rrf_k, 32)  # exact ties by first occurrence


def test_rrf_fuse_rejects_bad_arguments(torch_cuda):
    lists = np.zeros((2, 3, 5), np.int32)
    with pytest.raises(ValueError, match="weights"):
        _ops.rrf_fuse(lists, [0.5, float("nan")], k=3)
    with pytest.raises(ValueError, match="rrf_k"):
        _ops.rrf_fuse(lists, [0.5, 0.5], rrf_k=0, k=3)
    with pytest.raises(ValueError, match="k must be"):
        _ops.rrf_fuse(lists, [0.5, 0.5], k=11)


# ---- hybrid_search_batch -----------------------------------------------------------------------------------------------------
WORDS = ["gpu", "kernel", "memory", "bandwidth", "search", "vector", "keyword", "ranking", "fusion", "chunk", "document", "index",
         "query", "rerank", "embedding", "latency", "throughput", "cache", "tile", "wave", "matrix", "score", "token"]


def _bodies(rng, n):
    return [" ".join(rng.choice(WORDS, size=int(rng.integers(3, 25)))) for _ in range(n)]


def _queries(rng, n):
    qs = [" ".join(rng.choice(WORDS, size=int(rng.integers(1, 5)))) for _ in range(n)]
    qs[-1] = "zebra unicorn"  # no known stem: an empty keyword list
    return qs


@pytest.fixture
def fake_embedder():
    raglite_amd.set_embedder_factory(lambda config: FakeLlama(dim=64))
    yield raglite_amd.HotPathConfig(embedder="llama-cpp-python/fake/hybrid", vector_search_query_adapter=False)
    raglite_amd.set_embedder_factory(None)


def _index(rng, n, dim=64, keywords=True, rows=(1, 4), topic=lambda i: f"t{i % 3}"):
    mats = [rng.standard_normal((int(rng.integers(*rows)), dim)).astype(np.float32) for _ in range(n)]
    ids = [f"chunk-{i:06d}" for i in range(n)]
    meta = [{"topic": [topic(i)]} for i in range(n)]
    return raglite_amd.GpuIndex(ids, mats, metadata=meta, keyword_texts=_bodies(rng, n) if keywords else None)


def _same_as_loop(gi, cfg, queries, **kw):
    got = raglite_amd.hybrid_search_batch(queries, config=cfg, index=gi, **kw)
    want = [raglite_amd.hybrid_search(q, config=cfg, index=gi, **kw) for q in queries]
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], (b, kw)
        assert g[1] == w[1] and all(type(x) is float for x in g[1]), (b, kw)
    return got


@pytest.mark.parametrize("B", [1, 16, 257])
def test_batch_equals_the_loop(torch_cuda, fake_embedder, B):
    rng = np.random.default_rng(B)
    gi = _index(rng, 3000)
    try:
        queries = _queries(rng, B)
        got = _same_as_loop(gi, fake_embedder, queries)
        assert any(len(g[0]) == 3 for g in got)
        _same_as_loop(gi, fake_embedder, queries, num_results=1)
        _same_as_loop(gi, fake_embedder, queries, num_results=7, oversample=3, vector_search_weight=0.5, keyword_search_weight=0.5)
        _same_as_loop(gi, fake_embedder, queries, metadata_filter={"topic": "t1"})  # filter first
        assert all(g == ([], []) for g in _same_as_loop(gi, fake_embedder, queries, metadata_filter={"topic": "none"}))
        # precomputed query vectors: the same answers
        vecs = np.stack([raglite_amd.embed_strings([q], config=fake_embedder)[0, :] for q in queries])
        assert raglite_amd.hybrid_search_batch(queries, config=fake_embedder, index=gi, query_vectors=vecs) == got
        # the K_MAX limit: the same ValueError
        with pytest.raises(ValueError, match="2048"):
            raglite_amd.hybrid_search_batch(queries, num_results=1025, config=fake_embedder, index=gi)
        with pytest.raises(ValueError, match="2048"):
            raglite_amd.hybrid_search(queries[0], num_results=1025, config=fake_embedder, index=gi)
        with pytest.raises(NotImplementedError):
            raglite_amd.hybrid_search_batch(queries, config=raglite_amd.HotPathConfig(self_query=True), index=gi)
    finally:
        gi.close()


def test_large_num_results_and_unknown_stems(torch_cuda, fake_embedder):
    rng = np.random.default_rng(11)
    gi = _index(rng, 4000)
    try:
        queries = _queries(rng, 5)
        _same_as_loop(gi, fake_embedder, queries, num_results=100, oversample=2)  # n_each 200, num_hits 800
        _same_as_loop(gi, fake_embedder, queries, num_results=512, oversample=1)  # num_hits 2048: the limit itself
        _same_as_loop(gi, fake_embedder, ["zebra", "unicorn quagga"] * 3)
    finally:
        gi.close()


def test_order_first_filter_on_a_large_corpus(torch_cuda, fake_embedder):
    rng = np.random.default_rng(12)
    # ~210 000 rows: "big" (two chunks in three) matches more than 100 000 of them -> order first; "small" fewer -> filter first
    gi = _index(rng, 60_000, rows=(2, 5), topic=lambda i: "small" if i % 3 == 2 else "big")
    try:
        rows = np.diff(gi.index.chunk_offsets)
        assert rows[np.arange(len(rows)) % 3 != 2].sum() > 100_000 >= rows[np.arange(len(rows)) % 3 == 2].sum()
        queries = _queries(rng, 16)
        _same_as_loop(gi, fake_embedder, queries, metadata_filter={"topic": "big"}, num_results=8, oversample=4)
        _same_as_loop(gi, fake_embedder, queries, metadata_filter={"topic": "big"})
        _same_as_loop(gi, fake_embedder, queries, metadata_filter={"topic": "small"}, num_results=8, oversample=4)
        _same_as_loop(gi, fake_embedder, queries, num_results=8, oversample=4)
    finally:
        gi.close()


def test_without_keyword_side_and_after_lifecycle(torch_cuda, fake_embedder):
    rng = np.random.default_rng(13)
    plain = _index(rng, 500, keywords=False)
    gi = _index(rng, 800)
    try:
        queries = _queries(rng, 16)
        _same_as_loop(plain, fake_embedder, queries)
        _same_as_loop(plain, fake_embedder, queries, metadata_filter={"topic": "t2"})
        new = [rng.standard_normal((2, 64)).astype(np.float32) for _ in range(40)]
        gi.insert_chunks([f"new-{i}" for i in range(40)], new, metadata=[{"topic": ["t1"]}] * 40, keyword_texts=_bodies(rng, 40))
        _same_as_loop(gi, fake_embedder, queries)
        gi.delete_chunks([f"chunk-{i:06d}" for i in range(0, 800, 3)])
        _same_as_loop(gi, fake_embedder, queries)
        _same_as_loop(gi, fake_embedder, queries, metadata_filter={"topic": "t1"})
        gi.compact()
        _same_as_loop(gi, fake_embedder, queries)
        # an empty corpus
        empty = raglite_amd.GpuIndex([], [], keyword_texts=[])
        try:
            assert raglite_amd.hybrid_search_batch(queries[:3], config=fake_embedder, index=empty) == [([], [])] * 3
        finally:
            empty.close()
    finally:
        plain.close()
        gi.close()


def test_three_queries_of_five_hits_equal_single_query_calls(torch_cuda, fake_embedder):
    """The scratch of hybrid_search (csrc/scratch_layout.h: HybridLists) at odd sizes -- B = 3, n_each = 5, k = 3: lists of 15 and counts of
    3 words per search -- with the keyword side (two lists per query) and without."""
    rng = np.random.default_rng(15)
    gi = _index(rng, 2000)
    try:
        queries = _queries(rng, 3)
        Q = np.stack([raglite_amd.embed_strings([q], config=fake_embedder)[0, :] for q in queries]).astype(np.float32)
        terms = [gi.keyword_query_ids(q) for q in queries]
        for keyword in (gi.keyword, None):
            s, c, n = gi.index.hybrid_search(Q, 20, 5, 3, keyword=keyword, query_term_ids=terms)
            assert (n[:2] == 3).all()
            for b in range(3):
                s1, c1, n1 = gi.index.hybrid_search(Q[b:b + 1], 20, 5, 3, keyword=keyword, query_term_ids=terms[b:b + 1])
                assert np.array_equal(c[b], c1[0]) and n[b] == n1[0]
                assert np.array_equal(s[b].view(np.uint64), s1[0].view(np.uint64))
    finally:
        gi.close()


def test_device_tensors_equal_host_arrays(torch_cuda, fake_embedder):
    rng = np.random.default_rng(14)
    gi = _index(rng, 2000)
    try:
        queries = _queries(rng, 33)
        Q = np.stack([raglite_amd.embed_strings([q], config=fake_embedder)[0, :] for q in queries]).astype(np.float32)
        terms = [gi.keyword_query_ids(q) for q in queries]
        allowed = np.arange(2000) % 3 == 1
        for flt, keyword in ((None, gi.keyword), (allowed, gi.keyword), (None, None)):
            hs, hc, hn = gi.index.hybrid_search(Q, 40, 6, 6, keyword=keyword, query_term_ids=terms, chunk_filter=flt)
            ds, dc, dn = gi.index.hybrid_search(torch.as_tensor(Q, device="cuda"), 40, 6, 6, keyword=keyword, query_term_ids=terms,
                                                chunk_filter=flt)
            assert ds.is_cuda and dc.is_cuda and dn.is_cuda and ds.dtype == torch.float64
            torch.cuda.synchronize()
            assert np.array_equal(ds.cpu().numpy().view(np.uint64), hs.view(np.uint64))
            assert np.array_equal(dc.cpu().numpy(), hc) and np.array_equal(dn.cpu().numpy(), hn)
            assert (hn > 0).any()
    finally:
        gi.close()
