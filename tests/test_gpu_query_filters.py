"""Per-query metadata filters in one batch: row b of a batched call with per-query filters and rank limits is bit for
bit what the single call returns for query b alone with its own filter and limit (`DeviceIndex.search_chunks`, `KeywordIndex.search`,
`DeviceIndex.hybrid_search`), and `vector_search_batch` / `keyword_search_batch` / `hybrid_search_batch` with a list of filters equal the
loop of `vector_search` / `keyword_search` / `hybrid_search`.  The row searches run on integer-valued embeddings, where every route's
arithmetic is exact: a batch and a single query take different routes (half-bytes pass, stream, score GEMM, scan), which agree to the last
bit only there -- the same relation an unfiltered batch has to single calls (tests/test_gpu_hi_search.py uses the same data)."""

import numpy as np
import pytest
import torch

import raglite_amd
from oracle import oracle
from oracle.fake_embedder import FakeLlama
from raglite_amd import _keyword, _ops, _search
from tests import keyword_ref as ref

pytestmark = pytest.mark.gpu


def _filter_pool(rng, n_chunks):
    """None, all clear, one chunk, about 1 %, about 50 %, all set"""
    one = np.zeros(n_chunks, bool)
    one[int(rng.integers(n_chunks))] = True
    return [None, np.zeros(n_chunks, bool), one, rng.random(n_chunks) < 0.01, rng.random(n_chunks) < 0.5, np.ones(n_chunks, bool)]


def _draw(rng, pool, B):
    """one entry per query; with B > len(pool) several queries share one filter (the same object)"""
    return [pool[int(i)] for i in rng.integers(len(pool), size=B)]


def _corpus(rng, n_chunks, dim, metric, storage, seed):
    sizes = rng.integers(1, 4, size=n_chunks)
    off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    E = torch.empty((int(off[-1]), dim), dtype=torch.float32, device="cuda")
    raglite_amd.synth_fill(E, seed=seed, kind="small_int")
    return _ops.DeviceIndex(E, off, metric=metric, storage=storage)


def _int_queries(seed, B, dim):
    return oracle.synth_matrix(seed, B, dim, "small_int")


def _same_row(got, want, b, what):
    (s, c, n), (ws, wc, wn) = got, want
    assert int(n[b]) == int(wn), (what, b)
    assert np.array_equal(c[b], wc), (what, b)
    assert np.array_equal(s[b].view(np.uint32 if s.dtype == np.float32 else np.uint64), ws.view(np.uint32 if ws.dtype == np.float32 else np.uint64)), (what, b)


def _host(out):
    if isinstance(out[0], torch.Tensor):
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy() for t in out)
    return out


def _check_chunks(idx, Q, num_hits, k, filters, limits, device=False):
    q = torch.as_tensor(Q, device="cuda") if device else Q
    got = _host(idx.search_chunks(q, num_hits, k, query_filters=filters, rank_limit=limits))
    for b in range(len(Q)):
        lim = None if limits is None else limits[b]
        _same_row(got, idx.search_chunks(Q[b], num_hits, k, chunk_filter=filters[b], rank_limit=lim), b, ("chunks", len(Q), lim))


@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("metric", ["cosine", "dot", "l2"])
def test_search_chunks_per_query_equals_single_calls(torch_cuda, metric, storage):
    rng = np.random.default_rng(10 * ["cosine", "dot", "l2"].index(metric) + (storage == "f16"))
    idx = _corpus(rng, 36_000, 1024, metric, storage, seed=3)  # ~72 k rows: the half-bytes route takes B <= 16 (l2: <= 4)
    try:
        assert idx.n_rows >= 65_536
        pool = _filter_pool(rng, idx.n_chunks)
        limit_pool = [0, idx.n_rows // 3, idx.n_rows + 5]  # no cut, a cut, a limit above the rows
        for B in (1, 5, 16, 17, 40, 96, 130):
            Q = _int_queries(100 + B, B, 1024)
            filters = _draw(rng, pool, B)
            _check_chunks(idx, Q, 64, 10, filters, None)
            _check_chunks(idx, Q, 64, 10, filters, [limit_pool[int(i)] for i in rng.integers(3, size=B)])
        # tombstoned chunks never match, with or without a filter; CUDA tensors equal host arrays
        idx.delete_chunks(np.arange(0, idx.n_chunks, 5, dtype=np.int64))
        live_rows, _ = idx.live()
        for B in (3, 16, 40):
            Q = _int_queries(200 + B, B, 1024)
            filters = _draw(rng, pool, B)
            limits = [[0, live_rows // 2, live_rows][int(i)] for i in rng.integers(3, size=B)]
            _check_chunks(idx, Q, 64, 10, filters, None)
            _check_chunks(idx, Q, 64, 10, filters, limits)
            _check_chunks(idx, Q, 64, 10, filters, limits, device=True)
    finally:
        idx.close()


@pytest.mark.parametrize("metric", ["cosine", "dot", "l2"])
def test_wide_index_per_query_filters(torch_cuda, metric):
    rng = np.random.default_rng(7)
    idx = _corpus(rng, 34_000, 1536, metric, "f32", seed=5)  # dim 1536: the wide half-bytes route for up to four queries
    try:
        assert idx.n_rows >= 65_536
        pool = _filter_pool(rng, idx.n_chunks)
        for B in (1, 3, 4, 9):
            Q = _int_queries(300 + B, B, 1536)
            filters = _draw(rng, pool, B)
            _check_chunks(idx, Q, 32, 8, filters, None)
            _check_chunks(idx, Q, 32, 8, filters, [[0, 20_000, 10**9][b % 3] for b in range(B)])
    finally:
        idx.close()


def _keyword_corpus(rng, n_chunks, n_terms=3000):
    flat, off = ref.zipf_corpus(rng, n_chunks, n_terms, 40)
    return _ops.KeywordIndex(_keyword.build_from_term_ids(flat, off, n_terms))


def _term_lists(rng, B, n_terms=3000):
    terms = [sorted(set(int(x) for x in t)) for t in ref.zipf_queries(rng, B, n_terms)]
    terms[-1] = []  # a query without a known term
    return terms


def test_keyword_search_per_query_equals_single_calls(torch_cuda):
    rng = np.random.default_rng(21)
    kw = _keyword_corpus(rng, 30_000)
    try:
        pool = _filter_pool(rng, kw.n_chunks)
        for B in (1, 5, 17, 130):
            terms = _term_lists(rng, B)
            filters = _draw(rng, pool, B)
            got = kw.search(terms, 10, query_filters=filters)
            for b in range(B):
                ws, wc, wn = kw.search([terms[b]], 10, chunk_filter=filters[b])
                _same_row(got, (ws[0], wc[0], wn[0]), b, ("keyword", B))
        got, want = kw.search(terms, 10, query_filters=[None] * B), kw.search(terms, 10)  # no filter at all: the unfiltered call
        for b in range(B):
            _same_row(got, (want[0][b], want[1][b], want[2][b]), b, ("keyword unfiltered", B))
    finally:
        kw.close()


def test_hybrid_search_per_query_equals_single_calls(torch_cuda):
    rng = np.random.default_rng(22)
    n_chunks = 30_000
    sizes = rng.integers(1, 4, size=n_chunks)
    off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    idx = _ops.DeviceIndex(oracle.synth_matrix(23, int(off[-1]), 128, "small_int"), off)
    kw = _keyword_corpus(rng, n_chunks)
    try:
        idx.delete_chunks(np.arange(3, n_chunks, 11, dtype=np.int64))
        pool = _filter_pool(rng, n_chunks)
        for B in (1, 16, 40):
            Q = _int_queries(400 + B, B, 128)
            terms = _term_lists(rng, B)
            filters = _draw(rng, pool, B)
            limits = [[0, 5_000, 10**9][int(i)] for i in rng.integers(3, size=B)]
            for keyword in (kw, None):
                for device in (False, True):
                    q = torch.as_tensor(Q, device="cuda") if device else Q
                    got = _host(idx.hybrid_search(q, 64, 16, 16, keyword=keyword, query_term_ids=terms, query_filters=filters,
                                                  rank_limit=limits))
                    for b in range(B):
                        want = idx.hybrid_search(Q[b], 64, 16, 16, keyword=keyword, query_term_ids=[terms[b]], chunk_filter=filters[b],
                                                 rank_limit=limits[b])
                        _same_row(got, want, b, ("hybrid", B, keyword is None, device))
    finally:
        idx.close()
        kw.close()


# ---- the public functions -----------------------------------------------------------------------------------------------------
WORDS = ["gpu", "kernel", "memory", "bandwidth", "search", "vector", "keyword", "ranking", "fusion", "chunk", "document", "index",
         "query", "rerank", "embedding", "latency", "throughput", "cache", "tile", "wave", "matrix", "score", "token"]
FILTERS = [None, {"tenant": "t1"}, {"tenant": "nobody"}, {"lang": "en"}, {"tenant": ["t2"], "lang": "de"}, {}, {"tenant": "t1"}]


@pytest.fixture
def fake_embedder():
    raglite_amd.set_embedder_factory(lambda config: FakeLlama(dim=64))
    yield raglite_amd.HotPathConfig(embedder="llama-cpp-python/fake/query-filters", vector_search_query_adapter=False)
    raglite_amd.set_embedder_factory(None)


def _gi(rng, n, metadata=True):
    mats = [rng.standard_normal((int(rng.integers(1, 4)), 64)).astype(np.float32) for _ in range(n)]
    meta = [{"tenant": f"t{i % 5}", "lang": ["en", "de"][i % 2]} for i in range(n)] if metadata else None
    bodies = [" ".join(rng.choice(WORDS, size=int(rng.integers(3, 25)))) for _ in range(n)]
    return raglite_amd.GpuIndex([f"chunk-{i:06d}" for i in range(n)], mats, metadata=meta, keyword_texts=bodies)


def _queries(rng, n):
    qs = [" ".join(rng.choice(WORDS, size=int(rng.integers(1, 5)))) for _ in range(n)]
    qs[-1] = "zebra unicorn"  # no known stem
    return qs


def _same_outcome(batch, single, queries, filters, **kw):
    """The loop raises (a ValueError, for some element) -> the batch raises with the same message; else the same results."""
    per = filters if isinstance(filters, list) else [filters] * len(queries)
    try:
        want = [single(q, metadata_filter=f, **kw) for q, f in zip(queries, per)]
    except ValueError as e:
        with pytest.raises(ValueError) as got:
            batch(queries, metadata_filter=filters, **kw)
        assert str(got.value) == str(e), batch.__name__
        return None
    assert batch(queries, metadata_filter=filters, **kw) == want, batch.__name__
    return want


def _same_as_loop(batch, single, queries, filters, **kw):
    got = batch(queries, metadata_filter=filters, **kw)
    per = filters if isinstance(filters, list) else [filters] * len(queries)
    want = [single(q, metadata_filter=f, **kw) for q, f in zip(queries, per)]
    assert got == want, (batch.__name__, kw)
    assert all(type(x) is float for g in got for x in g[1])
    return got


PAIRS = [(raglite_amd.vector_search_batch, raglite_amd.vector_search), (raglite_amd.keyword_search_batch, raglite_amd.keyword_search),
         (raglite_amd.hybrid_search_batch, raglite_amd.hybrid_search)]


def test_public_batches_equal_the_loop(torch_cuda, fake_embedder, monkeypatch):
    rng = np.random.default_rng(31)
    gi = _gi(rng, 3000)
    try:
        queries = _queries(rng, 26)
        filters = [FILTERS[i % len(FILTERS)] for i in range(len(queries))]
        kw = dict(config=fake_embedder, index=gi)
        for scale in ("as configured", "both branches"):
            if scale == "both branches":  # a real cut at test scale: "lang en" matches ~3 000 rows > 500 -> order first, limit 800
                monkeypatch.setattr(_search, "FILTER_FIRST_MAX_ROWS", 500)
                monkeypatch.setattr(_search, "ORDER_FIRST_LIMIT", 800)
                assert gi.index.n_rows > 800
            for batch, single in PAIRS:
                got = _same_as_loop(batch, single, queries, filters, num_results=5, **kw)
                assert any(g[0] for g in got) and any(g == ([], []) for g in got)
                _same_as_loop(batch, single, queries, {"lang": "de"}, **kw)  # one dict for the batch
                _same_as_loop(batch, single, queries, None, **kw)
            _same_as_loop(raglite_amd.hybrid_search_batch, raglite_amd.hybrid_search, queries, filters, num_results=8, oversample=4, **kw)
            _same_as_loop(raglite_amd.vector_search_batch, raglite_amd.vector_search, queries, filters, num_results=12, oversample=2, **kw)
        # precomputed query vectors
        vecs = np.stack([raglite_amd.embed_strings([q], config=fake_embedder)[0, :] for q in queries])
        assert raglite_amd.vector_search_batch(queries, metadata_filter=filters, query_vectors=vecs, **kw) == \
            raglite_amd.vector_search_batch(queries, metadata_filter=filters, **kw)
        # queries given as vectors: hybrid_search runs no keyword half for them, and neither does the batch
        mixed = [vecs[b] if b % 3 == 0 else q for b, q in enumerate(queries)]
        _same_as_loop(raglite_amd.hybrid_search_batch, raglite_amd.hybrid_search, mixed, filters, **kw)
        _same_as_loop(raglite_amd.vector_search_batch, raglite_amd.vector_search, mixed, filters, **kw)
    finally:
        gi.close()


def test_public_batches_raise_as_the_loop(torch_cuda, fake_embedder):
    rng = np.random.default_rng(32)
    gi = _gi(rng, 400)
    bare = _gi(rng, 300, metadata=False)
    empty = raglite_amd.GpuIndex([], [], metadata=[], keyword_texts=[])
    try:
        queries = _queries(rng, 4)
        kw = dict(config=fake_embedder)
        nothing = [{"tenant": "nobody"}] * 4
        for batch, single in PAIRS:
            # no metadata: raises only where an element applies a filter
            assert _same_outcome(batch, single, queries, [None, {"tenant": "t1"}, None, None], index=bare, **kw) is None
            _same_as_loop(batch, single, queries, [None] * 4, index=bare, **kw)
            # an empty index
            assert _same_as_loop(batch, single, queries, FILTERS[:4], index=empty, **kw) == [([], [])] * 4
            with pytest.raises(NotImplementedError):
                batch(queries, index=gi, config=raglite_amd.HotPathConfig(self_query=True))
            with pytest.raises(ValueError, match="one entry per query"):
                batch(queries, metadata_filter=[None] * 3, index=gi, **kw)
            # the K_MAX limits: raised where the loop raises for some element
            for n in (1025, 2049):
                for filters in (nothing, nothing[:3] + [None], None):
                    _same_outcome(batch, single, queries, filters, num_results=n, index=gi, **kw)
        # vector_search returns before its limit check where the filter matches nothing
        assert _same_outcome(raglite_amd.vector_search_batch, raglite_amd.vector_search, queries, nothing, num_results=1025, index=gi,
                             **kw) == [([], [])] * 4
        assert _same_outcome(raglite_amd.vector_search_batch, raglite_amd.vector_search, queries, nothing[:3] + [None], num_results=1025,
                             index=gi, **kw) is None
    finally:
        gi.close()
        bare.close()
        empty.close()


def test_filter_sets_in_any_order_through_the_c_abi(torch_cuda):
    """query_filter naming the rows of chunk_filters in any order, and a row no query reads: the distinct filters of a sub-batch are
    expanded through the filter-id map (not in table order) -- rl_search_chunks_per_query and rl_hybrid_search_per_query, row b equal to
    the single call for query b."""
    from raglite_amd import _abi

    rng = np.random.default_rng(41)
    idx = _corpus(rng, 34_000, 1024, "cosine", "f32", seed=9)
    kw = _keyword_corpus(rng, idx.n_chunks)
    lib = _abi.lib()
    try:
        pool = _filter_pool(rng, idx.n_chunks)
        table = np.ascontiguousarray(np.stack([_ops.pack_bits(pool[i]) for i in (3, 4, 2, 5)]))  # row 3: read by no query
        w = np.asarray([0.75, 0.25], np.float64)
        for qf in ([2, -1, 0, 2, 1], [1, 0, -1, 2, 2, 0, 1, 1, -1, 2, 0, 1]):  # the half-bytes route, the score matrix
            B = len(qf)
            Q = _int_queries(500 + B, B, 1024)
            qfa = np.asarray(qf, np.int32)
            q_off, q_terms = _ops._term_csr(_term_lists(rng, B))  # noqa: SLF001
            for limits in (None, np.asarray([[0, 20_000, 10**9][b % 3] for b in range(B)], np.int64)):
                p_lim = None if limits is None else limits.ctypes.data
                s, c, n = np.empty((B, 8), np.float32), np.empty((B, 8), np.int32), np.empty(B, np.int32)
                _abi.check(lib.rl_search_chunks_per_query(idx._handle, Q.ctypes.data, B, 64, 8, table.ctypes.data, len(table), qfa.ctypes.data,  # noqa: SLF001
                                                          p_lim, s.ctypes.data, c.ctypes.data, n.ctypes.data, _abi.MEM_HOST, None))
                hs, hc, hn = np.empty((B, 8), np.float64), np.empty((B, 8), np.int32), np.empty(B, np.int32)
                _abi.check(lib.rl_hybrid_search_per_query(idx._handle, kw._handle, Q.ctypes.data, B, 64, 8, q_off.ctypes.data,  # noqa: SLF001
                                                          q_terms.ctypes.data, table.ctypes.data, len(table), qfa.ctypes.data, p_lim,
                                                          w.ctypes.data, 60, 8, hs.ctypes.data, hc.ctypes.data, hn.ctypes.data,
                                                          _abi.MEM_HOST, None))
                for b in range(B):
                    f = None if qf[b] < 0 else table[qf[b]]
                    lim = None if limits is None else int(limits[b])
                    _same_row((s, c, n), idx.search_chunks(Q[b], 64, 8, chunk_filter=f, rank_limit=lim), b, ("abi chunks", qf, lim))
                    terms_b = [q_terms[q_off[b]:q_off[b + 1]].tolist()]
                    want = idx.hybrid_search(Q[b], 64, 8, 8, keyword=kw, query_term_ids=terms_b, chunk_filter=f, rank_limit=lim)
                    _same_row((hs, hc, hn), want, b, ("abi hybrid", qf, lim))
    finally:
        idx.close()
        kw.close()
