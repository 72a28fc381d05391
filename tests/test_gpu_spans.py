"""Chunk spans on the device: the span kernel (rl_chunk_spans) against the restatement of `retrieve_chunk_spans`
(tests/spans_ref.py), the one-call pipeline (rl_search_rerank_spans_per_query) against the composition of the existing calls, the
public batched functions against a loop of the single-query ones and against `search_and_rerank_chunks` followed by the restatement,
and `retrieve_context`.  Equality is of ordinals, lengths, counts and the bits of the scores.

Embeddings, query vectors and token vectors are integer-valued in [-3, 3] wherever two routes are compared (DESIGN.md §4.9's rule)."""

import zlib

import numpy as np
import pytest
import torch

import raglite_amd
from raglite_amd import _ops, _search
from tests import spans_ref as ref
from tests import store_fixture
from tests.test_spans_host import last_bit_case, tie_case

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _layout(rng, n_chunks, max_doc=40, dead_every=0):
    """Positions for n_chunks chunks in documents of 1 to max_doc chunks with random gaps in `index`, in shuffled ordinal order.
    Document names are unpadded ("doc9", "doc10"), so their string order is not their numeric order."""
    positions, d = [], 0
    while len(positions) < n_chunks:
        size, at = int(rng.integers(1, max_doc + 1)), int(rng.integers(0, 3))
        for _ in range(min(size, n_chunks - len(positions))):
            positions.append((f"doc{d}", at))
            at += 1 if rng.random() < 0.8 else int(rng.integers(2, 5))
        d += 1
    positions = [positions[i] for i in rng.permutation(n_chunks)]
    if dead_every:
        positions = [None if o % dead_every == 0 else p for o, p in enumerate(positions)]
    return positions


def _device_table(positions):
    """(SpanTable, ref.Table keyed by ordinal) of a list of positions (None: no position), numbered as GpuIndex numbers them."""
    doc_no = {d: i for i, d in enumerate(sorted({p[0] for p in positions if p is not None}))}
    doc = np.array([-1 if p is None else doc_no[p[0]] for p in positions], np.int32)
    pos = np.array([0 if p is None else p[1] for p in positions], np.int32)
    return _ops.SpanTable(doc, pos), ref.Table({o: p for o, p in enumerate(positions) if p is not None})


def _unpack(out, b):
    """Row b of rl_chunk_spans' outputs as [(ordinals, score)], after checking its padding and counts."""
    chunks, lens, scores, n_spans, n_chunks = (np.asarray(x) for x in out)
    ns, nc = int(n_spans[b]), int(n_chunks[b])
    assert (lens[b, :ns] > 0).all() and int(lens[b, :ns].sum()) == nc
    assert (chunks[b, :nc] >= 0).all() and (chunks[b, nc:] == -1).all() and (lens[b, ns:] == 0).all() and (scores[b, ns:] == 0).all()
    at, spans = 0, []
    for length, score in zip(lens[b, :ns].tolist(), scores[b, :ns].tolist()):
        spans.append((chunks[b, at : at + length].tolist(), score))
        at += length
    return spans


def _same(got, want):
    assert [s[0] for s in got] == [s[0] for s in want]
    assert np.array_equal(_bits([s[1] for s in got]), _bits([s[-1] for s in want]))


# ---- 1. rl_chunk_spans against the restatement ------------------------------------------------------------------------------------
N_TABLE = 2000


@pytest.fixture(scope="module")
def table(torch_cuda):
    rng = np.random.default_rng(7)
    positions = _layout(rng, N_TABLE, dead_every=9)  # every ninth chunk is tombstoned
    dev, host = _device_table(positions)
    assert dev.info()[:2] == (N_TABLE, len(host.pos)) and dev.info()[2] >= 16 * len(host.pos)
    yield dev, host, positions
    dev.close()


def _row(rng, kind, n_in, host):
    live = np.array(sorted(host.pos), np.int32)
    if kind == 0:  # distinct live chunks (as many as there are: a longer list repeats them)
        row = np.concatenate([rng.permutation(live) for _ in range(-(-n_in // len(live)))])[:n_in]
    elif kind == 1:  # padding anywhere
        row = np.where(rng.random(n_in) < 0.3, -1, rng.choice(live, n_in))
    elif kind == 2:  # nothing but padding
        row = np.full(n_in, -1)
    elif kind == 3:  # duplicates: a small pool
        row = rng.choice(live[: max(2, n_in // 3)], n_in)
    elif kind == 4:  # tombstoned, out-of-range and negative entries among live ones
        odd = np.array([0, 9, 18, N_TABLE, N_TABLE + 5, 2 ** 31 - 1, -7, -2 ** 31])
        row = np.where(rng.random(n_in) < 0.5, rng.choice(odd, n_in), rng.choice(live, n_in))
    elif kind == 5:  # every chunk of one document, shuffled; the rest is padding
        by_doc = {}
        for o, p in host.pos.items():
            by_doc.setdefault(p[0], []).append(o)
        members = rng.permutation(max(by_doc.values(), key=len))
        row = np.full(n_in, -1)
        row[: min(n_in, len(members))] = members[:n_in]
    else:  # anything, with replacement
        row = rng.integers(0, N_TABLE, n_in)
    return row.astype(np.int64).astype(np.int32)


@pytest.mark.parametrize("B", [1, 7, 300])  # 300: more workgroups than compute units
def test_chunk_spans_equal_the_restatement(table, B):
    dev, host, positions = table
    rng = np.random.default_rng(B)
    for case, (n_in, neighbors) in enumerate([(1, (-1, 1)), (2, (-1, 1)), (8, (-1, 1)), (33, (-1, 1)), (1365, (-1, 1)), (4096, None),
                                              (8, ()), (8, (0, 1, 1, -2, 40)), (64, tuple(range(-32, 31)))]):
        if B == 300 and case >= 6:
            continue
        chunks = np.stack([_row(rng, (b + case) % 7, n_in, host) for b in range(B)])
        want = [ref.spans_of_entries(host, chunks[b].tolist(), neighbors) for b in range(B)]
        got = dev.chunk_spans(chunks, neighbors)
        assert got[0].shape == (B, n_in * (1 + len(neighbors or ()))) and got[2].dtype == np.float64
        for b in range(B):
            _same(_unpack(got, b), want[b])
        got_dev = dev.chunk_spans(torch.as_tensor(chunks, device="cuda"), neighbors)
        assert all(t.is_cuda for t in got_dev)
        for g, d in zip(got, (t.cpu().numpy() for t in got_dev)):
            assert g.dtype == d.dtype and np.array_equal(_bits(g), _bits(d)) if g.dtype == np.float64 else np.array_equal(g, d)
    if B == 1:
        assert any(len(s[0]) > 1 for s in want[0])  # the last case merged something


def test_the_tie_and_the_last_bit(torch_cuda):
    for t, ids, _ in (tie_case(), last_bit_case()):
        keys = sorted(t.pos)
        dev, host = _device_table([t.pos[k] for k in keys])
        try:
            chunks = np.array([[keys.index(i) for i in ids]], np.int32)
            got = _unpack(dev.chunk_spans(chunks, None), 0)
            want = ref.spans_of_ids(t, ids, None)
            _same([([keys[o] for o in s[0]], s[1]) for s in got], want)
        finally:
            dev.close()
    _, _, want = tie_case()
    assert [s[0] for s in want[1:3]] == [["a/0", "a/1"], ["b/0"]] and want[1][2] == want[2][2] == 0.5
    assert got[0][1] == last_bit_case()[2]


# ---- shared corpus ----------------------------------------------------------------------------------------------------------------
WORDS = ["gpu", "kernel", "memory", "bandwidth", "search", "vector", "keyword", "ranking", "fusion", "chunk", "document", "index",
         "query", "rerank", "embedding", "latency", "throughput", "cache", "tile", "wave", "matrix", "score", "token"]
DIM = 128


def _ints(rng, shape):
    return rng.integers(-3, 4, size=shape).astype(np.float32)


def _bodies(rng, n):
    return [" ".join(rng.choice(WORDS, size=int(rng.integers(3, 25)))) for _ in range(n)]


def _queries(rng, n):
    qs = [" ".join(rng.choice(WORDS, size=int(rng.integers(1, 5)))) + f" q{i}" for i in range(n)]
    qs[-1] = "zebra unicorn"  # no known stem: an empty keyword list
    return qs


def _index(rng, n=3000, dim=DIM, storage="f32"):
    mats = [_ints(rng, (int(rng.integers(1, 4)), dim)) for _ in range(n)]
    ids = [f"chunk-{i:06d}" for i in range(n)]
    return raglite_amd.GpuIndex(ids, mats, metric="dot", storage=storage, docs=[f"text of chunk {i}" for i in range(n)],
                                metadata=[{"topic": [f"t{i % 3}"]} for i in range(n)], keyword_texts=_bodies(rng, n),
                                positions=_layout(rng, n, max_doc=12))


@pytest.fixture(scope="module")
def corpus(torch_cuda):
    rng = np.random.default_rng(2025)
    gi = _index(rng)
    gi.delete_chunks([f"chunk-{i:06d}" for i in range(0, 3000, 7)])  # tombstones
    yield gi
    gi.close()


# ---- 2. DeviceIndex.search_rerank_spans against search_rerank -> chunk_spans -------------------------------------------------------
def _check_pipeline(gi, Q, V, terms, keyword, k, neighbors=(-1, 1), n_each=12, num_hits=40, device=False, **filters):
    kw = {"keyword": gi.keyword if keyword else None, "query_term_ids": terms if keyword else None}
    n_cand = min(16, (2 if keyword else 1) * n_each)
    k = min(k, n_cand)
    _, top, counts = gi.index.search_rerank(Q, num_hits, n_each, n_cand, V, k, **kw, **filters)
    want = (top, counts) + tuple(gi.spans.chunk_spans(top, neighbors))
    if device:
        Q, V = torch.as_tensor(Q, device="cuda"), torch.as_tensor(V, device="cuda")
    got = gi.index.search_rerank_spans(Q, num_hits, n_each, n_cand, V, k, gi.spans, neighbors, **kw, **filters)
    if device:
        assert all(t.is_cuda for t in got)
        got = tuple(t.cpu().numpy() for t in got)
    assert len(got) == len(want) == 7
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        assert np.array_equal(_bits(g), _bits(w)) if g.dtype == np.float64 else np.array_equal(g, w)
    return got


@pytest.mark.parametrize("nq", [1, 4, 32])
@pytest.mark.parametrize("B", [1, 16, 130])
def test_search_rerank_spans_equal_the_composition(corpus, B, nq):
    gi = corpus
    rng = np.random.default_rng(100 * B + nq)
    Q, V = _ints(rng, (B, DIM)), _ints(rng, (B, nq, DIM))
    terms = [gi.keyword_query_ids(q) for q in _queries(rng, B)]
    n_chunks = len(gi.chunk_ids)
    for keyword in (True, False):
        got = _check_pipeline(gi, Q, V, terms, keyword, 16)
        assert (got[1] > 0).all() and (got[5] > 0).all() and (got[6] >= got[1]).all()
        _check_pipeline(gi, Q, V, terms, keyword, 5, neighbors=None, device=True)
        # per-query filters: none, two masks, one that matches nothing
        masks = [None, np.arange(n_chunks) % 3 == 1, np.arange(n_chunks) % 5 != 0, np.zeros(n_chunks, bool)]
        qf = [masks[(b + 1) % 4] for b in range(B)]
        got = _check_pipeline(gi, Q, V, terms, keyword, 8, neighbors=(-2, -1, 1, 2), query_filters=qf)
        assert all(got[1][b] == 0 and got[5][b] == 0 and got[6][b] == 0 for b in range(B) if (b + 1) % 4 == 3)
        _check_pipeline(gi, Q, V, terms, keyword, 8, query_filters=qf, device=True)
    dead = set(range(0, 3000, 7))
    assert not dead.intersection(got[2][got[2] >= 0].tolist())  # no tombstoned chunk is a neighbour


@pytest.mark.parametrize("keyword", [True, False])
def test_search_rerank_spans_at_odd_sizes_equal_the_composition(corpus, keyword):
    """This call takes no MaxSim scores back, so the scores of the first k stay in the index's scratch (csrc/scratch_layout.h: RerankScratch
    with own_scores) -- at odd sizes: B = 3, nq = 3, n_each = 5, k = 3; n_cand = 5 from the vector search alone, 10 with the keyword list."""
    rng = np.random.default_rng(78)
    B, nq = 3, 3
    Q, V = _ints(rng, (B, DIM)), _ints(rng, (B, nq, DIM))
    terms = [corpus.keyword_query_ids(q) for q in _queries(rng, B)]
    got = _check_pipeline(corpus, Q, V, terms, keyword, 3, n_each=5, num_hits=20)
    assert (got[1] == 3).all()
    _check_pipeline(corpus, Q, V, terms, keyword, 3, n_each=5, num_hits=20, device=True)


def test_search_rerank_spans_on_an_fp16_stored_index_of_dim_1024(torch_cuda):
    rng = np.random.default_rng(3)
    gi = _index(rng, n=400, dim=1024, storage="f16")
    try:
        B, nq = 16, 32
        Q, V = _ints(rng, (B, 1024)), _ints(rng, (B, nq, 1024))
        terms = [gi.keyword_query_ids(q) for q in _queries(rng, B)]
        _check_pipeline(gi, Q, V, terms, True, 16)
        _check_pipeline(gi, Q, V, terms, False, 4, device=True)
        with pytest.raises(ValueError, match="span table covers another"):
            small, _ = _device_table([("d", 0)])
            gi.index.search_rerank_spans(Q, 40, 12, 16, V, 4, small)
        with pytest.raises(ValueError, match="4096"):
            gi.index.search_rerank_spans(Q, 40, 2048, 4096, V, 1366, gi.spans)
    finally:
        gi.close()


# ---- 3. the public functions ----------------------------------------------------------------------------------------------------
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


class _Chunk:
    def __init__(self, cid, text):
        self.id, self.text = cid, text

    def __str__(self):
        return self.text


def _by_id(gi):
    return ref.Table({cid: gi.positions[o] for cid, o in gi._id_to_ordinal.items() if gi.positions[o] is not None})  # noqa: SLF001


def _as_spans(want):
    return [_search.ChunkSpan(keys, doc, score) for keys, doc, score in want]


def _same_as_loop(gi, cfg, queries, search, filters=None, neighbors=(-1, 1), **kw):
    fn = raglite_amd.hybrid_search if search == "hybrid" else raglite_amd.vector_search
    per_query = filters if isinstance(filters, list) else [filters] * len(queries)
    got = raglite_amd.search_and_rerank_chunk_spans_batch(queries, search=search, config=cfg, index=gi, metadata_filter=filters,
                                                          neighbors=neighbors, **kw)
    loop = [raglite_amd.search_and_rerank_chunk_spans(q, search=fn, config=cfg, metadata_filter=f, neighbors=neighbors, **kw)
            for q, f in zip(queries, per_query)]
    assert got == loop, (search, filters, kw)  # (dataclass equality: the ids, the document and the float score)
    table = _by_id(gi)
    lookup = lambda ids: [_Chunk(c, gi.docs[gi.ordinal_of(c)]) for c in ids]  # noqa: E731
    for q, f, g in zip(queries, per_query, got):
        chunks = raglite_amd.search_and_rerank_chunks(q, search=fn, config=cfg, metadata_filter=f, chunk_lookup=lookup, **kw)
        assert g == _as_spans(ref.spans_of_chunks(table, [c.id for c in chunks], neighbors))
    assert got == raglite_amd.search_and_rerank_chunk_spans_batch(queries, search=fn, config=cfg, index=gi, metadata_filter=filters,
                                                                  neighbors=neighbors, **kw)
    return got


@pytest.mark.parametrize("search", ["hybrid", "vector"])
@pytest.mark.parametrize("B", [1, 16, 257])
def test_batch_equals_the_loop_and_the_restatement(corpus, pipeline, B, search):
    gi, cfg = corpus, pipeline
    queries = _queries(np.random.default_rng(B), B)
    got = _same_as_loop(gi, cfg, queries, search)  # num_results 8, oversample 4
    assert all(8 <= sum(len(s.chunk_ids) for s in spans) <= 24 and spans[0].score >= spans[-1].score for spans in got)
    assert any(len(s.chunk_ids) > 1 for spans in got for s in spans)
    if B == 257:
        return
    per_query = [[None, {"topic": "t1"}, {"topic": "none"}, {"topic": ["t2"]}][b % 4] for b in range(B)]
    out = _same_as_loop(gi, cfg, queries, search, filters=per_query, neighbors=(1,))
    assert all(out[b] == [] for b in range(B) if b % 4 == 2)
    _same_as_loop(gi, cfg, queries, search, neighbors=None, num_results=3, oversample=2)
    # no reranker: the search order
    plain = raglite_amd.HotPathConfig(vector_search_query_adapter=False)
    assert _same_as_loop(gi, plain, queries, search) != got or B == 1
    with pytest.raises(ValueError, match="4096"):
        raglite_amd.search_and_rerank_chunk_spans_batch(queries, search=search, config=cfg, index=gi, neighbors=tuple(range(64)),
                                                        num_results=64, oversample=1)


def test_another_reranker_runs_per_query(corpus, pipeline):
    class Reversed:  # any other reranker: outside the device path
        def rank(self, query, docs):
            return _search.RankedResults([_search.Result(doc_id=i, score=0.0, rank=0) for i in reversed(range(len(docs)))], query)

    cfg = raglite_amd.HotPathConfig(vector_search_query_adapter=False, reranker=Reversed())
    _same_as_loop(corpus, cfg, _queries(np.random.default_rng(1), 5), "hybrid")


def test_retrieve_chunk_spans_and_its_batch(corpus):
    gi = corpus
    table = _by_id(gi)
    rng = np.random.default_rng(5)
    live = sorted(table.pos)
    lists = [[live[i] for i in rng.integers(0, len(live), int(rng.integers(1, 30)))] for _ in range(9)]  # ragged, with duplicates
    lists[2] = []
    lists[3] = ["unknown", lists[3][0], "chunk-000000", lists[3][0]]  # an unknown id, a deleted chunk's id, a repeat
    for neighbors in ((-1, 1), None, (0, 3)):
        want = [_as_spans(ref.spans_of_ids(table, ids, neighbors)) for ids in lists]
        assert raglite_amd.retrieve_chunk_spans_batch(lists, neighbors=neighbors, index=gi) == want
        assert [raglite_amd.retrieve_chunk_spans(ids, neighbors=neighbors, index=gi) for ids in lists] == want
    # chunk objects are taken as they come: the last place's score stands
    objects = [_Chunk(c, "") for c in lists[0] + lists[0][:1]]
    assert raglite_amd.retrieve_chunk_spans(objects, index=gi) == _as_spans(ref.spans_of_chunks(table, [c.id for c in objects]))
    assert all(s.document_id == table.pos[s.chunk_ids[0]][0] for spans in want for s in spans)


def _rows(rng, n, dim=16):
    return [_ints(rng, (1, dim)) for _ in range(n)]


def test_the_table_follows_the_index(torch_cuda):
    rng = np.random.default_rng(11)
    ids = [f"c{i}" for i in range(12)]
    gi = raglite_amd.GpuIndex(ids, _rows(rng, 12), metric="dot", positions=[("doc9", i) for i in range(6)] + [("doc10", i) for i in range(6)])
    try:
        def check(asked):
            assert raglite_amd.retrieve_chunk_spans(asked, index=gi) == _as_spans(ref.spans_of_ids(_by_id(gi), asked))

        check(["c2", "c8"])
        assert [s.chunk_ids for s in raglite_amd.retrieve_chunk_spans(["c2", "c8"], index=gi)] == [["c1", "c2", "c3"], ["c7", "c8", "c9"]]
        gi.delete_chunks(["c3", "c7"])  # a deleted chunk is no neighbour any more, and asking for it gives nothing
        assert [s.chunk_ids for s in raglite_amd.retrieve_chunk_spans(["c2", "c8", "c3"], index=gi)] == [["c1", "c2"], ["c8", "c9"]]
        check(["c2", "c8", "c3"])
        gi.insert_chunks(["n0", "n1"], _rows(rng, 2), positions=[("doc9", 3), ("doc10", 6)])  # the freed position, and a new last one
        assert [s.chunk_ids for s in raglite_amd.retrieve_chunk_spans(["c2", "c11"], index=gi)] == [["c1", "c2", "n0"], ["c10", "c11", "n1"]]
        gi.compact()  # the ordinals change, the answers do not
        assert gi.spans.info()[:2] == (12, 12)
        assert [s.chunk_ids for s in raglite_amd.retrieve_chunk_spans(["c2", "c11"], index=gi)] == [["c1", "c2", "n0"], ["c10", "c11", "n1"]]
        check(["n1", "c0", "c4", "n0"])
        with pytest.raises(ValueError, match="two live chunks"):
            gi.insert_chunks(["n2"], _rows(rng, 1), positions=[("doc9", 3)])
        check(["n1", "c0", "c4", "n0"])
    finally:
        gi.close()


def test_the_table_follows_the_store(torch_cuda):
    rng = np.random.default_rng(12)
    engine = store_fixture.create_store()
    docs = store_fixture.synthetic_documents(rng, 4, 16)
    for doc_id, chunks in docs[:3]:
        store_fixture.insert_document(engine, doc_id, chunks)
    gi = raglite_amd.GpuIndex.from_store(engine, metric="dot")
    try:
        def expect(chunks, i):
            return [cid for cid, *_ in chunks[max(0, i - 1) : i + 2]]

        doc_id, chunks = docs[1]
        mid = len(chunks) // 2
        spans = raglite_amd.retrieve_chunk_spans([chunks[mid][0]], index=gi)
        assert [s.chunk_ids for s in spans] == [expect(chunks, mid)] and spans[0].document_id == doc_id
        store_fixture.insert_document(engine, *docs[3])
        store_fixture.delete_document(engine, docs[0][0])
        gi.sync()
        doc_id, chunks = docs[3]
        last = len(chunks) - 1
        spans = raglite_amd.retrieve_chunk_spans([chunks[last][0], docs[0][1][0][0]], index=gi)
        assert [s.chunk_ids for s in spans] == [expect(chunks, last)] and spans[0].document_id == doc_id
    finally:
        gi.close()


# ---- 4. retrieve_context -----------------------------------------------------------------------------------------------------------
def test_retrieve_context_accepts_what_the_reference_accepts(corpus, pipeline):
    gi, cfg = corpus, pipeline
    query = _queries(np.random.default_rng(4), 2)[0]
    table = _by_id(gi)

    def config(method):
        return raglite_amd.HotPathConfig(vector_search_query_adapter=False, reranker=cfg.reranker, search_method=method)

    # an (ids, scores) tuple: a BasicSearchMethod
    ids, _ = raglite_amd.vector_search(query, num_results=10, config=cfg)
    got = raglite_amd.retrieve_context(query, config=config(raglite_amd.GpuVectorSearch(gi)))
    assert len(ids) == 10 and got == _as_spans(ref.spans_of_ids(table, ids))
    # a list of chunk ids, and a list of chunk objects
    got = raglite_amd.retrieve_context(query, num_chunks=5, config=config(lambda q, *, num_results, **kw: ids[:num_results]))
    assert got == _as_spans(ref.spans_of_ids(table, ids[:5]))
    objects = [_Chunk(c, "") for c in ids[:4] + ids[:1]]
    got = raglite_amd.retrieve_context(query, config=config(lambda q, **kw: objects))
    assert got == _as_spans(ref.spans_of_chunks(table, [c.id for c in objects]))
    # a list of spans is returned as it is: search_and_rerank_chunk_spans as the search method
    def spans_method(q, *, num_results, metadata_filter=None, config=None):
        return raglite_amd.search_and_rerank_chunk_spans(q, num_results=num_results, metadata_filter=metadata_filter, config=cfg)

    got = raglite_amd.retrieve_context(query, num_chunks=8, config=config(spans_method))
    assert got == raglite_amd.search_and_rerank_chunk_spans_batch([query], config=cfg, index=gi)[0] and got
    assert raglite_amd.retrieve_context(query, config=config(lambda q, **kw: ([], []))) == []
