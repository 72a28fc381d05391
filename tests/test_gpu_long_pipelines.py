"""The one-call pipelines at long lists: `hybrid_search`, `search_rerank`, `search_rerank_spans` and the ragged rerank with num_hits up to
2048, n_each up to 2048, n_cand up to 4096 and k up to 4096 -- the sizes at which the lists they carve out of one scratch block
(csrc/scratch_layout.h: HybridLists, RerankScratch, the spans scratch) and hand from stage to stage with their -1 padding are long.

The expected result of every stage is computed on the HOST, with no device call: the vector half by `oracle.search_chunks_filtered` over
exact similarities (integer data), the keyword half by tests/keyword_ref.py over the postings the keyword index holds, the fusion by
tests/rrf_ref.py, the MaxSim scores by `oracle.maxsim_scores` (exact on this data), the order by tests/rerank_ref.py, the spans by
tests/spans_ref.py.  Every score bit, ordinal and count is compared, padded tails included, and each pipeline also against the
composition of the separate device calls, so a mismatch shows whether a stage or the plumbing is at fault."""

from types import SimpleNamespace

import numpy as np
import pytest
import torch

import raglite_amd
from oracle import oracle
from raglite_amd import _ops, _ragged
from tests import keyword_ref, rerank_ref, rrf_ref, spans_ref

pytestmark = pytest.mark.gpu

WORDS = ["gpu", "kernel", "memory", "bandwidth", "search", "vector", "keyword", "ranking", "fusion", "chunk", "document", "index",
         "query", "rerank", "embedding", "latency", "throughput", "cache", "tile", "wave", "matrix", "score", "token"]
DIM, N = 64, 3000
WEIGHTS, RRF_K = (0.75, 0.25), 60
# (num_hits, n_each, n_cand, k); the third with keywords (two lists of 2048), the fourth from the vector list alone
SIZES = [(300, 100, 200, 200), (2048, 700, 1400, 1000), (2048, 2048, 4096, 4096), (2048, 2048, 2048, 2048)]


def _ints(rng, shape):
    return rng.integers(-3, 4, size=shape).astype(np.float32)


def _positions(rng, n):
    """(document, index) per chunk: documents of 1 to 12 chunks with a few gaps, handed out in shuffled ordinal order."""
    positions, d = [], 0
    while len(positions) < n:
        at = int(rng.integers(0, 3))
        for _ in range(min(int(rng.integers(1, 13)), n - len(positions))):
            positions.append((f"doc{d}", at))
            at += 1 if rng.random() < 0.8 else int(rng.integers(2, 5))
        d += 1
    return [positions[i] for i in rng.permutation(n)]


class Corpus:
    """As tests/test_gpu_rerank_batch.py::_index -- 3000 chunks of 1 to 3 rows, integers in [-3, 3], bodies over 23 words, every seventh
    chunk tombstoned -- with positions for the spans, and the host's copy of everything the expected results need."""

    def __init__(self):
        rng = np.random.default_rng(2026)
        mats = [_ints(rng, (int(rng.integers(1, 4)), DIM)) for _ in range(N)]
        bodies = [" ".join(rng.choice(WORDS, size=int(rng.integers(3, 25)))) for _ in range(N)]
        self.gi = raglite_amd.GpuIndex([f"chunk-{i:06d}" for i in range(N)], mats, metric="dot", keyword_texts=bodies, positions=_positions(rng, N))
        self.gi.delete_chunks([f"chunk-{i:06d}" for i in range(0, N, 7)])
        self.E = np.concatenate(mats)
        self.off = np.concatenate(([0], np.cumsum([len(m) for m in mats]))).astype(np.int64)
        self.r2c = np.repeat(np.arange(N), np.diff(self.off))
        self.live = np.arange(N) % 7 != 0
        term_off, post_chunk, post_impact = self.gi.keyword.read()  # what the keyword index holds
        self.postings = SimpleNamespace(n_chunks=N, n_terms=len(term_off) - 1, term_off=term_off, post_chunk=post_chunk)
        self.impacts = post_impact
        self.table = spans_ref.Table({o: p for o, p in enumerate(self.gi.positions) if p is not None})
        assert set(self.table.pos) == set(np.nonzero(self.live)[0].tolist())
        self._lists = {}

    def queries(self, rng, B):
        # six to eight words: each occurs in well over 1000 chunks, together in more than 2048 live ones -- a keyword list of 2048 fills
        texts = [" ".join(rng.choice(WORDS, size=int(rng.integers(6, 9)))) + f" q{i}" for i in range(B)]
        return _ints(rng, (B, DIM)), [self.gi.keyword_query_ids(t) for t in texts]

    # ---- the expected results, host only ----
    def vector_list(self, q, num_hits, n_each, ok):
        _, c = oracle.search_chunks_filtered(self.E, self.r2c, q, num_hits, n_each, self.live if ok is None else ok & self.live, "dot")
        out = np.full(n_each, -1, np.int32)
        out[: len(c)] = c
        return out

    def keyword_list(self, terms, n_each, ok):
        _, c = keyword_ref.topk_f32(keyword_ref.scores_f32(self.postings, self.impacts, terms), n_each, self.live if ok is None else ok & self.live)
        out = np.full(n_each, -1, np.int32)
        out[: len(c)] = c
        return out

    def fused(self, Q, terms, keyword, num_hits, n_each, n_cand, filters):
        B = len(Q)
        lists = [np.stack([self.vector_list(Q[b], num_hits, n_each, filters[b]) for b in range(B)])]
        if keyword:
            lists.append(np.stack([self.keyword_list(terms[b], n_each, filters[b]) for b in range(B)]))
        return lists, rrf_ref.fuse(np.stack(lists), WEIGHTS[: len(lists)], RRF_K, n_cand)

    def maxsim_all(self, vecs):
        """MaxSim score of every chunk for each query's token vectors (float32: exact on integer data)."""
        return [oracle.maxsim_scores(self.E, self.off, v).astype(np.float32) for v in vecs]

    def spans(self, top_row, neighbors):
        return spans_ref.spans_of_entries(self.table, top_row.tolist(), neighbors)


@pytest.fixture(scope="module")
def corpus(torch_cuda):
    c = Corpus()
    yield c
    c.gi.close()


def _bits32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _bits64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _host(out):
    return tuple(t.cpu().numpy() if hasattr(t, "is_cuda") else t for t in out)


def _unpack_spans(out, b):
    chunks, lens, scores, n_spans, n_chunks = out
    ns, nc = int(n_spans[b]), int(n_chunks[b])
    assert (lens[b, :ns] > 0).all() and int(lens[b, :ns].sum()) == nc
    assert (chunks[b, :nc] >= 0).all() and (chunks[b, nc:] == -1).all() and (lens[b, ns:] == 0).all() and (scores[b, ns:] == 0).all()
    at, spans = 0, []
    for length, score in zip(lens[b, :ns].tolist(), scores[b, :ns].tolist()):
        spans.append((chunks[b, at : at + length].tolist(), score))
        at += length
    return spans


def _check(c, Q, terms, vecs, keyword, size, *, query_filters=None, device=False, ragged=False, spans=()):
    """hybrid_search, search_rerank (or its ragged form) and search_rerank_spans at one size against the host's results and against
    the composition of the separate device calls.  vecs: (B, nq, DIM), or a list of (nq_b, DIM) for the ragged call."""
    num_hits, n_each, n_cand, k = size
    if not keyword:
        n_cand = min(n_cand, n_each)
        k = min(k, n_cand)
    B, idx = len(Q), c.gi.index
    filters = query_filters if query_filters is not None else [None] * B
    kw = {"keyword": c.gi.keyword if keyword else None, "query_term_ids": terms if keyword else None}
    if query_filters is not None:
        kw["query_filters"] = query_filters
    where = f"B {B} keyword {keyword} size {size}"
    dev = (lambda x: torch.as_tensor(x, device="cuda")) if device else (lambda x: x)
    Qd = dev(Q)
    Vd = [dev(v) for v in vecs] if ragged else dev(vecs)

    # 1. the hybrid search: both lists and the fusion
    lists, (ws, wc, wn) = c.fused(Q, terms, keyword, num_hits, n_each, n_cand, filters)
    vs, vc, vn = _host(idx.search_chunks(Qd, num_hits, n_each, query_filters=query_filters))
    assert np.array_equal(vc, lists[0]) and np.array_equal(vn, (lists[0] >= 0).sum(axis=1)), f"{where}: the vector list"
    if keyword:
        ks, kc, kn = c.gi.keyword.search(terms, n_each, query_filters=query_filters)
        assert np.array_equal(kc, lists[1]) and np.array_equal(kn, (lists[1] >= 0).sum(axis=1)), f"{where}: the keyword list"
    out = idx.hybrid_search(Qd, num_hits, n_each, n_cand, **kw)
    assert not device or all(t.is_cuda for t in out)
    hs, hc, hn = _host(out)
    assert hs.shape == hc.shape == (B, n_cand) and np.array_equal(hn, wn), f"{where}: fused counts {hn.tolist()} expected {wn.tolist()}"
    assert np.array_equal(hc, wc) and np.array_equal(_bits64(hs), _bits64(ws)), f"{where}: the fused list"

    # 2. the rerank: MaxSim scores of the fused candidates, ordered, the first k
    all_scores = c.maxsim_all(vecs)
    scores = np.stack([np.where(wc[b] >= 0, all_scores[b][np.clip(wc[b], 0, None)], -np.inf) for b in range(B)]).astype(np.float32)
    es, ec, _, en = rerank_ref.order(scores, wc, k)
    if ragged:
        out = _ragged.search_rerank_ragged(idx, Qd, num_hits, n_each, n_cand, Vd, k, **kw)
        ms = _host((_ragged.maxsim_rerank_ragged(idx, Vd, dev(wc)),))[0]
    else:
        out = idx.search_rerank(Qd, num_hits, n_each, n_cand, Vd, k, **kw)
        ms = _host((idx.maxsim_rerank(Vd, dev(wc)),))[0]
    assert not device or all(t.is_cuda for t in out)
    rs, rc, rn = _host(out)
    assert np.array_equal(_bits32(ms)[wc >= 0], _bits32(scores)[wc >= 0]), f"{where}: maxsim_rerank of the fused candidates"
    assert rs.shape == rc.shape == (B, k) and np.array_equal(rn, en), f"{where}: rerank counts {rn.tolist()} expected {en.tolist()}"
    assert np.array_equal(rc, ec) and np.array_equal(_bits32(rs), _bits32(es)), f"{where}: the reranked list"
    os_, oc, _, on = _ops.rerank_order(np.where(wc >= 0, ms, -np.inf).astype(np.float32), wc, k)  # the composition's last step
    assert np.array_equal(oc, rc) and np.array_equal(on, rn) and np.array_equal(_bits32(os_), _bits32(rs)), f"{where}: rerank_order"

    # 3. the spans of the first k_s
    for k_s, neighbors in spans:
        if ragged:
            got = _host(_ragged.search_rerank_spans_ragged(idx, Qd, num_hits, n_each, n_cand, Vd, k_s, c.gi.spans, neighbors, **kw))
        else:
            got = _host(idx.search_rerank_spans(Qd, num_hits, n_each, n_cand, Vd, k_s, c.gi.spans, neighbors, **kw))
        n_off = len(neighbors or ())
        assert np.array_equal(got[0], ec[:, :k_s]) and np.array_equal(got[1], np.minimum(en, k_s)), f"{where}: the first {k_s} of the spans call"
        assert got[2].shape == (B, k_s * (1 + n_off)) and got[4].dtype == np.float64
        for b in range(B):
            have, want = _unpack_spans(got[2:], b), c.spans(ec[b, :k_s], neighbors)
            assert [s[0] for s in have] == [s[0] for s in want], f"{where}: spans of query {b}, k {k_s}"
            assert np.array_equal(_bits64([s[1] for s in have]), _bits64([s[2] for s in want])), f"{where}: span scores of query {b}, k {k_s}"
        comp = c.gi.spans.chunk_spans(got[0], neighbors)  # the composition: the separate spans call over the same first k_s
        for g, w in zip(got[2:], comp):
            assert g.dtype == w.dtype and (np.array_equal(_bits64(g), _bits64(w)) if g.dtype == np.float64 else np.array_equal(g, w))
    return wn, en


BIG_SPANS = ((1365, (-1, 1)), (4096, None))


@pytest.mark.parametrize("nq", [1, 32])
@pytest.mark.parametrize("B", [1, 5])
def test_pipelines_at_long_lists_equal_the_host(corpus, B, nq):
    rng = np.random.default_rng(10 * B + nq)
    Q, terms = corpus.queries(rng, B)
    V = _ints(rng, (B, nq, DIM))
    for size in SIZES[:3]:
        fused_n, top_n = _check(corpus, Q, terms, V, True, size, spans=BIG_SPANS if size == SIZES[2] else ((size[3], (-1, 1)),))
        assert (fused_n > size[1]).all() and (top_n == np.minimum(fused_n, size[3])).all()  # both lists contribute (at 2048: more than 2048)
    for size in (SIZES[0], SIZES[1], SIZES[3]):
        fused_n, top_n = _check(corpus, Q, terms, V, False, size, spans=((min(size[3], size[1], 1365), (-1, 1)),))
        if size == SIZES[3]:  # 2048 hits lie in fewer than 2048 chunks (1 to 3 rows each): a long list with a padded tail
            assert ((fused_n > 1000) & (fused_n < 2048)).all() and np.array_equal(top_n, fused_n)
        else:  # the vector list alone, full
            assert (fused_n == size[1]).all() and (top_n == min(size[3], size[1])).all()


def test_ragged_queries_at_long_lists(corpus):
    rng = np.random.default_rng(77)
    B = 5
    Q, terms = corpus.queries(rng, B)
    vecs = [_ints(rng, (n, DIM)) for n in (1, 32, 5, 17, 2)]
    _check(corpus, Q, terms, vecs, True, SIZES[2], ragged=True, spans=BIG_SPANS)
    _check(corpus, Q, terms, vecs, False, SIZES[3], ragged=True, spans=((1365, (-1, 1)),))
    _check(corpus, Q, terms, vecs, True, SIZES[1], ragged=True, device=True)


def test_per_query_filters_at_long_lists(corpus):
    rng = np.random.default_rng(78)
    B = 5
    Q, terms = corpus.queries(rng, B)
    V = _ints(rng, (B, 32, DIM))
    n = np.arange(N)
    qf = [None, n % 3 == 1, np.zeros(N, bool), n % 5 != 0, n < 400]  # no filter, a third, NOTHING, four fifths, 400 chunks (short lists)
    for keyword, size in ((True, SIZES[2]), (True, SIZES[1]), (False, SIZES[3])):
        fused_n, top_n = _check(corpus, Q, terms, V, keyword, size, query_filters=qf, spans=((1365, (-1, 1)),) if size != SIZES[1] else ())
        assert fused_n[2] == 0 and top_n[2] == 0 and 0 < fused_n[4] <= 400 - 58  # (58 of the first 400 chunks are tombstoned)
    _check(corpus, Q, terms, V, True, SIZES[2], query_filters=qf, device=True)


def test_device_tensors_at_long_lists(corpus):
    rng = np.random.default_rng(79)
    B = 5
    Q, terms = corpus.queries(rng, B)
    V = _ints(rng, (B, 32, DIM))
    _check(corpus, Q, terms, V, True, SIZES[2], device=True, spans=BIG_SPANS)
    _check(corpus, Q, terms, V, False, SIZES[3], device=True, spans=((1365, (-1, 1)),))
    _check(corpus, Q[:1], terms[:1], V[:1], True, SIZES[1], device=True)
