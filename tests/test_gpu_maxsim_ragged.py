"""The ragged MaxSim rerank on the device: `maxsim_ragged_kernel` and the backstop behind `rl_maxsim_rerank_ragged`
against the contract -- a query's scores are, bit for bit, the float32 sum in slab order of `maxsim_rerank` over its slabs of 32 vectors
alone -- and against float64; the two pipeline entries against the composition of the existing calls; the public batched functions
against the loop of the single-query ones.

Rows and token vectors are standard normal floats: every product is inexact and a sum's bits depend on its order, which integer data
could not show.  An fp16-stored index exists only at a multiple of 128 (`rl_index_create_f16`), so the dims below 128 and 272 run over
fp32 rows alone, and <false, 128> (a partial last k block) has no fp16 instantiation.  Each case's worst |kernel - float64| / bound
goes to profiles/maxsim_ragged_error.txt."""

import time
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch

import raglite_amd
from raglite_amd import _ops, _ragged, _search
from tests import maxsim_ref as mref
from tests import rerank_ref as ref

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 5, 8, 13, 15, 16, 17, 31, 32, 33, 40, 0]  # rows per chunk, cycled: the tile edges, two and three tiles, an empty chunk
SHORT = [1, 5, 16, 17, 31, 32]
U = 2.0 ** -24


def host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def _offsets(n_chunks):
    return np.concatenate(([0], np.cumsum([SIZES[c % len(SIZES)] for c in range(n_chunks)]))).astype(np.int64)


def _halves(rng, shape):
    """Standard normal values that are fp16 numbers: the same corpus under either storage."""
    return rng.standard_normal(shape).astype(np.float16)


def _index(rng, dim, storage, n_chunks=140, dead=(3, 50)):
    off = _offsets(n_chunks)
    rows = _halves(rng, (int(off[-1]), dim))
    idx = raglite_amd.DeviceIndex(rows if storage == "f16" else rows.astype(np.float32), off, metric="dot", storage=storage)
    if dead:
        idx.delete_chunks(list(dead))
    return idx, rows.astype(np.float32), off


def _vecs(rng, lengths, dim):
    return [rng.standard_normal((n, dim)).astype(np.float32) for n in lengths]


def _cands(rng, B, n_cand, n_chunks, pad=0.15):
    c = rng.integers(0, n_chunks, size=(B, n_cand)).astype(np.int32)
    c[rng.random((B, n_cand)) < pad] = -1  # padding anywhere in a list
    return c


def _slab_sum(idx, v, cand_row):
    """The contract's right-hand side for one query: float32 addition, left to right, of `maxsim_rerank` over the slabs of 32."""
    total = None
    for v0 in range(0, len(v), 32):
        s = np.asarray(host(idx.maxsim_rerank(np.ascontiguousarray(v[None, v0:v0 + 32]), cand_row[None])))[0].astype(np.float32)
        total = s if total is None else (total + s).astype(np.float32)
    return total


def _assert_contract(idx, vecs, cand, got=None):
    got = host(_ragged.maxsim_rerank_ragged(idx, vecs, cand)) if got is None else got
    assert got.dtype == np.float32 and got.shape == cand.shape
    for b, v in enumerate(vecs):
        want = _slab_sum(idx, v, cand[b])
        assert np.array_equal(ref.bits(got[b]), ref.bits(want)), (b, len(v), np.flatnonzero(ref.bits(got[b]) != ref.bits(want))[:5])
    return got


# ---- 1. short queries equal the single call -------------------------------------------------------------------------------------------
KERNEL_SHAPES = [(16, "f32"), (48, "f32"), (272, "f32"), (256, "f32"), (1024, "f32"), (256, "f16"), (384, "f16"), (1024, "f16")]


@pytest.mark.parametrize(("dim", "storage"), KERNEL_SHAPES)
def test_short_queries_equal_the_single_call(torch_cuda, dim, storage):
    rng = np.random.default_rng(dim + (7 if storage == "f16" else 0))
    idx, _, off = _index(rng, dim, storage)
    try:
        n_chunks = len(off) - 1
        lengths = [SHORT[i % 6] for i in rng.permutation(13)]
        assert len(set(lengths)) == 6
        vecs = _vecs(rng, lengths, dim)
        for n_cand in (1, 7, 70):
            cand = _cands(rng, 13, n_cand, n_chunks)
            if n_cand > 1:
                cand[0, :2] = (3, 50)  # tombstoned chunks
                cand[1, 0] = 13        # an empty chunk
            got = _assert_contract(idx, vecs, cand)
            dead = (cand < 0) | np.isin(cand, (3, 50)) | (np.diff(off)[np.maximum(cand, 0)] == 0)
            assert np.array_equal(np.isneginf(got), dead) and not np.isnan(got).any()
        # device pointers: ordinals outside [0, n_chunks) are not validated on the host and score -inf
        cand = _cands(rng, 13, 9, n_chunks, pad=0.0)
        cand[:, 2], cand[:, 5], cand[4, 0] = n_chunks, -7, 2 ** 31 - 1
        dv = [torch.as_tensor(v, device="cuda") for v in vecs]
        out = _ragged.maxsim_rerank_ragged(idx, dv, torch.as_tensor(cand, device="cuda"))
        assert out.is_cuda and out.dtype == torch.float32
        got = out.cpu().numpy()
        assert np.isneginf(got[:, [2, 5]]).all() and np.isneginf(got[4, 0])
        safe = np.where((cand >= 0) & (cand < n_chunks), cand, -1).astype(np.int32)
        _assert_contract(idx, vecs, safe, got)
    finally:
        idx.close()


def test_a_wave_passes_its_lookup_of_64_candidates_twice(torch_cuda):
    """n_cand = 600 in one slice: 260 queries leave one workgroup per query (512 / 260), whose eight waves take 75 candidates each."""
    rng = np.random.default_rng(600)
    idx, _, off = _index(rng, 16, "f32", n_chunks=700)
    try:
        B = 260
        vecs = _vecs(rng, [SHORT[b % 6] if b % 9 else 40 for b in range(B)], 16)
        cand = _cands(rng, B, 600, len(off) - 1)
        got = host(_ragged.maxsim_rerank_ragged(idx, vecs, cand))
        for b in list(range(0, B, 13)) + [B - 1]:
            assert np.array_equal(ref.bits(got[b]), ref.bits(_slab_sum(idx, vecs[b], cand[b]))), b
        # no query's bits depend on the others of the call
        alone = host(_ragged.maxsim_rerank_ragged(idx, vecs[5:6], cand[5:6]))
        assert np.array_equal(ref.bits(alone[0]), ref.bits(got[5]))
    finally:
        idx.close()


# ---- 2. long queries equal the slab sum; fp16 storage of the same halves gives the fp32-stored bits ----------------------------------
@pytest.mark.parametrize("dim", [256, 384, 1024])
def test_long_queries_equal_the_slab_sum_on_both_storages(torch_cuda, dim):
    rng = np.random.default_rng(dim)
    off = _offsets(140)
    rows = _halves(rng, (int(off[-1]), dim))
    lengths = [33, 5, 64, 65, 32, 100, 1]
    vecs = _vecs(rng, lengths, dim)
    cand = _cands(rng, len(lengths), 70, 140)
    i32 = raglite_amd.DeviceIndex(rows.astype(np.float32), off, metric="dot")
    i16 = raglite_amd.DeviceIndex(rows, off, metric="dot", storage="f16")
    try:
        got32 = _assert_contract(i32, vecs, cand)
        got16 = host(_ragged.maxsim_rerank_ragged(i16, vecs, cand))
        assert np.array_equal(ref.bits(got16), ref.bits(got32))  # the stored halves ARE the corpus
        short = [b for b, n in enumerate(lengths) if n <= 32]
        _assert_contract(i16, [vecs[b] for b in short], cand[short])  # ... where the single call takes them on fp16 rows
        with pytest.raises(ValueError, match="nq <= 32"):
            i16.maxsim_rerank(vecs[0][None], cand[:1])
    finally:
        i32.close()
        i16.close()


@pytest.mark.parametrize("dim", [16, 48, 272])
def test_long_queries_equal_the_slab_sum_at_partial_k_blocks(torch_cuda, dim):
    rng = np.random.default_rng(dim)
    idx, _, off = _index(rng, dim, "f32")
    try:
        vecs = _vecs(rng, [33, 5, 64, 65, 32, 100, 1], dim)
        _assert_contract(idx, vecs, _cands(rng, 7, 70, len(off) - 1))
    finally:
        idx.close()


# ---- 3. float64: the pairs kernel's bound per slab, the slabs' additions on top ------------------------------------------------------------
@pytest.fixture(scope="module")
def error_log():
    lines, t0 = [], time.time()
    yield lines
    try:  # (a read-only checkout keeps the committed figures)
        out = Path(__file__).resolve().parent.parent / "profiles" / "maxsim_ragged_error.txt"
        head = ("# tests/test_gpu_maxsim_ragged.py: the worst |rl_maxsim_rerank_ragged - float64| / bound over a case's scores; every figure is asserted\n"
                "# <= 1.  Per slab of 32 vectors the bound of the pairs kernel (tests/maxsim_ref.py: scores_bound, kernel 'pairs'); a longer query: the\n"
                "# sum of its slabs' bounds plus 2^-24 * sum |partial sums| for its (slabs - 1) float32 additions.  dim | storage | lengths | ratio\n")
        out.write_text(head + "".join(sorted(lines)) + f"# wall time of the module: {time.time() - t0:.0f} s\n")
    except OSError:
        pass


def _float64_bound(rows, off, v):
    """(float64 chunk scores, bound) of one query: the slabs' bounds added up, and per float32 addition of a slab's sum 2^-24 times the
    magnitude of the exact sum of its operands, which is at most |float64 partial sum| + the error bound so far (the recursion of
    tests/maxsim_ref.py: stream_scores_bound)."""
    total = bound = None
    for v0 in range(0, len(v), 32):
        sc, bd = mref.scores_bound(rows, off, v[v0:v0 + 32], 1.0, "pairs", "fp32_exact")
        if total is None:
            total, bound = sc, bd
        else:
            total = total + sc
            with np.errstate(invalid="ignore"):
                bound = bound + bd
                bound = np.where(np.isfinite(total), bound + U * (np.abs(total) + bound), 0.0)
    return total, bound


@pytest.mark.parametrize(("dim", "storage"), [(48, "f32"), (256, "f32"), (1024, "f16")])
def test_scores_are_within_the_float64_bound(torch_cuda, error_log, dim, storage):
    rng = np.random.default_rng(1000 + dim)
    idx, rows, off = _index(rng, dim, storage, dead=())
    try:
        lengths = [1, 17, 32, 33, 64, 100]
        vecs = _vecs(rng, lengths, dim)
        cand = _cands(rng, len(lengths), 70, len(off) - 1)
        got = host(_ragged.maxsim_rerank_ragged(idx, vecs, cand)).astype(np.float64)
        worst = 0.0
        for b, v in enumerate(vecs):
            sc, bd = _float64_bound(rows, off, v)
            want, bound = mref.take(sc, cand[b]), mref.take(bd, cand[b])
            fin = np.isfinite(want)
            assert np.array_equal(np.isneginf(got[b]), ~fin)
            ratio = float(np.max(np.abs(got[b][fin] - want[fin]) / bound[fin]))
            worst = max(worst, ratio)
        line = f"{dim} | {storage} | {lengths} | {worst:.4f}\n"
        print(line, end="")
        error_log.append(line)
        assert worst <= 1.0, line
    finally:
        idx.close()


# ---- 4. the backstop keeps the contract -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["f32", "f16"])
@pytest.mark.parametrize("dim", [128, 1536])
def test_backstop_shapes_keep_the_contract(torch_cuda, dim, storage):
    rng = np.random.default_rng(dim)
    idx, _, off = _index(rng, dim, storage, n_chunks=60)
    try:
        vecs = _vecs(rng, [8, 40], dim)
        _assert_contract(idx, vecs, _cands(rng, 2, 20, len(off) - 1))
    finally:
        idx.close()


def test_backstop_takes_any_dim_of_an_fp32_stored_index(torch_cuda):
    rng = np.random.default_rng(100)
    idx, _, off = _index(rng, 100, "f32", n_chunks=60)  # dim % 16 != 0: the VALU kernel behind `maxsim_rerank`
    try:
        _assert_contract(idx, _vecs(rng, [8, 40], 100), _cands(rng, 2, 20, len(off) - 1))
    finally:
        idx.close()


# ---- 5. the pipeline entries against the composition -----------------------------------------------------------------------------------
WORDS = ["gpu", "kernel", "memory", "bandwidth", "search", "vector", "keyword", "ranking", "fusion", "chunk", "document", "index",
         "query", "rerank", "embedding", "latency", "throughput", "cache", "tile", "wave", "matrix", "score", "token"]
DIM = 64
N = 2000
LENGTHS = [3, 7, 12, 20, 32, 40]  # six distinct query lengths, one beyond a slab
PUBLIC_LENGTHS = [3, 7, 12, 20, 27, 32]  # six within a slab: over fp32 rows a longer query keeps its per-length call


def _ints(rng, shape):
    return rng.integers(-3, 4, size=shape).astype(np.float32)


def _gpu_index(rng, make, n=N, dim=DIM, storage="f32"):
    mats = [make(rng, (int(rng.integers(1, 4)), dim)) for _ in range(n)]
    bodies = [" ".join(rng.choice(WORDS, size=int(rng.integers(3, 25)))) for _ in range(n)]
    return raglite_amd.GpuIndex([f"chunk-{i:06d}" for i in range(n)], mats, metric="dot", storage=storage,
                                docs=[f"text of chunk {i}" for i in range(n)], metadata=[{"topic": [f"t{i % 3}"]} for i in range(n)],
                                keyword_texts=bodies, positions=[(f"doc-{i // 10:04d}", i % 10) for i in range(n)])


def _texts(rng, n):
    qs = [" ".join(rng.choice(WORDS, size=int(rng.integers(1, 5)))) + f" q{i}" for i in range(n)]
    qs[-1] = "zebra unicorn"  # no known stem: an empty keyword list
    return qs


@pytest.fixture(scope="module")
def float_corpus(torch_cuda):
    gi = _gpu_index(np.random.default_rng(11), lambda rng, shape: rng.standard_normal(shape).astype(np.float32))
    gi.delete_chunks([f"chunk-{i:06d}" for i in range(0, N, 7)])
    yield gi
    gi.close()


def _check_pipeline(gi, Q, vecs, terms, keyword, k, device=False, spans=False, **filters):
    kw = {"keyword": gi.keyword if keyword else None, "query_term_ids": terms if keyword else None}
    n_each, num_hits = 12, 40
    n_cand = min(16, (2 if keyword else 1) * n_each)
    _, fused, _ = gi.index.hybrid_search(Q, num_hits, n_each, n_cand, **kw, **filters)
    scores = _ragged.maxsim_rerank_ragged(gi.index, vecs, fused)
    ws, wc, _, wn = ref.order(scores, fused, k)
    if device:
        Q, vecs = torch.as_tensor(Q, device="cuda"), [torch.as_tensor(v, device="cuda") for v in vecs]
    if spans:
        table = gi.span_table()
        res = [host(x) for x in _ragged.search_rerank_spans_ragged(gi.index, Q, num_hits, n_each, n_cand, vecs, k, table, (-1, 1), **kw, **filters)]
        assert np.array_equal(res[0], wc) and np.array_equal(res[1], wn)
        for g, w in zip(res[2:], table.chunk_spans(wc, (-1, 1))):
            assert np.array_equal(g, w)
        return
    s, c, n = (host(x) for x in _ragged.search_rerank_ragged(gi.index, Q, num_hits, n_each, n_cand, vecs, k, **kw, **filters))
    assert np.array_equal(c, wc) and np.array_equal(n, wn)
    assert np.array_equal(ref.bits(s), ref.bits(ws))
    return c, n, fused


@pytest.mark.parametrize("B", [1, 16, 130])
def test_search_rerank_ragged_equals_the_composition(float_corpus, B):
    gi = float_corpus
    rng = np.random.default_rng(B)
    Q = rng.standard_normal((B, DIM)).astype(np.float32)
    vecs = _vecs(rng, [LENGTHS[b % 6] for b in range(B)], DIM)
    terms = [gi.keyword_query_ids(q) for q in _texts(rng, B)]
    n_chunks = len(gi.chunk_ids)
    reordered = False
    for keyword in (True, False):
        c, n, fused = _check_pipeline(gi, Q, vecs, terms, keyword, 16 if keyword else 12)
        assert (n > 0).all()
        reordered = reordered or any(c[b, : n[b]].tolist() != fused[b, : n[b]].tolist() for b in range(B))
        _check_pipeline(gi, Q, vecs, terms, keyword, 5, device=True)
        masks = [None, np.arange(n_chunks) % 3 == 1, np.arange(n_chunks) % 5 != 0, np.zeros(n_chunks, bool)]  # one matches nothing
        qf = [masks[(b + 1) % 4] for b in range(B)]
        c, n, _ = _check_pipeline(gi, Q, vecs, terms, keyword, 8, query_filters=qf)
        assert all(n[b] == 0 for b in range(B) if (b + 1) % 4 == 3)
        _check_pipeline(gi, Q, vecs, terms, keyword, 8, query_filters=qf, device=True)
        _check_pipeline(gi, Q, vecs, terms, keyword, 4, spans=True)
        _check_pipeline(gi, Q, vecs, terms, keyword, 4, spans=True, query_filters=qf, device=True)
    assert reordered  # the rerank changed some query's order: the comparison shows something
    assert not set(range(0, N, 7)).intersection(c[c >= 0].tolist())  # no tombstoned chunk comes back


# ---- 6. the public batched functions: one pipeline call for queries of six lengths ------------------------------------------------------------
def _hash_rng(text):
    return np.random.default_rng(zlib.crc32(text.encode()))


def _encode(query):
    """Float token vectors, their number drawn from the query's text: six lengths in a batch."""
    rng = _hash_rng("tokens " + query)
    return rng.standard_normal((PUBLIC_LENGTHS[int(rng.integers(0, 6))], DIM)).astype(np.float32)


@pytest.fixture(scope="module")
def int_corpus(torch_cuda):
    """Integer rows and pooled query vectors: the searches are exact whatever route a batch or a single query takes, so
    batch and loop see the same candidates; the token vectors are floats."""
    gi = _gpu_index(np.random.default_rng(12), _ints)
    yield gi
    gi.close()


@pytest.fixture
def pipeline(int_corpus, monkeypatch):
    monkeypatch.setattr(_search, "embed_strings",
                        lambda strings, config=None: np.stack([_ints(_hash_rng(s), (DIM,)) for s in strings]))
    raglite_amd.attach_index(int_corpus)
    calls = {"ragged": 0, "spans_ragged": 0, "uniform": 0, "spans_uniform": 0}

    def counted(fn, key):
        def wrapper(*a, **kw):
            calls[key] += 1
            return fn(*a, **kw)
        return wrapper

    monkeypatch.setattr(_ragged, "search_rerank_ragged", counted(_ragged.search_rerank_ragged, "ragged"))
    monkeypatch.setattr(_ragged, "search_rerank_spans_ragged", counted(_ragged.search_rerank_spans_ragged, "spans_ragged"))
    monkeypatch.setattr(_ops.DeviceIndex, "search_rerank", counted(_ops.DeviceIndex.search_rerank, "uniform"))
    monkeypatch.setattr(_ops.DeviceIndex, "search_rerank_spans", counted(_ops.DeviceIndex.search_rerank_spans, "spans_uniform"))
    yield raglite_amd.HotPathConfig(vector_search_query_adapter=False, reranker=raglite_amd.MaxSimRanker(int_corpus, _encode)), calls
    raglite_amd.detach_index()


@pytest.mark.parametrize("search", ["hybrid", "vector"])
def test_public_batches_equal_the_loop_in_one_pipeline_call(int_corpus, pipeline, search):
    gi, (cfg, calls) = int_corpus, pipeline
    queries = _texts(np.random.default_rng(40), 40)
    assert {len(_encode(q)) for q in queries} == set(PUBLIC_LENGTHS)
    fn = raglite_amd.hybrid_search if search == "hybrid" else raglite_amd.vector_search
    lookup = lambda ids: [gi.docs[gi.ordinal_of(cid)] for cid in ids]  # noqa: E731
    want = [raglite_amd.search_and_rerank_chunks(q, search=fn, config=cfg, chunk_lookup=lookup) for q in queries]
    want_spans = [raglite_amd.search_and_rerank_chunk_spans(q, search=fn, config=cfg, index=gi) for q in queries]
    before = dict(calls)
    got = raglite_amd.search_and_rerank_chunks_batch(queries, search=search, config=cfg, index=gi, chunk_lookup=lookup)
    assert got == want and all(len(x) == 8 for x in got)
    assert {k: calls[k] - before[k] for k in calls} == {"ragged": 1, "spans_ragged": 0, "uniform": 0, "spans_uniform": 0}
    before = dict(calls)
    got_spans = raglite_amd.search_and_rerank_chunk_spans_batch(queries, search=search, config=cfg, index=gi)
    assert got_spans == want_spans
    assert {k: calls[k] - before[k] for k in calls} == {"ragged": 0, "spans_ragged": 1, "uniform": 0, "spans_uniform": 0}
    # with the route off: the same answers from one call per distinct length
    cfg.reranker.ragged = False
    before = dict(calls)
    assert raglite_amd.search_and_rerank_chunks_batch(queries, search=search, config=cfg, index=gi, chunk_lookup=lookup) == want
    assert {k: calls[k] - before[k] for k in calls} == {"ragged": 0, "spans_ragged": 0, "uniform": 6, "spans_uniform": 0}
    cfg.reranker.ragged = True
    # a batch of one length: today's call, no ragged one
    same = [q for q in queries if len(_encode(q)) == 12]
    before = dict(calls)
    assert raglite_amd.search_and_rerank_chunks_batch(same, search=search, config=cfg, index=gi,
                                                      chunk_lookup=lookup) == [want[queries.index(q)] for q in same]
    assert {k: calls[k] - before[k] for k in calls} == {"ragged": 0, "spans_ragged": 0, "uniform": 1, "spans_uniform": 0}


def test_rank_batch_of_mixed_lengths_equals_rank(int_corpus, pipeline):
    gi, (cfg, _) = int_corpus, pipeline
    ranker = cfg.reranker
    rng = np.random.default_rng(9)
    queries = _texts(rng, 12)
    lists = [rng.choice(N, size=int(rng.integers(1, 40))).tolist() for _ in queries]
    lists[2] = []
    for s, q, ids in zip(ranker.score_batch(queries, lists), queries, lists):
        assert np.array_equal(ref.bits(s), ref.bits(ranker.score(q, ids)) if ids else np.zeros(0, np.uint32))
    docs = [[gi.docs[i] for i in ids] for ids in lists]
    for g, q, d in zip(ranker.rank_batch(queries, docs), queries, docs):
        w = ranker.rank(query=q, docs=d)
        assert [r.doc_id for r in g.results] == [r.doc_id for r in w.results]
        assert np.array_equal(ref.bits([r.score for r in g.results]), ref.bits([r.score for r in w.results]))


# ---- 7. an fp16-stored index and a query of 40 vectors ------------------------------------------------------------------------------------
def test_a_long_query_ranks_on_an_fp16_stored_index(torch_cuda):
    """40 token vectors over an fp16-stored index of dim 1024: `rank` returns the order of a float64 restatement.  The candidates'
    scores are spread by construction: candidate j's rows are the query's mean direction times (1 + j / 8) plus a tenth of unit noise,
    so neighbouring scores differ by about 40 * 6 / 8 * |mean|^2 (hundreds) where the bound is tens: the test asserts the gap."""
    rng = np.random.default_rng(40)
    dim, n = 1024, 24
    V = rng.standard_normal((40, dim)).astype(np.float32)
    mean = V.mean(axis=0)
    mats = [((1.0 + j / 8.0) * 6.0 * mean + 0.1 * rng.standard_normal((1 + j % 3, dim))).astype(np.float16) for j in range(n)]
    gi = raglite_amd.GpuIndex([f"c{j}" for j in range(n)], mats, metric="dot", storage="f16", docs=[f"doc {j}" for j in range(n)])
    try:
        ranker = raglite_amd.MaxSimRanker(gi, lambda q: V)
        order = rng.permutation(n).tolist()
        res = ranker.rank(query="long", docs=[gi.docs[j] for j in order])
        rows = np.concatenate([m.astype(np.float32) for m in mats])
        off = np.concatenate(([0], np.cumsum([len(m) for m in mats]))).astype(np.int64)
        sc, bd = _float64_bound(rows, off, V)
        want = sorted(range(n), key=lambda i: -sc[order[i]])
        gaps = np.diff(np.sort(sc))
        assert gaps.min() > 2.0 * bd.max(), (gaps.min(), bd.max())
        assert [r.doc_id for r in res.results] == want
        got = np.array([r.score for r in sorted(res.results, key=lambda r: r.doc_id)])
        assert np.all(np.abs(got - sc[order]) <= bd[order])
        with pytest.raises(ValueError, match="nq <= 32"):  # the uniform entry keeps its limit
            gi.index.search_rerank(np.zeros((1, dim), np.float32), 8, 4, 4, np.zeros((1, 33, dim), np.float32), 2)
        ranker.ragged = False
        with pytest.raises(ValueError, match="nq <= 32"):
            ranker.rank(query="long", docs=[gi.docs[0]])
    finally:
        gi.close()
