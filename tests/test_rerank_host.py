"""Batched search-and-rerank, without a GPU: the order that rl_rerank_order implements (tests/rerank_ref.py) against
`MaxSimRanker.rank`, the argument checks of rl_rerank_order and rl_search_rerank_per_query that run before any HIP call, and the
Python argument errors of the new public functions."""

import ctypes as C

import numpy as np
import pytest

import raglite_amd
from raglite_amd import _abi, _ops, _search
from tests import rerank_ref as ref


# ---- the restatement against MaxSimRanker.rank -------------------------------------------------------------------------------------
class _StubDevice:
    def __init__(self, scores):
        self.scores = scores

    def maxsim_rerank(self, query_vecs, candidates):
        assert candidates.shape == (1, len(self.scores))
        return self.scores[None].copy()


class _StubIndex:
    """An index whose maxsim_rerank returns the given scores and whose docs are their own ordinals."""

    def __init__(self, scores):
        self.index = _StubDevice(scores)

    def ordinal_of_doc(self, doc):
        return int(doc)


def _rank(scores):
    ranker = raglite_amd.MaxSimRanker(_StubIndex(scores), lambda q: np.zeros((2, 4), np.float32))
    return ranker.rank(query="q", docs=[str(i) for i in range(len(scores))]).results


@pytest.mark.parametrize("n", [1, 2, 5, 33, 100])
def test_restatement_matches_maxsim_ranker_rank(n):
    rng = np.random.default_rng(n)
    for _ in range(20):
        scores, cand = ref.adversarial(rng, 1, n, pad=0.0)
        results = _rank(scores[0])
        out_s, out_c, out_p, counts = ref.order(scores, cand, n)
        assert counts[0] == n == len(results)
        assert [r.doc_id for r in results] == out_p[0].tolist() == ref.order_one(scores[0], cand[0]).tolist()
        assert np.array_equal(ref.bits(scores[0][out_p[0]]), ref.bits(out_s[0]))
        # float(score) keeps the value (a NaN stays a NaN, -0.0 stays -0.0)
        for r, s in zip(results, out_s[0]):
            assert (np.isnan(r.score) and np.isnan(s)) or (r.score == float(s) and np.signbit(r.score) == np.signbit(s))
        assert out_c[0].tolist() == cand[0][out_p[0]].tolist()


def test_signed_zeros_tie_and_nan_ranks_as_minus_infinity():
    nan = np.array([ref.NAN_B], np.uint32).view(np.float32)[0]
    scores = np.array([-0.0, 0.0, nan, -np.inf, 0.0, -0.0, np.nan, 1.0], np.float32)
    want = [7, 0, 1, 4, 5, 2, 3, 6]  # 1.0; the four zeros by position; NaN, -inf, NaN by position
    assert [r.doc_id for r in _rank(scores)] == want
    cand = np.arange(8, dtype=np.int32)[None]
    out_s, _, out_p, counts = ref.order(scores[None], cand, 8)
    assert out_p[0].tolist() == want and counts[0] == 8
    assert np.array_equal(ref.bits(out_s[0]), ref.bits(scores[want]))  # the score's own bits: that NaN, that zero


def test_padding_comes_last_and_is_not_counted():
    rng = np.random.default_rng(5)
    for pad in (0.0, 0.3, 1.0):
        scores, cand = ref.adversarial(rng, 6, 17, pad=pad)
        for k in (1, 5, 17):
            out_s, out_c, out_p, counts = ref.order(scores, cand, k)
            for b in range(6):
                real = int((cand[b] >= 0).sum())
                n = int(counts[b])
                assert n == min(k, real)
                assert np.all(out_c[b, :n] >= 0) and np.all(out_c[b, n:] == -1) and np.all(out_p[b, n:] == -1)
                assert np.all(out_s[b, n:] == -np.inf)
                # what rank gives for the real candidates alone, mapped back to their positions
                pos = np.nonzero(cand[b] >= 0)[0]
                results = _rank(scores[b][pos]) if real else []
                assert out_p[b, :n].tolist() == [int(pos[r.doc_id]) for r in results][:n]


# ---- argument checks of the C calls, before any HIP call ------------------------------------------------------------------------------
def _arr(ctype, values):
    return (ctype * len(values))(*values)


def _order(n_queries=2, n_cand=4, k=2, mem=_abi.MEM_HOST, null=()):
    f = _arr(C.c_float, [0.0] * 8)
    i = _arr(C.c_int32, [0] * 8)
    args = {"scores": f, "candidates": i, "out_scores": _arr(C.c_float, [0.0] * 8), "out_chunks": _arr(C.c_int32, [0] * 8),
            "out_pos": _arr(C.c_int32, [0] * 8), "out_counts": _arr(C.c_int32, [0] * 2)}
    for name in null:
        args[name] = None
    return _abi.lib().rl_rerank_order(args["scores"], args["candidates"], n_queries, n_cand, k, args["out_scores"], args["out_chunks"],
                                      args["out_pos"], args["out_counts"], mem, None)


@pytest.mark.parametrize("null", ["scores", "candidates", "out_scores", "out_chunks", "out_pos", "out_counts"])
def test_rerank_order_rejects_null_pointers(null):
    assert _order(null=(null,)) == _abi.RL_ERR_INVALID
    assert _abi.last_error() == "rl_rerank_order: null argument"


@pytest.mark.parametrize(("kwargs", "name"), [({"k": 0}, "k must"), ({"k": 5}, "k must"), ({"n_cand": 4097, "k": 1}, "n_cand"),
                                              ({"n_cand": 0, "k": 1}, "n_cand"), ({"mem": 7}, "bad mem"), ({"n_queries": -1}, "n_queries")])
def test_rerank_order_rejects_bad_sizes(kwargs, name):
    assert _order(**kwargs) == _abi.RL_ERR_INVALID
    msg = _abi.last_error()
    assert msg.startswith("rl_rerank_order") and name in msg, msg


def test_rerank_order_of_no_queries_is_ok():
    assert _order(n_queries=0, null=("scores", "candidates", "out_scores", "out_chunks", "out_pos", "out_counts")) == _abi.RL_OK


def _pipeline(nq=2, n_cand=2, k=2):
    q = _arr(C.c_float, [0.0] * 8)
    w = _arr(C.c_double, [0.75, 0.25])
    return _abi.lib().rl_search_rerank_per_query(None, None, q, 2, 4, 2, None, None, None, 0, None, None, w, 60, n_cand, q, nq, k,
                                                 _arr(C.c_float, [0.0] * 8), _arr(C.c_int32, [0] * 8), _arr(C.c_int32, [0] * 2),
                                                 _abi.MEM_HOST, None)


@pytest.mark.parametrize(("kwargs", "name"), [({}, "null index"), ({"nq": 0}, "nq must"), ({"n_cand": 4097}, "n_cand"),
                                              ({"k": 0}, "k must"), ({"k": 3}, "k must")])
def test_search_rerank_rejects_before_the_index_is_touched(kwargs, name):
    assert _pipeline(**kwargs) == _abi.RL_ERR_INVALID
    msg = _abi.last_error()
    assert msg.startswith("rl_search_rerank_per_query") and name in msg, msg


# ---- Python argument errors ---------------------------------------------------------------------------------------------------------
def test_ops_rerank_order_argument_errors():
    s, c = np.zeros((2, 4), np.float32), np.zeros((2, 4), np.int32)
    with pytest.raises(ValueError, match="n_queries, n_cand"):
        _ops.rerank_order(s, c[:, :3], 2)
    with pytest.raises(ValueError, match="n_queries, n_cand"):
        _ops.rerank_order(s[0], c[0], 2)
    for k in (0, 5):
        with pytest.raises(ValueError, match="k <= n_cand"):
            _ops.rerank_order(s, c, k)
    with pytest.raises(ValueError, match="k <= n_cand"):
        _ops.rerank_order(np.zeros((1, 4097), np.float32), np.zeros((1, 4097), np.int32), 1)


class _NoIndex:
    """Stands where a GpuIndex goes in calls that fail before they reach it."""


def test_public_batch_argument_errors():
    gi = _NoIndex()
    cfg = raglite_amd.HotPathConfig()
    with pytest.raises(ValueError, match="'hybrid' or 'vector'"):
        raglite_amd.search_and_rerank_chunks_batch(["q"], search="keyword", config=cfg, index=gi)
    with pytest.raises(ValueError, match="No GpuIndex attached"):
        raglite_amd.search_and_rerank_chunks_batch(["q"], config=cfg)
    assert raglite_amd.search_and_rerank_chunks_batch([], config=cfg, index=gi) == []
    with pytest.raises(ValueError, match="MaxSimRanker over the index"):
        raglite_amd.rerank_chunks_batch(["q"], [["a"]], config=cfg, index=gi)
    ranker = raglite_amd.MaxSimRanker(gi, lambda q: np.zeros((2, 4), np.float32))
    other = raglite_amd.HotPathConfig(reranker=raglite_amd.MaxSimRanker(_NoIndex(), ranker.query_encoder))
    with pytest.raises(ValueError, match="MaxSimRanker over the index"):  # a ranker over another index
        raglite_amd.rerank_chunks_batch(["q"], [["a"]], config=other, index=gi)
    cfg = raglite_amd.HotPathConfig(reranker=ranker)
    with pytest.raises(ValueError, match="one list of chunk ids per query"):
        raglite_amd.rerank_chunks_batch(["q", "r"], [["a"]], config=cfg, index=gi)
    with pytest.raises(ValueError, match="one list of docs per query"):
        ranker.rank_batch(["q", "r"], [["a"]])
    with pytest.raises(ValueError, match="one .nq, dim. matrix per query"):
        ranker.score_batch(["q", "r"], [[0], [1]], query_token_vectors=[np.zeros((2, 4), np.float32)])
    with pytest.raises(ValueError, match="one list of candidates per query"):
        ranker.score_batch(["q", "r"], [[0]])
    assert _search._groups_by_nq([np.zeros((2, 4)), np.zeros((3, 4)), np.zeros((2, 4))]) == [[0, 2], [1]]  # noqa: SLF001
