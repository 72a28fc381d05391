"""Sharded BM25 keyword and hybrid search without the hardware: 2 and 8 gloo ranks (uneven shards, one EMPTY) run
`ShardedIndex.attach_keywords`, `keyword_search` and `hybrid_search` with test doubles for the device: the oracle-backed row searcher of
tests/test_sharded_gloo.py, a keyword index over tests/keyword_ref.py's float32 restatement, and tests/shard_fuse_ref.py for
`rl_shard_hybrid_fuse`.  Results must equal the single-corpus restatement bit for bit -- with and without a filter, behind a global rank
cut -- and a rank whose local step fails must not leave anybody waiting."""

import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import oracle
from raglite_amd import _keyword
from raglite_amd._sharded import ShardedIndex
from tests import rrf_ref
from tests import shard_fuse_ref
from tests.keyword_ref import impacts_f32, scores_f32, topk_f32, zipf_corpus, zipf_queries
from tests.test_sharded_gloo import _free_port
from tests.test_sharded_gloo8 import CUTS as CUTS8, _Local, _corpus, _mask

CUTS = {2: [0, 61, 150], 8: CUTS8}


class _KwLocal:
    """Test double for raglite_amd.KeywordIndex: the float32 restatement of keyword.hip over one shard's postings."""

    def __init__(self, postings):
        self.p, self.imp = postings, impacts_f32(postings)

    def search(self, query_term_ids, k, chunk_filter=None):
        B = len(query_term_ids)
        S, C, N = np.full((B, k), -np.inf, np.float32), np.full((B, k), -1, np.int32), np.zeros(B, np.int32)
        for b, q in enumerate(query_term_ids):
            s, c = topk_f32(scores_f32(self.p, self.imp, q), k, None if chunk_filter is None else np.asarray(chunk_filter, bool))
            S[b, : len(s)], C[b, : len(c)], N[b] = s, c, len(c)
        return S, C, N


def _keyword_corpus(n_chunks):
    rng = np.random.default_rng(606)
    flat, off = zipf_corpus(rng, n_chunks, 90, 8)
    stems = [[f"w{t}" for t in flat[off[c] : off[c + 1]]] for c in range(n_chunks)]
    for c in (3, 17, 18, 70, 140):  # dead chunks on some shards
        stems[c] = None
    stems[100] = stems[100] + [_keyword.stem("onlyhere")]  # a stem of one shard only
    vocab, full = _keyword.build_from_stems(stems)
    ids = {s: i for i, s in enumerate(vocab)}
    queries = [sorted({ids[f"w{t}"] for t in q if f"w{t}" in ids}) for q in zipf_queries(rng, 3, 90)]
    queries[1] = sorted(set(queries[1]) | {ids[_keyword.stem("onlyhere")]})
    return stems, vocab, full, queries


def _want_hybrid(E, off, Q, full, queries, num_hits, n_each, k, ok, rank_limit, weights=(0.75, 0.25), rrf_k=60):
    """What ONE index plus keyword index over the whole corpus returns: the two lists, then weighted RRF."""
    r2c = np.repeat(np.arange(len(off) - 1), np.diff(off))
    imp = impacts_f32(full)
    every = np.ones(len(off) - 1, bool) if ok is None else ok
    vec, kw = np.full((len(Q), n_each), -1, np.int32), np.full((len(Q), n_each), -1, np.int32)
    for b in range(len(Q)):
        _, cc = oracle.search_chunks_ranked(E, r2c, Q[b], num_hits, n_each, every, len(r2c) if rank_limit is None else rank_limit, None, "dot", np.float32)
        vec[b, : len(cc)] = cc
        _, kc = topk_f32(scores_f32(full, imp, queries[b]), n_each, ok)
        kw[b, : len(kc)] = kc
    return rrf_ref.fuse(np.stack([vec, kw]), weights, rrf_k, k)


def _worker(rank, world, port, out_q):
    try:
        _worker_body(rank, world, port, out_q)
    except BaseException as exc:  # noqa: BLE001
        import traceback

        out_q.put({"rank": rank, "error": "".join(traceback.format_exception(type(exc), exc, exc.__traceback__))})
        raise


def _worker_body(rank, world, port, out_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        E, off, Q, _ = _corpus()
        stems, _, _, queries = _keyword_corpus(len(off) - 1)
        cuts = CUTS[world]
        c_lo, c_hi = cuts[rank], cuts[rank + 1]
        r_lo, r_hi = int(off[c_lo]), int(off[c_hi])
        local_off = off[c_lo : c_hi + 1] - off[c_lo]
        sh = ShardedIndex(_Local(E[r_lo:r_hi], local_off, "dot"), row_base=r_lo, chunk_base=c_lo, local_chunk_offsets=local_off)
        sh.shard_fuse = shard_fuse_ref.fuse
        sh.attach_keywords(stems[c_lo:c_hi], make_index=_KwLocal)
        ok = _mask(len(off) - 1)
        out = {"rank": rank, "vocab": sorted(sh._kw_vocab, key=sh._kw_vocab.get)}  # noqa: SLF001
        out["kw"] = sh.keyword_search(queries, 12)
        out["kw_f"] = sh.keyword_search(queries, 12, chunk_filter=ok)
        out["hy"] = sh.hybrid_search(Q, queries, 40, 8, 10)
        out["hy_f"] = sh.hybrid_search(Q, queries, 40, 8, 16, chunk_filter=ok)
        out["hy_cut"] = sh.hybrid_search(Q, queries, 40, 8, 16, chunk_filter=ok, rank_limit=150, weights=(1.0, 1.0), rrf_k=1)
        out["hy_vec"] = sh.hybrid_search(Q, None, 40, 8, 8)
        # failure on rank 1: its keyword search raises; it still enters the exchange, then raises; the others get poisoned queries
        if rank == 1:
            def boom(*a, **kw):
                raise MemoryError("keyword search failed (injected)")

            if sh.keyword is None:
                sh.keyword = _KwLocal(_keyword.build_from_stems([])[1])
            sh.keyword.search = boom
        for name, call in (("fail_kw", lambda: sh.keyword_search(queries, 12)), ("fail_hy", lambda: sh.hybrid_search(Q, queries, 40, 8, 10))):
            try:
                res = call()
                out[name] = ("poisoned", bool(np.isnan(res[0]).all()) and bool((res[1] == -1).all()) and bool((res[2] == 0).all()))
            except MemoryError as exc:
                out[name] = ("raised", str(exc))
        sh.check_failures = True
        try:
            sh.hybrid_search(Q, queries, 40, 8, 10)
            out["fail_checked"] = "no error"
        except MemoryError as exc:
            out["fail_checked"] = f"MemoryError: {exc}"
        except RuntimeError as exc:
            out["fail_checked"] = f"RuntimeError: {exc}"
        t = torch.tensor([rank], dtype=torch.int64)
        dist.all_reduce(t)
        out["after"] = int(t.item())
        out_q.put(out)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 8])
def test_sharded_keyword_and_hybrid_match_one_corpus(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = []
    for _ in range(world):
        results.append(q.get(timeout=240))
        assert "error" not in results[-1], results[-1]["error"]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    E, off, Q, _ = _corpus()
    stems, vocab, full, queries = _keyword_corpus(len(off) - 1)
    ok = _mask(len(off) - 1)
    imp = impacts_f32(full)

    def want_kw(k, allowed):
        S, C, N = np.full((len(queries), k), -np.inf, np.float32), np.full((len(queries), k), -1, np.int32), np.zeros(len(queries), np.int32)
        for b, qq in enumerate(queries):
            s, c = topk_f32(scores_f32(full, imp, qq), k, allowed)
            S[b, : len(s)], C[b, : len(c)], N[b] = s, c, len(c)
        return S, C, N

    expect = {"kw": want_kw(12, None), "kw_f": want_kw(12, ok),
              "hy": _want_hybrid(E, off, Q, full, queries, 40, 8, 10, None, None),
              "hy_f": _want_hybrid(E, off, Q, full, queries, 40, 8, 16, ok, None),
              "hy_cut": _want_hybrid(E, off, Q, full, queries, 40, 8, 16, ok, 150, weights=(1.0, 1.0), rrf_k=1)}
    r2c = np.repeat(np.arange(len(off) - 1), np.diff(off))
    vec = np.full((1, len(Q), 8), -1, np.int32)
    for b in range(len(Q)):
        _, cc = oracle.search_chunks_ranked(E, r2c, Q[b], 40, 8, np.ones(len(off) - 1, bool), len(r2c), None, "dot", np.float32)
        vec[0, b, : len(cc)] = cc
    expect["hy_vec"] = rrf_ref.fuse(vec, (0.75,), 60, 8)
    for out in sorted(results, key=lambda o: o["rank"]):
        rank = out["rank"]
        assert out["vocab"] == vocab, f"rank {rank}: the agreed vocabulary is not the single build's"
        for name, (ws, wi, wn) in expect.items():
            gs, gi, gn = out[name]
            assert np.array_equal(gn, wn) and np.array_equal(gi, wi), (rank, name)
            assert np.array_equal(np.asarray(gs).view(np.uint8), np.asarray(ws, dtype=np.asarray(gs).dtype).view(np.uint8)), (rank, name)
        if rank == 1:
            assert out["fail_kw"] == ("raised", "keyword search failed (injected)")
            assert out["fail_hy"] == ("raised", "keyword search failed (injected)")
            assert out["fail_checked"].startswith("MemoryError")
        else:
            assert out["fail_kw"] == ("poisoned", True) and out["fail_hy"] == ("poisoned", True), rank
            assert out["fail_checked"].startswith("RuntimeError: ShardedIndex.hybrid_search: another rank failed"), rank
        assert out["after"] == sum(range(world))


class _ReplayComm:
    """A Communicator double for ONE process (world 2, no torch.distributed), as in tests/test_sharded_gloo8.py: `allgather` answers with
    the partner's array from the previous pass, so that repeated passes converge on what two real ranks exchange."""

    world = 2

    def __init__(self, rank, known):
        self.rank, self.known, self.mine, self.complete = rank, known, [], True

    def allgather(self, t):
        j = len(self.mine)
        self.mine.append(t.clone())
        other = self.known[1 - self.rank][j] if j < len(self.known[1 - self.rank]) else None
        if other is None or other.shape != t.shape:
            self.complete, other = False, t
        return torch.stack([t, other] if self.rank == 0 else [other, t])


def test_vocabulary_exchange_through_a_communicator_only_index():
    """attach_keywords + keyword_search with a Communicator and no torch.distributed: the vocabulary, the int64 statistics and the
    merge all go through the communicator."""
    assert not (dist.is_available() and dist.is_initialized())
    E, off, _, _ = _corpus()
    stems, vocab, full, queries = _keyword_corpus(len(off) - 1)
    bounds = [(0, 61), (61, 150)]
    known = [[], []]
    for _ in range(8):
        outs, comms = [], []
        for rank, (c_lo, c_hi) in enumerate(bounds):
            comm = _ReplayComm(rank, known)
            loc = off[c_lo : c_hi + 1] - off[c_lo]
            sh = ShardedIndex(_Local(E[int(off[c_lo]) : int(off[c_hi])], loc, "dot"), row_base=int(off[c_lo]), chunk_base=c_lo,
                              local_chunk_offsets=loc, comm=comm)
            sh.attach_keywords(stems[c_lo:c_hi], make_index=_KwLocal)
            outs.append((sorted(sh._kw_vocab, key=sh._kw_vocab.get), sh.keyword_search(queries, 12), sh.keyword_query_ids("Onlyhere, nothing else")))  # noqa: SLF001
            comms.append(comm)
        stable = all(len(c.mine) == len(prev) and all(torch.equal(a, b) for a, b in zip(c.mine, prev)) for c, prev in zip(comms, known))
        known = [c.mine for c in comms]
        if stable and all(c.complete for c in comms):  # (every rank handed in what it handed in the pass before: a fixed point)
            break
    else:
        raise AssertionError("the replayed exchanges did not converge")
    imp = impacts_f32(full)
    for got_vocab, (gs, gi, gn), qids in outs:
        assert got_vocab == vocab
        assert qids == [vocab.index(_keyword.stem("onlyhere"))]
        for b, qq in enumerate(queries):
            s, c = topk_f32(scores_f32(full, imp, qq), 12)
            assert gn[b] == len(c) and np.array_equal(gi[b, : len(c)], c) and np.array_equal(gs[b, : len(s)].view(np.uint32), s.view(np.uint32))


def test_keyword_calls_need_attach_keywords_first():
    sh = ShardedIndex(object(), row_base=0, chunk_base=0, local_chunk_offsets=np.array([0, 1, 2]))
    with pytest.raises(ValueError, match="attach_keywords"):
        sh.keyword_search([[1]], 3)
    with pytest.raises(ValueError, match="one entry"):
        sh.attach_keywords([["a"]])
