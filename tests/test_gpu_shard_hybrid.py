"""Sharded keyword and hybrid search on the device (DESIGN.md "Sharded keyword and hybrid search").

1. `rl_shard_hybrid_fuse` alone against its NumPy restatement (tests/shard_fuse_ref.py): score bits, ids and counts, world 1 - 8, up
   to the LDS limits, ties across ranks, a chunk hit on several rows and ranks, padding anywhere, no keyword lists, SHARD_MISSING
   poisoning, host and device pointers; past the limits RL_ERR_UNSUPPORTED.
2. Two and four shards of a 200 k-chunk corpus on ONE device, one thread per "rank", the collectives stood in for by a barrier
   exchange: `ShardedIndex.keyword_search` == `KeywordIndex.search` over the whole corpus, `ShardedIndex.hybrid_search` ==
   `DeviceIndex.hybrid_search` over the whole corpus, bit for bit -- with a metadata filter, tombstoned chunks, a global rank cut and an
   empty shard.
"""

import threading

import numpy as np
import pytest

import raglite_amd
from raglite_amd import _keyword, _ops
from raglite_amd._abi import UnsupportedError
from raglite_amd._sharded import SHARD_MISSING, ShardedIndex, compose_hybrid_fuse, shard_bounds_by_chunk
from tests import shard_fuse_ref as ref
from tests.keyword_ref import zipf_corpus, zipf_queries

pytestmark = pytest.mark.gpu


def _check(g, *, device=False, **kw):
    import torch

    arg = torch.as_tensor(g, device="cuda") if device else g
    s, c, n = _ops.shard_hybrid_fuse(arg, **kw)
    if device:
        assert s.is_cuda and c.is_cuda and n.is_cuda
        s, c, n = s.cpu().numpy(), c.cpu().numpy(), n.cpu().numpy()
    ws, wc, wn = ref.fuse(g, **kw)
    assert np.array_equal(n, wn)
    assert np.array_equal(c, wc)
    assert np.array_equal(s.view(np.uint64), ws.view(np.uint64))


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_shard_fuse_kernel_equals_its_restatement(torch_cuda, world):
    rng = np.random.default_rng(world)
    for B, num_hits, n_each in ((1, 5, 3), (37, 40, 10), (300, 128, 32), (4, 4096 // world, min(2048, 4096 // world))):
        for keywords in (True, False):
            g = ref.random_records(rng, world, B, num_hits, n_each, keywords)
            R = 2 if keywords else 1
            for k in sorted({1, min(7, R * n_each), R * n_each}):
                _check(g, num_hits=num_hits, n_each=n_each, keywords=keywords, weights=(0.75, 0.25), rrf_k=60, k=k)
            _check(g, device=True, num_hits=num_hits, n_each=n_each, keywords=keywords, weights=(1.0, -0.5), rrf_k=1, k=R * n_each)


def test_shard_fuse_kernel_edge_cases(torch_cuda):
    rng = np.random.default_rng(11)
    # all padding; padding only at the front; every row of one chunk
    g = ref.random_records(rng, 4, 6, 16, 8, True)
    g[:, 0, :] = -1
    g[:, 1, 0 : 3 * 8] = -1
    g[:, 2, 2 : 3 * 16 : 3] = 77
    g[:, 3, 3 * 16 :] = -1
    _check(g, num_hits=16, n_each=8, keywords=True, weights=(0.75, 0.25), rrf_k=60, k=16)
    _check(g, device=True, num_hits=16, n_each=8, keywords=True, weights=(0.5, 0.5), rrf_k=60, k=5)
    # equal row scores across every rank: the rank order is the global row order
    h = ref.random_records(rng, 8, 3, 20, 6, True, pad=0.0)
    h[:, :, 0 : 3 * 20 : 3] = np.float32(1.0).view(np.int32)
    _check(h, num_hits=20, n_each=6, keywords=True, weights=(0.75, 0.25), rrf_k=60, k=12)
    # a rank that failed sent SHARD_MISSING: the queries come back poisoned (ids -1, scores NaN, count 0), on both sides
    m = ref.random_records(rng, 3, 5, 10, 4, True)
    m[1, 2, 1] = SHARD_MISSING
    m[2, 4, 3 * 10 + 1] = SHARD_MISSING
    _check(m, num_hits=10, n_each=4, keywords=True, weights=(0.75, 0.25), rrf_k=60, k=8)
    s, c, n = _ops.shard_hybrid_fuse(m, num_hits=10, n_each=4, keywords=True, weights=(0.75, 0.25), k=8)
    assert np.isnan(s[[2, 4]]).all() and (c[[2, 4]] == -1).all() and (n[[2, 4]] == 0).all() and (n[[0, 1, 3]] > 0).all()
    # past the LDS limits: unsupported (the Python layer composes), bad arguments: invalid
    with pytest.raises(UnsupportedError):
        _ops.shard_hybrid_fuse(np.zeros((8, 1, 3 * 513 + 2 * 4), np.int32), num_hits=513, n_each=4, keywords=True, weights=(1, 1), k=4)
    with pytest.raises(UnsupportedError):
        _ops.shard_hybrid_fuse(np.zeros((8, 1, 3 * 4 + 2 * 513), np.int32), num_hits=4, n_each=513, keywords=True, weights=(1, 1), k=4)
    with pytest.raises(ValueError, match="weights"):
        _ops.shard_hybrid_fuse(np.zeros((2, 1, 3 * 4 + 2 * 4), np.int32), num_hits=4, n_each=4, keywords=True, weights=(1, np.nan), k=4)


def test_composition_past_the_limits_equals_the_kernel_within_them(torch_cuda):
    rng = np.random.default_rng(5)
    g = ref.random_records(rng, 8, 20, 64, 16, True)
    for keywords in (True, False):
        gg = g if keywords else np.ascontiguousarray(g[:, :, : 3 * 64])
        kw = dict(num_hits=64, n_each=16, keywords=keywords, weights=(0.75, 0.25), rrf_k=60, k=16)
        a, b = _ops.shard_hybrid_fuse(gg, **kw), compose_hybrid_fuse(gg, **kw)
        assert all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(a, b))


# ---- shards on one device ----------------------------------------------------------------------------------------------------
class _Hub:
    """The collectives of `world` threads: every rank hands in its tensor, every rank gets the stack (a barrier times out instead of hanging)."""

    def __init__(self, world):
        self.world, self.slots, self.barrier = world, [None] * world, threading.Barrier(world, timeout=300)

    def exchange(self, rank, t):
        import torch

        torch.cuda.synchronize()
        self.slots[rank] = t.clone()
        torch.cuda.synchronize()
        self.barrier.wait()
        out = torch.stack(list(self.slots))
        self.barrier.wait()
        return out


class _ThreadComm:
    def __init__(self, hub, rank):
        self.hub, self.rank, self.world = hub, rank, hub.world

    def allgather(self, t):
        return self.hub.exchange(self.rank, t.contiguous())

    def allreduce_sum_(self, t):
        t.copy_(self.allgather(t).sum(0).to(t.dtype))
        return t


class _EmptyLocal:
    """A shard without chunks (DeviceIndex needs rows): empty lists of the right shapes."""

    n_rows = 0
    n_chunks = 0

    def search_rows(self, q, k, chunk_filter=None, rank_limit=None):
        import torch

        B = q.shape[0]
        return (torch.full((B, k), float("-inf"), device=q.device), torch.full((B, k), -1, dtype=torch.int32, device=q.device))


def _run_ranks(shards, fn):
    outs, errs = [None] * len(shards), [None] * len(shards)

    def body(r):
        try:
            raglite_amd.set_device(0)
            outs[r] = fn(shards[r])
        except BaseException as exc:  # noqa: BLE001
            errs[r] = exc
            shards[r].comm.hub.barrier.abort()

    threads = [threading.Thread(target=body, args=(r,)) for r in range(len(shards))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for e in errs:
        if e is not None:
            raise e
    return outs


@pytest.fixture(scope="module")
def corpus(torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(2024)
    n_chunks, d, n_terms = 200_000, 64, 3000
    sizes = rng.integers(1, 3, size=n_chunks)
    off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    E = torch.empty((int(off[-1]), d), dtype=torch.float32, device="cuda")
    raglite_amd.synth_fill(E, seed=41, kind="small_int")  # integer data: ties across shard boundaries
    flat, toff = zipf_corpus(rng, n_chunks, n_terms, 12)
    dead = np.sort(rng.choice(n_chunks, size=3000, replace=False))
    names = [f"s{t}" for t in range(n_terms)]  # (not zero-padded: the vocabulary order is the string order, not the id order)
    stems = [[names[t] for t in flat[toff[c] : toff[c + 1]]] for c in range(n_chunks)]
    for c in dead:
        stems[c] = None
    vocab, postings = _keyword.build_from_stems(stems)
    full = raglite_amd.DeviceIndex(E, off, metric="dot")
    full.delete_chunks(dead)
    kw_full = raglite_amd.KeywordIndex(postings)
    Q = torch.empty((48, d), dtype=torch.float32, device="cuda")
    raglite_amd.synth_fill(Q, seed=42, kind="small_int")
    ids = {s: i for i, s in enumerate(vocab)}
    qterms = [sorted({ids[names[t]] for t in q if names[t] in ids}) for q in zipf_queries(rng, 48, n_terms)]
    mask = rng.random(n_chunks) < 0.6
    yield dict(E=E, off=off, stems=stems, dead=dead, full=full, kw_full=kw_full, Q=Q, qterms=qterms, mask=mask)
    full.close()
    kw_full.close()


def _shards(c, bounds):
    hub = _Hub(len(bounds))
    out = []
    for r, (c_lo, c_hi) in enumerate(bounds):
        off = c["off"]
        r_lo, r_hi = int(off[c_lo]), int(off[c_hi])
        loc = off[c_lo : c_hi + 1] - off[c_lo]
        if c_hi > c_lo:
            local = raglite_amd.DeviceIndex(c["E"][r_lo:r_hi], loc, metric="dot")
            dead = c["dead"][(c["dead"] >= c_lo) & (c["dead"] < c_hi)] - c_lo
            if dead.size:
                local.delete_chunks(dead)
        else:
            local = _EmptyLocal()
        out.append(ShardedIndex(local, row_base=r_lo, chunk_base=c_lo, local_chunk_offsets=loc, comm=_ThreadComm(hub, r)))
    _run_ranks(out, lambda sh: sh.attach_keywords(c["stems"][sh.chunk_base : sh.chunk_base + len(sh.local_chunk_offsets) - 1]))
    return out


def _close(shards):
    for sh in shards:
        if hasattr(sh.local, "close"):
            sh.local.close()
        if sh.keyword is not None:
            sh.keyword.close()


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_keyword_and_hybrid_equal_one_index(corpus, world):
    import torch

    c = corpus
    shards = _shards(c, shard_bounds_by_chunk(c["off"], world))
    try:
        for filt in (None, c["mask"]):
            want = c["kw_full"].search(c["qterms"], 40, chunk_filter=filt)
            for got in _run_ranks(shards, lambda sh: sh.keyword_search(c["qterms"], 40, chunk_filter=filt)):
                assert np.array_equal(got[2], want[2]) and np.array_equal(got[1], want[1])
                assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
        cases = [dict(), dict(chunk_filter=c["mask"]), dict(rank_limit=5000), dict(chunk_filter=c["mask"], rank_limit=20000),
                 dict(weights=(1.0, 1.0), rrf_k=1)]
        for kw in cases:
            for num_hits, n_each, k in ((60, 20, 20), (256, 64, 100)):
                ws, wc, wn = c["full"].hybrid_search(c["Q"], num_hits, n_each, k, keyword=c["kw_full"], query_term_ids=c["qterms"], **kw)
                for s, ch, n in _run_ranks(shards, lambda sh: sh.hybrid_search(c["Q"], c["qterms"], num_hits, n_each, k, **kw)):
                    assert s.is_cuda and ch.is_cuda
                    assert torch.equal(n, wn) and torch.equal(ch, wc) and bool((s == ws).all()), (world, kw, num_hits)
        # the vector list alone (no query terms): rl_hybrid_search with kw == NULL
        ws, wc, wn = c["full"].hybrid_search(c["Q"], 60, 20, 20)
        for s, ch, n in _run_ranks(shards, lambda sh: sh.hybrid_search(c["Q"], None, 60, 20, 20)):
            assert torch.equal(n, wn) and torch.equal(ch, wc) and bool((s == ws).all())
        # host queries take the host transport and return host arrays, the same values
        qh = c["Q"][:5].cpu().numpy()
        ws, wc, wn = c["full"].hybrid_search(qh, 60, 20, 20, keyword=c["kw_full"], query_term_ids=c["qterms"][:5])
        for s, ch, n in _run_ranks(shards, lambda sh: sh.hybrid_search(qh, c["qterms"][:5], 60, 20, 20)):
            assert np.array_equal(n, wn) and np.array_equal(ch, wc) and np.array_equal(s.view(np.uint64), ws.view(np.uint64))
    finally:
        _close(shards)


def test_sharded_hybrid_with_an_empty_shard_and_past_the_kernel_limits(corpus):
    import torch

    c = corpus
    b = shard_bounds_by_chunk(c["off"], 2)
    bounds = [b[0], (b[1][0], b[1][0]), b[1]]  # the middle shard holds no chunk
    shards = _shards(c, bounds)
    try:
        want = c["kw_full"].search(c["qterms"], 30)
        for got in _run_ranks(shards, lambda sh: sh.keyword_search(c["qterms"], 30)):
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
        for num_hits, n_each, k in ((60, 20, 20), (1400, 1400, 50)):  # 3 x 1400 > 4096: the composition of the existing pieces
            ws, wc, wn = c["full"].hybrid_search(c["Q"][:8], num_hits, n_each, k, keyword=c["kw_full"], query_term_ids=c["qterms"][:8],
                                                 chunk_filter=c["mask"])
            outs = _run_ranks(shards, lambda sh: sh.hybrid_search(c["Q"][:8], c["qterms"][:8], num_hits, n_each, k, chunk_filter=c["mask"]))
            for s, ch, n in outs:
                assert torch.equal(n, wn) and torch.equal(ch, wc) and bool((s == ws).all()), (num_hits, n_each)
    finally:
        _close(shards)
