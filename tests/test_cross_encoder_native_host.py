"""The host side of the native cross-encoder rerank, without a GPU: the argument checks of the four new C entries
(every one returns before the first HIP call), the workspace layout behind `rl_encoder_classify_workspace_bytes` (the header's own walk,
compiled for the host), the head's bound held against an f32 emulation, and the packing and ordering of `rank_batch` over a fake
`classify_rows` that returns planted logits."""

import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from raglite_amd import _abi, _ops
from raglite_amd._cross_encoder import CrossEncoderShape, TorchCrossEncoderRanker
from raglite_amd._encoder import MAX_PACK_TOKENS, NativeEncoder
from raglite_amd._torch_embedder import pack_runs
from tests import encoder_head_ref as ref
from tests.encoder_ref import worst_ratio

ROOT = Path(__file__).resolve().parent.parent
P = 0x10000  # a "pointer" that is never followed: every call below is refused (or returns) before anything is read


# ---- the C entries ---------------------------------------------------------------------------------------------------------------------
def _refused(status, want, who):
    assert status == want, (status, _abi.last_error())
    assert f"{who}:" in _abi.last_error()


def test_head_argument_checks():
    lib = _abi.lib()
    good = dict(x=P, off=P, n_seqs=2, n_tokens=5, hidden=64, pw=P, pb=P, hw=P, hb=P, dtype=0, out=P, mem=_abi.MEM_DEVICE)

    def call(**kw):
        a = {**good, **kw}
        return lib.rl_encoder_head(a["x"], a["off"], a["n_seqs"], a["n_tokens"], a["hidden"], a["pw"], a["pb"], a["hw"], a["hb"], a["dtype"],
                                   a["out"], a["mem"], None)

    inv, uns = _abi.RL_ERR_INVALID, _abi.RL_ERR_UNSUPPORTED
    for kw, want in [(dict(mem=_abi.MEM_HOST), uns), (dict(hidden=8224), uns), (dict(hidden=48), inv), (dict(hidden=-32), inv),
                     (dict(dtype=2), inv), (dict(dtype=-1), inv), (dict(n_seqs=-1), inv), (dict(n_seqs=65536), inv), (dict(n_tokens=-1), inv),
                     (dict(n_tokens=2 ** 31), inv), (dict(n_tokens=0), inv),
                     *[({k: None}, inv) for k in ("x", "off", "pw", "pb", "hw", "hb", "out")],
                     *[({k: P + 8}, inv) for k in ("x", "pw", "pb", "hw", "hb")], *[({k: P + 2}, inv) for k in ("off", "out")]]:
        _refused(call(**kw), want, "rl_encoder_head")
    assert call(mem=_abi.MEM_HOST, hidden=48) == uns  # (mem comes first)
    assert call(n_seqs=0, x=None, off=None, out=None) == _abi.RL_OK  # nothing to do: no pointer is looked at, nothing is launched


def test_set_head_argument_checks():
    lib = _abi.lib()
    who = "rl_encoder_set_head"
    _refused(lib.rl_encoder_set_head(None, P, P, P, P), _abi.RL_ERR_INVALID, who)
    assert "null handle" in _abi.last_error()
    _refused(lib.rl_encoder_set_head(None, None, None, None, None), _abi.RL_ERR_INVALID, who)  # (clearing needs a handle too)
    assert "null handle" in _abi.last_error()
    for i in range(4):
        some = [P] * 4
        some[i] = None
        _refused(lib.rl_encoder_set_head(None, *some), _abi.RL_ERR_INVALID, who)
        assert "all four" in _abi.last_error()
        odd = [P] * 4
        odd[i] = P + 8
        _refused(lib.rl_encoder_set_head(None, *odd), _abi.RL_ERR_INVALID, who)
        assert "aligned" in _abi.last_error()


def test_classify_workspace_bytes_argument_checks():
    lib, n = _abi.lib(), C.c_int64(-1)
    who = "rl_encoder_classify_workspace_bytes"
    for n_tokens, n_seqs, out in [(-1, 1, C.byref(n)), (MAX_PACK_TOKENS + 1, 1, C.byref(n)), (8, -1, C.byref(n)), (8, 65536, C.byref(n)), (8, 1, None)]:
        _refused(lib.rl_encoder_classify_workspace_bytes(None, n_tokens, n_seqs, out), _abi.RL_ERR_INVALID, who)
        assert "null handle" not in _abi.last_error()
    _refused(lib.rl_encoder_classify_workspace_bytes(None, 8, 1, C.byref(n)), _abi.RL_ERR_INVALID, who)
    assert "null handle" in _abi.last_error() and n.value == -1


def test_classify_pack_argument_checks():
    lib = _abi.lib()
    who = "rl_encoder_classify_pack"
    good = dict(ids=P, pos=P, typ=P, off=P, n_seqs=2, n_tokens=5, max_len=3, out=P, ws=P, ws_bytes=1 << 20, mem=_abi.MEM_DEVICE)

    def call(**kw):
        a = {**good, **kw}
        return lib.rl_encoder_classify_pack(None, a["ids"], a["pos"], a["typ"], a["off"], a["n_seqs"], a["n_tokens"], a["max_len"], a["out"],
                                            a["ws"], a["ws_bytes"], a["mem"], None)

    inv, uns = _abi.RL_ERR_INVALID, _abi.RL_ERR_UNSUPPORTED
    for kw, want in [(dict(mem=_abi.MEM_HOST), uns), (dict(n_seqs=-1), inv), (dict(n_tokens=-1), inv), (dict(max_len=-1), inv),
                     (dict(n_seqs=65536), inv), (dict(n_tokens=MAX_PACK_TOKENS + 1), uns),
                     *[({k: None}, inv) for k in ("ids", "pos", "off", "out", "ws")],
                     *[({k: P + 2}, inv) for k in ("ids", "pos", "typ", "off", "out")], (dict(ws=P + 8), inv)]:
        _refused(call(**kw), want, who)
        assert "null handle" not in _abi.last_error(), kw
    _refused(call(), inv, who)
    assert "null handle" in _abi.last_error()
    _refused(call(typ=None, out=P + 4), inv, who)  # type ids may be NULL and the logits need 4 bytes only: all that is wrong is the handle
    assert "null handle" in _abi.last_error()


# ---- the workspace layout: scratch_layout.h's own walk, on the host ----------------------------------------------------------------------
_DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "scratch_layout.h"
int main() {
    const size_t rows[] = {0, 1, 2, 31, 255, 256, 257, 1000, 8191, 8192};
    const size_t shapes[][3] = {{64, 128, 1}, {192, 768, 2}, {384, 1536, 3}, {1024, 4096, 8}, {8192, 32768, 8}};
    for (auto& sh : shapes)
        for (size_t r : rows) {
            const size_t pack = rl::EncoderScratch().lay(rl::Carver(), r, sh[0], sh[1], sh[2]);
            rl::EncoderClassifyScratch sized;
            const size_t total = sized.lay(rl::Carver(), r, sh[0], sh[1], sh[2]);
            char* block = static_cast<char*>(std::aligned_alloc(256, total + 256));
            rl::EncoderClassifyScratch w;
            const size_t walked = w.lay(rl::Carver(block), r, sh[0], sh[1], sh[2]);
            rl::EncoderScratch alone;  // what the trunk's launches walk over the same block
            alone.lay(rl::Carver(block), r, sh[0], sh[1], sh[2]);
            const int same = alone.x == w.trunk.x && alone.x1 == w.trunk.x1 && alone.qkv == w.trunk.qkv && alone.attn == w.trunk.attn &&
                             alone.mid == w.trunk.mid && alone.part == w.trunk.part;
            std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %d\n", sh[0], sh[1], sh[2], r, pack, total, walked,
                        (size_t)(reinterpret_cast<char*>(w.final_rows) - block), same);
            std::free(block);
        }
    return 0;
}
"""


@pytest.fixture(scope="module")
def layout_records(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("classify_layout")
    (d / "drv.cpp").write_text(_DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O1", f"-I{ROOT / 'raglite_amd' / 'csrc'}", str(d / "drv.cpp"), "-o", str(d / "drv")], check=True)
    run = subprocess.run([str(d / "drv")], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    return [tuple(int(v) for v in line.split()) for line in run.stdout.splitlines()]


def test_classify_workspace_is_the_pack_workspace_plus_the_final_rows(layout_records):
    assert len(layout_records) == 50
    by_shape = {}
    for hidden, ffn, ksplit, rows, pack, total, walked, final_at, same in layout_records:
        assert total == walked, "size and pointers come from one walk"
        assert same == 1, "the trunk's scratch lies where rl_encoder_forward_pack's own walk puts it"
        assert final_at % 16 == 0 and final_at >= pack, "the final rows start behind the trunk's scratch, on a 16-byte boundary"
        assert final_at + 2 * rows * hidden == total
        assert pack <= total <= pack + 2 * rows * hidden + 16, "at least the pack bytes; the rows and padding only on top"
        by_shape.setdefault((hidden, ffn, ksplit), []).append((rows, total))
    for sizes in by_shape.values():
        assert all(b[1] >= a[1] for a, b in zip(sizes, sizes[1:])), "monotone in n_tokens"
        assert sizes[0] == (0, 0)


# ---- the bound of the head, against an f32 emulation of its rounding points -------------------------------------------------------------
@pytest.mark.parametrize("case", ref.head_cases(), ids=[c.name for c in ref.head_cases()])
def test_head_bound_holds_for_the_emulation_and_refuses_a_moved_logit(case):
    truth, a, _, _ = ref.head_f64(case)
    c = 2.0 * ref.tanh_c(a.float(), torch.tanh(a.float()))  # the allowance measured the way the GPU test measures it, on the CPU's tanh
    bound1 = ref.head_bound(case, c, 1.0)
    assert ref.bound_is_sane(case, c)
    got = ref.head_emulated(case).double()
    assert worst_ratio(got, truth, bound1) <= 1.0
    moved = ref.moved_by_bound(got, truth, bound1)
    off = got != truth
    assert bool(off.any()) and bool(((moved - truth).abs() > bound1)[off].all())


def test_offsets_cases_cover_what_they_name():
    cases = ref.offsets_cases()
    assert sorted(len(rows) for _, rows in cases.values()) == [1, 1, 1, 1, 4, 17, 300]
    firsts = {r for _, rows in cases.values() for r in rows if r is not None}
    assert {0, 255, 256, ref.N_TOKENS - 1} <= firsts
    assert sum(r is None for r in cases["seventeen"][1]) == 1
    assert min(cases["clamped"][0]) < 0 and max(cases["clamped"][0]) > ref.N_TOKENS


# ---- rank_batch over planted logits ---------------------------------------------------------------------------------------------------
SHAPE = CrossEncoderShape(vocab_size=500, hidden=64, layers=1, heads=2, ffn=128, max_positions=64, n_ctx=64)


class FakeNative:
    """`classify_rows` with planted logits: a function of the pair's own ids, NaN for some, so that what a pair gets does not depend on
    the pack it arrives in -- the property the real one has."""

    def __init__(self):
        self.calls = []  # per call: (rows, type_rows)
        self.pack_forwards = 0

    @staticmethod
    def planted(row):
        h = sum((i + 1) * t for i, t in enumerate(row)) % 101
        return float("nan") if h % 13 == 5 else (h % 17) / 4.0 - 2.0  # 17 levels: equal scores are common

    def classify_rows(self, rows, type_rows):
        self.calls.append(([list(r) for r in rows], [list(t) for t in type_rows]))
        self.pack_forwards += 1
        return torch.tensor([self.planted(r) for r in rows], dtype=torch.float32)


def _order_restated(scores, cand, k):
    """`rl_rerank_order`'s contract in NumPy (raglite_amd/_ops_retrieval.py: score descending, NaN as -inf, ties by position, padding last)."""
    scores, cand = np.asarray(scores), np.asarray(cand)
    assert scores.dtype == np.float32 and cand.dtype == np.int32 and scores.shape == cand.shape and k == scores.shape[1]
    pos = np.full(scores.shape, -1, np.int32)
    counts = np.zeros(scores.shape[0], np.int32)
    for b in range(scores.shape[0]):
        real = np.flatnonzero(cand[b] >= 0)
        key = np.where(np.isnan(scores[b, real]), -np.inf, scores[b, real])
        order = real[np.lexsort((real, -key))]
        pos[b, : len(order)], counts[b] = order, len(order)
    return None, None, pos, counts


@pytest.fixture()
def planted(monkeypatch):
    ranker = TorchCrossEncoderRanker(SHAPE, device="cpu", forward="native", max_length=48)
    fake, seen = FakeNative(), []
    monkeypatch.setattr(ranker, "_native_applies", lambda: True)
    monkeypatch.setattr(ranker, "_native_encoder", lambda: fake)

    def order(scores, cand, k):
        seen.append((np.array(scores), np.array(cand)))
        return _order_restated(scores, cand, k)

    monkeypatch.setattr(_ops, "rerank_order", order)
    return ranker, fake, seen


def _batch(B, rng):  # noqa: N803
    words = [f"w{i}" for i in range(60)]
    text = lambda n: " ".join(rng.choice(words, size=n))  # noqa: E731
    queries = [text(int(rng.integers(1, 9))) for _ in range(B)]
    docs = []
    for b in range(B):
        n = 0 if b % 7 == 3 else int(rng.integers(1, 12))
        ds = [text(int(rng.integers(1, 70))) for _ in range(n)]  # (up to 70 words against max_length 48: some pairs are truncated)
        if n > 2:
            ds[-1] = ds[0]  # a duplicate doc: equal scores keep input order
        docs.append(ds)
    return queries, docs


def _same(a, b):
    assert a.query == b.query and len(a.results) == len(b.results)
    for x, y in zip(a.results, b.results):
        assert (x.doc_id, x.rank, x.text) == (y.doc_id, y.rank, y.text)
        assert np.float32(x.score).tobytes() == np.float32(y.score).tobytes()


@pytest.mark.parametrize("B", [1, 7, 40, 300])
def test_rank_batch_packs_in_pair_order_and_orders_like_rank(planted, B):  # noqa: N803
    ranker, fake, seen = planted
    queries, docs = _batch(B, np.random.default_rng(B))
    ids = [None if b % 2 else [100 + 3 * i for i in range(len(d))] for b, d in enumerate(docs)]
    got = ranker.rank_batch(queries, docs, ids)
    batch_calls, fake.calls = fake.calls, []
    # pair order: all queries' pairs, query by query, doc by doc -- and each pair's type ids: 0 over [CLS] q [SEP], 1 behind
    pairs = [p for q, d in zip(queries, docs) for p in ranker.encode_pairs(q, d)]
    assert [r for rows, _ in batch_calls for r in rows] == [p[0] for p in pairs]
    assert [t for _, types in batch_calls for t in types] == [[0] * f + [1] * (len(r) - f) for r, f in pairs]
    assert all(len(r) <= 48 for r, _ in pairs) and any(len(r) == 48 for r, _ in pairs)
    # the cuts: greedy packs of at most 8192 tokens (pack_tokens' default is larger: the native cap holds)
    lens = [len(p[0]) for p in pairs]
    assert [len(rows) for rows, _ in batch_calls] == [hi - lo for lo, hi in pack_runs(lens, MAX_PACK_TOKENS)]
    assert all(sum(map(len, rows)) <= MAX_PACK_TOKENS for rows, _ in batch_calls)
    if B == 300:
        assert len(batch_calls) >= 2, "this batch is meant to be cut"
    assert len(batch_calls) < max(2, B), "one forward per pack, not per query"
    # ragged padding: one call, (B, longest list), candidates 0 .. n - 1 then -1
    (scores, cand), = seen
    assert scores.shape == cand.shape == (B, max(len(d) for d in docs))
    for b, d in enumerate(docs):
        assert cand[b].tolist() == list(range(len(d))) + [-1] * (cand.shape[1] - len(d))
    assert B == 1 or np.isnan(scores[cand >= 0]).any(), "the planted NaNs must reach the ordering"
    # the loop of rank gives the same results (NaN last, ties in input order) -- and an empty list an empty result
    for b in range(B):
        want = ranker.rank(queries[b], docs[b], ids[b])
        _same(got[b], want)
        key = [-np.inf if np.isnan(r.score) else r.score for r in want.results]
        assert key == sorted(key, reverse=True)
        if not docs[b]:
            assert got[b].results == []
    assert len(fake.calls) == sum(1 for d in docs if d)  # (the loop: one forward per query with docs)


def test_pack_tokens_below_the_cap_cuts_earlier(planted):
    ranker, fake, _ = planted
    ranker.pack_tokens = 100
    queries, docs = _batch(7, np.random.default_rng(5))
    ranker.rank_batch(queries, docs)
    assert len(fake.calls) > 1 and all(sum(map(len, rows)) <= 100 for rows, _ in fake.calls)


def test_rank_batch_refuses_mismatched_lists(planted):
    ranker, _, _ = planted
    with pytest.raises(ValueError, match="per query"):
        ranker.rank_batch(["a", "b"], [["x"]])
    with pytest.raises(ValueError, match="per query"):
        ranker.rank_batch(["a"], [["x"]], [[1], [2]])
    assert ranker.rank_batch([], []) == []
    assert [r.results for r in ranker.rank_batch(["a", "b"], [[], []])] == [[], []]


# ---- forward= validation and the fall-back ---------------------------------------------------------------------------------------------
def test_forward_is_validated_and_defaults_to_torch():
    with pytest.raises(ValueError, match="forward"):
        TorchCrossEncoderRanker(SHAPE, device="cpu", forward="hip")
    assert TorchCrossEncoderRanker(SHAPE, device="cpu").forward == "torch"
    assert NativeEncoder.supports(SHAPE, torch.bfloat16, 8, "cuda", classify=True)
    assert not NativeEncoder.supports(SHAPE, torch.bfloat16, 8, "cpu", classify=True)
    assert not NativeEncoder.supports(SHAPE, torch.float32, 8, "cuda", classify=True)
    assert NativeEncoder.supports_pack(SHAPE, torch.float16, MAX_PACK_TOKENS, "cuda", classify=True)
    assert not NativeEncoder.supports_pack(SHAPE, torch.float16, MAX_PACK_TOKENS + 1, "cuda", classify=True)
    plain = CrossEncoderShape(vocab_size=500, hidden=64, layers=1, heads=2, ffn=128, max_positions=64, n_ctx=64, classifier=False)
    assert NativeEncoder.supports(plain, torch.bfloat16, 8, "cuda") and not NativeEncoder.supports(plain, torch.bfloat16, 8, "cuda", classify=True)
    odd = CrossEncoderShape(vocab_size=500, hidden=48, layers=1, heads=1, ffn=128, max_positions=64, n_ctx=64)
    assert not NativeEncoder.supports(odd, torch.bfloat16, 8, "cuda", classify=True)


@pytest.mark.parametrize("batching", ["padded", "packed"])
def test_on_the_cpu_native_takes_the_old_route_and_makes_no_handle(monkeypatch, batching):
    def boom(*a, **kw):
        raise AssertionError("a native handle was constructed")

    monkeypatch.setattr(NativeEncoder, "__init__", boom)
    monkeypatch.setattr(_ops, "rerank_order", boom)
    native = TorchCrossEncoderRanker(SHAPE, device="cpu", forward="native", batching=batching, max_length=48)
    plain = TorchCrossEncoderRanker(SHAPE, device="cpu", batching=batching, max_length=48)
    queries, docs = _batch(7, np.random.default_rng(11))
    got = native.rank_batch(queries, docs)
    for b, (q, d) in enumerate(zip(queries, docs)):
        _same(got[b], plain.rank(q, d))
        _same(native.rank(q, d), plain.rank(q, d))
        assert torch.equal(native.logits(q, d), plain.logits(q, d))
    for z, w in zip(native.logits_batch(queries, docs), native.score_batch(queries, docs)):
        assert z.dtype == torch.float32 and w.dtype == np.float32 and len(z) == len(w)
    assert native.native is None


def test_search_entries_leave_other_rerankers_alone():
    """`_native_cross_encoder` picks ONE native cross-encoder and nothing else: a dict, a "torch" ranker and a bare `rank` object go the
    way they went."""
    from types import SimpleNamespace

    from raglite_amd import _search

    native = TorchCrossEncoderRanker(SHAPE, device="cpu", forward="native")
    plain = TorchCrossEncoderRanker(SHAPE, device="cpu")
    pick = lambda r: _search._native_cross_encoder(SimpleNamespace(reranker=r))  # noqa: E731, SLF001
    assert pick(native) is native
    assert pick(plain) is None and pick({"en": native, "other": native}) is None and pick(None) is None and pick(SimpleNamespace(rank=None)) is None
    assert _search._native_cross_encoder(SimpleNamespace()) is None  # noqa: SLF001


def test_rerank_chunks_batch_takes_a_native_cross_encoder_with_a_lookup(planted):
    from types import SimpleNamespace

    from raglite_amd import _search

    ranker, fake, _ = planted
    texts = {f"c{i}": " ".join(f"w{(7 * i + j) % 60}" for j in range(3 + i % 9)) for i in range(30)}
    lookups = []

    class Chunk:
        def __init__(self, cid):
            self.id = cid

        def __str__(self):
            return texts[self.id]

    def lookup(ids):
        lookups.append(list(ids))
        return [Chunk(i) for i in ids]

    cfg = SimpleNamespace(reranker=ranker)
    queries = ["w1 w2", "w3", "w4 w5 w6", "w7"]
    id_lists = [[f"c{i}" for i in range(0, 9)], [], [f"c{i}" for i in range(20, 30)], ["c5", "c5", "c6"]]
    got = _search.rerank_chunks_batch(queries, id_lists, config=cfg, chunk_lookup=lookup)
    assert lookups == [ids for ids in id_lists if ids], "ids are resolved once per query"
    assert len(fake.calls) == 1, "one forward for the batch"
    for q, ids, (got_ids, got_scores) in zip(queries, id_lists, got):
        want = _search.rerank_chunks(q, ids, config=cfg, chunk_lookup=lookup)
        assert got_ids == [c.id for c in want]
        res = ranker.rank(q, [texts[i] for i in ids])
        assert [np.float32(s).tobytes() for s in got_scores] == [np.float32(r.score).tobytes() for r in res.results]
    with pytest.raises(ValueError, match="chunk_lookup"):
        _search.rerank_chunks_batch(queries, id_lists, config=cfg)
    with pytest.raises(ValueError, match="per query"):
        _search.rerank_chunks_batch(queries[:2], id_lists, config=cfg, chunk_lookup=lookup)
