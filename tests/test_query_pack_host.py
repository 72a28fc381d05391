"""The packed native forward for a batch of text queries (`rl_encoder_forward_pack`, `rl_encoder_pack_workspace_bytes`,
`rl_encoder_linear_pack`, `rl_adapter_apply_rows`) without a GPU: every argument check of the new entries returns
before the first HIP call with its code and message, the handle last; and the Python routing -- which batches go through ONE
`embed_pack` call and which embed one by one exactly as before.  `rl_pool_norm` needs a device, so the routing tests put a NumPy
stand-in in its place: what is under test here is who gets called with what, not the pooling.

`rl_encoder_create` allocates the handle's scratch, so a handle exists only where there is a GPU: the one test that needs one (the
workspace size against the handle's own scratch) is marked `gpu`."""

import ctypes as C
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import raglite_amd
from raglite_amd import _abi, _embed, _ops, _search
from raglite_amd._encoder import MAX_PACK_TOKENS, MAX_TOKENS, NativeEncoder
from raglite_amd._torch_embedder import EncoderShape, TorchTokenEmbedder

INVALID, UNSUPPORTED = _abi.RL_ERR_INVALID, _abi.RL_ERR_UNSUPPORTED
BF16, F16 = _abi.ATTN_DTYPES["bfloat16"], _abi.ATTN_DTYPES["float16"]
EPI = _abi.ENCODER_EPILOGUES
P = 4096  # a non-null, 16-byte aligned "device pointer": no check dereferences it, and every call here fails before the first HIP call


# ---- the C entries ---------------------------------------------------------------------------------------------------------------------
def _forward_pack(enc=None, ids=P, positions=P, type_ids=None, seq_offsets=P, n_seqs=1, n_tokens=300, max_len=8, out=P, workspace=P,
                  workspace_bytes=1 << 30, mem=_abi.MEM_DEVICE):
    st = _abi.lib().rl_encoder_forward_pack(enc, ids, positions, type_ids, seq_offsets, n_seqs, n_tokens, max_len, out, workspace, workspace_bytes,
                                            mem, None)
    return st, _abi.last_error()


@pytest.mark.parametrize(("kw", "code", "text"), [
    ({"mem": _abi.MEM_HOST}, UNSUPPORTED, "device pointers only"),
    ({"n_seqs": -1}, INVALID, "negative size"),
    ({"n_tokens": -1}, INVALID, "negative size"),
    ({"max_len": -1}, INVALID, "negative size"),
    ({"n_seqs": 65536}, INVALID, "n_seqs must be <= 65535"),
    ({"n_tokens": MAX_PACK_TOKENS + 1}, UNSUPPORTED, "n_tokens must be <= RL_ENCODER_MAX_PACK_TOKENS (8192)"),
    ({"ids": None}, INVALID, "null argument"),
    ({"positions": None}, INVALID, "null argument"),
    ({"seq_offsets": None}, INVALID, "null argument"),
    ({"out": None}, INVALID, "null argument"),
    ({"ids": P + 2}, INVALID, "aligned"),
    ({"positions": P + 1}, INVALID, "aligned"),
    ({"type_ids": P + 2}, INVALID, "aligned"),
    ({"seq_offsets": P + 3}, INVALID, "aligned"),
    ({"out": P + 8}, INVALID, "aligned"),
    ({"workspace": None}, INVALID, "workspace is null"),
    ({"workspace": P + 8}, INVALID, "workspace must be 16-byte aligned"),
    ({}, INVALID, "null handle"),                               # everything else in order: the handle is looked at last
    ({"n_tokens": MAX_PACK_TOKENS}, INVALID, "null handle"),    # the cap itself is inside
    ({"n_tokens": MAX_TOKENS}, INVALID, "null handle"),
    ({"n_tokens": 0, "ids": None, "out": None, "workspace": None, "workspace_bytes": 0}, INVALID, "null handle"),
    ({"workspace_bytes": 0}, INVALID, "null handle"),           # (a workspace's size is measured against the handle's shape: after it)
    ({"workspace_bytes": -1}, INVALID, "null handle"),
])
def test_forward_pack_refuses_before_the_first_hip_call(kw, code, text):
    st, msg = _forward_pack(**kw)
    assert st == code and msg.startswith("rl_encoder_forward_pack:") and text in msg, (st, msg)


def test_forward_pack_checks_in_the_order_of_forward():
    """Two faults at once: the earlier check speaks -- the order is rl_encoder_forward's, the workspace behind it."""
    for kw, text in (({"mem": _abi.MEM_HOST, "n_tokens": -1}, "device pointers only"), ({"n_tokens": -1, "n_seqs": 65536}, "negative size"),
                     ({"n_seqs": 65536, "n_tokens": MAX_PACK_TOKENS + 1}, "n_seqs must be"), ({"n_tokens": MAX_PACK_TOKENS + 1, "ids": None}, "n_tokens must be"),
                     ({"ids": None, "out": P + 8}, "null argument"), ({"out": P + 8, "workspace": None}, "aligned"),
                     ({"workspace": None}, "workspace is null")):
        st, msg = _forward_pack(**kw)
        assert st in (INVALID, UNSUPPORTED) and text in msg, (kw, msg)


def test_workspace_bytes_refuses():
    n = C.c_int64(-7)
    lib = _abi.lib()
    for tokens, out, text in ((-1, True, "n_tokens must be in [0, RL_ENCODER_MAX_PACK_TOKENS]"), (MAX_PACK_TOKENS + 1, True, "n_tokens must be in"),
                              (16, False, "bytes is null"), (16, True, "null handle"), (0, True, "null handle"), (MAX_PACK_TOKENS, True, "null handle")):
        st = lib.rl_encoder_pack_workspace_bytes(None, tokens, C.byref(n) if out else None)
        msg = _abi.last_error()
        assert st == INVALID and msg.startswith("rl_encoder_pack_workspace_bytes:") and text in msg and n.value == -7, (tokens, msg)


def _linear_pack(x=P, M=300, K=64, W=P, N=64, bias=P, epilogue=EPI["bias"], dtype=BF16, out16=P, part=None, mem=_abi.MEM_DEVICE):  # noqa: N803
    st = _abi.lib().rl_encoder_linear_pack(x, M, K, W, N, bias, epilogue, dtype, out16, part, mem, None)
    return st, _abi.last_error()


PARTIAL = {"epilogue": EPI["partial"], "out16": None, "part": P, "bias": None}


@pytest.mark.parametrize(("kw", "code", "text"), [
    ({"mem": _abi.MEM_HOST}, UNSUPPORTED, "device pointers only"),
    ({"M": -1}, INVALID, "M must be in [0, RL_ENCODER_MAX_PACK_TOKENS]"),
    ({"M": MAX_PACK_TOKENS + 1}, INVALID, "M must be in [0, RL_ENCODER_MAX_PACK_TOKENS]"),
    ({"K": 0}, INVALID, "positive multiples of 32"),
    ({"K": 80}, INVALID, "positive multiples of 32"),
    ({"N": 16}, INVALID, "positive multiples of 32"),
    ({"N": 65}, INVALID, "positive multiples of 32"),
    ({"dtype": 2}, INVALID, "unknown dtype"),
    ({"epilogue": 3}, INVALID, "unknown epilogue"),
    ({"epilogue": -1}, INVALID, "unknown epilogue"),
    ({"x": None}, INVALID, "null argument"),
    ({"W": None}, INVALID, "null argument"),
    ({"bias": None}, INVALID, "read bias, which is null"),
    ({"epilogue": EPI["gelu"], "bias": None}, INVALID, "read bias, which is null"),
    ({"out16": None}, INVALID, "write out16, which is null"),
    ({"out16": None, "part": P}, INVALID, "write out16, which is null"),
    ({**PARTIAL, "part": None}, INVALID, "writes part, which is null"),
    ({**PARTIAL, "part": None, "out16": P}, INVALID, "writes part, which is null"),
    ({"x": P + 8}, INVALID, "16-byte aligned"),
    ({"W": P + 8}, INVALID, "16-byte aligned"),
    ({**PARTIAL, "part": P + 8}, INVALID, "16-byte aligned"),
    ({"bias": P + 4}, INVALID, "8-byte aligned"),
    ({"out16": P + 2}, INVALID, "8-byte aligned"),
    ({"epilogue": EPI["gelu"], "dtype": F16, "out16": P + 4}, INVALID, "8-byte aligned"),
])
def test_linear_pack_refuses_before_the_first_hip_call(kw, code, text):
    st, msg = _linear_pack(**kw)
    assert st == code and msg.startswith("rl_encoder_linear_pack:") and text in msg, (st, msg)


def test_zero_rows_are_a_no_op():
    assert _linear_pack(M=0, x=None, out16=None)[0] == _abi.RL_OK
    assert _linear_pack(M=0, K=48)[0] == INVALID  # ... but not before the sizes are looked at


def test_adapter_apply_rows_refuses():
    lib = _abi.lib()
    for args, text in (((P, P, 1, 0, P, None), "bad size"), ((P, P, -1, 8, P, None), "bad size"), ((None, P, 1, 8, P, None), "null input"),
                       ((P, None, 1, 8, P, None), "null input"), ((P, P, 1, 8, None, None), "no output requested")):
        assert lib.rl_adapter_apply_rows(*args, _abi.MEM_HOST, None) == INVALID
        assert _abi.last_error() == f"rl_adapter_apply_rows: {text}"
    assert lib.rl_adapter_apply_rows(P, None, 0, 8, P, None, _abi.MEM_HOST, None) == _abi.RL_OK  # no queries: nothing to do


def test_the_caps_are_the_header_constants():
    header = (Path(__file__).resolve().parent.parent / "include" / "raglite_hip.h").read_text()
    assert int(re.search(r"#define RL_ENCODER_MAX_PACK_TOKENS (\d+)", header).group(1)) == MAX_PACK_TOKENS == _abi.ENCODER_MAX_PACK_TOKENS == 8192
    assert int(re.search(r"#define RL_ENCODER_MAX_TOKENS (\d+)", header).group(1)) == MAX_TOKENS == 256  # the old cap stays
    assert MAX_PACK_TOKENS % MAX_TOKENS == 0


@pytest.mark.gpu
def test_workspace_bytes_is_monotone_and_meets_the_handle_at_the_cap(torch_cuda):
    shape = EncoderShape(vocab_size=300, hidden=64, layers=1, heads=2, ffn=512, max_positions=80, n_ctx=64)  # two K slices in `part`
    emb = TorchTokenEmbedder(shape, device="cuda")
    native = NativeEncoder(emb.encoder, shape)
    try:
        sizes = [native.workspace_bytes(n) for n in (0, 1, 2, 31, 32, 255, 256, 257, 512, 1000, MAX_PACK_TOKENS)]
        assert sizes[0] == 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
        info = native.info(33)
        assert native.workspace_bytes(MAX_TOKENS) == info["scratch_bytes"] and native.workspace_bytes(33) == info["used_bytes"]
        with pytest.raises(ValueError, match="rl_encoder_pack_workspace_bytes: n_tokens must be in"):
            native.workspace_bytes(MAX_PACK_TOKENS + 1)
    finally:
        native.close()


def test_supports_pack():
    shape = EncoderShape(vocab_size=500, hidden=64, layers=1, heads=2, ffn=128, max_positions=80, n_ctx=64)
    assert NativeEncoder.supports_pack(shape, torch.bfloat16, 1) and NativeEncoder.supports_pack(shape, torch.float16, MAX_PACK_TOKENS)
    assert NativeEncoder.supports_pack(shape, torch.bfloat16, MAX_TOKENS + 1, device="cuda:0")
    assert not NativeEncoder.supports_pack(shape, torch.bfloat16, 0) and not NativeEncoder.supports_pack(shape, torch.bfloat16, MAX_PACK_TOKENS + 1)
    assert not NativeEncoder.supports_pack(shape, torch.bfloat16, 300, device="cpu") and not NativeEncoder.supports_pack(shape, torch.float32, 300)
    assert not NativeEncoder.supports_pack(EncoderShape(hidden=64, heads=4, ffn=128), torch.bfloat16, 300)  # head width 16
    assert not NativeEncoder.supports(shape, torch.bfloat16, MAX_TOKENS + 1)  # (`embed()`'s own cap is where it was)


# ---- routing ---------------------------------------------------------------------------------------------------------------------------
DIM = 8


def _numpy_pool_norm(tokens, span_begin, span_end, *, normalize=True, eps=0.0, want_f32=False, want_f16=True):  # noqa: ARG001
    """What `rl_pool_norm` computes, for a host without a device (float64 mean, optional L2 normalisation, one fp16 rounding)."""
    tok = np.asarray(tokens, dtype=np.float64)
    out = np.stack([tok[int(b):int(e)].mean(axis=0) for b, e in zip(np.asarray(span_begin), np.asarray(span_end))])
    if normalize:
        out = out / np.linalg.norm(out, axis=1, keepdims=True)
    return None, out.astype(np.float16)


def _rows_of(text):
    """A deterministic (len(text.split()) + 2, DIM) float32 token matrix per text."""
    rng = np.random.default_rng(sum(text.encode()))
    return rng.standard_normal((len(text.split()) + 2, DIM)).astype(np.float32)


class StubEmbedder:
    """The llama-like surface `_embed.py` touches, with every `embed` and `embed_pack` call recorded."""

    n_batch = 512

    def __init__(self, pack="yes"):
        self.calls, self.pack = [], pack
        if pack != "absent":
            self.embed_pack = self._embed_pack

    def n_ctx(self):
        return 512

    def tokenize(self, data, add_bos=True, special=False):  # noqa: ARG002, FBT002
        return [0] * int(add_bos) + [1000 if w == _embed.SENTINEL else 7 for w in data.decode().replace(_embed.SENTINEL, f" {_embed.SENTINEL} ").split()]

    def detokenize(self, tokens):
        return " ".join(_embed.SENTINEL if t == 1000 else "w" for t in tokens).encode()

    def embed(self, text):
        self.calls.append(("embed", text))
        return _rows_of(text) if isinstance(text, str) else [_rows_of(t) for t in text]

    def _embed_pack(self, texts):
        self.calls.append(("embed_pack", list(texts)))
        return None if self.pack == "none" else [_rows_of(t) for t in texts]


QUERIES = ["which kernel streams the weights", "a second query", "one", "the fourth query of the batch is longer than the rest"]
GI = SimpleNamespace(query_adapter=None)  # what `_embed_queries` reads of the index


@pytest.fixture
def host_pool(monkeypatch):
    monkeypatch.setattr(_ops, "pool_norm", _numpy_pool_norm)
    yield
    raglite_amd.set_embedder_factory(None)


def _cfg(stub):
    raglite_amd.set_embedder_factory(lambda config: stub)
    return raglite_amd.HotPathConfig(vector_search_query_adapter=False)


def test_strings_go_through_one_embed_pack_call(host_pool):
    stub, loop = StubEmbedder(), StubEmbedder("absent")
    got = _search._embed_queries(QUERIES, None, _cfg(stub), GI)  # noqa: SLF001
    assert stub.calls == [("embed_pack", QUERIES)]  # one call, every string, in order -- and no embed()
    want = _search._embed_one_by_one(QUERIES, None, _cfg(loop), GI)  # noqa: SLF001
    assert loop.calls == [("embed", q) for q in QUERIES]
    assert got.dtype == np.float32 and got.shape == (len(QUERIES), DIM) and np.array_equal(got, want)
    one = StubEmbedder()
    assert np.array_equal(_search._embed_queries(QUERIES[:1], None, _cfg(one), GI), want[:1]) and one.calls == [("embed_pack", QUERIES[:1])]  # noqa: SLF001


def test_mixed_lists_keep_their_vectors(host_pool):
    rng = np.random.default_rng(2)
    v1, v3 = rng.standard_normal(DIM).astype(np.float32), rng.standard_normal(DIM).astype(np.float16)
    mixed = [QUERIES[0], v1, QUERIES[1], v3, QUERIES[2]]
    stub, loop = StubEmbedder(), StubEmbedder("absent")
    got = _search._embed_queries(mixed, None, _cfg(stub), GI)  # noqa: SLF001
    assert stub.calls == [("embed_pack", [QUERIES[0], QUERIES[1], QUERIES[2]])]
    want = _search._embed_one_by_one(mixed, None, _cfg(loop), GI)  # noqa: SLF001
    assert np.array_equal(got, want) and np.array_equal(got[1], v1) and np.array_equal(got[3], v3.astype(np.float32))


@pytest.mark.parametrize("pack", ["none", "absent"])
def test_without_a_pack_route_the_calls_are_the_loops(host_pool, pack):
    stub, loop = StubEmbedder(pack), StubEmbedder("absent")
    got = _search._embed_queries(QUERIES, None, _cfg(stub), GI)  # noqa: SLF001
    asked = [("embed_pack", QUERIES)] if pack == "none" else []
    assert stub.calls == asked + [("embed", q) for q in QUERIES]
    assert np.array_equal(got, _search._embed_one_by_one(QUERIES, None, _cfg(loop), GI))  # noqa: SLF001


def test_query_vectors_and_raw_vectors_touch_no_embedder(host_pool):
    stub = StubEmbedder()
    cfg = _cfg(stub)
    qv = np.random.default_rng(3).standard_normal((len(QUERIES), DIM)).astype(np.float32)
    assert np.array_equal(_search._embed_queries(QUERIES, qv, cfg, GI), qv)  # noqa: SLF001
    assert np.array_equal(_search._embed_queries(list(qv), None, cfg, GI), qv)  # noqa: SLF001
    assert np.array_equal(_search._embed_queries(QUERIES, torch.as_tensor(qv), cfg, GI), qv)  # noqa: SLF001
    assert stub.calls == []
    with pytest.raises(ValueError, match="query_vectors must be"):
        _search._embed_queries(QUERIES, qv[:2], cfg, GI)  # noqa: SLF001


def test_strings_the_loop_would_refuse_go_to_the_loop(host_pool):
    """The sentinel inside a query, an empty query, a query of no tokens: `embed_strings([q])` has its own say on those (it raises, or
    apportions token rows over a count of zero), and the batch must say the same, so such a batch is the loop's."""
    stub = StubEmbedder()
    with pytest.raises(AssertionError, match="appears in document"):
        _search._embed_queries([QUERIES[0], f"a {_embed.SENTINEL} b"], None, _cfg(stub), GI)  # noqa: SLF001
    assert stub.calls == [("embed", QUERIES[0]), ]  # (the loop got as far as the second query's token count; no pack was asked for)
    for bad in ("", "   "):  # "   ": the stub's tokenizer finds no token in it, and says so only once asked
        stub, loop = StubEmbedder(), StubEmbedder("absent")
        with np.errstate(all="ignore"):
            got = _search._embed_queries([QUERIES[0], bad], None, _cfg(stub), GI)  # noqa: SLF001
            want = _search._embed_one_by_one([QUERIES[0], bad], None, _cfg(loop), GI)  # noqa: SLF001
        assert [c for c in stub.calls if c[0] == "embed"] == loop.calls == [("embed", QUERIES[0]), ("embed", bad)]
        assert np.array_equal(got, want, equal_nan=True)


def test_a_standard_embedder_is_not_asked_for_a_pack(host_pool):
    class Api(StubEmbedder):
        def __call__(self, strings):
            self.calls.append(("api", list(strings)))
            return np.stack([_rows_of(s)[0] for s in strings])

    stub = Api()
    raglite_amd.set_embedder_factory(lambda config: stub)
    cfg = raglite_amd.HotPathConfig(embedder="text-embedding-3-large", vector_search_query_adapter=False)
    got = _search._embed_queries(QUERIES[:2], None, cfg, GI)  # noqa: SLF001
    assert stub.calls == [("api", [q]) for q in QUERIES[:2]] and got.shape == (2, DIM)


@pytest.mark.parametrize("short_forward", ["torch", "native"])
def test_a_real_embedder_on_the_cpu_embeds_one_by_one(host_pool, short_forward):
    # (a vocabulary large enough that the hashing tokenizer's ids do not depend on the order in which it meets the pieces)
    shape = EncoderShape(vocab_size=100_003, hidden=64, layers=1, heads=2, ffn=128, max_positions=80, n_ctx=64)
    emb = TorchTokenEmbedder(shape, device="cpu", short_forward=short_forward)
    assert emb.embed_pack(QUERIES) is None and emb.embed_calls == 0 and emb._native is None  # noqa: SLF001 - a CPU has no pack route
    seen = []
    real = emb.embed
    emb.embed = lambda text: seen.append(text) or real(text)
    got = _search._embed_queries(QUERIES, None, _cfg(emb), GI)  # noqa: SLF001
    assert seen == QUERIES and emb.embed_calls == len(QUERIES)
    plain = TorchTokenEmbedder(shape, device="cpu")
    want = _search._embed_one_by_one(QUERIES, None, _cfg(plain), GI)  # noqa: SLF001
    assert got.shape == (len(QUERIES), 64) and np.array_equal(got, want)


def test_the_ranker_asks_for_one_pack_and_applies_encodes_lines(host_pool):
    stub, loop = StubEmbedder(), StubEmbedder("absent")
    packed = _search.MaxSimRanker.from_embedder(None, stub, max_vectors=4)
    single = _search.MaxSimRanker.from_embedder(None, loop, max_vectors=4)
    got, want = packed._token_vectors(QUERIES), single._token_vectors(QUERIES)  # noqa: SLF001
    assert stub.calls == [("embed_pack", QUERIES)] and loop.calls == [("embed", q) for q in QUERIES]
    assert [g.shape for g in got] == [(min(len(q.split()) + 2, 4), DIM) for q in QUERIES]
    assert all(g.dtype == np.float32 and np.array_equal(g, w) for g, w in zip(got, want))
    # given vectors skip both; a None from embed_pack falls back to the loop
    given = [w + 1 for w in want]
    assert all(np.array_equal(g, w) for g, w in zip(packed._token_vectors(QUERIES, given), given)) and len(stub.calls) == 1  # noqa: SLF001
    none = StubEmbedder("none")
    fell = _search.MaxSimRanker.from_embedder(None, none, max_vectors=4)._token_vectors(QUERIES)  # noqa: SLF001
    assert none.calls == [("embed_pack", QUERIES)] + [("embed", q) for q in QUERIES] and all(np.array_equal(g, w) for g, w in zip(fell, want))
    # a ranker made from a plain callable has no batch encoder
    plain = _search.MaxSimRanker(None, lambda q: _rows_of(q))
    assert plain.query_batch_encoder is None and np.array_equal(plain._token_vectors(QUERIES[:1])[0], _rows_of(QUERIES[0]))  # noqa: SLF001


def test_one_pack_serves_both_sides_when_the_embedder_is_shared(host_pool):
    stub = StubEmbedder()
    cfg = _cfg(stub)
    ranker = _search.MaxSimRanker.from_embedder(None, stub)
    pack, mats = _search._shared_pack(cfg, ranker, QUERIES, None, None)  # noqa: SLF001
    assert stub.calls == [("embed_pack", QUERIES)] and pack[0] == list(range(len(QUERIES))) and mats is pack[1]
    Q = _search._embed_queries(QUERIES, None, cfg, GI, pack)  # noqa: N806, SLF001
    vecs = ranker._token_vectors(QUERIES, None, mats)  # noqa: SLF001
    assert len(stub.calls) == 1  # neither side embedded again
    loop = StubEmbedder("absent")
    assert np.array_equal(Q, _search._embed_one_by_one(QUERIES, None, _cfg(loop), GI))  # noqa: SLF001
    want = _search.MaxSimRanker.from_embedder(None, loop)._token_vectors(QUERIES)  # noqa: SLF001
    assert all(np.array_equal(g, w) for g, w in zip(vecs, want))
    # another embedder behind the ranker, given vectors on either side, or a raw vector among the queries: each side for itself
    other = _search.MaxSimRanker.from_embedder(None, StubEmbedder())
    _cfg(stub)
    for args in ((cfg, other, QUERIES, None, None), (cfg, ranker, QUERIES, np.zeros((4, DIM), np.float32), None), (cfg, ranker, QUERIES, None, [None] * 4),
                 (cfg, ranker, [*QUERIES[:3], np.zeros(DIM, np.float32)], None, None)):
        assert _search._shared_pack(*args) == (None, None)  # noqa: SLF001
