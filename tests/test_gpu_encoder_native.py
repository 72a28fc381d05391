"""The native encoder forward for short packs on the GPU (`rl_encoder_forward`, raglite_amd/csrc/encoder.hip).

Three forwards per case, all with the same 16-bit-rounded weights: TRUTH, the same `Encoder` module on the CPU in float64; REFERENCE,
torch's 16-bit `forward_packed` on the GPU (the route a short query took before); UNDER TEST, the native forward.  The native forward
rounds at a subset of the points where torch's route rounds, so per case its RMS error against truth must be at most 1.1 x the
reference's (the 10 % is the case-to-case scatter of an RMS over a few hundred to a few thousand elements; an indexing or lane-map
mistake gives errors of the size of the values themselves, two orders above).  Every case's two RMS values are written to
profiles/encoder_native_error.txt.  Shapes are chosen for the tile edges of the linear kernel (32-column slabs, 64-element K chunks with
a 32 tail, four waves per slab, K slices), not for the workload."""

import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

import raglite_amd
from raglite_amd import _abi
from raglite_amd._encoder import MAX_TOKENS, NativeEncoder
from raglite_amd._torch_embedder import EncoderShape, TorchTokenEmbedder, _build_encoder, packed_inputs

pytestmark = pytest.mark.gpu

CAP = MAX_TOKENS
SEVENTEEN = [2, 9, 30, 5, 17, 3, 21, 11, 2, 7, 33, 4, 19, 6, 40, 12, 2]  # 223 tokens; length 2 first, in the middle and last
PACKS = [[2], [3], [31], [32], [33], [64], [65], [CAP - 1], [CAP],  # one sequence at every token-tile edge (tiles of 32; 1, 2, 4, 8 tiles)
         [2, 40, 23], [30, 2, 32], [17, 14, 2], SEVENTEEN]           # 65, 64 and 33 tokens in three sequences; seventeen sequences


def _xlmr(hidden, heads, ffn, layers):
    return EncoderShape(vocab_size=1000, hidden=hidden, layers=layers, heads=heads, ffn=ffn, max_positions=CAP + 4, n_ctx=CAP + 2)


SHAPES = {
    "h64_f128": _xlmr(64, 2, 128, 2),      # hidden 2 x 32: one K chunk, three of four waves idle
    "h192_f320": _xlmr(192, 3, 320, 2),    # hidden 3 x 64, ffn 5 x 64: N and K no powers of two, head width 64
    "h128_f96": _xlmr(128, 4, 96, 1),      # ffn < hidden, K = 96 ends in a chunk of 32
    "h64_f512": _xlmr(64, 1, 512, 1),      # the down projection in two K slices (encoder_ksplit(64, 512) == 2)
    "bert_h64": EncoderShape(vocab_size=1000, hidden=64, layers=2, heads=2, ffn=128, max_positions=CAP, n_ctx=CAP, type_vocab=2,
                             position_offset=0, pad_id=0, bos_id=101, eos_id=102),  # type ids, positions from 0
}


class Case:
    """One (shape, dtype): the 16-bit module on the GPU, its float64 twin on the CPU, and the native forward over the former."""

    def __init__(self, shape, dtype, seed=3):
        self.shape, self.dtype = shape, dtype
        state = torch.random.get_rng_state()
        torch.manual_seed(seed)
        self.module = _build_encoder(shape).to(device="cuda", dtype=dtype).eval()
        torch.random.set_rng_state(state)
        self.twin = _build_encoder(shape).double().eval()
        self.twin.load_state_dict({k: v.double().cpu() for k, v in self.module.state_dict().items()})
        self.native = NativeEncoder(self.module, shape)

    def inputs(self, lens, seed=0):
        rng = np.random.default_rng(seed + 1000 * len(lens) + sum(lens))
        rows = [rng.integers(0, self.shape.vocab_size, size=n).tolist() for n in lens]
        types = [(rng.integers(0, 2, size=n) if self.shape.type_vocab > 1 else np.zeros(n, np.int64)).tolist() for n in lens]
        return rows, (types if self.shape.type_vocab > 1 else None)

    def three(self, rows, types):
        ids, off, lens, typ = packed_inputs(rows, "cuda", types)
        with torch.inference_mode():
            truth = self.twin.forward_packed(ids.cpu(), off.cpu(), lens, None if typ is None else typ.cpu())
            ref = self.module.forward_packed(ids, off, lens, typ)
            got = self.native.forward(ids, off, lens, typ)
        assert got.shape == ref.shape and got.dtype == self.dtype and got.is_cuda
        return truth, ref.double().cpu(), got.double().cpu()


@pytest.fixture(scope="module")
def cases(torch_cuda):
    made = {}

    def get(name, dtype):
        if (name, dtype) not in made:
            made[name, dtype] = Case(SHAPES[name], dtype)
        return made[name, dtype]

    yield get
    for c in made.values():
        c.native.close()


@pytest.fixture(scope="module")
def error_log():
    lines = []
    yield lines
    try:  # (a read-only checkout keeps the committed figures)
        out = Path(__file__).resolve().parent.parent / "profiles" / "encoder_native_error.txt"
        head = ("# tests/test_gpu_encoder_native.py: RMS error against the float64 forward of the same 16-bit weights, per case\n"
                "# shape dtype lengths | torch forward_packed (reference) | native | native / reference  (asserted <= 1.1)\n")
        out.write_text(head + "".join(sorted(lines)))
    except OSError:
        pass


def _rms(a, b):
    return float(torch.sqrt(torch.mean((a - b) ** 2)))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_native_is_as_accurate_as_the_torch_route(cases, error_log, name, dtype):
    case = cases(name, dtype)
    worse = []
    for lens in PACKS:
        truth, ref, got = case.three(*case.inputs(lens))
        assert bool(torch.isfinite(got).all())
        e_ref, e_got = _rms(ref, truth), _rms(got, truth)
        label = "+".join(map(str, lens)) if len(lens) < 17 else "17 sequences"
        line = f"{name} {str(dtype).split('.')[-1]} {label} | {e_ref:.4e} | {e_got:.4e} | {e_got / e_ref:.3f}\n"
        print(line, end="")
        error_log.append(line)
        if not e_got <= 1.1 * e_ref:
            worse.append(line)
    assert not worse, "".join(worse)


def test_the_k_split_case_splits(torch_cuda):
    """h64_f512 is in SHAPES for the two-slice down projection: make sure it still is what exercises it (the scratch says so: `part`
    holds two slices of [rows x hidden] f32 instead of one)."""
    one, two = NativeEncoder(_build_encoder(SHAPES["h64_f128"]).to("cuda", torch.bfloat16), SHAPES["h64_f128"]), None
    try:
        two = NativeEncoder(_build_encoder(SHAPES["h64_f512"]).to("cuda", torch.bfloat16), SHAPES["h64_f512"])
        fixed = lambda sh: 32 * 2 * (6 * sh.hidden + sh.ffn)  # noqa: E731 - the 16-bit buffers of 32 rows: x, x1, qkv (3), attn, mid
        assert one.info(32)["used_bytes"] - fixed(SHAPES["h64_f128"]) == 32 * 64 * 4
        assert two.info(32)["used_bytes"] - fixed(SHAPES["h64_f512"]) == 2 * 32 * 64 * 4
        assert one.info()["launches"] == 1 + 7 * 2 and one.info()["max_tokens"] == CAP
    finally:
        one.close()
        if two is not None:
            two.close()


@pytest.mark.parametrize("name", ["h192_f320", "h64_f512", "bert_h64"])
def test_same_bits_run_to_run_alone_and_anywhere_in_a_pack(cases, name):
    case = cases(name, torch.bfloat16)
    rows, types = case.inputs([30, 41, 2, 33, 64])
    types = types or [None] * len(rows)

    def run(order):
        r, t = [rows[i] for i in order], ([types[i] for i in order] if types[0] is not None else None)
        ids, off, lens, typ = packed_inputs(r, "cuda", t)
        return dict(zip(order, torch.split(case.native.forward(ids, off, lens, typ), lens)))

    full = run([0, 1, 2, 3, 4])
    again = run([0, 1, 2, 3, 4])
    moved = run([4, 3, 1, 0, 2])  # other offsets, other token tiles (MT = 8 either way), other neighbours
    for i in range(5):
        assert torch.equal(full[i], again[i]) and torch.equal(full[i], moved[i]), i
        alone = run([i])[i]  # one, two or three token tiles instead of eight
        assert torch.equal(full[i], alone), i


def test_guard_rows_behind_out_and_behind_the_scratch_in_use(cases):
    case = cases("h192_f320", torch.float16)
    lib, n, hidden = _abi.lib(), 33, 192
    rows, _ = case.inputs([20, 13])
    ids, off, lens, _ = packed_inputs(rows, "cuda")
    want = case.native.forward(ids, off, lens)
    info = case.native.info(n)
    total, used = info["scratch_bytes"], info["used_bytes"]
    assert 0 < used < case.native.info(n + 1)["used_bytes"] <= case.native.info(CAP)["used_bytes"] <= total
    torch.cuda.synchronize()
    fill = np.full(total, 0xA5, np.uint8)
    _abi.check(lib.rl_memcpy_h2d(info["scratch"], fill.ctypes.data, total, None))
    _abi.check(lib.rl_stream_sync(None))
    out = torch.full((n + 3, hidden), -7.0, dtype=torch.float16, device="cuda")
    pos = torch.tensor([t + 2 for ln in lens for t in range(ln)], dtype=torch.int32, device="cuda")
    got = case.native.forward_i32(ids.to(torch.int32), pos, off, None, 2, n, max(lens), out=out[:n])
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and torch.equal(out[:n], want)
    assert bool((out[n:] == -7.0).all()), "rows behind out were written"
    after = np.empty(total, np.uint8)
    _abi.check(lib.rl_memcpy_d2h(after.ctypes.data, info["scratch"], total, None))
    _abi.check(lib.rl_stream_sync(None))
    assert (after[used:] == 0xA5).all(), "the scratch behind this call's rows was written"
    assert (after[:used] != 0xA5).mean() > 0.9  # ... and the rows in use were (the check looks at the right block)


def test_a_side_stream(cases):
    case = cases("h64_f128", torch.bfloat16)
    rows, _ = case.inputs([19, 2, 44])
    ids, off, lens, _ = packed_inputs(rows, "cuda")
    want = case.native.forward(ids, off, lens)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = case.native.forward(ids, off, lens)
    side.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(case.native.forward(ids, off, lens), want)  # and back on the default stream


TINY = EncoderShape(vocab_size=2000, hidden=64, layers=2, heads=2, ffn=128, max_positions=CAP + 8, n_ctx=CAP + 6)


def _count_forwards(monkeypatch):
    calls = []
    real = _abi.lib().rl_encoder_forward
    monkeypatch.setattr(_abi.lib(), "rl_encoder_forward", lambda *a: calls.append(a[6]) or real(*a))  # (n_tokens of every call)
    return calls


def test_new_weights_and_a_new_dtype_are_picked_up(torch_cuda, monkeypatch):
    q = "which kernel streams the weights"
    emb = TorchTokenEmbedder(TINY, device="cuda", seed=1, short_forward="native")
    other = TorchTokenEmbedder(TINY, device="cuda", seed=2, short_forward="native")
    calls = _count_forwards(monkeypatch)
    first, second = emb.embed(q), other.embed(q)
    assert first.dtype == torch.float32 and first.is_cuda and first.shape == second.shape == (len(emb.tokenizer.encode(q)) + 2, 64)
    assert not torch.equal(first, second)
    emb.load_state_dict(other.encoder.state_dict())  # in place or not: the next call reads the new weights
    assert torch.equal(emb.embed(q), second)
    emb.encoder.to(torch.float16)                    # reallocates every parameter: another handle, another dtype
    half = TorchTokenEmbedder(TINY, device="cuda", seed=2, dtype=torch.float16, short_forward="native")
    half.load_state_dict({k: v.to(torch.float16) for k, v in other.encoder.state_dict().items()})
    got = emb.embed(q)
    assert torch.equal(got, half.embed(q)) and not torch.equal(got, second)
    assert len(calls) == 5 and len(set(calls)) == 1  # every embed() above went through the native forward


def test_the_cap_through_embed(torch_cuda, monkeypatch):
    native = TorchTokenEmbedder(TINY, device="cuda", short_forward="native")
    plain = {b: TorchTokenEmbedder(TINY, device="cuda", batching=b) for b in ("padded", "packed")}
    at_cap, over = "ab " * ((CAP - 2) // 2), " ".join(["ab"] * (CAP // 2))  # CAP - 2 and CAP - 1 tokens between <s> and </s>
    calls = _count_forwards(monkeypatch)
    assert native.embed(at_cap).shape == (CAP, 64) and calls == [CAP]
    got = native.embed(over)  # one token too many: torch's route, silently
    assert got.shape == (CAP + 1, 64) and calls == [CAP] and torch.equal(got, plain["padded"].embed(over))
    packed_native = TorchTokenEmbedder(TINY, device="cuda", batching="packed", short_forward="native")
    assert torch.equal(packed_native.embed(over), plain["packed"].embed(over)) and calls == [CAP]
    # a list goes as one pack while it fits, and as a whole by the batching route when it does not
    short = ["first query", "", "a third, longer query about kernels"]
    mats = native.embed(short)
    assert len(calls) == 2 and calls[1] == sum(len(m) for m in mats) and [len(m) for m in mats][1] == 2
    for g, alone in zip(mats, (native.embed(s) for s in short)):
        assert torch.equal(g, alone)  # a string's bits do not depend on its pack
    n_before = len(calls)
    for g, w in zip(native.embed([*short, over]), plain["padded"].embed([*short, over])):
        assert torch.equal(g, w)
    assert len(calls) == n_before


# ---- end to end at a tiny shape -------------------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _separated(rng, target, cosines):
    """Unit rows at the given cosines to `target` (a unit vector): well separated in similarity, whatever the encoder's weights are."""
    noise = rng.standard_normal((len(cosines), target.shape[0]))
    noise = _unit(noise - np.outer(noise @ target, target))
    c = np.asarray(cosines)[:, None]
    return (c * target[None, :] + np.sqrt(1 - c * c) * noise).astype(np.float32)


def test_end_to_end_text_queries_agree_with_the_torch_route(torch_cuda, monkeypatch):
    """`embed_strings([q])`, `vector_search(str)` and `MaxSimRanker.from_embedder(...).rank` with short_forward="native" against
    "torch" on an fp16 encoder.  Tolerances are those of tests/test_gpu_packed_encoder.py for two routes of one model: the error against
    the fp32 twin at most twice the other route's, unit fp16 rows to 2e-3 -- and the same ids, best first."""
    q = "Which matrix core instruction does the skinny linear layer use?"
    kw = {"device": "cuda", "dtype": torch.float16, "seed": 5}
    torch_emb, native_emb = TorchTokenEmbedder(TINY, **kw), TorchTokenEmbedder(TINY, short_forward="native", **kw)
    twin = TorchTokenEmbedder(TINY, device="cpu", dtype=torch.float32)
    twin.encoder.load_state_dict({k: v.float().cpu() for k, v in torch_emb.encoder.state_dict().items()})
    cfg = raglite_amd.HotPathConfig(vector_search_query_adapter=False)
    calls = _count_forwards(monkeypatch)
    want, got, truth = (raglite_amd.embed_strings([q], config=cfg, embedder=e) for e in (torch_emb, native_emb, twin))
    assert calls and got.dtype == np.float16 and got.shape == want.shape == (1, 64)
    err = lambda a: float(np.abs(a.astype(np.float64) - truth.astype(np.float64)).max())  # noqa: E731
    print(f"embed_strings: max error against fp32  native {err(got):.4g}  torch {err(want):.4g}")
    assert err(got) <= 2.0 * max(err(want), 2.0 ** -11)  # (the fp16 output's own rounding where torch's route happens to hit it)
    np.testing.assert_allclose(got.astype(np.float32), want.astype(np.float32), atol=2e-3)

    rng = np.random.default_rng(11)
    cosines = [0.2, 0.9, 0.5, 0.7, 0.3, 0.8, 0.4, 0.6]
    rows = _separated(rng, _unit(truth.astype(np.float64))[0], cosines)
    ids = [f"chunk-{i}" for i in range(len(cosines))]
    docs = [f"the text of chunk {i}" for i in range(len(cosines))]
    tok = _unit(twin.embed(q).numpy().astype(np.float64))[:32]  # (MaxSimRanker keeps the first 32 token vectors)
    assert len(tok) < 64
    apart = np.linalg.svd(tok)[2][-1]  # a unit vector orthogonal to every query token vector
    # vector search: one row per chunk at a known cosine to the query.  Rerank: chunk i holds, per query token t, the unit row
    # c_i t + sqrt(1 - c_i^2) apart, so its MaxSim score is c_i per token: chunks 0.1 x tokens apart
    gi = raglite_amd.GpuIndex(ids, [r[None, :] for r in rows], docs=docs)
    gi_tokens = raglite_amd.GpuIndex(ids, [(c * tok + np.sqrt(1 - c * c) * apart[None, :]).astype(np.float32) for c in cosines], docs=docs)
    try:
        results = {}
        for name, e in (("torch", torch_emb), ("native", native_emb)):
            raglite_amd.set_embedder_factory(lambda config, e=e: e)
            n_calls = len(calls)
            results[name] = raglite_amd.vector_search(q, num_results=5, config=cfg, index=gi)
            assert (len(calls) > n_calls) == (name == "native")
        best = [ids[i] for i in np.argsort(-np.asarray(cosines))[:5]]
        assert results["native"][0] == results["torch"][0] == best
        np.testing.assert_allclose(results["native"][1], results["torch"][1], atol=2e-3)
        ranked = {}
        for name, e in (("torch", torch_emb), ("native", native_emb)):
            ranker = raglite_amd.MaxSimRanker.from_embedder(gi_tokens, e)
            ranked[name] = ranker.rank(q, docs).results
        order = lambda r: [x.doc_id for x in r]  # noqa: E731
        assert order(ranked["native"]) == order(ranked["torch"]) == np.argsort(-np.asarray(cosines)).tolist()
        np.testing.assert_allclose([x.score for x in ranked["native"]], [x.score for x in ranked["torch"]], atol=2e-3 * len(tok))
    finally:
        raglite_amd.set_embedder_factory(None)
        gi.close()
        gi_tokens.close()
