"""The packed encoder forward on the GPU (raglite_amd/_torch_embedder.py): fp32 through the per-sequence fallback
against the padded forward, bf16 through `attention_varlen` against an fp32 CPU run of the same weights next to the padded bf16 route,
the packed cross-encoder, and `embed_strings_batch` / `split_documents_batch(embed="batch")` against their per-document loops."""

import numpy as np
import pytest
import torch

import raglite_amd
from oracle.fake_embedder import FakeLlama, make_sentences
from raglite_amd import _chunklets
from raglite_amd._cross_encoder import CrossEncoderShape, TorchCrossEncoderRanker
from raglite_amd._torch_embedder import EncoderShape, TorchTokenEmbedder, pack_runs

pytestmark = pytest.mark.gpu

LATE = raglite_amd.HotPathConfig(embedder="llama-cpp-python/fake/packed")
TEXTS = ["".join(make_sentences(20 + i, n)) for i, n in enumerate((1, 6, 2, 11, 1, 4, 8))]  # 32 .. 368 tokens, mixed


def _shape(hidden, heads):
    return EncoderShape(vocab_size=20_000, hidden=hidden, layers=2, heads=heads, ffn=2 * hidden, max_positions=400, n_ctx=384)


def _fp32_twin(embedder, cls=TorchTokenEmbedder, **kw):
    """The same weights (the values the GPU model holds, widened) in fp32 on the CPU: only the arithmetic differs."""
    twin = cls(embedder.shape, device="cpu", dtype=torch.float32, **kw)
    twin.encoder.load_state_dict({k: v.float().cpu() for k, v in embedder.encoder.state_dict().items()})
    return twin


def test_fp32_packed_takes_the_fallback_and_equals_padded(torch_cuda):
    shape = _shape(128, 2)
    padded = TorchTokenEmbedder(shape, device="cuda", dtype=torch.float32)
    packed = TorchTokenEmbedder(shape, device="cuda", dtype=torch.float32, batching="packed", pack_tokens=300)
    for g, w in zip(packed.embed(TEXTS), padded.embed(TEXTS)):
        assert g.is_cuda and g.dtype == torch.float32
        torch.testing.assert_close(g, w, atol=2e-4, rtol=1e-4)


@pytest.mark.parametrize(("hidden", "heads"), [(128, 2), (96, 3)], ids=["head64", "head32"])
def test_bf16_packed_through_the_kernel_is_as_accurate_as_padded(torch_cuda, hidden, heads, monkeypatch):
    from raglite_amd import _abi

    shape = _shape(hidden, heads)
    padded = TorchTokenEmbedder(shape, device="cuda")
    packed = TorchTokenEmbedder(shape, device="cuda", batching="packed", pack_tokens=300)
    assert packed.dtype == torch.bfloat16
    truth = _fp32_twin(padded).embed(TEXTS)
    calls = []
    real = _abi.lib().rl_attention_varlen
    monkeypatch.setattr(_abi.lib(), "rl_attention_varlen", lambda *a: calls.append(a[2]) or real(*a))  # (n_seqs of every launch)
    got = packed.embed(TEXTS)
    packs = pack_runs([len(packed.tokenizer.encode(t)) + 2 for t in TEXTS], 300)
    assert len(packs) >= 2 and calls == [hi - lo for lo, hi in packs for _ in range(shape.layers)], calls  # every layer of every pack: the kernel
    err_packed = max(float((g.cpu() - t).abs().max()) for g, t in zip(got, truth))
    err_padded = max(float((g.cpu() - t).abs().max()) for g, t in zip(padded.embed(TEXTS), truth))
    print(f"hidden {hidden} heads {heads}: max |bf16 - fp32|  packed {err_packed:.4g}  padded {err_padded:.4g}")
    assert all(bool(torch.isfinite(g).all()) for g in got)
    assert err_packed <= 2.0 * err_padded


def test_cross_encoder_bf16_packed_against_fp32(torch_cuda):
    shape = CrossEncoderShape(vocab_size=20_000, hidden=128, layers=2, heads=4, ffn=256, max_positions=256, n_ctx=256)
    ranker = TorchCrossEncoderRanker(shape, device="cuda", batching="packed", pack_tokens=400)
    want = _fp32_twin(ranker, TorchCrossEncoderRanker).logits("which passage is about this", TEXTS)
    got = ranker.logits("which passage is about this", TEXTS).cpu()
    print(f"cross-encoder: max |bf16 packed - fp32| = {float((got - want).abs().max()):.4g}, max |fp32| = {float(want.abs().max()):.4g}")
    assert float((got - want).abs().max()) < 0.08 * (float(want.abs().max()) + 1.0)


def _documents():
    return [make_sentences(31, 30), ["A single sentence. "], make_sentences(32, 3), make_sentences(33, 5), make_sentences(34, 12)]


def test_embed_strings_batch_with_a_packed_bf16_embedder(torch_cuda):
    shape = EncoderShape(vocab_size=20_000, hidden=128, layers=2, heads=2, ffn=256, max_positions=200, n_ctx=160)
    emb = TorchTokenEmbedder(shape, device="cuda", batching="packed", pack_tokens=400)
    docs = _documents()
    truth = [raglite_amd.embed_strings(d, config=LATE, embedder=_fp32_twin(emb)) for d in docs]
    loop = [raglite_amd.embed_strings(d, config=LATE, embedder=emb) for d in docs]
    calls = emb.embed_calls
    got = raglite_amd.embed_strings_batch(docs, config=LATE, embedder=emb)
    assert emb.embed_calls - calls < calls
    err_batch = err_loop = 0.0
    for g, w, t, d in zip(got, loop, truth, docs):
        assert g.dtype == np.float16 and g.shape == (len(d), shape.hidden)
        np.testing.assert_allclose(np.linalg.norm(g.astype(np.float64), axis=1), 1.0, atol=2e-3)  # unit rows, to fp16 rounding
        err_batch = max(err_batch, float(np.abs(g.astype(np.float64) - t.astype(np.float64)).max()))
        err_loop = max(err_loop, float(np.abs(w.astype(np.float64) - t.astype(np.float64)).max()))
    print(f"embed_strings_batch (packed bf16): max error against fp32 {err_batch:.4g}; the loop of embed_strings {err_loop:.4g}")
    assert err_batch <= 2.0 * err_loop


def test_embed_strings_batch_equals_the_loop_through_the_pooling_kernel(torch_cuda):
    docs = _documents()
    loop_emb, batch_emb = FakeLlama(dim=64, n_ctx=128), FakeLlama(dim=64, n_ctx=128)
    want = [raglite_amd.embed_strings(d, config=LATE, embedder=loop_emb) for d in docs]
    got = raglite_amd.embed_strings_batch(docs, config=LATE, embedder=batch_emb)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and batch_emb.embed_calls < loop_emb.embed_calls


@pytest.fixture()
def markdown_parse(monkeypatch):
    """`markdown_chunklet_boundaries` needs markdown-it-py; where it is absent, a stand-in that marks headings and list items."""
    try:
        import markdown_it  # noqa: F401
    except ImportError:
        monkeypatch.setattr(_chunklets, "markdown_chunklet_boundaries",
                            lambda sentences: np.asarray([1.0 if s.startswith("#") else 0.25 if s.startswith("- ") else 0.0 for s in sentences]))


def test_split_documents_batch_with_batched_embedding_equals_the_loop(torch_cuda, markdown_parse):
    config = raglite_amd.HotPathConfig(embedder="llama-cpp-python/fake/packed", chunk_max_size=400)
    docs = _documents()
    loop_emb, batch_emb = FakeLlama(dim=64), FakeLlama(dim=64)
    loop = raglite_amd.split_documents_batch(docs, config=config, embedder=loop_emb)
    got = raglite_amd.split_documents_batch(docs, config=config, embedder=batch_emb, embed="batch")
    assert len(got) == len(docs) and batch_emb.embed_calls < loop_emb.embed_calls
    for (chunks, mats), (want_chunks, want_mats) in zip(got, loop):
        assert chunks == want_chunks and len(mats) == len(want_mats)
        assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(mats, want_mats))
