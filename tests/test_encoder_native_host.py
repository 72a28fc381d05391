"""The native encoder forward (`rl_encoder_*`, raglite_amd/_encoder.py) without a GPU: every argument check of the four
entry points returns before the first HIP call with its code and message, the Python route switch, and the CPU fall-through."""

import ctypes as C
import re
from pathlib import Path

import pytest
import torch

from raglite_amd import _abi
from raglite_amd._encoder import MAX_TOKENS, NativeEncoder
from raglite_amd._torch_embedder import EncoderShape, TorchTokenEmbedder

INVALID, UNSUPPORTED = _abi.RL_ERR_INVALID, _abi.RL_ERR_UNSUPPORTED
BF16 = _abi.ATTN_DTYPES["bfloat16"]
P = 4096  # a non-null, 16-byte aligned "device pointer": no check dereferences it, and every call here fails before the first HIP call


def _create(vocab=100, hidden=64, layers=2, heads=2, ffn=128, max_positions=40, type_vocab=1, eps=1e-5, dtype=BF16, tok=P, pos=P, typ=P, ln_w=P,
            ln_b=P, layer_params="aligned", out=True):
    h = C.c_void_p(7)
    if layer_params == "aligned":
        layer_params = (C.c_void_p * (12 * max(layers, 1)))(*([P] * (12 * max(layers, 1))))
    st = _abi.lib().rl_encoder_create(C.byref(h) if out else None, vocab, hidden, layers, heads, ffn, max_positions, type_vocab, eps, dtype, tok, pos,
                                      typ, ln_w, ln_b, layer_params)
    assert not out or not h.value  # no handle comes back from a refused call
    return st, _abi.last_error()


def _layers_with(i, value):
    a = (C.c_void_p * 24)(*([P] * 24))
    a[i] = value
    return a


@pytest.mark.parametrize(("kw", "code", "text"), [
    ({"out": False}, INVALID, "out is null"),
    ({"vocab": 0}, INVALID, "every size must be >= 1"),
    ({"hidden": 0}, INVALID, "every size must be >= 1"),
    ({"layers": 0}, INVALID, "every size must be >= 1"),
    ({"heads": 0}, INVALID, "every size must be >= 1"),
    ({"ffn": -32}, INVALID, "every size must be >= 1"),
    ({"max_positions": 0}, INVALID, "every size must be >= 1"),
    ({"type_vocab": 0}, INVALID, "every size must be >= 1"),
    ({"hidden": 64, "heads": 3}, INVALID, "multiple of heads"),
    ({"eps": float("nan")}, INVALID, "eps must be finite"),
    ({"eps": float("inf")}, INVALID, "eps must be finite"),
    ({"eps": -1e-5}, INVALID, "eps must be finite"),
    ({"dtype": 2}, INVALID, "unknown dtype"),
    ({"hidden": 65536 * 2, "heads": 65536}, INVALID, "heads must be <= 65535"),
    ({"hidden": 64, "heads": 4}, UNSUPPORTED, "head width must be 32 or 64"),   # 16
    ({"hidden": 256, "heads": 2}, UNSUPPORTED, "head width must be 32 or 64"),  # 128
    ({"ffn": 100}, UNSUPPORTED, "multiples of 32"),
    ({"hidden": 16384, "heads": 256, "ffn": 64}, UNSUPPORTED, "hidden must be <= 8192"),
    ({"ffn": 32768 + 32}, UNSUPPORTED, "ffn <= 32768"),
    ({"tok": None}, INVALID, "null argument"),
    ({"pos": None}, INVALID, "null argument"),
    ({"typ": None}, INVALID, "null argument"),
    ({"ln_w": None}, INVALID, "null argument"),
    ({"ln_b": None}, INVALID, "null argument"),
    ({"layer_params": None}, INVALID, "null argument"),
    ({"tok": P + 8}, INVALID, "layer norm must be 16-byte aligned"),
    ({"ln_b": P + 2}, INVALID, "layer norm must be 16-byte aligned"),
    ({"layer_params": _layers_with(13, None)}, INVALID, "null layer parameter"),
    ({"layer_params": _layers_with(23, P + 8)}, INVALID, "16-byte aligned"),
])
def test_create_refuses_before_the_first_hip_call(kw, code, text):
    st, msg = _create(**kw)
    assert st == code and msg.startswith("rl_encoder_create:") and text in msg, (st, msg)


def _forward(enc=None, ids=P, positions=P, type_ids=None, seq_offsets=P, n_seqs=1, n_tokens=8, max_len=8, out=P, mem=_abi.MEM_DEVICE):
    st = _abi.lib().rl_encoder_forward(enc, ids, positions, type_ids, seq_offsets, n_seqs, n_tokens, max_len, out, mem, None)
    return st, _abi.last_error()


@pytest.mark.parametrize(("kw", "code", "text"), [
    ({"mem": _abi.MEM_HOST}, UNSUPPORTED, "device pointers only"),
    ({"n_seqs": -1}, INVALID, "negative size"),
    ({"n_tokens": -1}, INVALID, "negative size"),
    ({"max_len": -1}, INVALID, "negative size"),
    ({"n_seqs": 65536}, INVALID, "n_seqs must be <= 65535"),
    ({"n_tokens": MAX_TOKENS + 1}, UNSUPPORTED, "n_tokens must be <= RL_ENCODER_MAX_TOKENS"),
    ({"ids": None}, INVALID, "null argument"),
    ({"positions": None}, INVALID, "null argument"),
    ({"seq_offsets": None}, INVALID, "null argument"),
    ({"out": None}, INVALID, "null argument"),
    ({"ids": P + 2}, INVALID, "aligned"),
    ({"positions": P + 1}, INVALID, "aligned"),
    ({"type_ids": P + 2}, INVALID, "aligned"),
    ({"seq_offsets": P + 3}, INVALID, "aligned"),
    ({"out": P + 8}, INVALID, "aligned"),
    ({}, INVALID, "null handle"),                    # everything else in order: the handle is looked at last
    ({"n_tokens": MAX_TOKENS}, INVALID, "null handle"),  # the cap itself is inside
    ({"n_tokens": 0, "ids": None, "out": None}, INVALID, "null handle"),
])
def test_forward_refuses_before_the_first_hip_call(kw, code, text):
    st, msg = _forward(**kw)
    assert st == code and msg.startswith("rl_encoder_forward:") and text in msg, (st, msg)


def test_info_and_destroy_without_a_handle():
    lib = _abi.lib()
    cap = C.c_int32(-1)
    assert lib.rl_encoder_info(None, 0, C.byref(cap), None, None, None, None) == INVALID
    assert _abi.last_error() == "rl_encoder_info: null handle" and cap.value == -1
    for n in (-1, MAX_TOKENS + 1):
        assert lib.rl_encoder_info(None, n, None, None, None, None, None) == INVALID
        assert _abi.last_error().startswith("rl_encoder_info: n_tokens must be in")
    assert lib.rl_encoder_destroy(None) == _abi.RL_OK  # like free(NULL)


def test_the_cap_is_the_header_constant():
    header = (Path(__file__).resolve().parent.parent / "include" / "raglite_hip.h").read_text()
    assert int(re.search(r"#define RL_ENCODER_MAX_TOKENS (\d+)", header).group(1)) == MAX_TOKENS == _abi.ENCODER_MAX_TOKENS
    assert MAX_TOKENS >= 128


SHAPE = EncoderShape(vocab_size=500, hidden=64, layers=1, heads=2, ffn=128, max_positions=80, n_ctx=64)


def test_short_forward_rejects_unknown_values():
    with pytest.raises(ValueError, match='short_forward must be "torch" or "native"'):
        TorchTokenEmbedder(SHAPE, device="cpu", short_forward="hip")
    assert TorchTokenEmbedder(SHAPE, device="cpu").short_forward == "torch"  # the default


def test_supports():
    ok = (SHAPE, torch.bfloat16, 16)
    assert NativeEncoder.supports(*ok) and NativeEncoder.supports(SHAPE, torch.float16, MAX_TOKENS) and NativeEncoder.supports(SHAPE, torch.bfloat16, 1)
    assert NativeEncoder.supports(*ok, device="cuda:0")
    assert not NativeEncoder.supports(*ok, device="cpu")
    assert not NativeEncoder.supports(SHAPE, torch.float32, 16)
    assert not NativeEncoder.supports(SHAPE, torch.bfloat16, MAX_TOKENS + 1)
    assert not NativeEncoder.supports(SHAPE, torch.bfloat16, 0)
    for bad in (EncoderShape(hidden=64, heads=4, ffn=128), EncoderShape(hidden=256, heads=2, ffn=512), EncoderShape(hidden=64, heads=2, ffn=100),
                EncoderShape(hidden=96, heads=2, ffn=128), EncoderShape(hidden=16384, heads=256, ffn=4096), EncoderShape(hidden=64, heads=2, ffn=65536)):
        assert not NativeEncoder.supports(bad, torch.bfloat16, 16), bad  # head 16, head 128, ffn % 32, head 48, hidden and ffn over their limits


@pytest.mark.parametrize("batching", ["padded", "packed"])
def test_native_on_the_cpu_gives_the_bits_of_torch(batching):
    texts = ["a short query", "", "another one, a little longer than the first"]
    plain = TorchTokenEmbedder(SHAPE, device="cpu", batching=batching)
    native = TorchTokenEmbedder(SHAPE, device="cpu", batching=batching, short_forward="native")
    for g, w in zip(native.embed(texts), plain.embed(texts)):
        assert g.dtype == torch.float32 and torch.equal(g, w)
    assert torch.equal(native.embed(texts[0]), plain.embed(texts[0])) and native._native is None  # noqa: SLF001 - no handle was made
