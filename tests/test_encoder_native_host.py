"""The native encoder forward (`rl_encoder_*`, raglite_amd/_encoder.py) without a GPU: every argument check of the four
entry points of the handle, and of the four that run its launches one at a time, returns before the first HIP call with its code and
message; the Python route switch, and the CPU fall-through."""

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


# ---- the forward's launches one at a time: rl_encoder_embed, rl_encoder_linear, rl_encoder_layer_norm, rl_encoder_linear_slices -----------
F16 = _abi.ATTN_DTYPES["float16"]
EPI = _abi.ENCODER_EPILOGUES
NAN, INF = float("nan"), float("inf")


def _embed(ids=P, positions=P, type_ids=None, n_tokens=8, tok=P, vocab=50, pos=P, max_positions=20, typ=P, type_vocab=1, ln_w=P, ln_b=P, hidden=64,
           eps=1e-5, dtype=BF16, out=P, mem=_abi.MEM_DEVICE):
    st = _abi.lib().rl_encoder_embed(ids, positions, type_ids, n_tokens, tok, vocab, pos, max_positions, typ, type_vocab, ln_w, ln_b, hidden, eps,
                                     dtype, out, mem, None)
    return st, _abi.last_error()


@pytest.mark.parametrize(("kw", "code", "text"), [
    ({"mem": _abi.MEM_HOST}, UNSUPPORTED, "device pointers only"),
    ({"n_tokens": -1}, INVALID, "n_tokens must be in"),
    ({"n_tokens": MAX_TOKENS + 1}, INVALID, "n_tokens must be in"),
    ({"vocab": 0}, INVALID, "at least one row"),
    ({"max_positions": 0}, INVALID, "at least one row"),
    ({"type_vocab": -1}, INVALID, "at least one row"),
    ({"hidden": 0}, INVALID, "positive multiple of 32"),
    ({"hidden": -32}, INVALID, "positive multiple of 32"),
    ({"hidden": 48}, INVALID, "positive multiple of 32"),
    ({"hidden": 8192 + 32}, UNSUPPORTED, "hidden must be <= 8192"),
    ({"eps": NAN}, INVALID, "eps must be finite"),
    ({"eps": INF}, INVALID, "eps must be finite"),
    ({"eps": -1e-5}, INVALID, "eps must be finite"),
    ({"dtype": 2}, INVALID, "unknown dtype"),
    ({"dtype": -1}, INVALID, "unknown dtype"),
    ({"ids": None}, INVALID, "null argument"),
    ({"positions": None}, INVALID, "null argument"),
    ({"tok": None}, INVALID, "null argument"),
    ({"pos": None}, INVALID, "null argument"),
    ({"typ": None}, INVALID, "null argument"),
    ({"ln_w": None}, INVALID, "null argument"),
    ({"ln_b": None}, INVALID, "null argument"),
    ({"out": None}, INVALID, "null argument"),
    ({"ids": P + 2}, INVALID, "4-byte aligned"),
    ({"positions": P + 1}, INVALID, "4-byte aligned"),
    ({"type_ids": P + 3}, INVALID, "4-byte aligned"),
    ({"tok": P + 8}, INVALID, "tables must be 16-byte aligned"),
    ({"pos": P + 8}, INVALID, "tables must be 16-byte aligned"),
    ({"typ": P + 4}, INVALID, "tables must be 16-byte aligned"),
    ({"ln_w": P + 4}, INVALID, "must be 8-byte aligned"),
    ({"ln_b": P + 2}, INVALID, "must be 8-byte aligned"),
    ({"out": P + 4}, INVALID, "must be 8-byte aligned"),
])
def test_embed_refuses_before_the_first_hip_call(kw, code, text):
    st, msg = _embed(**kw)
    assert st == code and msg.startswith("rl_encoder_embed:") and text in msg, (st, msg)


def _linear(x=P, M=8, K=64, W=P, N=64, bias=P, epilogue=EPI["bias"], dtype=BF16, out16=P, part=None, mem=_abi.MEM_DEVICE):  # noqa: N803
    st = _abi.lib().rl_encoder_linear(x, M, K, W, N, bias, epilogue, dtype, out16, part, mem, None)
    return st, _abi.last_error()


PARTIAL = {"epilogue": EPI["partial"], "out16": None, "part": P, "bias": None}


@pytest.mark.parametrize(("kw", "code", "text"), [
    ({"mem": _abi.MEM_HOST}, UNSUPPORTED, "device pointers only"),
    ({"M": -1}, INVALID, "M must be in"),
    ({"M": MAX_TOKENS + 1}, INVALID, "M must be in"),
    ({"K": 0}, INVALID, "positive multiples of 32"),
    ({"K": -64}, INVALID, "positive multiples of 32"),
    ({"K": 80}, INVALID, "positive multiples of 32"),
    ({"N": 0}, INVALID, "positive multiples of 32"),
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
    ({"out16": None, "part": P}, INVALID, "write out16, which is null"),  # the only output given is the one this epilogue does not use
    ({"epilogue": EPI["gelu"], "out16": None, "part": P}, INVALID, "write out16, which is null"),
    ({**PARTIAL, "part": None}, INVALID, "writes part, which is null"),
    ({**PARTIAL, "part": None, "out16": P}, INVALID, "writes part, which is null"),
    ({"x": P + 8}, INVALID, "16-byte aligned"),
    ({"W": P + 8}, INVALID, "16-byte aligned"),
    ({**PARTIAL, "part": P + 8}, INVALID, "16-byte aligned"),
    ({"bias": P + 4}, INVALID, "8-byte aligned"),
    ({"out16": P + 2}, INVALID, "8-byte aligned"),
    ({"epilogue": EPI["gelu"], "dtype": F16, "out16": P + 4}, INVALID, "8-byte aligned"),
])
def test_linear_refuses_before_the_first_hip_call(kw, code, text):
    st, msg = _linear(**kw)
    assert st == code and msg.startswith("rl_encoder_linear:") and text in msg, (st, msg)


def _layer_norm(part=P, slices=1, M=8, hidden=64, bias=P, resid=P, ln_w=P, ln_b=P, eps=1e-5, dtype=BF16, out=P, mem=_abi.MEM_DEVICE):  # noqa: N803
    st = _abi.lib().rl_encoder_layer_norm(part, slices, M, hidden, bias, resid, ln_w, ln_b, eps, dtype, out, mem, None)
    return st, _abi.last_error()


@pytest.mark.parametrize(("kw", "code", "text"), [
    ({"mem": _abi.MEM_HOST}, UNSUPPORTED, "device pointers only"),
    ({"M": -1}, INVALID, "M must be in"),
    ({"M": MAX_TOKENS + 1}, INVALID, "M must be in"),
    ({"slices": 0}, INVALID, "slices must be in [1, 8]"),
    ({"slices": 9}, INVALID, "slices must be in [1, 8]"),
    ({"hidden": 0}, INVALID, "positive multiple of 32"),
    ({"hidden": 1000}, INVALID, "positive multiple of 32"),
    ({"hidden": 8192 + 32}, UNSUPPORTED, "hidden must be <= 8192"),
    ({"eps": NAN}, INVALID, "eps must be finite"),
    ({"eps": INF}, INVALID, "eps must be finite"),
    ({"eps": -1.0}, INVALID, "eps must be finite"),
    ({"dtype": 7}, INVALID, "unknown dtype"),
    ({"part": None}, INVALID, "null argument"),
    ({"bias": None}, INVALID, "null argument"),
    ({"resid": None}, INVALID, "null argument"),
    ({"ln_w": None}, INVALID, "null argument"),
    ({"ln_b": None}, INVALID, "null argument"),
    ({"out": None}, INVALID, "null argument"),
    ({"part": P + 8}, INVALID, "part must be 16-byte aligned"),
    ({"bias": P + 4}, INVALID, "8-byte aligned"),
    ({"resid": P + 2}, INVALID, "8-byte aligned"),
    ({"ln_w": P + 4}, INVALID, "8-byte aligned"),
    ({"ln_b": P + 6}, INVALID, "8-byte aligned"),
    ({"out": P + 4}, INVALID, "8-byte aligned"),
])
def test_layer_norm_refuses_before_the_first_hip_call(kw, code, text):
    st, msg = _layer_norm(**kw)
    assert st == code and msg.startswith("rl_encoder_layer_norm:") and text in msg, (st, msg)


def test_zero_rows_are_a_no_op_and_the_limits_are_inside():
    """M = 0 returns RL_OK before any pointer is looked at (and before any HIP call: there is no device here)."""
    assert _embed(n_tokens=0, ids=None, out=None)[0] == _abi.RL_OK
    assert _linear(M=0, x=None, out16=None)[0] == _abi.RL_OK
    assert _layer_norm(M=0, part=None, out=None)[0] == _abi.RL_OK
    assert _linear(M=0, K=48)[0] == INVALID and _layer_norm(M=0, slices=9)[0] == INVALID  # ... but not before the sizes are
    assert _embed(n_tokens=0, hidden=8192, eps=0.0, dtype=F16)[0] == _abi.RL_OK and _layer_norm(M=0, hidden=8192, slices=8, eps=0.0)[0] == _abi.RL_OK


@pytest.mark.parametrize(("N", "K", "out", "text"), [
    (0, 64, True, "positive multiples of 32"),
    (64, 0, True, "positive multiples of 32"),
    (-32, 64, True, "positive multiples of 32"),
    (48, 64, True, "positive multiples of 32"),
    (64, 100, True, "positive multiples of 32"),
    (64, 64, False, "slices is null"),
])
def test_linear_slices_refuses(N, K, out, text):  # noqa: N803
    s = C.c_int32(-7)
    st = _abi.lib().rl_encoder_linear_slices(N, K, C.byref(s) if out else None)
    msg = _abi.last_error()
    assert st == INVALID and msg.startswith("rl_encoder_linear_slices:") and text in msg and s.value == -7, (st, msg)


def test_the_epilogue_names_are_the_header_constants():
    header = (Path(__file__).resolve().parent.parent / "include" / "raglite_hip.h").read_text()
    named = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define RL_ENC_EPI_([A-Z]+) (\d+)", header)}
    assert named == EPI == {"bias": 0, "gelu": 1, "partial": 2}
