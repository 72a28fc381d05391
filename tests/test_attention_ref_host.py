"""The references of the variable-length attention kernel agree with torch and with each other on the CPU, and `rl_attention_varlen`
refuses bad arguments before any HIP call (tests/attention_ref.py; the kernel itself: tests/test_gpu_attention_varlen.py)."""

import ctypes as C
import math

import pytest
import torch

from raglite_amd import _abi
from tests import attention_ref as ref

CASES = ref.cases()
IDS = [c.name for c in CASES]


def test_cases_cover_what_the_kernel_branches_on():
    assert len(set(IDS)) == len(IDS)
    assert {c.dtype for c in CASES} == {"bfloat16", "float16"} and {c.head_dim for c in CASES} == {32, 64}
    for c in CASES:
        assert c.qkv.shape == (sum(c.lengths), 3 * ref.HEADS * c.head_dim) and c.max_len >= max(c.lengths)
    assert any(0 in c.lengths for c in CASES) and any(c.max_len > max(c.lengths) for c in CASES)
    assert any(len(c.lengths) == 40 for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_equals_torch_float64_attention(case):
    out, a = ref.attention_f64(case)
    torch.testing.assert_close(out, ref.sdpa_per_sequence(case), atol=1e-12, rtol=1e-12)
    assert bool(torch.isfinite(out).all()) and bool((a >= out.abs() - 1e-12).all())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_emulated_roundings_stay_within_the_undoubled_bound(case):
    """So the inputs are known to be passable before a GPU sees them."""
    truth, a = ref.attention_f64(case)
    got = ref.attention_emulated(case).double()
    assert bool(torch.isfinite(got).all())
    err, lim = (got - truth).abs(), ref.bound(a, case.dtype, factor=1.0)
    worst = float((err / lim.clamp_min(1e-300)).max())
    print(f"{case.name}: emulation max err / bound = {worst:.3f}")
    assert bool((err <= lim).all()), worst


def _call(lib, *, qkv=0x1000, off=0x1000, n_seqs=1, n_tokens=4, max_len=4, heads=2, head_dim=64, dtype=0, scale=0.125, out=0x1000,
          mem=_abi.MEM_DEVICE):
    return lib.rl_attention_varlen(qkv, off, n_seqs, n_tokens, max_len, heads, head_dim, dtype, scale, out, mem, None)


@pytest.mark.parametrize(("kw", "status", "text"), [
    ({"qkv": None}, _abi.RL_ERR_INVALID, "null"),
    ({"off": None}, _abi.RL_ERR_INVALID, "null"),
    ({"out": None}, _abi.RL_ERR_INVALID, "null"),
    ({"n_seqs": -1}, _abi.RL_ERR_INVALID, "negative"),
    ({"n_tokens": -1}, _abi.RL_ERR_INVALID, "negative"),
    ({"max_len": -1}, _abi.RL_ERR_INVALID, "negative"),
    ({"heads": 0}, _abi.RL_ERR_INVALID, "heads"),
    ({"scale": math.inf}, _abi.RL_ERR_INVALID, "finite"),
    ({"scale": math.nan}, _abi.RL_ERR_INVALID, "finite"),
    ({"dtype": 2}, _abi.RL_ERR_INVALID, "dtype"),
    ({"n_seqs": 65536}, _abi.RL_ERR_INVALID, "n_seqs"),
    ({"qkv": 0x1008}, _abi.RL_ERR_INVALID, "aligned"),
    ({"head_dim": 128}, _abi.RL_ERR_UNSUPPORTED, "head_dim"),
    ({"head_dim": 0}, _abi.RL_ERR_UNSUPPORTED, "head_dim"),
    ({"mem": _abi.MEM_HOST}, _abi.RL_ERR_UNSUPPORTED, "device"),
])
def test_argument_checks_come_before_any_hip_call(kw, status, text):
    lib = _abi.lib()
    assert _call(lib, **kw) == status
    msg = _abi.last_error()
    assert msg.startswith("rl_attention_varlen: ") and text in msg, msg


def test_no_tokens_is_ok_and_touches_nothing():
    assert _call(_abi.lib(), qkv=None, off=None, out=None, n_seqs=0, n_tokens=0, max_len=0) == _abi.RL_OK


def test_binding_takes_cuda_tensors_only():
    import raglite_amd

    with pytest.raises(ValueError, match="CUDA tensors only"):
        raglite_amd.attention_varlen(torch.zeros((4, 3 * 2 * 64), dtype=torch.bfloat16), torch.tensor([0, 4], dtype=torch.int32), 4, 2)
    assert C.sizeof(C.c_float) == 4 and _abi._SIGNATURES["rl_attention_varlen"][8] is C.c_float  # noqa: SLF001
