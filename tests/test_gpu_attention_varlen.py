"""The variable-length attention kernel (raglite_amd/csrc/attention_varlen.hip) against the float64 restatement of
tests/attention_ref.py, under |out - truth| <= 2 (2 u + 2^-12) A elementwise, on every case of `attention_ref.cases()`: bf16 and fp16,
head widths 32 and 64, three heads, sequence lengths around every tile edge (32-key sub-tile, 64-key tile, 64-row query tile), an empty
sequence, forty sequences in one pack, scores of tens (q * 8), a key that forces a late rescale and one that never does, and a max_len
larger than needed.  Every run writes between sentinel guard rows, which must stay as they were."""

import pytest
import torch

import raglite_amd
from tests import attention_ref as ref

pytestmark = pytest.mark.gpu

CASES = ref.cases()
IDS = [c.name for c in CASES]
GUARD = 7  # rows of sentinel before and after `out`
SENTINEL = 12345.0


def run_kernel(case, *, qkv=None, offsets=None, max_len=None):
    """The kernel's output (n_tokens, HEADS, head_dim) on the GPU.  `attention_varlen` allocates its own output, so the guard rows are
    checked through the C ABI directly: `out` is the middle of a sentinel-filled buffer."""
    from raglite_amd import _abi

    dev = torch.device("cuda")
    qkv = (case.qkv if qkv is None else qkv).to(dev)
    off = torch.tensor(case.offsets if offsets is None else offsets, dtype=torch.int32, device=dev)
    n, width = qkv.shape[0], ref.HEADS * case.head_dim
    buf = torch.full((n + 2 * GUARD, width), SENTINEL, dtype=qkv.dtype, device=dev)
    out = buf[GUARD : GUARD + n]
    assert out.data_ptr() % 8 == 0
    _abi.check(_abi.lib().rl_attention_varlen(qkv.data_ptr(), off.data_ptr(), off.numel() - 1, n, case.max_len if max_len is None else max_len,
                                             ref.HEADS, case.head_dim, _abi.ATTN_DTYPES[case.dtype], case.scale, out.data_ptr(),
                                             _abi.MEM_DEVICE, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n :] == SENTINEL).all()), "guard rows were written"
    return out.clone().view(n, ref.HEADS, case.head_dim)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernel_against_float64_under_the_bound(torch_cuda, case):
    truth, a = ref.attention_f64(case)
    got = run_kernel(case)
    lim = ref.bound(a, case.dtype)
    got64 = got.double().cpu()
    assert bool((got64 != SENTINEL).all())  # every row belongs to a sequence: nothing of `out` keeps the sentinel
    assert bool(torch.isfinite(got64).all())
    worst = float(((got64 - truth).abs() / lim.clamp_min(1e-300)).max())
    sdpa = ref.sdpa_per_sequence(case, dtype=getattr(torch, case.dtype), device="cuda").double().cpu()
    worst_sdpa = float(((sdpa - truth).abs() / lim.clamp_min(1e-300)).max())
    print(f"{case.name}: kernel max err / bound = {worst:.3f}   torch SDPA max err / bound = {worst_sdpa:.3f}")
    assert bool(((got64 - truth).abs() <= lim).all()), worst
    # the wrapper gives the same bits, and so does a second run
    mine = raglite_amd.attention_varlen(case.qkv.cuda(), torch.tensor(case.offsets, dtype=torch.int32, device="cuda"), case.max_len,
                                        ref.HEADS, scale=case.scale)
    assert mine.shape == (got.shape[0], ref.HEADS * case.head_dim) and mine.dtype == got.dtype
    assert torch.equal(mine.view_as(got), got) and torch.equal(run_kernel(case), got)


@pytest.mark.parametrize("case", [c for c in CASES if c.name.endswith(("around64", "mixed_with_empty-q8"))],
                         ids=[c.name for c in CASES if c.name.endswith(("around64", "mixed_with_empty-q8"))])
def test_a_sequence_alone_gives_the_bits_it_gives_in_the_pack(torch_cuda, case):
    packed = run_kernel(case)
    for lo, hi in zip(case.offsets[:-1], case.offsets[1:]):
        if hi > lo:
            alone = run_kernel(case, qkv=case.qkv[lo:hi].contiguous(), offsets=[0, hi - lo], max_len=hi - lo)
            assert torch.equal(alone, packed[lo:hi])
    assert torch.equal(run_kernel(case, max_len=case.max_len + 1000), packed)  # nor do they depend on max_len


def test_default_scale_and_a_side_stream(torch_cuda):
    case = next(c for c in CASES if c.name == "bfloat16-d64-around128")
    want = run_kernel(case)
    qkv, off = case.qkv.cuda(), torch.tensor(case.offsets, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = raglite_amd.attention_varlen(qkv, off, case.max_len, ref.HEADS)  # scale defaults to head_dim ** -0.5
    side.synchronize()
    assert torch.equal(got.view_as(want), want)


def test_offsets_that_break_the_contract_stay_inside_the_buffers(torch_cuda):
    """Wrong numbers are allowed, an access outside qkv / out is not: the guard rows stay, and the run ends clean."""
    case = next(c for c in CASES if c.name == "float16-d32-around32")
    n = case.qkv.shape[0]
    for bad in ([0, n + 500, n], [-40, 10, n + 7], [n, 0, 5, 2 * n]):
        got = run_kernel(case, offsets=bad, max_len=2 * n)
        assert got.shape[0] == n
