"""The cross-encoder's head kernel ALONE on the GPU (`rl_encoder_head`, raglite_amd/csrc/encoder_head.hip): every logit
held to the float64 restatement and the bound of tests/encoder_head_ref.py (whose docstrings carry the kernel's order and the bound's
derivation), in bf16 and fp16.

hidden 32 (one 32-wide chunk: 8 lanes with data, one turn per wave), 64, 96, 192, 384 (MiniLM's), 1024 (four passes of a lane); data that
is normal, that cancels, and that saturates tanh; n_seqs 1, 17 and 300 over one x of 300 rows, with first tokens at rows 0, 255, 256 (a
token-block edge of the trunk) and 299, one empty sequence (NaN) and offsets outside [0, n_tokens) (clamped: finite, no fault).  One float64
product per case serves every set of offsets.  The logits lie between guard elements that must keep their bits.  Each case's worst error /
bound goes to profiles/encoder_head_error.txt with the measured tanh allowance."""

from pathlib import Path

import pytest
import torch

from raglite_amd import _abi
from raglite_amd import _encoder as enc
from tests import encoder_head_ref as ref
from tests.encoder_ref import worst_ratio

pytestmark = pytest.mark.gpu

DEVICE = "cuda"
GUARD, SENTINEL = 8, -7.0
CASES = ref.head_cases()
OFFSETS = ref.offsets_cases()
_ids = lambda cases: [c.name for c in cases]  # noqa: E731


def _bits(t):
    return t.cpu().contiguous().view(torch.int32)


class Run:
    """A case's operands on the device, and the kernel over a list of offsets: (n_seqs,) float32 on the CPU, guards checked."""

    def __init__(self, case):
        self.case = case
        self.args = [t.to(DEVICE) for t in (case.x, case.pooler_w, case.pooler_b, case.head_w, case.head_b)]

    def __call__(self, offsets):
        n = len(offsets) - 1
        flat = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device=DEVICE)
        off = torch.tensor(offsets, dtype=torch.int32, device=DEVICE)
        got = enc.encoder_head(self.args[0], off, *self.args[1:], out=flat[GUARD: GUARD + n])
        assert got.data_ptr() == flat[GUARD:].data_ptr()
        host = flat.cpu()
        assert bool((host[:GUARD] == SENTINEL).all()) and bool((host[GUARD + n:] == SENTINEL).all()), "a guard element was written"
        return host[GUARD: GUARD + n].clone()


@pytest.fixture(scope="module")
def error_log():
    lines = []
    yield lines
    try:  # (a read-only checkout keeps the committed figures)
        out = Path(__file__).resolve().parent.parent / "profiles" / "encoder_head_error.txt"
        head = ("# tests/test_gpu_encoder_head.py: the worst |kernel - float64| / bound over a case's logits (every set of offsets); every figure is\n"
                "# asserted <= 1.  Bound: tests/encoder_head_ref.py (head_bound, factor 2).\n")
        out.write_text(head + "".join(sorted(lines)))
    except OSError:
        pass


@pytest.fixture(scope="module")
def tanh_allowance(torch_cuda, error_log):
    """(c_torch, c): torch's own float32 tanh on the GPU against float64 at every case's pre-activations, in units of u, and what the
    kernel's tanhf is allowed: twice that (the measure of `gelu_allowance` in tests/test_gpu_encoder_kernels.py)."""
    worst = 0.0
    for case in CASES:
        v32 = ref.head_f64(case)[1].float()
        worst = max(worst, ref.tanh_c(v32, torch.tanh(v32.to(DEVICE))))
    assert 0.0 < worst < 64.0, worst
    error_log.append(f"# tanh: torch's float32 tanh on this GPU is within c = {worst:.3f} u of float64 on the cases' pre-activations; the kernel is "
                     f"allowed 2 c = {2 * worst:.3f}\n")
    return worst, 2.0 * worst


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_head_against_float64(torch_cuda, error_log, tanh_allowance, case):
    truth, _, _, _ = ref.head_f64(case)
    c = tanh_allowance[1]
    bound2, bound1 = ref.head_bound(case, c, 2.0), ref.head_bound(case, c, 1.0)
    assert ref.bound_is_sane(case, c)
    run, worst = Run(case), 0.0
    for name, (offsets, rows) in OFFSETS.items():
        got = run(offsets)
        empty = [s for s, r in enumerate(rows) if r is None]
        real = [s for s, r in enumerate(rows) if r is not None]
        assert bool(torch.isnan(got[empty]).all()), f"{name}: an empty sequence must give NaN"
        idx = torch.tensor([rows[s] for s in real])
        g = got[real].double()
        assert bool(torch.isfinite(g).all()), name
        ratio = worst_ratio(g, truth[idx], bound2[idx])
        print(f"{case.name} {name} | {ratio:.4f}")
        assert ratio <= 1.0, (name, ratio)
        worst = max(worst, ratio)
        # the un-doubled bound refuses every logit moved away from the truth by that bound's own size
        moved = ref.moved_by_bound(g, truth[idx], bound1[idx])
        off = g != truth[idx]
        assert bool(((moved - truth[idx]).abs() > bound1[idx])[off].all()), name
        assert bool(off.any()) or len(real) < 4, name  # (float32 logits that all equal their float64 truth would test nothing)
    line = f"head {case.name} | {worst:.4f}\n"
    error_log.append(line)


@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "normal"], ids=_ids([c for c in CASES if c.kind == "normal"]))
def test_bits_depend_on_the_row_alone(torch_cuda, case):
    """The same bits run to run, and for a row whatever n_seqs and its index s are: alone, among 17 and among 300."""
    run = Run(case)
    many, rows = run(OFFSETS["three-hundred"][0]), OFFSETS["three-hundred"][1]
    assert torch.equal(_bits(many), _bits(run(OFFSETS["three-hundred"][0])))
    by_row = {r: many[s] for s, r in enumerate(rows)}
    for name in ("one-at-0", "one-at-255", "one-at-256", f"one-at-{ref.N_TOKENS - 1}", "seventeen", "clamped"):
        offsets, rs = OFFSETS[name]
        got = run(offsets)
        for s, r in enumerate(rs):
            if r is not None:
                assert torch.equal(_bits(got[s]), _bits(by_row[r])), (name, s, r)
    # reversed "offsets" (each read on its own: the kernel looks at seq_offsets[s] and whether seq_offsets[s + 1] equals it): row r at index 299 - r
    rev = list(range(ref.N_TOKENS - 1, -1, -1)) + [-1]
    got = run(rev)
    for s, r in enumerate(rev[:-1]):
        assert torch.equal(_bits(got[s]), _bits(by_row[r])), (s, r)


def test_n_seqs_zero_writes_nothing(torch_cuda):
    run = Run(CASES[0])
    got = enc.encoder_head(run.args[0], torch.zeros(1, dtype=torch.int32, device=DEVICE), *run.args[1:])
    assert tuple(got.shape) == (0,) and got.dtype == torch.float32


def test_argument_checks(torch_cuda):
    """Each refusal has its status, names the entry, and comes before any HIP call (nothing is launched: the output keeps its bits)."""
    lib = _abi.lib()
    case = CASES[0]
    h = case.hidden
    x, pw, pb, hw, hb = (t.to(DEVICE) for t in (case.x, case.pooler_w, case.pooler_b, case.head_w, case.head_b))
    off = torch.tensor([0, 1, 2], dtype=torch.int32, device=DEVICE)
    out = torch.full((2,), SENTINEL, dtype=torch.float32, device=DEVICE)
    good = dict(x=x.data_ptr(), off=off.data_ptr(), n_seqs=2, n_tokens=ref.N_TOKENS, hidden=h, pw=pw.data_ptr(), pb=pb.data_ptr(),
                hw=hw.data_ptr(), hb=hb.data_ptr(), dtype=_abi.ATTN_DTYPES[case.dtype], out=out.data_ptr(), mem=_abi.MEM_DEVICE)

    def call(**kw):
        a = {**good, **kw}
        return lib.rl_encoder_head(a["x"], a["off"], a["n_seqs"], a["n_tokens"], a["hidden"], a["pw"], a["pb"], a["hw"], a["hb"], a["dtype"],
                                   a["out"], a["mem"], None)

    bad = [(dict(mem=_abi.MEM_HOST), _abi.RL_ERR_UNSUPPORTED), (dict(hidden=8224), _abi.RL_ERR_UNSUPPORTED),
           (dict(hidden=48), _abi.RL_ERR_INVALID), (dict(hidden=0), _abi.RL_ERR_INVALID), (dict(dtype=2), _abi.RL_ERR_INVALID),
           (dict(n_seqs=-1), _abi.RL_ERR_INVALID), (dict(n_seqs=65536), _abi.RL_ERR_INVALID), (dict(n_tokens=-1), _abi.RL_ERR_INVALID),
           (dict(n_tokens=2 ** 31), _abi.RL_ERR_INVALID), (dict(n_tokens=0), _abi.RL_ERR_INVALID)]
    bad += [({k: None}, _abi.RL_ERR_INVALID) for k in ("x", "off", "pw", "pb", "hw", "hb", "out")]
    bad += [({k: good[k] + 8}, _abi.RL_ERR_INVALID) for k in ("x", "pw", "pb", "hw", "hb")]
    bad += [({k: good[k] + 2}, _abi.RL_ERR_INVALID) for k in ("off", "out")]
    for kw, status in bad:
        assert call(**kw) == status, kw
        assert "rl_encoder_head:" in _abi.last_error(), kw
    torch.cuda.synchronize()
    assert bool((out.cpu() == SENTINEL).all())
    assert call(n_seqs=0, x=None, out=None) == _abi.RL_OK
    assert call() == _abi.RL_OK
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.cpu()).all()) and bool((out.cpu() != SENTINEL).all())
    with pytest.raises(ValueError, match="encoder_head"):
        enc.encoder_head(x, off, pw, pb[:-1], hw, hb)
    with pytest.raises(ValueError, match="encoder_head"):
        enc.encoder_head(x.float(), off, pw, pb, hw, hb)


def test_side_stream(torch_cuda):
    case = next(c for c in CASES if c.hidden == 384 and c.kind == "normal" and c.dtype == "bfloat16")
    run = Run(case)
    want = run(OFFSETS["seventeen"][0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = run(OFFSETS["seventeen"][0])
    side.synchronize()
    assert torch.equal(_bits(got), _bits(want))
