"""The kernels of the native encoder forward ONE BY ONE on the GPU (`rl_encoder_embed`, `rl_encoder_linear`, `rl_encoder_layer_norm`;
raglite_amd/csrc/encoder.hip), each held ELEMENTWISE to the float64 restatements and bounds of tests/encoder_ref.py, in
bf16 and fp16.  tests/test_gpu_encoder_native.py compares whole forwards by an RMS; here an error in one slab's bias column, one token row
at a tile edge, one dropped k-step of one slice or a second rounding in an epilogue has nowhere to hide.

Shapes are chosen for branches, not for the workload (the linear kernel: 32-column slabs, 64-element K chunks dealt to four waves, G
chunks loaded per group -- G = 4 at M <= 64, 2 above --, a 32-element tail, K slices for the partial epilogue):

    (N, K)       what it takes
    (32, 32)     a tail-only chunk, three idle waves, one slab
    (96, 96)     a full chunk and a tail on wave 1, three slabs
    (64, 320)    one slice of 5 chunks, wave 0 owns two: the G = 2 group at M > 64, singles below
    (32, 1056)   17 chunks.  bias, GELU: the G = 4 group at M <= 64, two G = 2 groups above, then the tail on wave 0.  partial: 4 slices
                 of 5, 5, 5, 2 chunks, the last with the tail on wave 1 and nothing for waves 2 and 3
    (96, 1344)   21 chunks: a group, then singles, in one wave.  partial: 5 slices, the last a single chunk
    (64, 544)    partial: 2 slices, the tail in the second
    (64, 2080)   partial: 7 slices, the last with 3 chunks, the tail on wave 2
    and the four projections of bge-m3: (1024, 1024) out, partial, 4 slices x 4 chunks; (1024, 4096) down, partial, 8 x 8; (3072, 1024)
    QKV, bias; (4096, 1024) up, GELU.

M runs over 1, 31, 32, 33, 64, 65, 128, 129, 255, 256 at (96, 96) and (32, 1056), over 1, 33, 129 at the other small shapes and over 5, 33
at the bge-m3 shapes: rows 0 .. M - 1 of one x, so one float64 product per case serves them all.  The layer norms run hidden 32, 192, 1024
(all 256 threads), 1056, 4096, 8192 (more than one pass) with 1, 4 and 8 slices.  Every output lies between guard rows that must keep
their bits.  Each case's worst error / bound goes to profiles/encoder_kernels_error.txt, with the GELU allowance measured here."""

from pathlib import Path

import pytest
import torch

from raglite_amd import _encoder as enc
from raglite_amd._attention import attention_varlen
from raglite_amd._torch_embedder import EncoderShape, _build_encoder
from tests import encoder_ref as ref

pytestmark = pytest.mark.gpu

DEVICE = "cuda"
GUARD, SENTINEL = 2, -7.0  # guard rows in front of and behind every output, and what they hold
LINEAR = ref.linear_cases()
LN = ref.ln_cases()
EMBED = ref.embed_cases()
_ids = lambda cases: [c.name for c in cases]  # noqa: E731


def _dev(t):
    return None if t is None else t.to(DEVICE)


def _bits(t):
    """The tensor's bit patterns (CPU): equality of these is equality bit for bit, NaN payloads and the sign of zero included."""
    return t.cpu().contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


class Guarded:
    """An output of `shape` between GUARD rows (of the last dimension's width) of SENTINEL on either side."""

    def __init__(self, shape, dtype):
        n, pad = 1, GUARD * shape[-1]
        for s in shape:
            n *= s
        self.flat = torch.full((pad + n + pad,), SENTINEL, dtype=dtype, device=DEVICE)
        self.out, self.n, self.pad = self.flat[pad: pad + n].view(shape), n, pad

    def take(self):
        """The output on the CPU, once the guards have been seen untouched."""
        flat = self.flat.cpu()
        assert bool((flat[: self.pad] == SENTINEL).all()), "the rows in front of the output were written"
        assert bool((flat[self.pad + self.n:] == SENTINEL).all()), "the rows behind the output were written"
        return flat[self.pad: self.pad + self.n].view(self.out.shape).clone()


class LinearRun:
    """A linear case's operands on the device, and the kernel over its first M rows."""

    def __init__(self, case, x=None):
        self.case = case
        self.x, self.W, self.bias = _dev(case.x if x is None else x), _dev(case.W), _dev(case.bias)
        self.slices = enc.encoder_linear_slices(case.N, case.K)
        assert self.slices == ref.ksplit(case.N, case.K)

    def __call__(self, M, epilogue):  # noqa: N803
        c = self.case
        if epilogue == "partial":
            g = Guarded((self.slices, M, c.N), torch.float32)  # (the rows behind the LAST slice are guard rows too)
            got = enc.encoder_linear(self.x[:M], self.W, None, "partial", out=g.out)
        else:
            g = Guarded((M, c.N), ref.tdtype(c.dtype))
            got = enc.encoder_linear(self.x[:M], self.W, self.bias, epilogue, out=g.out)
        assert got.data_ptr() == g.out.data_ptr()
        return g.take()


@pytest.fixture(scope="module")
def error_log():
    lines = []
    yield lines
    try:  # (a read-only checkout keeps the committed figures)
        out = Path(__file__).resolve().parent.parent / "profiles" / "encoder_kernels_error.txt"
        head = ("# tests/test_gpu_encoder_kernels.py: the worst |kernel - float64| / bound over a case's elements (and, for the linear layer, over\n"
                "# its M values); every figure is asserted <= 1.  Bounds: tests/encoder_ref.py.  exact-data bias / partial lines are 0 by construction:\n"
                "# they are compared bit for bit.\n")
        out.write_text(head + "".join(sorted(lines)))
    except OSError:
        pass


@pytest.fixture(scope="module")
def gelu_allowance(torch_cuda, error_log):
    """(c_torch, c): torch's own float32 erf-GELU on the GPU against float64 on the pre-activations of every GELU case, in units of
    u max(|v|, 1), and what the kernel is allowed: twice that (the kernel's erff and torch's are the same library function reached through
    different code)."""
    worst = 0.0
    for case in LINEAR:
        if "gelu" in case.epilogues:
            v32 = ref.linear_f64(case)[0].float()
            worst = max(worst, ref.gelu_c(v32, torch.nn.functional.gelu(_dev(v32))))
    assert 0.0 < worst < 64.0, worst  # (float32 on a CPU measures 5.6 on [-8, 8])
    error_log.append(f"# GELU: torch's float32 erf-GELU on this GPU is within c = {worst:.3f} u max(|v|, 1) of float64 on the cases' pre-activations; "
                     f"the kernel is allowed 2 c = {2 * worst:.3f}\n")
    return worst, 2.0 * worst


def _log(error_log, kernel, name, what, ratio):
    line = f"{kernel} {name}{' ' + what if what else ''} | {ratio:.4f}\n"
    print(line, end="")
    error_log.append(line)


# ---- linear ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LINEAR, ids=_ids(LINEAR))
def test_linear_against_float64(torch_cuda, error_log, gelu_allowance, case):
    """Exact data: partial slices and the bias output bit for bit, GELU within its own rounding and erff.  Real data: the bounds."""
    run, dt = LinearRun(case), ref.tdtype(case.dtype)
    v, _ = ref.linear_f64(case)
    slices = ref.linear_slices_f64(case)
    c = gelu_allowance[1]
    worst = dict.fromkeys(case.epilogues, 0.0)
    for M in case.Ms:  # noqa: N806
        for epi in case.epilogues:
            got = run(M, epi)
            if epi == "partial":
                assert got.shape == (len(slices), M, case.N)
                if case.kind == "exact":
                    for s, (lo, hi, p, _) in enumerate(slices):
                        assert torch.equal(got[s].double(), p[:M]), f"M={M}: slice {s} (k {lo}..{hi}) is not the exact sum"
                    continue
                per, total = ref.partial_bounds(case)
                ratios = [ref.worst_ratio(got[s], p[:M], per[s][:M]) for s, (_, _, p, _) in enumerate(slices)]
                acc = got[0].clone()
                for s in range(1, len(slices)):
                    acc += got[s]  # f32, in slice order: what the layer norm adds up
                ratios.append(ref.worst_ratio(acc, sum(p for _, _, p, _ in slices)[:M], total[:M]))
                assert max(ratios) <= 1.0, f"M={M}: partial, worst error / bound per slice and of their sum {ratios}"
                worst[epi] = max(worst[epi], *ratios)
            elif epi == "bias":
                assert got.shape == (M, case.N) and got.dtype == dt
                if case.kind == "exact":
                    assert torch.equal(got, v[:M].to(dt)), f"M={M}: the bias output is not the exact sum rounded once"
                    continue
                r = ref.worst_ratio(got, v[:M], ref.bias_bound(case)[:M])
                assert r <= 1.0, f"M={M}: bias, worst error / bound {r}"
                worst[epi] = max(worst[epi], r)
            else:
                bound = ref.exact_gelu_bound(v, case.dtype, c) if case.kind == "exact" else ref.gelu_bound(case, c)
                r = ref.worst_ratio(got, ref.gelu64(v)[:M], bound[:M])
                assert r <= 1.0, f"M={M}: gelu, worst error / bound {r}"
                worst[epi] = max(worst[epi], r)
    for epi, r in worst.items():
        _log(error_log, "linear", case.name, epi, r)


ONE_SLICE = [c for c in LINEAR if ref.ksplit(c.N, c.K) == 1 and len(c.epilogues) == 3]


@pytest.mark.parametrize("case", ONE_SLICE, ids=_ids(ONE_SLICE))
def test_epilogue_rounds_the_accumulator_once(torch_cuda, error_log, gelu_allowance, case):
    """Where there is one K slice the partial epilogue IS the accumulator: the bias output must be (part + bias) rounded once, bit for bit,
    and GELU is held to gelu64 of that very f32 pre-activation -- the epilogue's arithmetic alone, whatever the product's error."""
    run, dt = LinearRun(case), ref.tdtype(case.dtype)
    worst = 0.0
    for M in case.Ms:  # noqa: N806
        y32 = run(M, "partial")[0] + case.bias.float()
        assert _same_bits(run(M, "bias"), y32.to(dt)), f"M={M}"
        r = ref.worst_ratio(run(M, "gelu"), ref.gelu64(y32), ref.exact_gelu_bound(y32, case.dtype, gelu_allowance[1]))
        assert r <= 1.0, f"M={M}: worst error / bound {r}"
        worst = max(worst, r)
    _log(error_log, "linear", case.name, "gelu-of-its-own-accumulator", worst)


FULL = [c for c in LINEAR if max(c.Ms) == ref.MAX_TOKENS]


@pytest.mark.parametrize("case", FULL, ids=_ids(FULL))
def test_linear_row_bits_do_not_depend_on_m(torch_cuda, case):
    """1, 2, 4 or 8 token tiles per wave (and G = 4 or 2 chunks per group): the same sums in the same order."""
    run = LinearRun(case)
    for epi in case.epilogues:
        full = run(ref.MAX_TOKENS, epi)
        for M in (1, 33, 65, 129):  # noqa: N806
            assert _same_bits(run(M, epi), full[..., :M, :].contiguous()), (epi, M)


@pytest.mark.parametrize("case", [c for c in FULL if c.kind == "real"], ids=_ids([c for c in FULL if c.kind == "real"]))
def test_linear_rows_do_not_leak(torch_cuda, case):
    """One x row of NaN: exactly that output row is NaN (in every slice), every other row keeps its bits."""
    clean = LinearRun(case)
    for M, row in ((1, 0), (33, 31), (65, 64), (129, 32), (256, 255)):  # noqa: N806 - either side of a tile edge, the first and the last row
        x = case.x.clone()
        x[row] = float("nan")
        run = LinearRun(case, x)
        for epi in case.epilogues:
            want, got = clean(M, epi), run(M, epi)
            others = [r for r in range(M) if r != row]
            assert bool(torch.isnan(got[..., row, :]).all()), (epi, M, row)
            assert _same_bits(got[..., others, :], want[..., others, :]), (epi, M, row)


# ---- layer norm ------------------------------------------------------------------------------------------------------------------------
def _layer_norm(case, rows=None):
    """The kernel over the case's rows (or the given selection of them, in that order), guard rows checked."""
    part, resid = (case.part, case.resid) if rows is None else (case.part[:, rows].contiguous(), case.resid[rows].contiguous())
    g = Guarded(tuple(resid.shape), ref.tdtype(case.dtype))
    got = enc.encoder_layer_norm(_dev(part), _dev(case.bias), _dev(resid), _dev(case.ln_w), _dev(case.ln_b), case.eps, out=g.out)
    assert got.data_ptr() == g.out.data_ptr()
    return g.take()


@pytest.mark.parametrize("case", LN, ids=_ids(LN))
def test_layer_norm_against_float64(torch_cuda, error_log, case):
    truth, bound, _ = ref.ln_f64(case)
    got = _layer_norm(case)
    assert got.shape == (case.M, case.hidden) and got.dtype == ref.tdtype(case.dtype)
    r = ref.worst_ratio(got, truth, bound)
    _log(error_log, "layer_norm", case.name, "", r)
    assert r <= 1.0, f"worst error / bound {r}"


@pytest.mark.parametrize("case", [c for c in LN if c.M == ref.MAX_TOKENS], ids=_ids([c for c in LN if c.M == ref.MAX_TOKENS]))
def test_layer_norm_row_bits_depend_on_neither_m_nor_position(torch_cuda, case):
    full = _layer_norm(case)
    for rows in ([0], [255], [7], list(range(33)), list(range(255, -1, -1)), [200, 3, 3, 77]):
        assert _same_bits(_layer_norm(case, rows), full[rows].contiguous()), rows[:4]


# ---- embedding layer norm --------------------------------------------------------------------------------------------------------------
def _embed(case, clamp=False):
    ids, pos, typ = case.ids, case.positions, case.type_ids
    if clamp:
        ids, pos = ids.clamp(0, ref.VOCAB - 1), pos.clamp(0, ref.POSITIONS - 1)
        typ = None if typ is None else typ.clamp(0, case.type_vocab - 1)
    g = Guarded((case.n_tokens, case.hidden), ref.tdtype(case.dtype))
    got = enc.encoder_embed(_dev(ids), _dev(pos), _dev(typ), _dev(case.tok), _dev(case.pos), _dev(case.typ), _dev(case.ln_w), _dev(case.ln_b),
                            case.eps, out=g.out)
    assert got.data_ptr() == g.out.data_ptr()
    return g.take()


@pytest.mark.parametrize("case", EMBED, ids=_ids(EMBED))
def test_embed_against_float64(torch_cuda, error_log, case):
    """Indices of -1, the table's size and 2^31 - 1 among ids, positions and type ids: the clamped row's result, to the bound and to the
    bits of the call that was handed the clamped indices."""
    truth, bound, _ = ref.embed_f64(case)
    got = _embed(case)
    assert got.shape == (case.n_tokens, case.hidden) and got.dtype == ref.tdtype(case.dtype)
    r = ref.worst_ratio(got, truth, bound)
    _log(error_log, "embed", case.name, "", r)
    assert r <= 1.0, f"worst error / bound {r}"
    assert _same_bits(got, _embed(case, clamp=True))


# ---- the pieces chained by hand are the forward ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ref.DTYPES)
def test_the_entries_chained_by_hand_give_the_bits_of_the_forward(torch_cuda, dtype):
    """One layer at hidden 64 (one head of 64: the attention scale 1 / 8 is exact however it is computed): the stand-alone entries run the
    kernels rl_encoder_forward runs, with its arguments."""
    shape = EncoderShape(vocab_size=300, hidden=64, layers=1, heads=1, ffn=128, max_positions=80, n_ctx=64)
    state = torch.random.get_rng_state()
    torch.manual_seed(11)
    module = _build_encoder(shape).to(device=DEVICE, dtype=ref.tdtype(dtype)).eval()
    torch.random.set_rng_state(state)
    lens = [17, 2, 30]  # 49 rows: two token tiles
    n = sum(lens)
    g = torch.Generator().manual_seed(5)
    ids = _dev(torch.randint(0, shape.vocab_size, (n,), generator=g, dtype=torch.int32))
    pos = _dev(torch.tensor([t + shape.position_offset for ln in lens for t in range(ln)], dtype=torch.int32))
    off = _dev(torch.tensor([0, 17, 19, 49], dtype=torch.int32))
    native = enc.NativeEncoder(module, shape)
    try:
        want = native.forward_i32(ids, pos, off, None, len(lens), n, max(lens))
    finally:
        torch.cuda.synchronize()
        native.close()
    p = {k: v.data for k, v in module.named_parameters()}
    eps, L = float(shape.layer_norm_eps), "layers.0."  # noqa: N806
    x = enc.encoder_embed(ids, pos, None, p["tok.weight"], p["pos.weight"], p["typ.weight"], p["ln.weight"], p["ln.bias"], eps)
    qkv = enc.encoder_linear(x, p[L + "qkv.weight"], p[L + "qkv.bias"], "bias")
    attn = attention_varlen(qkv, off, max(lens), shape.heads, scale=0.125)
    part = enc.encoder_linear(attn, p[L + "out.weight"], None, "partial")
    x1 = enc.encoder_layer_norm(part, p[L + "out.bias"], x, p[L + "ln1.weight"], p[L + "ln1.bias"], eps)
    mid = enc.encoder_linear(x1, p[L + "up.weight"], p[L + "up.bias"], "gelu")
    part = enc.encoder_linear(mid, p[L + "down.weight"], None, "partial")
    got = enc.encoder_layer_norm(part, p[L + "down.bias"], x1, p[L + "ln2.weight"], p[L + "ln2.bias"], eps)
    assert bool(torch.isfinite(want.float()).all()) and _same_bits(got, want)
