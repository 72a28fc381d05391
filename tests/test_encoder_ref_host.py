"""tests/encoder_ref.py without a GPU: the float32 emulations of the encoder kernels' rounding points stay inside the UN-doubled form of
every bound on every case (so the doubled form the kernels are held to has the room of a whole second analysis, and no more); the bounds
are not vacuous (an output one 16-bit ulp off the correctly rounded truth is refused nearly everywhere); the exact-data cases are exact;
and `rl_encoder_linear_slices` is the K split the references assume."""

import ctypes as C

import pytest
import torch

from raglite_amd import _abi
from tests import encoder_ref as ref

LINEAR = ref.linear_cases()
LN = ref.ln_cases()
EMBED = ref.embed_cases()
_ids = lambda cases: [c.name for c in cases]  # noqa: E731


def test_half_ulp_is_half_the_spacing():
    for dtype, one_ulp in (("bfloat16", 2.0 ** -7), ("float16", 2.0 ** -10)):
        t = torch.tensor([1.0, 1.5, 1.999, 2.0, -3.0, 0.75, 0.0, 2.0 ** -20, 2.0 ** -14, 1e-40], dtype=torch.float64)
        hu = ref.half_ulp(t, dtype).tolist()
        assert hu[:6] == [one_ulp / 2, one_ulp / 2, one_ulp / 2, one_ulp, one_ulp, one_ulp / 4]
        if dtype == "float16":
            assert hu[6] == hu[7] == hu[9] == 2.0 ** -25 and hu[8] == 2.0 ** -25  # subnormals, and the first normal binade: spacing 2^-24
        else:
            assert hu[7] == 2.0 ** -28 and hu[6] == hu[9] == 2.0 ** -134
        x = (torch.randn(4096) * 3).double()  # (float32 values: a float64 goes to 16 bits through float32, rounded twice)
        assert bool(((x.to(ref.tdtype(dtype)).double() - x).abs() <= ref.half_ulp(x, dtype)).all())
        off = ref.one_ulp_off(x, dtype).double() - x.to(ref.tdtype(dtype)).double()
        assert bool((off.abs() >= 2 * ref.half_ulp(x, dtype)).all()) and bool((off.sign() == x.sign()).all())


@pytest.mark.parametrize("case", LINEAR, ids=_ids(LINEAR))
def test_linear_emulation_is_inside_the_undoubled_bounds(case):
    v, _ = ref.linear_f64(case)
    if "bias" in case.epilogues:
        assert ref.worst_ratio(ref.linear_emulated(case, "bias"), v, ref.bias_bound(case, 1.0)) <= 1.0
    if "gelu" in case.epilogues:
        v32 = v.float()
        c = ref.gelu_c(v32, ref.gelu32(v32))  # this machine's float32 erf-GELU at these pre-activations
        assert 0.0 < c < 16.0, c
        assert ref.worst_ratio(ref.linear_emulated(case, "gelu"), ref.gelu64(v), ref.gelu_bound(case, c, 1.0)) <= 1.0
    if "partial" in case.epilogues:
        got = ref.linear_emulated(case, "partial")
        per, total = ref.partial_bounds(case, 1.0)
        slices = ref.linear_slices_f64(case)
        assert got.shape[0] == len(slices) == ref.ksplit(case.N, case.K)
        for s, (_, _, p, _) in enumerate(slices):
            assert ref.worst_ratio(got[s], p, per[s]) <= 1.0, s
        acc = got[0].clone()
        for s in range(1, got.shape[0]):
            acc += got[s]
        assert ref.worst_ratio(acc, sum(p for _, _, p, _ in slices), total) <= 1.0


@pytest.mark.parametrize("case", [c for c in LINEAR if c.kind == "exact"], ids=_ids([c for c in LINEAR if c.kind == "exact"]))
def test_exact_data_is_exact_in_float32(case):
    """What the GPU test's bit-for-bit comparisons rest on: the float64 values ARE float32 values, slice by slice and summed."""
    v, _ = ref.linear_f64(case)
    assert torch.equal(v.float().double(), v)
    assert float(v.abs().max()) >= 6.0 and float(v.abs().max()) <= 24.0  # both tails of erf are reached, nothing is far outside
    for lo, hi, p, _ in ref.linear_slices_f64(case):
        assert torch.equal(p.float().double(), p) and hi - lo >= 32
    if "partial" in case.epilogues:
        got = ref.linear_emulated(case, "partial")
        assert all(torch.equal(got[s].double(), p) for s, (_, _, p, _) in enumerate(ref.linear_slices_f64(case)))
    if "bias" in case.epilogues:
        assert torch.equal(ref.linear_emulated(case, "bias"), v.to(ref.tdtype(case.dtype)))


@pytest.mark.parametrize("case", [c for c in LINEAR if c.K == 32], ids=_ids([c for c in LINEAR if c.K == 32]))
def test_linear_bound_refuses_one_ulp(case):
    v, _ = ref.linear_f64(case)
    bad = ref.one_ulp_off(v, case.dtype).double()
    share = float(((bad - v).abs() > ref.bias_bound(case)).double().mean())
    print(f"{case.name}: one ulp off exceeds the bound on {100 * share:.1f} % of the elements")
    assert share >= 0.85


@pytest.mark.parametrize("case", LN, ids=_ids(LN))
def test_layer_norm_emulation_is_inside_the_undoubled_bound(case):
    truth, _, b1 = ref.ln_f64(case)
    assert ref.worst_ratio(ref.ln_emulated(case), truth, b1) <= 1.0


@pytest.mark.parametrize("case", [c for c in LN if c.kind == "normal"], ids=_ids([c for c in LN if c.kind == "normal"]))
def test_layer_norm_bound_refuses_one_ulp(case):
    truth, b2, _ = ref.ln_f64(case)
    bad = ref.one_ulp_off(truth, case.dtype).double()
    share = float(((bad - truth).abs() > b2).double().mean())
    print(f"{case.name}: one ulp off exceeds the bound on {100 * share:.1f} % of the elements")
    assert share >= 0.90


def test_layer_norm_bound_refuses_a_one_pass_variance():
    """What the large-mean rows are for: var = E[v^2] - mean^2 in float32 is far outside their (wide) bound."""
    for case in (c for c in LN if c.kind == "mean100" and c.hidden >= 1024):
        truth, b2, _ = ref.ln_f64(case)
        v = sum(t.float() for t in case.terms64())
        mean = v.mean(-1, keepdim=True)
        var = (v * v).mean(-1, keepdim=True) - mean * mean
        got = ((v - mean) / torch.sqrt(var.clamp(min=0) + case.eps) * case.ln_w.float() + case.ln_b.float()).to(ref.tdtype(case.dtype))
        assert ref.worst_ratio(got, truth, b2) > 2.0, case.name


def test_layer_norm_cases_cover_the_issue():
    seen = {(c.hidden, c.slices, c.kind, c.eps) for c in LN if c.M == 3}
    assert len(seen) == 6 * 3 * 4 and {c.M for c in LN if c.hidden == 1024} == {1, 3, 256}
    for c in LN:
        if c.kind == "const":
            truth, _, _ = ref.ln_f64(c)
            assert float((truth - c.ln_b.double()).abs().max()) < 1e-9  # a constant row normalises to ln_b
        if c.kind == "mean100":
            v = sum(c.terms64())
            assert abs(float(v.mean()) - 100.0) < 0.01 and 0.005 < float(v.std(-1).mean()) < 0.02


@pytest.mark.parametrize("case", EMBED, ids=_ids(EMBED))
def test_embed_emulation_is_inside_the_undoubled_bound(case):
    truth, _, b1 = ref.embed_f64(case)
    assert truth.shape == (case.n_tokens, case.hidden)
    assert ref.worst_ratio(ref.embed_emulated(case), truth, b1) <= 1.0


def test_embed_cases_leave_their_tables():
    for n in (1, 7):
        for c in (c for c in EMBED if c.n_tokens == n and c.type_ids is not None):
            for idx, size in ((c.ids, ref.VOCAB), (c.positions, ref.POSITIONS), (c.type_ids, c.type_vocab)):
                assert bool(((idx < 0) | (idx >= size)).any())
    big = [c for c in EMBED if c.n_tokens == 7]
    assert all({-1, ref.VOCAB, ref.BIG} <= set(c.ids.tolist()) and {-1, ref.POSITIONS, ref.BIG} <= set(c.positions.tolist()) for c in big)
    assert all({-1, c.type_vocab, ref.BIG} <= set(c.type_ids.tolist()) for c in big if c.type_ids is not None and c.type_vocab == 2)


def test_linear_slices_is_the_restated_k_split():
    lib, s = _abi.lib(), C.c_int32()
    for N in range(32, 4096 + 1, 32):  # noqa: N806
        for K in range(32, 8192 + 1, 32):  # noqa: N806
            assert lib.rl_encoder_linear_slices(N, K, C.byref(s)) == _abi.RL_OK
            if s.value != ref.ksplit(N, K):
                pytest.fail(f"rl_encoder_linear_slices({N}, {K}) = {s.value}, restated {ref.ksplit(N, K)}")
    for K in range(32, 8192 + 1, 32):  # noqa: N806 - the split's properties: a function of the chunk count and N's slabs alone
        for N in (32, 64, 96, 1024, 2048, 2080, 4096):  # noqa: N806
            chunks = ref.slice_chunks(N, K)
            sizes = [e - b for b, e in chunks]
            assert 1 <= len(chunks) <= 8 and min(sizes) >= 1 and chunks[0][0] == 0 and chunks[-1][1] == (K + 63) // 64
            assert all(a[1] == b[0] for a, b in zip(chunks[:-1], chunks[1:]))
            assert len(chunks) == 1 or min(sizes[:-1]) >= 4, (N, K, sizes)


def test_the_shapes_take_the_branches_they_are_there_for():
    """The table of tests/test_gpu_encoder_kernels.py's docstring, from the restated split."""
    sizes = lambda N, K: [e - b for b, e in ref.slice_chunks(N, K)]  # noqa: E731, N803
    assert [ref.ksplit(N, K) for N, K in ((32, 32), (96, 96), (64, 320))] == [1, 1, 1]
    assert sizes(32, 1056) == [5, 5, 5, 2] and sizes(96, 1344) == [5, 5, 5, 5, 1] and sizes(64, 544) == [5, 4]
    assert sizes(64, 2080) == [5, 5, 5, 5, 5, 5, 3]
    assert sizes(1024, 1024) == [4] * 4 and sizes(1024, 4096) == [8] * 8
