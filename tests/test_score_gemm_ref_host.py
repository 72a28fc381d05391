"""tests/score_gemm_ref.py without a GPU: the bounds hold for the restated split, un-doubled, and refuse the defects the score GEMMs can
have -- each on the input chosen for it; the restatement's own identities; every argument check of `rl_score_gemm` (all of them come
before the first HIP call)."""

import numpy as np
import pytest

from raglite_amd import _abi
from tests import scan_ref
from tests import score_gemm_ref as ref
from tests.util import sim_fp32_exact

S13 = 2.0 ** 13  # the split scale of data below 1: the largest |e s| lies in [2^13, 2^14) where max |e| >= 0.5


def _share_outside(got, want, bound, where=None):
    mask = (bound > 0) if where is None else where & (bound > 0)
    return float(np.mean(np.abs(got - want)[mask] > bound[mask]))


# ---- the bounds hold for the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.elementwise_cases(), ids=lambda c: c.name)
def test_representation_bound_holds_for_the_restated_split(case):
    """|float64 dot - d_split| <= rep_bound on every element of every GPU case: the a-priori bound of the split rules covers the split
    as restated.  (The accumulation bound is the device's to keep.)"""
    E, Q = case.data()  # noqa: N806
    s = ref.pow2_scale(E)
    ratio = scan_ref.assert_within(ref.d_split(E, Q, s), ref.d_exact(E, Q), ref.rep_bound(E, Q, s), case.name)
    assert ratio <= 1.0


@pytest.mark.parametrize("case", ref.probe_cases(), ids=lambda c: c.name)
def test_probe_bound_holds_for_the_restated_split(case):
    """One-hot rows: the restated split is within 0.47 of 2^-19 |e q| at dim 1024 (and at dim 96), which leaves the three accumulations
    their 0.125."""
    E, Q = case.data()  # noqa: N806
    ratio = scan_ref.assert_within(ref.d_split(E, Q, ref.pow2_scale(E)), ref.d_exact(E, Q), ref.probe_bound(E, Q), case.name)
    assert ratio <= 0.47, ratio
    assert np.all(np.sum(E != 0, axis=1) == 1) and np.all(np.sum(E != 0, axis=0) >= 1)  # one product per row; every k position in some row


def test_basis_probe_at_dim_1024_as_the_module_states():
    E, Q = ref.one_hot_rows(1, 2048, 1024), ref.uniform(2, 64, 1024)  # noqa: N806
    assert scan_ref.assert_within(ref.d_split(E, Q, S13), ref.d_exact(E, Q), ref.probe_bound(E, Q)) <= 0.47


# ---- dropped products -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kept, name", [(("hh", "hl"), "el.qh"), (("hh", "lh"), "eh.ql")])
def test_a_dropped_lo_product_leaves_the_probe_bound(kept, name):
    """One-hot rows of U(0.25, 1), U(-1, 1) queries, dim 1024: at least 95 % of the nonzero elements leave 2^-19 |e q|."""
    E, Q = ref.one_hot_rows(1, 2048, 1024), ref.uniform(2, 64, 1024)  # noqa: N806
    share = _share_outside(ref.d_split(E, Q, S13, kept), ref.d_exact(E, Q), ref.probe_bound(E, Q))
    print(f"dropped {name}: {share:.4f} of the nonzero elements outside the probe bound")
    assert share >= 0.95, share


@pytest.mark.parametrize("dim", [32, 64, 96])
def test_a_dropped_el_qh_leaves_the_accumulation_bound_on_same_sign_data(dim):
    """U(0.25, 1) on both sides: every element leaves T 2^-23 sum |e q| (measured against d_split, the kernels' exact value)."""
    E, Q = ref.positive(3, 130, dim), ref.positive(4, 97, dim)  # noqa: N806
    err = np.abs(ref.d_split(E, Q, S13, ("hh", "hl")) - ref.d_split(E, Q, S13))
    ratio = err / ref.acc_bound(E, Q, True)
    print(f"dim {dim}: smallest error / bound {ratio.min():.2f}")
    assert ratio.min() > 1.0, ratio.min()


def test_at_dim_1024_the_worst_case_bound_no_longer_separates_a_dropped_el_qh():
    """Why the probes exist: the same defect stays INSIDE the accumulation bound on most same-sign elements at dim 1024."""
    E, Q = ref.positive(3, 130, 1024), ref.positive(4, 97, 1024)  # noqa: N806
    err = np.abs(ref.d_split(E, Q, S13, ("hh", "hl")) - ref.d_split(E, Q, S13))
    ratio = err / ref.acc_bound(E, Q, True)
    assert ratio.min() < 1.0 and 0.5 < np.median(ratio) < 1.0, (ratio.min(), np.median(ratio))


# ---- structural defects -------------------------------------------------------------------------------------------------------------
def _weighted(dim, n=130, B=97):  # noqa: N803
    """Same-sign data whose slabs differ: slab g of the rows is scaled by 2^((g // NSLOT) % 2), so a slab and the one NSLOT before it
    never look alike."""
    E = np.array(ref.positive(5, n, dim))  # noqa: N806
    g = np.arange(dim) // ref.GK
    E *= (2.0 ** ((g // ref.NSLOT) % 2)).astype(np.float32)[None, :]
    return E, ref.positive(6, B, dim)


@pytest.mark.parametrize("dim", [32, 96, 160, 288, 1024])
def test_a_dropped_slab_leaves_the_bound_everywhere(dim):
    E, Q = _weighted(dim)  # noqa: N806
    want, bound = ref.d_split(E, Q, S13), ref.acc_bound(E, Q, True)
    for g in sorted({0, dim // ref.GK // 2, dim // ref.GK - 1}):
        assert _share_outside(ref.defect_dropped_slab(E, Q, S13, g), want, bound) == 1.0, g


@pytest.mark.parametrize("dim", [160, 288, 1024])
def test_a_stale_slab_leaves_the_bound_everywhere(dim):
    """Slab g - NSLOT in place of slab g (both operands, or the rows alone); also at the 128 x 256 kernel's ring of three."""
    E, Q = _weighted(dim)  # noqa: N806
    want, bound = ref.d_split(E, Q, S13), ref.acc_bound(E, Q, True)
    for g in sorted({ref.NSLOT, dim // ref.GK - 1}):
        assert _share_outside(ref.defect_stale_slab(E, Q, S13, g), want, bound) == 1.0, g
        assert _share_outside(ref.defect_stale_rows(E, Q, S13, g), want, bound) == 1.0, g


@pytest.mark.parametrize("dim", [32, 96, 1024])
def test_a_kept_accumulator_leaves_the_bound_on_every_element_it_touches(dim):
    E, Q = ref.positive(5, 300, dim), ref.positive(6, 97, dim)  # noqa: N806
    got, touched = ref.defect_kept_accumulator(E, Q, S13)
    assert touched.any() and _share_outside(got, ref.d_split(E, Q, S13), ref.acc_bound(E, Q, True), touched) == 1.0


@pytest.mark.parametrize("dim", [32, 96, 1024])
def test_a_neighbours_q_scale_leaves_the_bound_on_every_element_it_touches(dim):
    """Queries scaled by powers of two that differ between neighbours (the `scaled` queries of the GPU cases, made same-sign)."""
    E = ref.positive(5, 130, dim)  # noqa: N806
    Q = np.abs(ref.scaled_queries(7, 97, dim)) + np.float32(0)  # noqa: N806
    got, touched = ref.defect_neighbour_scale(E, Q, S13)
    assert touched[:-1].all()
    assert _share_outside(got, ref.d_split(E, Q, S13), ref.acc_bound(E, Q, True), touched & (np.abs(ref.d_exact(E, Q)) > 0)) == 1.0


@pytest.mark.parametrize("slab, kq", [(0, 0), (1, 3), (31, 2)])
def test_a_swapped_chunk_fails_on_the_probe(slab, kq):
    """The lo chunk in the hi chunk's place at one (slab, kq): the rows whose one product lies there leave the probe bound -- and only they."""
    E, Q = ref.one_hot_rows(1, 2048, 1024), ref.uniform(2, 64, 1024)  # noqa: N806
    got, ks = ref.defect_swapped_chunk(E, Q, S13, slab, kq)
    want, bound = ref.d_exact(E, Q), ref.probe_bound(E, Q)
    touched = np.isin(np.arange(len(E)) % 1024, ks)[None, :] & np.ones((len(Q), 1), dtype=bool)
    assert touched.sum() == 16 * len(Q)
    assert _share_outside(got, want, bound, touched) >= 0.95
    assert _share_outside(got, want, bound, ~touched) == 0.0


# ---- the restatement's own identities -----------------------------------------------------------------------------------------------
def test_hi_plus_lo_reproduces_x_to_the_stated_residual():
    E, Q = ref.spread_rows(8, 257, 96), ref.scaled_queries(9, 97, 96)  # noqa: N806
    eh, el, x = ref.split_rows(E, ref.pow2_scale(E))
    EL = np.maximum(2.0 ** -10 * np.abs(x), 2.0 ** -24)  # noqa: N806
    assert np.all(np.abs(eh) <= np.abs(x)) and np.all(np.abs(x - eh) <= EL) and np.all(np.abs(el) <= np.abs(x - eh))  # truncation, twice
    assert np.all(np.abs(x - eh - el) <= np.maximum(2.0 ** -10 * EL, 2.0 ** -24))
    qh, ql, y, qs = ref.split_queries(Q)
    DQ = np.maximum(2.0 ** -11 * np.abs(y), 2.0 ** -25)  # noqa: N806
    assert np.all(np.abs(y - qh) <= DQ) and np.all(np.abs(y - qh - ql) <= np.maximum(2.0 ** -11 * DQ, 2.0 ** -25))
    assert np.all(np.abs(y).max(axis=1) >= 2.0 ** 13) and np.all(np.abs(y).max(axis=1) < 2.0 ** 14)


def test_integer_data_has_all_zero_lo_halves():
    """The gap itself: on the integer data of the bit-exact tests every lo half is zero on both sides, so el.qh and eh.ql are multiplied
    by zero."""
    E, Q = scan_ref.int_data(11, 130, 288), scan_ref.int_data(12, 97, 288)  # noqa: N806
    _, el, _ = ref.split_rows(E, 2.0 ** 10)
    _, ql, _, _ = ref.split_queries(Q)
    assert not el.any() and not ql.any()
    assert np.array_equal(ref.d_split(E, Q, 2.0 ** 10, ("hh",)), ref.d_exact(E, Q))
    _, el, _ = ref.split_rows(ref.uniform(13, 130, 288), S13)
    assert el.any()


def test_q_scale_is_the_stated_power_of_two():
    Q = np.zeros((6, 32), dtype=np.float32)  # noqa: N806
    Q[1, 3], Q[2, 5], Q[3, 7], Q[4, 9], Q[5, 0] = 1.0, -0.75, 3.0e-5, 2.0 ** -120, 1.9999
    want = [2.0 ** 14, 2.0 ** 13, 2.0 ** 14, 2.0 ** 29, 2.0 ** 114, 2.0 ** 13]  # zero query: ex = 0; 1 = 0.5 2^1; 2^-120: ex = -119, clamped at -100
    assert ref.query_scale(Q).tolist() == want
    qh, ql, _, _ = ref.split_queries(Q)
    assert not qh[0].any() and not ql[0].any()


def test_exact_scores_are_sim_fp32_exact():
    E, Q = scan_ref.int_data(21, 131, 96), scan_ref.int_data(22, 5, 96)  # noqa: N806
    for metric in scan_ref.METRICS:
        want = np.stack([sim_fp32_exact(E, q, metric) for q in Q])
        assert np.array_equal(ref.exact_scores(E, Q, metric).view(np.uint32), want.view(np.uint32)), metric
    rn, rs = ref.int_norms(E)
    for metric in ref.METRICS:  # ... and the float32 epilogue on exact dots and exact |q|^2 gives the same bits
        qss = np.sum(Q.astype(np.float64) ** 2, axis=1).astype(np.float32)
        got = ref.epilogue_f32(ref.exact_scores(E, Q, "raw"), metric, qss, rn, rs)
        assert np.array_equal(got.view(np.uint32), ref.exact_scores(E, Q, metric).view(np.uint32)), metric


def test_epilogue_bound_covers_the_float32_epilogue():
    """score_bound with bd = the rounding of the dot to float32 covers `epilogue_f32` on float32 dots and a float32 |q|^2."""
    E, Q = ref.uniform(31, 130, 96), ref.scaled_queries(32, 41, 96)  # noqa: N806
    rn, rs = ref.given_norms(E)
    d = ref.d_exact(E, Q)
    d32 = d.astype(np.float32)
    qss32 = np.sum(Q.astype(np.float64) ** 2, axis=1).astype(np.float32)
    for metric in ref.METRICS:
        got = ref.epilogue_f32(d32, metric, qss32, rn, rs)
        scan_ref.assert_within(got, ref.score_ref(d, metric, Q, rn, rs), ref.score_bound(d, scan_ref.U * np.abs(d), metric, Q, rn, rs), metric)


def test_cases_are_small_and_named_once():
    cases = ref.elementwise_cases() + ref.probe_cases() + ref.walk_cases()
    assert len({c.name for c in cases}) == len(cases)
    assert all(c.n * c.B * c.dim < 10 ** 9 for c in cases)
    el = ref.elementwise_cases()
    assert {c.dim for c in el} >= set(ref.DIMS) and {c.n for c in el} >= set(ref.ROWS) and {c.B for c in el} >= set(ref.BATCHES)


# ---- rl_score_gemm: every argument check comes before the first HIP call ---------------------------------------------------------------
INVALID, UNSUPPORTED = _abi.RL_ERR_INVALID, _abi.RL_ERR_UNSUPPORTED
_BUF = np.zeros(4096, dtype=np.float32)
P = _BUF.ctypes.data  # a 16-byte aligned host pointer (NumPy aligns to 16 and more); the checks below never read through it
assert P % 16 == 0


def _call(**kw):
    a = dict(E=P, n_rows=8, dim=32, Q=P, n_queries=4, metric=0, row_norm=P, row_sumsq=P, split_scale=0.0, kernel=0, max_workgroups=0, out=P,
             ld=8, out_q_sumsq=None, out_q_scale=None, mem=_abi.MEM_DEVICE)
    a.update(kw)
    st = _abi.lib().rl_score_gemm(a["E"], a["n_rows"], a["dim"], a["Q"], a["n_queries"], a["metric"], a["row_norm"], a["row_sumsq"],
                                  a["split_scale"], a["kernel"], a["max_workgroups"], a["out"], a["ld"], a["out_q_sumsq"], a["out_q_scale"],
                                  a["mem"], None)
    return st, _abi.last_error()


@pytest.mark.parametrize("kw, code, text", [
    (dict(mem=7), INVALID, "bad mem"),
    (dict(n_rows=0), INVALID, "must be >= 1"),
    (dict(n_queries=0), INVALID, "must be >= 1"),
    (dict(dim=0), INVALID, "must be >= 1"),
    (dict(E=None), INVALID, "null argument"),
    (dict(Q=None), INVALID, "null argument"),
    (dict(out=None), INVALID, "null argument"),
    (dict(ld=7), INVALID, "ld must be >= n_rows"),
    (dict(metric=4), INVALID, "unknown metric"),
    (dict(metric=-1), INVALID, "unknown metric"),
    (dict(kernel=4), INVALID, "kernel must be"),
    (dict(kernel=-1), INVALID, "kernel must be"),
    (dict(max_workgroups=-1), INVALID, "max_workgroups"),
    (dict(dim=48), UNSUPPORTED, "multiple of 32"),
    (dict(dim=16), UNSUPPORTED, "multiple of 32"),
    (dict(metric=1, row_norm=None), INVALID, "cosine reads row_norm"),
    (dict(metric=3, row_sumsq=None), INVALID, "l2 reads row_sumsq"),
    (dict(split_scale=3.0), INVALID, "power of two"),
    (dict(split_scale=-2.0), INVALID, "power of two"),
    (dict(split_scale=float("inf")), INVALID, "power of two"),
    (dict(split_scale=float("nan")), INVALID, "power of two"),
    (dict(kernel=2), INVALID, "split arithmetic only"),
    (dict(kernel=3), INVALID, "split arithmetic only"),
    (dict(out_q_scale=P), INVALID, "out_q_scale"),
    (dict(kernel=3, split_scale=1024.0, out_q_sumsq=P), INVALID, "read back kernels 0 to 2"),
    (dict(E=P + 4), INVALID, "16-byte aligned"),
    (dict(Q=P + 8), INVALID, "16-byte aligned"),
])
def test_score_gemm_refuses(kw, code, text):
    st, msg = _call(**kw)
    assert st == code and msg.startswith("rl_score_gemm:") and text in msg, (st, msg)


def test_score_gemm_wrapper_refuses_before_the_library():
    from raglite_amd._score_gemm import score_gemm

    E, Q = np.zeros((8, 32), np.float32), np.zeros((4, 32), np.float32)  # noqa: N806
    with pytest.raises(ValueError, match="Unsupported metric"):
        score_gemm(E, Q, "manhattan")
    with pytest.raises(ValueError, match="E must be"):
        score_gemm(E, np.zeros((4, 64), np.float32))
    with pytest.raises(ValueError, match="out must be"):
        score_gemm(E, Q, out=np.zeros((4, 9), np.float32))
    with pytest.raises(ValueError, match="rows of out must be contiguous"):
        score_gemm(E, Q, out=np.zeros((8, 4), np.float32).T)
