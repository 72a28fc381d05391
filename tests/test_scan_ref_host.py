"""tests/scan_ref.py on the CPU: the float64 reference agrees with the oracle's statements of the similarity, the integer data is exact,
and every same-sign case of tests/test_gpu_scan.py is DISCRIMINATING: a kernel that lost one column of the dot, or of the row norm, would
be more than twice the bound away from the reference on every row -- a condition on the test data, not a measurement of the device."""

import numpy as np
import pytest

from oracle import oracle
from tests import scan_ref as ref
from tests.test_oracle_props import DUCKDB_GAP_ULPS
from tests.util import sim_fp32_exact


@pytest.mark.parametrize("kind", ["unit_fp16", "uniform", "same_sign"])
@pytest.mark.parametrize("metric", ref.METRICS)
def test_reference_agrees_with_the_oracle(kind, metric):
    """`oracle.similarity` (float64) is the same statement up to float64 rounding; `oracle.similarity_duckdb_fp32` (float32, element-order
    sums, one root) stays within the gap tests/test_oracle_props.py allows between the formulations."""
    n, d = 300, 1024
    E, q = oracle.synth_matrix(11, n, d), oracle.synth_matrix(12, 1, d)[0]
    if kind == "unit_fp16":
        E = (E / np.linalg.norm(E, axis=1, keepdims=True)).astype(np.float16).astype(np.float32)
        q = (q / np.linalg.norm(q)).astype(np.float16).astype(np.float32)
    elif kind == "same_sign":
        E, Q = ref.float_case(d, n=n, B=1)
        q = Q[0]
    mine = ref.reference(E, q, metric)
    truth = oracle.similarity(E, q, metric)
    scale = max(1.0, float(np.abs(truth).max()))
    assert float(np.abs(mine - truth).max()) <= 64 * 2.0 ** -53 * d * scale  # float64 sums of d terms in two orders
    duck = oracle.similarity_duckdb_fp32(E, q, metric).astype(np.float64)
    assert float(np.abs(mine - duck).max()) <= DUCKDB_GAP_ULPS * 2.0 ** -24 * scale
    assert np.array_equal(ref.reference(E, q[None, :], metric)[0], mine)
    if metric == "dot":
        assert np.array_equal(ref.reference(E, q, "raw") + 1.0, mine)


@pytest.mark.parametrize("dim", [1, 63, 257, 1028, 2047, 2052, 4096])
@pytest.mark.parametrize("metric", ref.METRICS)
def test_reference_is_exact_on_integer_data(dim, metric):
    """Integer data: the float64 reference rounds to `sim_fp32_exact`'s bits wherever the finishing operations are exact (dot always; l2
    and cosine within one fp32 rounding of each finishing operation: the bound), and the bound covers the rest."""
    E, Q = ref.int_case(dim, 64, 2)
    E = E.copy()
    E[E.sum(axis=1) == 0, 0] = 1.0  # (dim 1: no zero row, whose cosine is NaN on both sides)
    Q = np.where(np.abs(Q).sum(axis=1, keepdims=True) == 0, 1.0, Q).astype(np.float32)
    for b in range(2):
        exact = sim_fp32_exact(E, Q[b], metric)
        mine = ref.reference(E, Q[b], metric)
        if metric == "dot":
            assert np.array_equal(mine.astype(np.float32).view(np.uint32), exact.view(np.uint32))
        storage, aligned = "f32", dim % 4 == 0
        assert np.all(np.abs(exact.astype(np.float64) - mine) <= ref.bound(E, Q[b], metric, storage, aligned))
    ne, ss = ref.row_norms(E)
    assert np.array_equal(ss, (E.astype(np.float64) ** 2).sum(axis=1)) and np.array_equal(ne, np.sqrt(ss))


def test_instantiations_restate_the_dispatchers():
    """Class ends of the three families (scan.hip: launch_scan_rows / launch_row_norms; scan16.hip)."""
    want = {4: 1, 256: 1, 260: 2, 512: 2, 516: 3, 768: 3, 772: 4, 1024: 4, 1028: 6, 1536: 6, 1540: 8, 2048: 8, 2052: 16, 4096: 16}
    assert {d: ref.instantiation(d)["nv"] for d in ref.VEC4_DIMS} == want
    assert [ref.instantiation(d)["nv"] for d in ref.SCALAR_DIMS] == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16, 32, 32]
    assert [ref.instantiation(d, aligned=False)["nv"] for d in ref.MISALIGNED_DIMS] == [1, 2, 4, 8, 16, 32]
    assert [ref.instantiation(d)["norm_nv"] for d in (256, 260, 516, 1028, 2052)] == [1, 2, 4, 8, 16]
    assert [ref.instantiation(d)["norm_nv"] for d in (1, 255, 257, 1023, 1025, 2047)] == [4, 4, 16, 16, 32, 32]
    assert [ref.instantiation(d, "f16")["nv"] for d in ref.F16_L2_DIMS + ref.F16_WIDE_DIMS] == [1, 1, 2, 2, 4, 4, 6, 6, 8, 8]
    assert [ref.instantiation(d, "f16")["norm_nv"] for d in (128, 512, 640, 1024, 1152, 4096)] == [1, 1, 2, 2, 8, 8]
    assert ref.instantiation(1028)["live"] == 4 and ref.instantiation(2052)["live"] == 8  # NV = 6: slot 5 all masked; NV = 16: slot 8
    assert ref.dropped_columns(2052) == [0, 2048, 2051] and ref.dropped_columns(2047) == [0, 1984, 2046]
    with pytest.raises(ValueError):
        ref.instantiation(2050)
    with pytest.raises(ValueError):
        ref.instantiation(4096, aligned=False)


def test_bound_grows_with_the_chain_and_is_small():
    """The bound is a function of the instantiation: at dim 516 the 16-byte family sums 3 * 4 terms per lane and the scalar family 16,
    at dim 1152 fp32 rows 6 * 4 and fp16 rows 4 * 8; at the widest case the bound stays three orders inside the scores."""
    E, Q = ref.float_case(516, n=16, B=2)
    for metric in ref.METRICS:
        assert np.all(ref.bound(E, Q, metric, aligned=True) < ref.bound(E, Q, metric, aligned=False))
    E, Q = ref.float_case(1152, "f16", n=16, B=2)
    for metric in ref.METRICS:
        assert np.all(ref.bound(E, Q, metric, "f32") < ref.bound(E, Q, metric, "f16"))
    E, Q = ref.float_case(4096, n=16, B=2)
    for metric in ref.METRICS:
        assert np.all(ref.bound(E, Q, metric) < 2e-3 * np.maximum(1.0, np.abs(ref.reference(E, Q, metric))))


@pytest.mark.parametrize("case", ref.float_cases(), ids=lambda c: f"{c[1]}-{'a' if c[2] else 'u'}-{c[0]}")
def test_same_sign_cases_are_discriminating(case):
    """For every case of the GPU file: the reference with one column dropped from the dot (the squared distance), and with one column
    dropped from the row norm (cosine), differs from the full reference by MORE THAN TWICE the bound on every row of every query -- so no
    output can be within the bound of both.  Columns: the first, the last, the first of the last live vector slot."""
    dim, storage, aligned, metrics, n, B = case
    E, Q = ref.float_case(dim, storage, n, B)
    assert np.all((E >= 0.5) & (E <= 1.0)) and np.all((Q >= -1.0) & (Q <= -0.5))
    if storage == "f16":
        assert np.array_equal(E.astype(np.float16).astype(np.float32), E)
    for metric in metrics:
        full, bnd = ref.reference(E, Q, metric), ref.bound(E, Q, metric, storage, aligned)
        assert np.all(np.isfinite(full)) and np.all(bnd > 0)
        for col in ref.dropped_columns(dim, storage, aligned):
            with np.errstate(invalid="ignore", divide="ignore"):
                lost = [ref.reference(E, Q, metric, drop_dot=col)]
                if metric == "cosine":
                    lost.append(ref.reference(E, Q, metric, drop_norm=col))
                for x in lost:
                    far = ~(np.abs(x - full) <= 2.0 * bnd)  # (dim 1 without its only column: NaN / inf, as far as can be)
                    assert far.all(), (metric, col, float(np.nanmin(np.abs(x - full) / bnd)))


def test_comparator_excepts_nothing():
    E, Q = ref.float_case(63, n=40, B=2)
    full = ref.reference(E, Q, "dot")
    bnd = ref.bound(E, Q, "dot", aligned=False)
    order = np.stack([oracle.topk_desc(full[b], 42)[1] for b in range(2)])
    pad = np.full((2, 2), -1)
    S = np.concatenate([np.take_along_axis(full, order, 1), np.full((2, 2), -np.inf)], axis=1).astype(np.float32)
    R = np.concatenate([order, pad], axis=1).astype(np.int32)
    got, ratio = ref.assert_search(S, R, E, Q, "dot", aligned=False)
    assert ratio <= 1.0 and got.shape == (2, 40)
    bad = S.copy()
    bad[1, 17] += 4 * bnd[1, R[1, 17]] + np.spacing(bad[1, 17])  # one score of one query
    with pytest.raises(AssertionError):
        ref.assert_search(bad, R, E, Q, "dot", aligned=False)
    swapped = R.copy()
    swapped[0, [3, 4]] = swapped[0, [4, 3]]  # order no longer follows the scores
    with pytest.raises(AssertionError):
        ref.assert_search(S, swapped, E, Q, "dot", aligned=False)
    lost = R.copy()
    lost[0, 39] = lost[0, 38]  # a row twice, a row never
    with pytest.raises(AssertionError):
        ref.scatter(S, lost, 40)
    short = S.copy()
    short[1, 41] = 0.0  # padding
    with pytest.raises(AssertionError):
        ref.scatter(short, R, 40)
    assert ref.ordered([3.0, 2.0, 2.0, 1.0], [5, 1, 2, 0]) and not ref.ordered([3.0, 2.0, 2.0], [5, 2, 1])
