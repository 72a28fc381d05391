"""CPU checks of what tests/test_gpu_pool_norm.py is built from (tests/pool_norm_ref.py): the committed random batches meet the
comparator's condition (the kernels' arithmetic, restated in float64, has NO excepted element against the reference on them), the
comparator accepts and refuses what it should, and the midpoint set of the cast test is exact and discriminating."""

import numpy as np
import pytest

from tests import pool_norm_ref as ref


def check_emulated(batch, settings):
    for normalize, eps in settings:
        r64, r16, bnd = batch.ref(normalize, eps)
        emu = ref.emulate(batch.tokens, batch.begins, batch.ends, normalize, eps)
        with np.errstate(all="ignore"):
            assert np.all((np.abs(emu - r64) <= bnd) | (np.isnan(emu) & np.isnan(r64)) | (emu == r64)), "the bound does not cover the restated arithmetic"
            assert ref.assert_rounds_like(emu.astype(np.float32), r64, bnd, np.float32, f"float32 {normalize} {eps}") == 0
            assert ref.assert_rounds_like(emu.astype(np.float16), r64, bnd, np.float16, f"float16 {normalize} {eps}") == 0
            assert np.array_equal(r64.astype(np.float16).view(np.uint16), r16.view(np.uint16))


SETTINGS = [(True, 0.0), (False, 0.0)]


@pytest.mark.parametrize("dim", ref.VEC4_DIMS + ref.SCALAR_DIMS)
def test_registers_batches_have_no_excepted_element(dim):
    batch = ref.registers_batch(dim)
    lengths = sorted((batch.ends - batch.begins).tolist())
    assert {0, 1, 2, 3, 4, 5, 7, 8, 9, 11} <= set(lengths) and batch.n_spans == 14 < 64
    assert not np.all(np.diff(batch.begins) >= 0)  # out of order
    check_emulated(batch, SETTINGS + [(True, 2.2e-16)])


def test_instantiations_named_by_the_widths():
    """The widths of the register test reach all 7 + 6 instantiations of `launch_pool_norm`, each at both ends of its range."""
    seen = {}
    for dim in ref.VEC4_DIMS + ref.SCALAR_DIMS:
        seen.setdefault(ref.instantiation(dim), []).append(dim)
    assert seen == {(1, 4): [4, 256], (2, 4): [260, 512], (3, 4): [516, 768], (4, 4): [772, 1024], (6, 4): [1028, 1536],
                    (8, 4): [1540, 2048], (16, 4): [2052, 4096], (1, 1): [1, 63], (2, 1): [65, 127], (4, 1): [129, 254],
                    (8, 1): [257, 510], (16, 1): [513, 1022], (32, 1): [1025, 2047]}


def test_stride_batch_has_no_excepted_element():
    batch = ref.stride_batch()
    assert batch.n_spans == 70_000 > 65_536 and set((batch.ends - batch.begins).tolist()) == {0, 1, 2}
    check_emulated(batch, SETTINGS)


@pytest.mark.parametrize("dim", ref.DMA_DIMS)
def test_dma_batches_have_no_excepted_element(dim):
    for n_spans in ref.DMA_SPANS:
        batch = ref.dma_batch(dim, n_spans)
        lengths = batch.ends - batch.begins
        assert batch.n_spans == n_spans and set(lengths.tolist()) <= set(ref.dma_lengths(dim)) | {300, ref.DMA_ROWS}
        assert 300 in lengths and ref.DMA_ROWS in lengths
        if n_spans >= 130:
            assert set(ref.dma_lengths(dim)) <= set(lengths.tolist())
        check_emulated(batch, SETTINGS)


def test_capped_grid_batch_has_no_excepted_element():
    batch = ref.capped_grid_batch()
    assert batch.n_spans == 20_000 > 64 * 304 and set((batch.ends - batch.begins).tolist()) == {0, 1, 2, 3}
    check_emulated(batch, SETTINGS)


@pytest.mark.parametrize("dim", [256, 1024])
def test_empty_span_and_nonfinite_batches_have_no_excepted_element(dim):
    for case in ref.EMPTY_CASES:
        batch, emptied = ref.empties_batch(dim, case)
        assert batch.n_spans == 512 and np.array_equal(np.flatnonzero(batch.begins == batch.ends), emptied)
        check_emulated(batch, SETTINGS)
    for healthy in (True, False):
        check_emulated(ref.isolation_batch(dim, healthy), SETTINGS)
    r64 = ref.isolation_batch(dim, False).ref(False)[0]
    assert np.all(np.isnan(r64[[10, 40]])) and np.all(r64[41] == np.finfo(np.float32).max) and np.all(r64[77] == np.inf)


@pytest.mark.parametrize("n_spans", [12, 70])
def test_zero_rows_batches_have_no_excepted_element(n_spans):
    batch, zero = ref.zero_rows_batch(n_spans)
    check_emulated(batch, [(True, 2.2e-16), (True, 0.0), (False, 0.0)])
    assert np.all(batch.ref(True, 2.2e-16)[0][zero] == 0) and np.all(np.isnan(batch.ref(True, 0.0)[0][zero]))


def test_the_comparator():
    ref64 = np.asarray([1.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -40, np.nan, -0.0, 65519.99, 65520.0, 1e-9, -np.inf])
    with np.errstate(over="ignore"):
        want = ref64.astype(np.float16)  # 1, 1 (tie to even), 1 + 2^-10, nan, -0, 65504, inf, 0, -inf
    assert want.view(np.uint16).tolist() == [0x3C00, 0x3C00, 0x3C01, 0x7E00, 0x8000, 0x7BFF, 0x7C00, 0x0000, 0xFC00]
    assert ref.assert_rounds_like(want, ref64, 0.0, np.float16) == 0
    assert ref.assert_rounds_like(want.view(np.uint16), ref64, 0.0, np.float16) == 0  # bits are taken as bits
    flipped = want.copy()
    flipped[4] = 0.0  # +0 for -0: equal
    flipped[3] = np.float16(np.nan)
    assert ref.assert_rounds_like(flipped, ref64, 0.0, np.float16) == 0
    # the other neighbour is accepted only where the reference is within the bound of the boundary between the two
    for i, other, dist in ((1, 0x3C01, 0.0), (2, 0x3C00, 2.0 ** -40), (5, 0x7C00, 0.01), (6, 0x7BFF, 0.0), (0, 0x3C01, 2.0 ** -11), (0, 0x3BFF, 2.0 ** -12)):
        got = want.copy().view(np.uint16)
        got[i] = other
        assert ref.assert_rounds_like(got, ref64, dist * (1 + 1e-9), np.float16) == 1
        if dist > 0:
            with pytest.raises(AssertionError, match="rounded once"):
                ref.assert_rounds_like(got, ref64, dist * 0.99, np.float16)
    for i, other in ((0, 0x3C02), (0, 0xBC00), (3, 0x3C00), (0, 0x7E00), (7, 0x0002), (6, 0x7BFE), (8, 0x7C00)):  # never: two steps, sign, NaN
        got = want.copy().view(np.uint16)
        got[i] = other
        with pytest.raises(AssertionError, match="rounded once"):
            ref.assert_rounds_like(got, ref64, 1.0, np.float16)
    # float32, including its overflow boundary
    r32 = np.asarray([1.0 + 2.0 ** -24 + 2.0 ** -50, float(np.finfo(np.float32).max) + 2.0 ** 103 + 2.0 ** 80])  # just past the boundary to inf
    with np.errstate(over="ignore"):
        w32 = r32.astype(np.float32)
    assert w32.view(np.uint32).tolist() == [0x3F800001, 0x7F800000]
    assert ref.assert_rounds_like(w32, r32, 0.0, np.float32) == 0
    assert ref.assert_rounds_like(np.asarray([0x3F800000, 0x7F7FFFFF], np.uint32), r32, np.asarray([2.0 ** -50, 2.0 ** 80]), np.float32) == 2
    with pytest.raises(AssertionError):
        ref.assert_rounds_like(np.asarray([0x3F800000, 0x7F800000], np.uint32), r32, 2.0 ** -51, np.float32)
    assert ref.cap(999_999) == 0 and ref.cap(3_073_024) == 3


def test_bound_scales_with_the_sum_of_magnitudes_not_the_mean():
    """A column that cancels (1e8 - 1e8 + 1) keeps the bound of its magnitudes; one row costs the reciprocal multiply alone."""
    tokens = np.asarray([[1e8, 1.0], [-1e8, 1.0], [1.0, 1.0]], np.float32)
    b = ref.bound(tokens, [0, 0], [3, 1], normalize=False)
    assert b[0, 0] == pytest.approx(1.01 * 7 * ref.U * (2e8 + 1) / 3) and b[0, 1] == pytest.approx(1.01 * 7 * ref.U)
    assert b[1, 0] == pytest.approx(1.01 * 3 * ref.U * 1e8)
    bn = ref.bound(tokens, [0], [3], normalize=True)
    assert np.all(bn > b[0] / np.linalg.norm([1 / 3, 1.0])) and np.all(bn < 1e-6)
    assert np.all(np.isnan(ref.bound(tokens, [1], [1], normalize=False)))
    z = np.zeros((2, 8), np.float32)
    assert np.all(ref.bound(z, [0], [2], normalize=True, eps=2.2e-16) == 0) and np.all(np.isnan(ref.bound(z, [0], [2], normalize=True)))


def test_midpoint_set_is_exact_and_discriminates():
    row0, row1, mean = ref.midpoints()
    assert len(mean) == 190_464 == 6 * 31_744
    m = np.abs(row0[0::6]) / 2
    t = np.abs(row1[0::6])
    assert m[0] == 2.0 ** -25 and m[-1] == 65520.0 and np.all(np.diff(m) > 0)
    assert np.all(t == np.exp2(np.floor(np.log2(m)) - 30))
    # 2 m and t are float32 values, nothing overflows float32, and the float64 means are exact
    assert np.array_equal(row0.astype(np.float32).astype(np.float64), row0) and np.array_equal(row1.astype(np.float32).astype(np.float64), row1)
    assert np.all(np.isfinite(row0.astype(np.float32))) and np.abs(row0).max() == 131040.0
    s = np.tile([1.0, 1.0, 1.0, -1.0, -1.0, -1.0], len(m))
    k = np.tile([-1.0, 0.0, 1.0, -1.0, 0.0, 1.0], len(m))
    assert np.array_equal((row0 + row1) * 0.5, s * (np.repeat(m, 6) + k * np.repeat(t, 6) / 2)) and np.array_equal(mean, (row0 + row1) * 0.5)
    assert np.array_equal(np.abs(mean[1::6]), m)
    # every m is a midpoint of two neighbouring float16 values (or of 65504 and 2^16)
    h = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float64)
    assert np.array_equal(2 * m, h + np.concatenate((h[1:], [65536.0])))
    with np.errstate(over="ignore"):
        direct = mean.astype(np.float16)
        twice = mean.astype(np.float32).astype(np.float16)
    differs = direct.view(np.uint16) != twice.view(np.uint16)
    assert 4 * int(differs.sum()) >= len(mean)
    assert 3 * int(differs.sum()) == len(mean)  # the value on the far side of the tie from the even neighbour, per sign
    assert int(np.isinf(direct).sum()) == 4
    for dim in (256, 512, 1024, 4096):
        tokens, begins, ends, spans_mean = ref.midpoint_spans(dim)
        assert len(begins) == {256: 744, 512: 372, 1024: 186, 4096: 47}[dim]
        r64, r16 = ref.reference(tokens, begins, ends, normalize=False)
        with np.errstate(over="ignore"):
            want16 = spans_mean.astype(np.float16)
        assert np.array_equal(r64, spans_mean) and np.array_equal(r16.view(np.uint16), want16.view(np.uint16))
        assert np.array_equal(ref.emulate(tokens, begins, ends, normalize=False), spans_mean)
