"""The VALU row scan (scan.hip, scan16.hip) against float64 (tests/scan_ref.py): every instantiation the dispatchers can produce.

  scan_rows_kernel<NV, 4, BQ>        NV = 1, 2, 3, 4 (BQ = 4, 2, 1), 6, 8, 16 (BQ = 1): both ends of every width class      `test_vec4_family`
  scan_rows_kernel<NV, 1, BQ>        NV = 1, 2, 4, 8, 16 (BQ = 4, 2, 1), 32 (BQ = 1): odd widths, and misaligned tensors       `test_scalar_family`,
                                                                                                                                `test_misaligned_*`
  row_norms_kernel<NV, 4 / 1>        all eight, through the cosine of the same cases
  scan_rows16_kernel<NV, BQ>         NV = 1, 2; scan_rows16_wide_kernel<NV, BQ, L2>  NV = 4, 6, 8; row_norms16_kernel<1, 2, 8>    `test_f16_*`
  cast_f16_kernel                    both trips                                                                                  `test_adapter_*`

Small corpora, k >= n: EVERY row's score of every query comes back through `search_rows` and is compared.  Integer data ({-3..3}): the bits
of `tests.util.sim_fp32_exact` and the oracle's order (ties to the lowest row).  Same-sign float data (rows in [0.5, 1], queries in
[-1, -0.5]): `scan_ref.assert_search` -- every row within the derived bound, order consistent with the scores, padding (-inf, -1), no element
excepted; tests/test_scan_ref_host.py shows that a kernel losing one column would be more than twice the bound away on every row.
No tolerance is tuned; scripts/scan_error.py prints how far inside the bound the kernels sit (profiles/scan_error.txt)."""

import numpy as np
import pytest

import raglite_amd
from oracle import oracle
from raglite_amd._abi import UnsupportedError
from tests import scan_ref as ref
from tests.util import ragged_offsets, sim_fp32_exact

pytestmark = pytest.mark.gpu

K_MAX = 2048  # rl_search_rows: k <= 2048


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def mfma_route(dim):
    """fp32 widths that leave the scan from five queries up (api.hip: score_rows): the stream kernels' dims, and a wide index whose dim the
    GEMM takes (dim % 32 == 0)."""
    return dim in ref.STREAM_DIMS or (dim > 1024 and dim % 32 == 0)


def make_index(E, metric, storage="f32", offsets=None):
    return raglite_amd.DeviceIndex(E.astype(np.float16) if storage == "f16" and isinstance(E, np.ndarray) else E, offsets, metric=metric, storage=storage)


def search_all(idx, Q, n):
    """Every row of every query, k = n + 2 (two slots of padding) -> (S, R) as NumPy."""
    S, R = idx.search_rows(Q, min(n + 2, K_MAX))
    return host(S), host(R)


def by_row_windows(idx, Q, n, window=K_MAX):
    """Scores [B, n] by row of a corpus with more rows than one call returns: chunk filters (one row per chunk) that each admit a window of
    rows, the windows covering every row.  A filtered-out row must never come back, an admitted one always."""
    Q = np.atleast_2d(Q)
    out = np.empty((len(Q), n), dtype=np.float32)
    for lo in range(0, n, window):
        hi = min(n, lo + window)
        mask = np.zeros(n, dtype=bool)
        mask[lo:hi] = True
        S, R = idx.search_rows(Q, window, chunk_filter=mask)
        S, R = host(S), host(R)
        for b in range(len(Q)):
            assert np.array_equal(np.sort(R[b, :hi - lo]), np.arange(lo, hi)), f"window [{lo}, {hi}) query {b}: not exactly the admitted rows"
            assert np.all(R[b, hi - lo:] == -1) and np.all(np.isneginf(S[b, hi - lo:]))
            assert ref.ordered(S[b, :hi - lo], R[b, :hi - lo])
            out[b, R[b, :hi - lo]] = S[b, :hi - lo]
    return out


def check_int(idx, E, Q, metric, what, known=None):
    S, R = search_all(idx, Q, len(E))
    ref.assert_exact(S, R, E, Q, metric, what, known)
    return S, R


def check_float(idx, E, Q, metric, storage="f32", aligned=True, norms_aligned=None, what="", known=None):
    S, R = search_all(idx, Q, len(E))
    return ref.assert_search(S, R, E, Q, metric, storage, aligned, norms_aligned, what, known)[0]


def run_width(dim, metric, storage, batches, n=ref.N_ROWS, pin=None):
    """One width, one metric: integer data exactly, same-sign data through the comparator, at every batch size (the reference of the
    largest batch is computed once; a smaller batch is its first queries)."""
    aligned = storage == "f16" or dim % 4 == 0
    for kind in ("int", "float"):
        E, Q = ref.int_case(dim, n, max(batches)) if kind == "int" else ref.float_case(dim, storage, n, max(batches))
        known = ref.exact_ranked(E, Q, metric) if kind == "int" else (ref.reference(E, Q, metric), ref.bound(E, Q, metric, storage, aligned))
        idx = make_index(E, metric, storage)
        try:
            with idx.options(**(pin or {})):
                for B in batches:
                    what = f"{storage} dim {dim} {metric} {kind} B {B}"
                    if kind == "int":
                        check_int(idx, E, Q[:B], metric, what, known)
                    else:
                        check_float(idx, E, Q[:B], metric, storage, aligned, what=what, known=known)
        finally:
            idx.close()


# ---- 1. fp32 index: both ends of every width class --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ref.METRICS)
@pytest.mark.parametrize("dim", ref.VEC4_DIMS)
def test_vec4_family(dim, metric):
    """`scan_rows_kernel<NV, 4, BQ>` and `row_norms_kernel<NV, 4>`: NV = 1 (4, 256), 2 (260, 512), 3 (516, 768), 4 (772, 1024), 6 (1028 -- two
    all-masked slots -- and 1536), 8 (1540, 2048), 16 (2052 -- one lane of slot 8 live -- and 4096).  Batches of 1, 2, 3, 4, 7 split into passes
    of 4 / 2 / 1 queries (NV <= 4) or of one; a width the MFMA routes take from five queries up keeps B <= 4 (corpus far below the stream
    threshold of 64 Mi elements, fewer rows than the half-bytes search takes)."""
    run_width(dim, metric, "f32", (1, 2, 3, 4) if mfma_route(dim) else (1, 2, 3, 4, 7))


@pytest.mark.parametrize("metric", ref.METRICS)
@pytest.mark.parametrize("dim", ref.SCALAR_DIMS)
def test_scalar_family(dim, metric):
    """`scan_rows_kernel<NV, 1, BQ>` and `row_norms_kernel<4 / 16 / 32, 1>` (dim % 4 != 0): NV = 1 (1, 63), 2 (65, 127), 4 (129, 255), 8 (257, 511),
    16 (513, 1023), 32 (1025, 2047).  No other kernel takes these widths: every batch size scans, 33 queries in eight passes of four and one."""
    run_width(dim, metric, "f32", (1, 2, 3, 4, 7, 33))


def shifted(torch, x):
    """x [r, c] -> a contiguous CUDA view into a larger buffer whose data pointer is 4 bytes past 16-byte alignment."""
    x = np.asarray(x, dtype=np.float32)
    flat = torch.zeros(x.size + 8, device="cuda")
    assert flat.data_ptr() % 16 == 0
    flat[1:1 + x.size] = torch.tensor(np.array(x).ravel(), device="cuda")
    v = flat[1:1 + x.size].view(*x.shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize("metric", ref.METRICS)
@pytest.mark.parametrize("dim", ref.MISALIGNED_DIMS)
def test_misaligned_rows_take_the_scalar_family(torch_cuda, dim, metric):
    """Borrowed rows that start 4 bytes past 16-byte alignment: the scalar family with a FULL last slot (dim 64 .. 2048 = 64 NV), which no odd
    width reaches, for the scan and for the row norms.  Bit equality with the aligned run is not required -- a lane sums other columns, in
    another order -- so the scores go through the comparator with the scalar chain; integer data is exact.  The stream kernels and the GEMM
    over the rows decline misaligned rows; the GEMM over an image of them is pinned off, so every batch size scans."""
    for kind in ("int", "float"):
        E, Q = ref.int_case(dim, ref.N_ROWS, 7) if kind == "int" else ref.float_case(dim, "f32", ref.N_ROWS, 7)
        idx = raglite_amd.DeviceIndex(shifted(torch_cuda, E), metric=metric)
        try:
            with idx.options(planes_gemm=0, fused_topk=0):  # (dim 2048, seven queries: the GEMM over an image of the rows would take them)
                for B in (1, 2, 3, 4, 7):
                    what = f"misaligned rows dim {dim} {metric} {kind} B {B}"
                    if kind == "int":
                        check_int(idx, E, Q[:B], metric, what)
                    else:
                        check_float(idx, E, Q[:B], metric, "f32", aligned=False, what=what)
        finally:
            idx.close()


@pytest.mark.parametrize("metric", ref.METRICS)
@pytest.mark.parametrize("dim", ref.MISALIGNED_DIMS)
def test_misaligned_queries_take_the_scalar_family(torch_cuda, dim, metric):
    """An aligned corpus (its norms measured by `row_norms_kernel<NV, 4>`) with a query tensor 4 bytes past 16-byte alignment: the scan falls
    back to scalar loads for rows and queries (`launch_scan_rows`: both must be aligned)."""
    for kind in ("int", "float"):
        E, Q = ref.int_case(dim, ref.N_ROWS, 7) if kind == "int" else ref.float_case(dim, "f32", ref.N_ROWS, 7)
        idx = raglite_amd.DeviceIndex(E, metric=metric)
        try:
            with idx.options(planes_gemm=0, fused_topk=0):  # (dim 2048, seven queries: the GEMM over the image would take them)
                for B in (1, 3, 4, 7):
                    what = f"misaligned queries dim {dim} {metric} {kind} B {B}"
                    q = shifted(torch_cuda, Q[:B])
                    if kind == "int":
                        ref.assert_exact(*search_all(idx, q, len(E)), E, Q[:B], metric, what)
                    else:
                        S, R = search_all(idx, q, len(E))
                        ref.assert_search(S, R, E, Q[:B], metric, "f32", aligned=False, norms_aligned=True, what=what)
        finally:
            idx.close()


# ---- 2. row counts and the persistent loop -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ref.METRICS)
@pytest.mark.parametrize("dim", [63, 260])
def test_small_row_counts(dim, metric):
    """n = 1 .. 33: a grid of one block up to five, a wave's second row present (`has1`) or not, the last row on either member of a pair."""
    for n in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33):
        run_width(dim, metric, "f32", (3,), n=n)


@pytest.mark.parametrize("metric", ref.METRICS)
@pytest.mark.parametrize("dim,n", [(5, 40_000), (8, 40_000), (2052, 20_000)])
def test_second_and_third_trip(dim, n, metric):
    """More rows than the resident grid covers in one trip (at most 8 blocks of 256 threads per CU, 8 rows per block and trip: 16 384 rows on
    256 CUs; the 2052-wide kernel, with its registers, far fewer): every row read back through chunk filters of 2048 rows each.  The corpus
    repeats 509 base rows, so the reference is computed once for those."""
    B = 2 if dim < 1024 else 1
    for kind in ("int", "float"):
        base, Q = ref.int_case(dim, ref.TILE_PERIOD, B) if kind == "int" else ref.float_case(dim, "f32", ref.TILE_PERIOD, B)
        rows = np.arange(n) % ref.TILE_PERIOD
        idx = raglite_amd.DeviceIndex(ref.tiled(base, n), metric=metric)
        try:
            got = by_row_windows(idx, Q, n)
        finally:
            idx.close()
        if kind == "int":
            want = np.stack([sim_fp32_exact(base, Q[b], metric) for b in range(B)])[:, rows]
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan]), (dim, n, metric)
        else:
            aligned = dim % 4 == 0
            ref.assert_within(got, ref.reference(base, Q, metric)[:, rows], ref.bound(base, Q, metric, "f32", aligned)[:, rows], f"dim {dim} n {n} {metric}")


# ---- 3. bit-equality promises ------------------------------------------------------------------------------------------------------------------------
BATCH_PLACE_CASES = [(d, "f32", m) for d in (63, 260, 772, 2052) for m in ref.METRICS] + [(512, "f16", "l2")] + \
                    [(d, "f16", m) for d in (1152, 3200) for m in ref.METRICS]  # (an fp16-stored index up to dim 1024 scans only for l2)


@pytest.mark.parametrize("dim,storage,metric", BATCH_PLACE_CASES)
def test_a_query_scores_the_same_wherever_it_sits_in_the_batch(dim, storage, metric):
    """Query b of a batch of 2, 3, 4 and 7 has the bits of the single-query call: the passes of 4, 2 and 1 queries (`BQ`) and the lane that
    finishes a query (`lane == b`) change nothing."""
    n = ref.N_ROWS
    batches = (2, 3, 4) if storage == "f16" and dim <= 1024 else (2, 3, 4, 7)
    E, Q = ref.float_case(dim, storage, n, 7)
    idx = make_index(E, metric, storage)
    try:
        with idx.options(planes_gemm=0, fused_topk=0):
            single = np.stack([ref.scatter(*search_all(idx, Q[b], n), n)[0] for b in range(7)])
            for B in batches:
                got = ref.scatter(*search_all(idx, Q[:B], n), n)
                assert np.array_equal(bits(got), bits(single[:B])), (dim, storage, metric, B)
    finally:
        idx.close()


@pytest.mark.parametrize("metric", ref.METRICS)
@pytest.mark.parametrize("dim", [63, 260])
def test_a_row_scores_the_same_wherever_it_sits(dim, metric):
    """What `search_rows_hi` relies on when it re-scores gathered candidates: a row's score does not depend on its position.  20 000 rows
    (past one trip of the grid): the index over E[37:] and the index over E in reversed row order return, row for row, the bits of the
    index over E."""
    n, B = 20_000, 2
    base, Q = ref.float_case(dim, "f32", ref.TILE_PERIOD, B)
    E = ref.tiled(base, n)
    got = {}
    for name, rows in (("original", E), ("from row 37", E[37:]), ("reversed", E[::-1])):
        idx = raglite_amd.DeviceIndex(np.ascontiguousarray(rows), metric=metric)
        try:
            got[name] = by_row_windows(idx, Q, len(rows))
        finally:
            idx.close()
    assert np.array_equal(bits(got["from row 37"]), bits(got["original"][:, 37:])), (dim, metric)
    assert np.array_equal(bits(got["reversed"]), bits(got["original"][:, ::-1])), (dim, metric)
    rows = np.arange(n) % ref.TILE_PERIOD
    ref.assert_within(got["original"], ref.reference(base, Q, metric)[:, rows], ref.bound(base, Q, metric, "f32", dim % 4 == 0)[:, rows], f"dim {dim} {metric}")


@pytest.mark.parametrize("metric", ref.METRICS)
@pytest.mark.parametrize("dim", [63, 260])
def test_host_arrays_and_device_tensors_give_the_same_bits(torch_cuda, dim, metric):
    n, B = ref.N_ROWS, 3
    E, Q = ref.float_case(dim, "f32", n, B)
    h = raglite_amd.DeviceIndex(E, metric=metric)
    d = raglite_amd.DeviceIndex(torch_cuda.tensor(np.array(E), device="cuda"), metric=metric)
    try:
        want = search_all(h, Q, n)
        for idx, q in ((h, torch_cuda.tensor(np.array(Q), device="cuda")), (d, Q), (d, torch_cuda.tensor(np.array(Q), device="cuda"))):
            S, R = search_all(idx, q, n)
            assert np.array_equal(bits(S), bits(want[0])) and np.array_equal(R, want[1])
    finally:
        h.close()
        d.close()


@pytest.mark.parametrize("metric", ref.METRICS)
@pytest.mark.parametrize("dim", [63, 2052])
def test_an_appended_index_scores_like_a_fresh_one(dim, metric):
    """Two appends (1 row, 300 rows): rows and the row norms of the appended tail (`launch_row_norms` on the tail alone) give the bits of an
    index created over all the rows."""
    n0, B = ref.N_ROWS, 3
    n = n0 + 301
    E, Q = ref.float_case(dim, "f32", n, B)
    grown = raglite_amd.DeviceIndex(E[:n0], metric=metric)
    fresh = raglite_amd.DeviceIndex(E, metric=metric)
    try:
        grown.append(E[n0:n0 + 1])
        grown.append(E[n0 + 1:])
        S, R = search_all(grown, Q, n)
        want = search_all(fresh, Q, n)
        assert np.array_equal(bits(S), bits(want[0])) and np.array_equal(R, want[1])
        ref.assert_search(S, R, E, Q, metric, "f32", dim % 4 == 0, what=f"appended dim {dim} {metric}")
    finally:
        grown.close()
        fresh.close()


# ---- 4. fp16-stored index ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", ref.F16_L2_DIMS)
def test_f16_l2_scan(dim):
    """`scan_rows16_kernel<1>` (128, 512) and `<2>` (768, 1024): the l2 route of up to four queries, passes of 4, 2 and 1.  768 is the
    narrowest width of `<2>` an index can have: see `test_f16_width_640_cannot_be_created`."""
    run_width(dim, "l2", "f16", (1, 2, 3, 4))


def test_f16_width_640_cannot_be_created():
    """`scan_rows16_kernel<2>` would take 520 .. 1024, but up to 1024 an fp16-stored index exists only at the stream kernels' widths: 640 is
    refused at creation (every metric), so no search reaches the scan with it."""
    for metric in ref.METRICS:
        with pytest.raises(UnsupportedError, match="rl_index_create_f16: dim must be one of 128, 256, 384, 512, 768, 1024"):
            make_index(ref.int_case(640, 8, 1)[0], metric, "f16")


@pytest.mark.parametrize("metric", ref.METRICS)
@pytest.mark.parametrize("dim", ref.F16_WIDE_DIMS)
def test_f16_wide_scan(dim, metric):
    """`scan_rows16_wide_kernel<NV, BQ, L2>`, the only row scorer of a wide fp16-stored index without an image: NV = 4 (1152, 2048; passes of
    4, 2, 1), 6 (2176, 3072; 2, 1), 8 (3200, 4096; 2, 1), L2 on and off; norms by `row_norms16_kernel<8>`.  From five queries up the GEMM over
    the image would take the batch: pinned off, so that seven queries scan."""
    run_width(dim, metric, "f16", (1, 2, 3, 4, 7), n=ref.N_ROWS_F16_WIDE, pin={"planes_gemm": 0, "fused_topk": 0})


@pytest.mark.parametrize("dim", [128, 512, 768, 1024, 1152])
def test_f16_row_norms_and_f32_parity_on_integer_data(dim):
    """`row_norms16_kernel<1>` (128, 512), `<2>` (768, 1024), `<8>` (1152) through the cosine, `|e|^2` through l2; and in every metric the
    fp16-stored index returns the scores and rows of an fp32 index holding the same values (integer data: exact on both)."""
    n = ref.N_ROWS
    E, Q = ref.int_case(dim, n, 2)
    for metric in ref.METRICS:
        h = make_index(E, metric, "f16")
        f = make_index(E, metric, "f32")
        try:
            for B in (1, 2):
                S, R = check_int(h, E, Q[:B], metric, f"f16 dim {dim} {metric} B {B}")
                S32, R32 = search_all(f, Q[:B], n)
                assert np.array_equal(R, R32) and np.array_equal(bits(S), bits(S32)), (dim, metric, B)
        finally:
            h.close()
            f.close()


# ---- 5. non-finite and degenerate rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ref.METRICS)
@pytest.mark.parametrize("dim", [63, 260])
def test_non_finite_and_zero_rows_beside_healthy_ones(dim, metric):
    """40 rows = 5 blocks = 20 waves: wave w scores rows w and w + 20 together.  A zero row, a row with one inf and a row with one NaN are
    planted once among the first members of a pair (rows 2, 5, 7) and once among the second (rows 25, 31, 36), and query 1 of 3 is zero.
    Healthy rows keep the bits they have without the planted rows; NaN scores rank last as `oracle.topk_desc` orders them; a zero row (and
    a zero query) under cosine is 0 / 0 = NaN, per `finish_score` as written."""
    n, B = 40, 3
    E0, Q0 = ref.float_case(dim, "f32", n, B)
    E, Q = E0.copy(), Q0.copy()
    Q[1] = 0.0
    planted = {2: "zero", 25: "zero", 5: "inf", 31: "inf", 7: "nan", 36: "nan"}
    for r, what in planted.items():
        if what == "zero":
            E[r] = 0.0
        else:
            E[r, dim // 2] = np.inf if what == "inf" else np.nan
    healthy = np.setdiff1d(np.arange(n), list(planted))
    clean = raglite_amd.DeviceIndex(E0, metric=metric)
    dirty = raglite_amd.DeviceIndex(E, metric=metric)
    try:
        want = ref.scatter(*search_all(clean, Q0, n), n)
        S, R = search_all(dirty, Q, n)
    finally:
        clean.close()
        dirty.close()
    got = np.empty((B, n), dtype=np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        full = ref.reference(E, Q, metric)
    for b in range(B):
        assert np.array_equal(np.sort(R[b, :n]), np.arange(n)) and np.all(R[b, n:] == -1) and np.all(np.isneginf(S[b, n:]))
        got[b, R[b, :n]] = S[b, :n]
        assert np.array_equal(R[b, :n], oracle.topk_desc(got[b], n)[1]), f"query {b}: NaN scores must rank last, ties by row"
    for b in (0, 2):
        assert np.array_equal(bits(got[b, healthy]), bits(want[b, healthy])), f"query {b}: a healthy row changed beside the planted rows"
    assert np.array_equal(np.isnan(got), np.isnan(full)), "NaN scores are not where the reference has them"
    inf = np.isinf(full)
    assert np.array_equal(got[inf].astype(np.float64), full[inf])
    if metric == "cosine":
        assert np.all(np.isnan(got[:, [2, 25]])) and np.all(np.isnan(got[1]))
    fin = np.isfinite(full)
    fin[:, healthy] &= np.array([False, True, False])[:, None]  # (the healthy rows of queries 0 and 2 were compared bit for bit above)
    if fin.any():
        Ez = np.where(np.isfinite(E), E, 0.0)
        bnd = ref.bound(Ez, Q, metric, "f32", dim % 4 == 0)
        bnd = np.where(np.isfinite(bnd), bnd, 0.0) + 2.0 ** -24  # (a zero row against a zero query: exactly 1)
        assert np.all(np.abs(got[fin].astype(np.float64) - full[fin]) <= bnd[fin])


# ---- 6. the query adapter at scan-only widths ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", ref.ADAPTER_DIMS)
def test_adapter_apply_at_scan_only_widths(dim):
    """`rl_adapter_apply` = the scan in raw-dot mode over the rows of A.  No MFMA kernel takes these widths, so every batch size scans:
    against Q A^T in float64 with the raw-dot bound, integer data exactly; the fp16 output is the fp32 output cast once."""
    A, Q = ref.float_case(dim, "f32", dim, 7)
    Ai, Qi = ref.int_case(dim, dim, 7)
    for B in (1, 2, 4, 7):
        out = raglite_amd.adapter_apply(A, Q[:B])
        ref.assert_within(out, ref.reference(A, Q[:B], "raw"), ref.bound(A, Q[:B], "raw", "f32", False), f"adapter dim {dim} B {B}")
        outi = raglite_amd.adapter_apply(Ai, Qi[:B])
        assert np.array_equal(outi, (Qi[:B].astype(np.float64) @ Ai.astype(np.float64).T).astype(np.float32))
        h = raglite_amd.adapter_apply(A, Q[:B], want_f16=True)
        assert h.dtype == np.float16 and np.array_equal(h.view(np.uint16), out.astype(np.float16).view(np.uint16))


def test_adapter_f16_cast_second_trip():
    """300 x 2047 = 614 100 outputs: more than the 2048 x 256 threads of `cast_f16_kernel`'s grid, so its loop takes a second trip."""
    dim, B = 2047, 300
    A = ref.float_case(dim, "f32", dim, 1)[0]
    Q = ref.same_sign_queries(9000 + dim, B, dim)
    out = raglite_amd.adapter_apply(A, Q)
    assert B * dim > 2048 * 256
    ref.assert_within(out, ref.reference(A, Q, "raw"), ref.bound(A, Q, "raw", "f32", False), "adapter 300 x 2047")
    h = raglite_amd.adapter_apply(A, Q, want_f16=True)
    assert np.array_equal(h.view(np.uint16), out.astype(np.float16).view(np.uint16))


# ---- 7. MaxSim over the same odd widths -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [63, 257, 2047])
def test_maxsim_at_odd_widths_integer_exact(dim):
    """`launch_maxsim_generic`'s scalar instantiations: ragged chunks with empty ones, three query vectors, integer data -- `maxsim_scores`
    and `search_chunks` bit-equal to the oracle (as tests/test_gpu_parity.py::test_fuzz_ragged_shapes_integer_exact does at its widths)."""
    n, nq = 300, 3
    off = ragged_offsets(np.random.default_rng(dim), n, 1, 15, empty_every=7)
    sizes = np.diff(off)
    assert (sizes == 0).any()
    E, Q = ref.int_case(dim, n, nq)
    idx = raglite_amd.DeviceIndex(E, off, metric="dot")
    try:
        want = oracle.maxsim_scores(E, off, Q).astype(np.float32)
        assert np.array_equal(idx.maxsim_scores(Q), want)
        r2c = np.repeat(np.arange(len(sizes)), sizes)
        gs, gc, cnt = idx.search_chunks(Q[0], 20, 5)
        ws, wc = oracle.search_chunks(E, r2c, Q[0], 20, 5, "dot", np.float32)
        assert int(cnt) == len(wc) and np.array_equal(gc[: len(wc)], wc) and np.array_equal(gs[: len(wc)], ws)
    finally:
        idx.close()


# ---- 8. width limits --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ref.METRICS)
def test_creation_and_search_agree_on_the_widths(torch_cuda, metric):
    """No index may be created that no search can answer: above 2048 an fp32 index needs dim % 4 == 0 and 16-byte aligned borrowed rows, and
    `rl_index_create` says so with one message for every metric; what it accepts, every search answers."""
    message = "dim above 2048 must be a multiple of 4"
    for dim in (2049, 2050, 2051, 3001, 4095):
        with pytest.raises(UnsupportedError, match=message):
            raglite_amd.DeviceIndex(np.ones((4, dim), dtype=np.float32), metric=metric)
    E, Q = ref.int_case(2052, 9, 2)
    with pytest.raises(UnsupportedError, match=message):
        raglite_amd.DeviceIndex(shifted(torch_cuda, E), metric=metric)
    with pytest.raises(UnsupportedError, match="dim must be <= 4096"):
        raglite_amd.DeviceIndex(np.ones((4, 4100), dtype=np.float32), metric=metric)
    for dim, rows in ((2047, None), (2048, "shifted"), (2052, None), (4092, None), (4096, None)):
        E, Q = ref.int_case(dim, 9, 2)
        idx = raglite_amd.DeviceIndex(shifted(torch_cuda, E) if rows else E, metric=metric)
        try:
            check_int(idx, E, Q, metric, f"dim {dim} {metric}")
            if dim > 2048:  # a misaligned device query over such an index: refused by the search, not answered wrongly
                with pytest.raises(UnsupportedError, match="similarity scan"):
                    idx.search_rows(shifted(torch_cuda, Q), 4)
        finally:
            idx.close()
