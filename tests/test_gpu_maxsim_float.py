"""The exact MaxSim kernels ONE BY ONE on the GPU, on FLOAT data, through the public binding only: every chunk score of every case of
tests/maxsim_ref.py held to the float64 reference within the bound derived there from the kernel's own code.  The integer-data tests
(test_gpu_parity.py, test_gpu_pairs_packed.py, test_gpu_wide_dim.py) cannot see a defect of the arithmetic: every lo half is zero, every sum
exact, no scale matters.

  `DeviceIndex.maxsim_scores`      maxsim_stream_kernel mode 0 at its six widths, both query-tile counts, in f16_split, after
                                   `set_exact_fp32()` and over fp16-stored rows; 33 and 70 vectors (accumulating passes); a workgroup that
                                   walks five tiles and more; maxsim_generic_kernel at both ends of its eight instantiations, with a
                                   misaligned query or row tensor; maxsim_pairs_wide_kernel<true> over every chunk of a wide fp16 index
  `DeviceIndex.maxsim_rerank`      maxsim_cand_kernel (dim 128) in its three arithmetics and two tile counts; the pairs kernels under
                                   `options(pairs_packed=0 / 1 / 2)` over fp32 and fp16-stored rows, the wide kernel beyond 1024; the generic
                                   kernel (more than 32 vectors, widths that are no multiple of 16, a misaligned query tensor)
  `DeviceIndex.maxsim_topk_batch`  two queries of 17 .. 32 vectors over an index with empty chunks: maxsim_stream2_kernel over fp32 rows
                                   (split) and fp16-stored rows.  Each returned score against float64 of the returned chunk.

Every score goes through `scan_ref.assert_within`; -inf stands exactly where the reference has it; nothing is NaN; the queries times a
power of two give the scores times that power, bit for bit.  Each case's worst error / bound goes to profiles/maxsim_float_error.txt.

The pairs kernels at dim 128: `maxsim_rerank` gives that width to the cand kernel, and the routes of `maxsim_topk_batch` that re-score with the
pairs kernels need the HI plane, which an index builds from 64 Mi elements on (half a million rows at this width): no quick test reaches
them.  The instantiations that width would run, <true, 128> and the packed ones, run here at dim 384.

Instantiations the binding cannot reach (tests/test_maxsim_ref_host.py counts the rest):
  maxsim_pairs_kernel<false, 128, true>            an fp16-stored index has a stream width or a multiple of 128 (rl_index_create_f16)
  maxsim_pairs_packed_kernel<256, false, DBG != 0>  experiment builds only
  maxsim_stream_kernel / maxsim_stream2_kernel with TRACE, SPLR != 6   experiment builds only
  maxsim_stream_kernel mode 1                       row scores: out of scope here (tests/test_gpu_scan.py, tests/test_gpu_score_gemm.py)
"""

import time
from pathlib import Path

import numpy as np
import pytest

import raglite_amd
from tests import maxsim_ref as ref
from tests import scan_ref

pytestmark = pytest.mark.gpu

_ids = lambda cases: [c.name for c in cases]  # noqa: E731
POW2 = 2.0 ** -3  # the queries times this: every score times this, exactly


def host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def shifted(torch, x):
    """A contiguous CUDA view whose data pointer is 4 bytes past 16-byte alignment."""
    x = np.asarray(x, dtype=np.float32)
    flat = torch.zeros(x.size + 8, device="cuda")
    flat[1:1 + x.size] = torch.tensor(np.array(x).ravel(), device="cuda")
    v = flat[1:1 + x.size].view(*x.shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.fixture(scope="module")
def error_log():
    lines, t0 = [], time.time()
    yield lines
    try:  # (a read-only checkout keeps the committed figures)
        out = Path(__file__).resolve().parent.parent / "profiles" / "maxsim_float_error.txt"
        head = ("# tests/test_gpu_maxsim_float.py: the worst |kernel - float64| / bound over a case's chunk scores (all its queries); every figure is\n"
                "# asserted <= 1.  Bounds: tests/maxsim_ref.py.  One line per (case, kernel, arithmetic); the case's name says which branch it takes.\n"
                "# Bit-for-bit comparisons (queries times a power of two) are not listed: they have no figure.\n"
                "# Found by these tests: maxsim_cand_kernel over fp16-stored rows split the query into fp16 (hi, lo) WITHOUT scaling it first, so the lo\n"
                "# half of every element below 2^-2 was subnormal.  Before the fix `cand_nq1_cand1_f16_stored` failed: the scores of the queries times 2^-3\n"
                "# were not 2^-3 times the scores, bit for bit (the only cand case over fp16 rows whose list the binding took in that run: the others asked\n"
                "# for an ordinal past the last chunk, which a host list may not hold); its error / bound against float64 was inside 1,\n"
                "# because the bound charged the unscaled split its 2^-25 floor.  The kernel now scales the query as it does over fp32 rows.\n")
        out.write_text(head + "".join(sorted(lines)) + f"# wall time of the module: {time.time() - t0:.0f} s\n")
    except OSError:
        pass


def _log(error_log, c, ratio):
    line = f"{c.name} | {c.kernel} ({c.inst}) | {c.arith} | {ratio:.4f}\n"
    print(line, end="")
    error_log.append(line)
    assert ratio <= 1.0, line


def _index(c, torch):
    E, off, _, _ = c.data()  # noqa: N806
    rows = shifted(torch, E) if c.shift == "rows" else (E.astype(np.float16) if c.storage == "f16" else E)
    idx = raglite_amd.DeviceIndex(rows, off, metric="dot", storage=c.storage)
    if c.exact:
        idx.set_exact_fp32()
    assert idx.arithmetic == c.arith, f"{c.name}: the index selected {idx.arithmetic}"
    return idx


def _launch(c, idx, torch, Q, cand, k=0):  # noqa: N803
    q = shifted(torch, Q) if c.shift == "queries" else Q
    if c.entry == "scores":
        return np.stack([host(idx.maxsim_scores(q[b])) for b in range(len(Q))])
    if c.entry == "rerank":
        cd = torch.tensor(np.array(cand), device="cuda") if c.shift == "queries" else np.array(cand)  # (one call, one side)
        if c.packed < 0:
            return host(idx.maxsim_rerank(q, cd))
        with idx.options(pairs_packed=c.packed):
            return host(idx.maxsim_rerank(q, cd))
    S, C = idx.maxsim_topk_batch(q, k)  # noqa: N806
    return host(S), host(C)


def _within(c, got, want, bound):
    """No NaN, -inf exactly where the reference has it, every other score within its bound -> the largest error / bound."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape and not np.isnan(got).any(), f"{c.name}: NaN"
    fin = np.isfinite(want)
    assert np.array_equal(np.isneginf(got), ~fin) and np.all(np.isfinite(got[fin])), f"{c.name}: -inf is not exactly where the reference has it"
    return scan_ref.assert_within(got[fin], want[fin], bound[fin], c.name) if fin.any() else 0.0


def _check_topk(c, S, C, refs):  # noqa: N803
    """`assert_topk_close` with the derived bound in place of a tolerance: each returned score against float64 of the RETURNED chunk;
    non-increasing; distinct chunks; as many finite scores as there are to return; nothing clearly better left out."""
    worst = 0.0
    for b, (want, bound) in enumerate(refs):
        s, ch = S[b].astype(np.float64), C[b].astype(np.int64)
        assert not np.isnan(s).any() and np.all(s[:-1] >= s[1:]), f"{c.name} query {b}"
        live = ch >= 0
        assert len(set(ch[live].tolist())) == int(live.sum()) and np.all(np.isneginf(s[~live]))
        assert int(np.isfinite(s).sum()) == min(len(s), int(np.isfinite(want).sum())), f"{c.name} query {b}: finite scores returned"
        worst = max(worst, _within(c, s[live], want[ch[live]], bound[ch[live]]))
        rest = np.setdiff1d(np.nonzero(np.isfinite(want))[0], ch[live])  # nothing clearly better was missed: a chunk left out scored, on the
        if rest.size:                                                    # device, no more than the last one returned
            assert np.all(want[rest] - bound[rest] <= s[-1]), f"{c.name} query {b}: a chunk better than the last returned one was left out"
    return worst


def _run_case(torch, error_log, c):
    E, off, Q, cand = c.data()  # noqa: N806
    refs = ref.references(c)
    idx = _index(c, torch)
    try:
        k = min(len(off) - 1, 2048)  # (top-k cases: every chunk comes back where the index has no more than the largest k)
        got = _launch(c, idx, torch, Q, cand, k)
        scaled = _launch(c, idx, torch, Q * np.float32(POW2), cand, k)
        if c.entry == "topk":
            # (what sends two queries of 17 .. 32 vectors through ONE pass of the two-query kernel: the option, the arithmetic asserted above,
            # and empty chunks, which the bound-filtered routes decline)
            assert idx.get_option("query_pairs") == 1 and np.any(np.diff(off) == 0) and len(Q) == 2 and 16 < c.nq <= 32
            worst = _check_topk(c, got[0], got[1], refs)
            assert np.array_equal(got[1], scaled[1]), f"{c.name}: the queries times 2^-3 rank differently"
            got, scaled = got[0], scaled[0]
        else:
            worst = 0.0
            for b, (want, bound) in enumerate(refs):
                w, bd = (ref.take(want, cand[b]), ref.take(bound, cand[b])) if c.entry == "rerank" else (want, bound)
                worst = max(worst, _within(c, got[b], w, np.where(np.isfinite(w), bd, 0.0)))
        assert np.array_equal(_bits(scaled), _bits(got * np.float32(POW2))), f"{c.name}: the queries times 2^-3 do not give the scores times 2^-3"
        _log(error_log, c, worst)
    finally:
        idx.close()


STREAM, GENERIC, CAND, PAIRS, TOPK = ref.stream_cases(), ref.generic_cases(), ref.cand_cases(), ref.pairs_cases(), ref.topk_cases()


@pytest.mark.parametrize("case", STREAM, ids=_ids(STREAM))
def test_stream_kernel(torch_cuda, error_log, case):
    """`maxsim_scores` at a stream width: `maxsim_stream_kernel<KW, NQT, 0, ...>` in the arithmetic the case names."""
    _run_case(torch_cuda, error_log, case)


@pytest.mark.parametrize("case", GENERIC, ids=_ids(GENERIC))
def test_generic_kernel(torch_cuda, error_log, case):
    """`maxsim_scores` outside the stream widths, `maxsim_rerank` where the MFMA kernels decline: `maxsim_generic_kernel<NV, VEC>`."""
    _run_case(torch_cuda, error_log, case)


@pytest.mark.parametrize("case", CAND, ids=_ids(CAND))
def test_cand_kernel(torch_cuda, error_log, case):
    """`maxsim_rerank` at dim 128: `maxsim_cand_kernel<NQT, F16, SPLIT>`; several queries per launch, lists of 1 .. 300 candidates."""
    _run_case(torch_cuda, error_log, case)


@pytest.mark.parametrize("case", PAIRS, ids=_ids(PAIRS))
def test_pairs_kernels(torch_cuda, error_log, case):
    """`maxsim_rerank` at the other multiples of 16 (and `maxsim_scores` over a wide fp16 index): the kernel `pairs_choice` names."""
    _run_case(torch_cuda, error_log, case)


@pytest.mark.parametrize("case", TOPK, ids=_ids(TOPK))
def test_topk_batch(torch_cuda, error_log, case):
    """`maxsim_topk_batch`: two queries per pass (`maxsim_stream2_kernel`)."""
    _run_case(torch_cuda, error_log, case)


# ---- rerank over every chunk against the scores of the same query ---------------------------------------------------------------------------
AGREE = [(d, st, ex) for d in ref.STREAM_DIMS + (48, 100, 2048) for st, ex in (("f32", False), ("f32", True), ("f16", False))
         if st == "f32" or d in ref.STREAM_DIMS + (2048,)]  # (an fp16-stored index has a stream width or a multiple of 128)


@pytest.mark.parametrize("dim, storage, exact", AGREE)
def test_rerank_of_every_chunk_agrees_with_scores(torch_cuda, dim, storage, exact):
    """Two kernels, one query: `maxsim_rerank` over the list 0 .. n_chunks - 1 and `maxsim_scores` differ by at most the sum of their bounds."""
    by_scores = "stream" if dim in ref.STREAM_DIMS else "pairs" if storage == "f16" else "generic"
    by_rerank = "cand" if dim == 128 else "pairs" if dim % 16 == 0 else "generic"
    a = ref.Case("agree", "scores", by_scores, "", dim, 17, n=131, storage=storage, exact=exact)
    b = ref.Case("agree", "rerank", by_rerank, "", dim, 17, n=131, storage=storage, exact=exact)
    (want, bound_a), (_, bound_b) = ref.references(a)[0], ref.references(b)[0]
    E, off, Q, _ = a.data()  # noqa: N806
    idx = _index(a, torch_cuda)
    try:
        s = host(idx.maxsim_scores(Q[0])).astype(np.float64)
        r = host(idx.maxsim_rerank(Q, np.arange(len(off) - 1, dtype=np.int32)[None, :]))[0].astype(np.float64)
    finally:
        idx.close()
    fin = np.isfinite(want)
    assert np.array_equal(np.isneginf(s), ~fin) and np.array_equal(np.isneginf(r), ~fin)
    assert np.all(np.abs(s[fin] - r[fin]) <= (bound_a + bound_b)[fin])
    _within(a, s, want, bound_a)
    _within(b, r, want, bound_b)


# ---- the row scale -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [128, 1024])
def test_scores_are_consistent_with_the_restated_row_scale(torch_cuda, dim):
    """The binding has no accessor for the index's `e_scale`; `maxsim_ref.row_scale` restates the rule.  Rows of 21-bit integers are exact
    as an fp16 (hi, lo) pair at that scale (the largest, 2^21 - 1, lands just below 2^14); one-hot +-1 query vectors make every dot one
    element: the split kernels must return the integers' sums bit for bit, through the stream kernel and (dim 128) the cand kernel."""
    rng = np.random.default_rng(dim)
    n, nq = 131, 5
    E = rng.integers(-(2 ** 21) + 1, 2 ** 21, (n, dim)).astype(np.float32)  # noqa: N806
    E[7, 3] = 2.0 ** 21 - 1
    off = ref.make_offsets("ragged", 9, n)
    Q = np.zeros((1, nq, dim), dtype=np.float32)  # noqa: N806
    Q[0, np.arange(nq), rng.integers(0, dim, nq)] = [1, -1, 1, -1, 1]
    s = ref.row_scale(E)
    assert s == 2.0 ** -7 and np.array_equal(ref.d_restated(E, Q[0], s, "stream", "f16_split"), ref.dots(E, Q[0]))
    assert np.abs(ref.split_rows(E, s)[2]).max() == (2.0 ** 21 - 1) / 128
    want = ref.scores(E, off, Q[0])
    idx = raglite_amd.DeviceIndex(E, off, metric="dot")
    try:
        assert idx.arithmetic == "f16_split"
        got = host(idx.maxsim_scores(Q[0])).astype(np.float64)
        assert np.array_equal(got, want)
        if dim == 128:
            cand = np.arange(len(off) - 1, dtype=np.int32)[None, :]
            assert np.array_equal(host(idx.maxsim_rerank(Q, cand))[0].astype(np.float64), want)
    finally:
        idx.close()
