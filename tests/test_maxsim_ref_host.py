"""tests/maxsim_ref.py without a GPU: the reference is the oracle's on integer data; the restated split and the fp32 chains restated in
NumPy float32 stay inside their own bounds on every case (the largest ratio is printed: the bounds are not too tight for a correct
kernel); every planted defect exceeds the bound on a named case of every kernel it applies to (the bounds are not too loose); the restated
launcher choices hold against the conditions in the source; every case names an arithmetic the index will really select."""

import re
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle
from tests import maxsim_ref as ref
from tests import scan_ref

CSRC = Path(__file__).resolve().parent.parent / "raglite_amd" / "csrc"
CASES = ref.all_cases()
SMALL = tuple(c for c in CASES if c.n < 5000)  # (the long-walk cases repeat the arithmetic of the small ones over more rows)
HALVES = ("f16_split", "f16_stored")


def _split_kernel(c):
    return c.kernel in ("stream", "stream2", "cand") and c.arith in HALVES


def _scale(c, E):  # noqa: N803
    return ref.row_scale(E) if c.arith == "f16_split" else 0.0


def _ratio(got, want, bound):
    """Largest |got - want| / bound over the finite scores; the -inf pattern must agree."""
    fin = np.isfinite(want)
    assert np.array_equal(np.isneginf(got), ~fin)
    if not fin.any():
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got - want)[fin] / bound[fin]
    return float(np.nanmax(np.where(bound[fin] > 0, r, np.where(got[fin] == want[fin], 0.0, np.inf))))


# ---- the reference -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim, nq, layout", [(128, 17, "ragged"), (100, 5, "big"), (1024, 32, "rows"), (48, 70, "ragged")])
def test_reference_is_the_oracle_on_integer_data(dim, nq, layout):
    n = 403
    E, Q = scan_ref.int_data(11 + dim, n, dim), scan_ref.int_data(12 + dim, nq, dim)  # noqa: N806
    off = ref.make_offsets(layout, 5, n)
    want = oracle.maxsim_scores(E, off, Q)
    got = ref.scores(E, off, Q)
    assert np.array_equal(got, want) and np.isneginf(got).sum() == int((np.diff(off) == 0).sum())
    cand = np.array(ref.make_candidates(7, 1, 60, len(off) - 1)[0])
    ok = (cand >= 0) & (cand < len(off) - 1)
    assert np.array_equal(ref.take(got, cand)[ok], oracle.maxsim_candidates(E, off, Q, cand[ok]))
    assert np.all(np.isneginf(ref.take(got, cand)[~ok])) and (~ok).sum() == 2 and np.all(cand[~ok] == -1)


# ---- restatements inside their own bounds ----------------------------------------------------------------------------------------------
def _generic_f32(E, Q, aligned):  # noqa: N803
    """`maxsim_generic_kernel`'s dot in float32: lane l runs an fma chain over its slots (v * 64 + l) * VEC + j, then the butterfly."""
    E32, Q32 = np.asarray(E, dtype=np.float32), np.asarray(Q, dtype=np.float32)  # noqa: N806
    dim = E32.shape[1]
    nv, vec = ref.generic_instantiation(dim, aligned)
    lanes = np.arange(64)
    acc = np.zeros((64, len(Q32), len(E32)), dtype=np.float32)
    for v in range(nv):
        for j in range(vec):
            c = (v * 64 + lanes) * vec + j
            live = c < dim
            cc = np.where(live, c, 0)
            x = np.where(live[:, None], E32[:, cc].T, 0).astype(np.float64)
            q = np.where(live[:, None], Q32[:, cc].T, 0).astype(np.float64)
            acc = (acc.astype(np.float64) + q[:, :, None] * x[:, None, :]).astype(np.float32)  # (an fma: one rounding)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lanes ^ o]
    return acc[0].astype(np.float64)


def _generic_sum_f32(V, off):  # noqa: N803
    """The generic kernel's sum over the vectors: lane-strided partial sums, then the butterfly."""
    m = ref.chunk_max(V, off).astype(np.float32)
    t = np.zeros((64, m.shape[1]), dtype=np.float32)
    with np.errstate(invalid="ignore"):
        for i in range(m.shape[0]):
            t[i % 64] = t[i % 64] + m[i]
        for o in (32, 16, 8, 4, 2, 1):
            t = t + t[np.arange(64) ^ o]
    return t[0].astype(np.float64)


def _restated_scores(c, E, off, q):  # noqa: N803
    """A correct kernel's chunk scores, restated on the host: the split in exact arithmetic, or the fp32 chain in float32."""
    if c.kernel == "generic":
        return _generic_sum_f32(_generic_f32(E, q, c.aligned), off)
    total = None
    for v0 in range(0, len(q), 32):
        qp = q[v0:v0 + 32]
        if _split_kernel(c):
            d = ref.d_restated(E, qp, _scale(c, E), c.kernel, c.arith)
            assert np.all(np.abs(d - ref.dots(E, qp)) <= ref.rep_bound(E, qp, _scale(c, E), c.kernel, c.arith)), f"{c.name}: the restated split leaves rep_bound"
        else:
            d = ref.chain_f32(E, qp, c.kernel)
        part = ref.sum_f32(d, off)
        with np.errstate(invalid="ignore"):
            total = part if total is None else (total.astype(np.float32) + part.astype(np.float32)).astype(np.float64)
    return total


@pytest.mark.parametrize("kernel", ["stream", "stream2", "cand", "pairs", "generic"])
def test_restatements_stay_inside_their_bounds(kernel):
    """Every small case of the kernel: the host restatement of a CORRECT kernel is within the score bound on every chunk."""
    worst, where = 0.0, ""
    for c in SMALL:
        if c.kernel != kernel:
            continue
        E, off, Q, _ = c.data()  # noqa: N806
        for q, (want, bound) in zip(Q, ref.references(c)):
            r = _ratio(_restated_scores(c, E, off, q), want, bound)
            assert r <= 1.0, (c.name, r)
            if r > worst:
                worst, where = r, c.name
    print(f"{kernel}: largest restatement error / bound {worst:.4f} ({where})")
    assert 0.0 < worst <= 1.0


# ---- planted defects --------------------------------------------------------------------------------------------------------------------
def _defect(name, c, E, off, q):  # noqa: N803
    s = _scale(c, E)
    if name == "dropped_el_qh":
        return ref.defect_dropped_lo(E, off, q, s, c.kernel, c.arith, "lh") if _split_kernel(c) and c.arith == "f16_split" else None
    if name == "dropped_eh_ql":
        return ref.defect_dropped_lo(E, off, q, s, c.kernel, c.arith, "hl") if _split_kernel(c) else None
    if name == "neighbour_scale":
        return ref.defect_neighbour_scale(E, off, q, s, c.kernel, c.arith) if _split_kernel(c) and c.kernel != "cand" else None
    if name == "row_past_end":
        return ref.defect_row_past_end(E, off, q)
    if name == "padded_vector":
        return ref.defect_padded_vector(E, off, q) if c.kernel != "generic" and len(q) % 16 else None
    if name == "carried_max":
        return ref.defect_carried_max(E, off, q)
    if name == "zero_max":
        return ref.defect_zero_max(E, off, q)
    if name == "skipped_tail":
        return ref.defect_skipped_tail(E, off, q) if c.kernel == "pairs" and c.dim % 128 and c.dim > 128 else None
    raise ValueError(name)


DEFECTS = ("dropped_el_qh", "dropped_eh_ql", "neighbour_scale", "row_past_end", "padded_vector", "carried_max", "zero_max", "skipped_tail")
APPLIES = {"dropped_el_qh": ("stream", "stream2", "cand"), "dropped_eh_ql": ("stream", "stream2", "cand"), "neighbour_scale": ("stream", "stream2"),
           "row_past_end": ("stream", "stream2", "cand", "pairs", "generic"), "padded_vector": ("stream", "stream2", "cand", "pairs"),
           "carried_max": ("stream", "stream2", "cand", "pairs", "generic"), "zero_max": ("stream", "stream2", "cand", "pairs", "generic"),
           "skipped_tail": ("pairs",)}


def _best(name, cases):
    best, where = 0.0, ""
    for c in cases:
        if len(c.data()[2][0]) > 32 and c.kernel != "generic":
            continue  # (the defects are stated per pass)
        E, off, Q, _ = c.data()  # noqa: N806
        got = _defect(name, c, E, off, Q[0])
        if got is None:
            continue
        want, bound = ref.references(c)[0]
        fin = np.isfinite(want)
        with np.errstate(invalid="ignore", divide="ignore"):
            r = float(np.max(np.abs(got - want)[fin] / bound[fin])) if fin.any() else 0.0
        if r > best:
            best, where = r, c.name
    return best, where


@pytest.mark.parametrize("name, kernel", [(d, k) for d in DEFECTS for k in APPLIES[d]])
def test_every_planted_defect_exceeds_the_bound(name, kernel):
    best, where = _best(name, [c for c in SMALL if c.kernel == kernel])
    print(f"{name} in {kernel}: error / bound {best:.1f} on {where}")
    assert best > 1.0, (name, kernel, best, where)


@pytest.mark.parametrize("name, arith", [("dropped_el_qh", "f16_split"), ("dropped_eh_ql", "f16_split"), ("dropped_eh_ql", "f16_stored")])
def test_a_dropped_lo_term_is_separated_at_dim_1024(name, arith):
    """What the one-hot probes are for: on dense data the worst-case accumulation bound hides the defect at this width
    (tests/score_gemm_ref.py, "Why probes")."""
    probes = [c for c in SMALL if c.kernel == "stream" and c.dim == 1024 and c.arith == arith and "one_hot_rows" in c.name]
    assert len(probes) == 2
    for c in probes:
        best, where = _best(name, [c])
        print(f"{name} at dim 1024, {arith}: error / bound {best:.1f} on {where}")
        assert best > 1.0, (name, best, where)
    dense = [c for c in SMALL if c.name == f"stream_dim1024_nq32_{arith}"]
    assert len(dense) == 1 and _best(name, dense)[0] < 1.0  # the defect that dense data lets through


# ---- the launchers, restated ---------------------------------------------------------------------------------------------------------------
def test_generic_instantiation_restates_the_launcher():
    want = {4: (1, 4), 256: (1, 4), 260: (2, 4), 512: (2, 4), 516: (4, 4), 1024: (4, 4), 1028: (8, 4), 2048: (8, 4), 2052: (16, 4), 4096: (16, 4),
            1: (2, 1), 127: (2, 1), 129: (8, 1), 511: (8, 1), 513: (32, 1), 2047: (32, 1)}
    assert {d: ref.generic_instantiation(d) for d in want} == want
    assert [ref.generic_instantiation(d, False) for d in (64, 128, 132, 512, 516, 2048)] == [(2, 1), (2, 1), (8, 1), (8, 1), (32, 1), (32, 1)]
    with pytest.raises(ValueError):
        ref.generic_instantiation(2052, False)
    src = (CSRC / "maxsim_generic.hip").read_text()
    assert "const int nv = (dim + 255) / 256;" in src and "const int nv = (dim + 63) / 64;" in src
    assert re.findall(r"nv <= (\d+)\) st = generic_t<(\d+), (\d)>", src) == [("1", "1", "4"), ("2", "2", "4"), ("4", "4", "4"), ("8", "8", "4"), ("16", "16", "4"),
                                                                              ("2", "2", "1"), ("8", "8", "1"), ("32", "32", "1")]
    assert "const bool vec4 = (dim % 4 == 0) && ((reinterpret_cast<uintptr_t>(D) & 15) == 0) &&" in src
    got = {c.inst for c in CASES if c.kernel == "generic"}
    assert got == {"maxsim_generic_kernel<%d, %d>" % i for i in [(1, 4), (2, 4), (4, 4), (8, 4), (16, 4), (2, 1), (8, 1), (32, 1)]}  # all eight


def test_pairs_choice_restates_the_launcher():
    p = ref.pairs_choice
    assert [p(d, 0) for d in (16, 48, 144, 128, 384, 256, 1024)] == ["maxsim_pairs_kernel<false, 128, false>"] * 3 + ["maxsim_pairs_kernel<true, 128, false>"] * 2 + \
        ["maxsim_pairs_kernel<true, 256, false>"] * 2
    assert [p(d, 1) for d in (144, 384, 256)] == ["maxsim_pairs_kernel<false, 128, false>", "maxsim_pairs_packed_kernel<128, false>", "maxsim_pairs_packed_kernel<256, false>"]
    assert [p(d, 2) for d in (144, 384, 1024)] == ["maxsim_pairs_kernel<false, 128, false>"] + ["maxsim_pairs_packed_kernel<128, false, 0, 16>"] * 2
    assert [p(d, 2, True) for d in (384, 1024, 1152)] == ["maxsim_pairs_packed_kernel<128, true>", "maxsim_pairs_packed_kernel<256, true>", "maxsim_pairs_wide_kernel<true>"]
    assert p(256, 0, True) == "maxsim_pairs_kernel<true, 256, true>" and p(384, 0, True) == "maxsim_pairs_kernel<true, 128, true>" and p(4096, 0) == "maxsim_pairs_wide_kernel<false>"
    for bad in (8, 100, 1100, 4224):
        with pytest.raises(ValueError):
            p(bad, 2)
    src = (CSRC / "maxsim_generic.hip").read_text()
    for line in ("const bool full = dim % 128 == 0;", "packed = packed && full;", "const bool wide = packed && packed_mode == 2 && !rows16;",
                 "else if (packed && dim % 256 == 0) RL_PACKED(256);", "else if (packed && dim % 128 == 0) RL_PACKED(128);",
                 "else if (dim % 256 == 0) RL_PAIRS(true, 256);", "else if (dim % 128 == 0) RL_PAIRS(true, 128);", "else RL_PAIRS(false, 128);",
                 "if (dim > 1024) {  // wider than a CU's LDS holds a query", "if (dim % PW_KW) return RL_ERR_UNSUPPORTED;",
                 "if (nq < 1 || nq > 32 || dim % 16 || dim < 16 || dim > PAIRS_MAX_DIM || !candidates) return RL_ERR_UNSUPPORTED;"):
        assert line in src, line
    reached = {c.inst for c in CASES if c.kernel == "pairs"}
    want = {f"maxsim_pairs_kernel<{f}, {kb}, {r}>" for f, kb in (("true", 256), ("true", 128), ("false", 128)) for r in ("false", "true")}
    want |= {f"maxsim_pairs_packed_kernel<{kb}, {r}>" for kb in (128, 256) for r in ("false", "true")}
    want |= {"maxsim_pairs_packed_kernel<128, false, 0, 16>", "maxsim_pairs_wide_kernel<false>", "maxsim_pairs_wide_kernel<true>"}
    assert want - reached == {"maxsim_pairs_kernel<false, 128, true>"}  # (no fp16-stored index has such a width: rl_index_create_f16)
    assert reached <= want


def test_query_tiles_restate_the_launchers():
    assert [ref.nqt(n) for n in (1, 16, 17, 32)] == [1, 1, 2, 2]
    assert "if (a.mode == 0) { if (a.nq <= 16) RL_STREAM(1, 0); else RL_STREAM(2, 0); }" in (CSRC / "maxsim_stream.hip").read_text()
    src = (CSRC / "maxsim_generic.hip").read_text()
    assert "if (f16) { if (nq <= 16) RL_CAND(1, true); else RL_CAND(2, true); }" in src
    assert "else if (split_scale > 0.f) { if (nq <= 16) RL_CAND(1, false, true); else RL_CAND(2, false, true); }" in src
    stream = {c.inst for c in CASES if c.kernel == "stream"}
    flags = ("false, true", "false, false", "true, false")
    assert stream == {f"maxsim_stream_kernel<{d // 4}, {t}, 0, false, 6, {f}>" for d in ref.STREAM_DIMS for t in (1, 2) for f in flags}  # KW x NQT x arithmetic
    assert {c.inst for c in CASES if c.kernel == "cand"} == {f"maxsim_cand_kernel<{t}, {f}>" for t in (1, 2) for f in flags}
    assert {c.inst for c in CASES if c.kernel == "stream2"} == {f"maxsim_stream2_kernel<{d // 4}, false, {r}>" for d in ref.STREAM_DIMS for r in ("false", "true")}


def test_row_scale_restates_update_split_scale():
    src = (CSRC / "api.hip").read_text()
    assert "idx->split_scale = std::ldexp(1.f, 14 - std::max(-100, ex));" in src and "if (!(idx->max_abs / idx->min_row_max <= 1024.f)) return;" in src
    E = np.zeros((3, 8), dtype=np.float32)  # noqa: N806
    assert ref.row_scale(E) == 1.0
    E[1, 2], E[2, 5] = -0.75, 0.001
    assert ref.row_scale(E) == 2.0 ** 14 and ref.split_eligible(E)  # 0.75 = 0.75 2^0
    E[2, 5] = 0.0007
    assert not ref.split_eligible(E)  # 0.75 / 0.0007 > 1024 (the all-zero row does not count)
    assert ref.row_scale(E * np.float32(2.0 ** 40)) == 2.0 ** -26


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
def test_every_case_names_the_arithmetic_the_index_selects():
    """An fp32 index keeps the split only while its row maxima lie within 2^10 of each other: the data of every case is chosen accordingly."""
    assert len({c.name for c in CASES}) == len(CASES)
    for c in CASES:
        E, off, Q, cand = c.data()  # noqa: N806
        assert E.shape == (c.n, c.dim) and Q.shape == (c.n_queries, c.nq, c.dim) and off[-1] == c.n
        if c.storage == "f16":
            assert c.arith == "f16_stored" and np.array_equal(E, E.astype(np.float16).astype(np.float32))
        else:
            assert c.arith == ("f16_split" if ref.split_eligible(E) and not c.exact else "fp32_exact"), c.name
        assert (cand is not None) == (c.entry == "rerank")
        assert c.n <= 403 or c.n == ref.WALK_ROWS or c.rows == "one_hot"  # a few hundred rows everywhere but the walks (and dim + 19 probes)


def test_the_cases_cover_what_the_issue_lists():
    by = lambda k: [c for c in CASES if c.kernel == k]  # noqa: E731
    assert {c.dim for c in by("pairs") if c.entry == "rerank"} >= set(ref.PAIRS_DIMS + ref.WIDE_DIMS)
    assert {c.nq for c in by("stream")} >= set(ref.NQS + ref.PASS_NQS) and {c.nq for c in by("cand")} >= set(ref.NQS)
    assert {c.nq for c in by("generic")} >= {65, 130} and {c.shift for c in by("generic")} == {"", "rows", "queries"}
    assert {c.n_cand for c in by("cand")} >= set(ref.CAND_LENGTHS)
    assert {c.dim for c in CASES if c.n == ref.WALK_ROWS and c.kernel == "stream"} == set(ref.STREAM_DIMS)
    for kind in ("neg", "spread", "quarters", "f16", "lo_one_quarter", "one_hot"):
        assert {c.dim for c in by("stream") if c.queries == kind} == set(ref.STREAM_DIMS), kind
    assert {c.pow2 for c in by("stream")} == {-40, 0, 40} and {c.rows for c in by("stream")} == {"normal", "pos", "one_hot"}
    assert all(np.all(ref.dots(*c.data()[:1], c.data()[2][0]) < 0) for c in CASES if c.queries == "neg" and c.n < 5000)  # all dots negative
