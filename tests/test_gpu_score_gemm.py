"""The dense score GEMMs ONE BY ONE on the GPU through `rl_score_gemm`: score_gemm.hip's 128 x 128 kernel in split and in exact fp32
arithmetic (kernel 1), its 128 x 256 kernel (kernel 2) and the row-score mode of maxsim_gemm.hip over a pre-split image (kernel 3), each
held ELEMENTWISE to the float64 restatements and derived bounds of tests/score_gemm_ref.py.  The searches reach these kernels with integer
data (every lo half zero), one tile per workgroup, two dims and a top-k in between; here

  * float data runs every slab count around the pipeline depths (dim 32 .. 1024), every row and batch size around the tiles, in the four
    metrics with norms the TEST chose (a wrong row index in an epilogue shows);
  * one-hot rows make every k position of every chunk, both halves and both operands, some element's only product (bound 2^-19 |e q|);
  * `max_workgroups` 1, 2, 3, 8 make one workgroup walk up to 32 tiles: the ring, the register sets and the accumulators cross tile
    boundaries, padded row tiles come up in the middle of a walk -- outputs must keep the bits of the default grid;
  * 128 x 128 and 128 x 256 tiles must agree bit for bit (the same three MFMAs per slab and accumulator, in the same order);
  * the metric launches must equal the float32 restatement of `transform_score` on the raw launch's dots, bit for bit.

Every output lies between guard cells (in front, behind, and between its rows: ld > n_rows) that must keep their bits.  Each case's worst
error / bound goes to profiles/score_gemm_error.txt; above 1 is a failure."""

from pathlib import Path

import numpy as np
import pytest
import torch

from raglite_amd._score_gemm import score_gemm
from tests import scan_ref
from tests import score_gemm_ref as ref

pytestmark = pytest.mark.gpu

DEVICE = "cuda"
FRONT, SENTINEL = 8, -7.0  # guard floats in front of and behind every output (8: the output starts 16-byte aligned), and what they hold
SPLIT_KERNELS = (1, 2, 3)
_ids = lambda cases: [c.name for c in cases]  # noqa: E731


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    """Bit for bit, except that a NaN equals any NaN (0 / 0 carries no agreed sign or payload)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(_bits(a)[~nan], _bits(b)[~nan])


class Run:
    """A case's operands on the device and one launch over them into a guarded output."""

    def __init__(self, E, Q, row_norm=None, row_sumsq=None):  # noqa: N803
        self.n, self.B = len(E), len(Q)
        dev = lambda a: None if a is None else torch.tensor(np.asarray(a, dtype=np.float32), device=DEVICE)  # noqa: E731 (a copy: the makers' arrays are read-only)
        self.E, self.Q, self.rn, self.rs = dev(E), dev(Q), dev(row_norm), dev(row_sumsq)

    def __call__(self, metric, kernel, s, grid=0, ld=None, front=FRONT, readback=False):
        n, B = self.n, self.B  # noqa: N806
        ld = (n + 3) // 4 * 4 + 4 if ld is None else ld
        flat = torch.full((front + (B - 1) * ld + n + FRONT,), SENTINEL, dtype=torch.float32, device=DEVICE)
        out = torch.as_strided(flat, (B, n), (ld, 1), front)
        got = score_gemm(self.E, self.Q, metric, row_norm=self.rn, row_sumsq=self.rs, split_scale=s, kernel=kernel, max_workgroups=grid, out=out,
                         readback=readback)
        host = flat.cpu().numpy()
        idx = front + np.arange(B)[:, None] * ld + np.arange(n)[None, :]
        guard = np.ones(host.shape, dtype=bool)
        guard[idx] = False
        assert np.array_equal(_bits(host[guard]), _bits(np.full(int(guard.sum()), SENTINEL, np.float32))), "a cell outside the output was written"
        res = host[idx]
        if readback:
            return res, got[1].cpu().numpy(), None if got[2] is None else got[2].cpu().numpy()
        return res


@pytest.fixture(scope="module")
def error_log():
    lines = []
    yield lines
    try:  # (a read-only checkout keeps the committed figures)
        out = Path(__file__).resolve().parent.parent / "profiles" / "score_gemm_error.txt"
        head = ("# tests/test_gpu_score_gemm.py: the worst |kernel - float64| / bound over a case's elements; every figure is asserted <= 1.\n"
                "# Bounds: tests/score_gemm_ref.py.  kernel 1: 128 x 128 tiles, 2: 128 x 256, 3: over a pre-split image; f32: the exact fp32 MFMAs.\n"
                "# `acc`: the raw dot against the restated split (accumulation error alone).  Bit-for-bit comparisons are not listed: they have no figure.\n"
                "# Found by these tests: before the epilogues of score_gemm.hip stored `d` in raw mode, every `kernel1 raw` / `kernel2 raw` line failed --\n"
                "# dim32_slabs1 kernel1 raw: 12610 of 12610 scores outside the bound, each s * q_scale = 2^28 times the dot (the scaled sum was stored).\n")
        out.write_text(head + "".join(sorted(lines)))
    except OSError:
        pass


def _log(error_log, name, what, ratio):
    line = f"{name} {what} | {ratio:.4f}\n"
    print(line, end="")
    error_log.append(line)
    assert ratio <= 1.0, line


def _variants(s):
    """(label, kernel, split scale) of the four kernels under test."""
    return [(f"kernel{k}", k, s) for k in SPLIT_KERNELS] + [("kernel1_f32", 1, 0.0)]


# ---- elementwise against float64 ---------------------------------------------------------------------------------------------------------
ELEMENTWISE = ref.elementwise_cases()


@pytest.mark.parametrize("case", ELEMENTWISE, ids=_ids(ELEMENTWISE))
def test_every_element_against_float64(torch_cuda, error_log, case):
    """Kernels 1, 2, 3 in split arithmetic and kernel 1 in exact fp32, raw / cosine / dot / l2, no element excepted; the raw dot of the
    split kernels also against the restated split with the accumulation bound alone; 128 x 128 against 128 x 256 bit for bit; the
    launcher's own choice (kernel 0) equal to the kernel it names."""
    E, Q = case.data()  # noqa: N806
    s = ref.pow2_scale(E)
    rn, rs = ref.given_norms(E)
    run = Run(E, Q, rn, rs)
    tiles, autos = {}, {}
    for label, kernel, scale in _variants(s):
        d, _, dsplit, bd, bacc = ref.references(case, scale)
        for metric in ref.METRICS:
            # raw / dot: rows 16-byte aligned (the vector store); cosine / l2: ld odd (from the second query on: the scalar stores)
            ld = None if metric in ("raw", "dot") else (case.n + 4) | 1
            got = run(metric, kernel, scale, ld=ld)
            want, bound = ref.score_ref(d, metric, Q, rn, rs), ref.score_bound(d, bd, metric, Q, rn, rs)
            _log(error_log, case.name, f"{label} {metric}", scan_ref.assert_within(got, want, bound, f"{case.name} {label} {metric}"))
            if metric == "raw" and dsplit is not None:
                _log(error_log, case.name, f"{label} acc", scan_ref.assert_within(got, dsplit, bacc, f"{case.name} {label} raw vs the restated split"))
            if kernel in (1, 2) and scale:
                tiles[kernel, metric] = got
            if metric == "raw" and kernel == 1:
                autos[scale] = run("raw", 0, scale)
                assert scale or _same_bits(autos[scale], got), "kernel 0 in exact fp32 is the 128 x 128 kernel"
    for metric in ref.METRICS:
        assert _same_bits(tiles[1, metric], tiles[2, metric]), f"{metric}: 128 x 128 and 128 x 256 tiles differ"
    named = 2 if case.B > 128 else 1
    assert _same_bits(autos[s], tiles[named, "raw"]), f"kernel 0 in split arithmetic at {case.B} queries is kernel {named}"


# ---- basis probes --------------------------------------------------------------------------------------------------------------------------
PROBES = ref.probe_cases()


@pytest.mark.parametrize("case", PROBES, ids=_ids(PROBES))
def test_basis_probes(torch_cuda, error_log, case):
    """One-hot rows: every k position of every chunk is some row's only product; a dropped or misplaced lo product moves 95 % and more
    of the elements out of 2^-19 |e q| (tests/test_score_gemm_ref_host.py)."""
    E, Q = case.data()  # noqa: N806
    run = Run(E, Q)
    want, bound = ref.d_exact(E, Q), ref.probe_bound(E, Q)
    for k in SPLIT_KERNELS:
        got = run("raw", k, ref.pow2_scale(E))
        _log(error_log, case.name, f"kernel{k} raw", scan_ref.assert_within(got, want, bound, f"{case.name} kernel {k}"))
    got = run("raw", 1, 0.0)  # (the fp32 kernel: one product, exact up to its own rounding)
    _log(error_log, case.name, "kernel1_f32 raw", scan_ref.assert_within(got, want, ref.acc_bound(E, Q, False), f"{case.name} fp32"))


# ---- many tiles per workgroup ----------------------------------------------------------------------------------------------------------
WALKS = ref.walk_cases()


@pytest.mark.parametrize("case", WALKS, ids=_ids(WALKS))
def test_a_workgroup_walks_many_tiles(torch_cuda, error_log, case):
    """max_workgroups 1, 2, 3, 8 against the default grid.  Float data: within the bound and the default grid's bits.  Integer data: the
    bits of `sim_fp32_exact` in every metric on every grid."""
    E, Q = case.data()  # noqa: N806
    s = ref.pow2_scale(E)
    run = Run(E, Q)
    for label, kernel, scale in _variants(s)[:2] + _variants(s)[3:]:
        d, _, _, bd, _ = ref.references(case, scale)
        base = run("raw", kernel, scale)
        _log(error_log, case.name, f"{label} raw", scan_ref.assert_within(base, d, bd, f"{case.name} {label}"))
        for grid in ref.WALK_GRIDS:
            assert _same_bits(run("raw", kernel, scale, grid=grid), base), f"{label}: {grid} workgroups change the bits of the default grid"
    Ei, Qi = ref.make("int", 300 + case.dim, case.n, case.dim), ref.make("int", 400 + case.dim, case.B, case.dim)  # noqa: N806
    si = ref.pow2_scale(Ei)
    run = Run(Ei, Qi, *ref.int_norms(Ei))
    for metric in scan_ref.METRICS:
        want = ref.exact_scores(Ei, Qi, metric)
        for label, kernel, scale in _variants(si)[:2] + _variants(si)[3:]:
            for grid in (0,) + ref.WALK_GRIDS:
                assert _same_bits(run(metric, kernel, scale, grid=grid), want), f"{label} {metric}, {grid} workgroups: integer data is not bit-exact"


@pytest.mark.parametrize("dim", [96, 160])
def test_position_independence(torch_cuda, dim):
    """Every (row, query) sums K in the same fixed order: a corpus shifted by 37 rows and a query moved to another place in the batch keep
    their bits, on one workgroup and on the default grid."""
    E, Q = ref.uniform(500 + dim, 700, dim), ref.uniform(600 + dim, 300, dim)  # noqa: N806
    s = ref.pow2_scale(E)
    perm = np.random.default_rng(dim).permutation(len(Q))
    for _, kernel, scale in _variants(s)[:2] + _variants(s)[3:]:
        base = Run(E, Q)("raw", kernel, scale)
        for grid in (0, 1):
            assert _same_bits(Run(E[37:], Q)("raw", kernel, scale, grid=grid), base[:, 37:]), (kernel, scale, grid, "rows shifted by 37")
            assert _same_bits(Run(E, Q[perm])("raw", kernel, scale, grid=grid), base[perm]), (kernel, scale, grid, "queries permuted")


# ---- the epilogue, bit for bit -----------------------------------------------------------------------------------------------------------
EPILOGUES = [c for c in ELEMENTWISE if c.name in ("dim96_slabs3", "rows1003", "batch257", "scaled_queries_dim1024", "spread_rows_dim288",
                                                  "same_sign_dim64_two_query_tiles")]


@pytest.mark.parametrize("case", EPILOGUES, ids=_ids(EPILOGUES))
def test_epilogue_bit_for_bit(torch_cuda, error_log, case):
    """With the raw launch's d, the given row_norm / row_sumsq and the |q|^2 read back, every metric's output is the float32 restatement
    of `transform_score`; |q|^2 is within its gamma bound and q_scale is the stated power of two."""
    E, Q = case.data()  # noqa: N806
    s = ref.pow2_scale(E)
    rn, rs = ref.given_norms(E)
    run = Run(E, Q, rn, rs)
    qss_ref, qss_bound = ref.q_sumsq_bound(Q)
    qss = None
    for label, kernel, scale in _variants(s):
        if kernel == 3:
            d32 = run("raw", kernel, scale)  # (no read-back with kernel 3: the same query_sumsq_kernel wrote its |q|^2)
        else:
            d32, qss_k, qsc = run("raw", kernel, scale, readback=True)
            assert qss is None or _same_bits(qss_k, qss)
            qss = qss_k
            assert (qsc is None) == (scale == 0.0) and (qsc is None or np.array_equal(qsc.astype(np.float64), ref.query_scale(Q)))
            _log(error_log, case.name, f"{label} q_sumsq", scan_ref.assert_within(qss, qss_ref, qss_bound, f"{case.name} |q|^2"))
        for metric in scan_ref.METRICS:
            got = run(metric, kernel, scale)
            assert _same_bits(got, ref.epilogue_f32(d32, metric, qss, rn, rs)), f"{label} {metric}: not the float32 epilogue of the raw dots"


def test_zero_row_and_zero_query(torch_cuda):
    """Cosine of a zero row (norm 0) or a zero query is 0 / 0 = NaN, as scan_ref states; raw, dot and l2 stay finite and exact there."""
    E, Q = np.array(ref.uniform(41, 130, 96)), np.array(ref.uniform(42, 97, 96))  # noqa: N806
    E[5], Q[3], Q[96] = 0.0, 0.0, 0.0
    rn, rs = ref.given_norms(E)
    assert rn[5] == 0.0 and rs[5] == 0.0
    run = Run(E, Q, rn, rs)
    zero = np.zeros((97, 130), dtype=bool)
    zero[:, 5], zero[3], zero[96] = True, True, True
    none = np.zeros(zero.shape)  # (every product of a zero row or query is zero: the dot is exactly 0 there)
    want, bound = ref.score_ref(none, "l2", Q, rn, rs), ref.score_bound(none, none, "l2", Q, rn, rs)
    for _, kernel, scale in _variants(ref.pow2_scale(E)):
        cos = run("cosine", kernel, scale)
        assert np.array_equal(np.isnan(cos), zero), (kernel, scale)
        assert np.all(run("raw", kernel, scale)[zero] == 0.0) and np.all(run("dot", kernel, scale)[zero] == 1.0)
        l2 = run("l2", kernel, scale)
        assert np.all(np.isfinite(l2))
        assert np.all(np.abs(l2 - want)[zero] <= bound[zero])


# ---- stores ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [130, 127, 128])
def test_stores(torch_cuda, n):
    """ld odd (rows of the output not 16-byte aligned from the second query on), n_rows % 4 != 0, the output offset by one float: the
    scalar store branch gives the vector branch's bits and writes nothing else (the guard cells are checked by every launch)."""
    E, Q = ref.uniform(51, n, 96), ref.uniform(52, 131, 96)  # noqa: N806
    rn, rs = ref.given_norms(E)
    run = Run(E, Q, rn, rs)
    for _, kernel, scale in _variants(ref.pow2_scale(E)):
        base = run("cosine", kernel, scale)
        for ld, front in (((n + 4) | 1, FRONT), (None, FRONT + 1), (n, FRONT), (n, FRONT + 3), ((n + 4) | 1, FRONT + 2)):
            assert _same_bits(run("cosine", kernel, scale, ld=ld, front=front), base), (kernel, scale, ld, front)


# ---- kernel 3 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [96, 288])
def test_image_kernel_groups_and_pair_ranges(torch_cuda, error_log, dim):
    """300 queries (no multiple of 32 or of 256): a group of 32 integer queries (its lo flag clear: the third product is skipped), a group
    of floats, a group of integers with ONE float query, then floats, over 1100 float rows: 5 row tiles x 2 query tiles = 10 pairs, which
    1, 3 and 7 workgroups cut inside a query tile and inside a row tile.  Raw and the two metrics that read a row norm."""
    E = ref.uniform(700 + dim, 1100, dim)  # noqa: N806
    Q = np.concatenate((ref.grouped_queries(800 + dim, dim), ref.uniform(900 + dim, 204, dim)))  # noqa: N806
    s = ref.pow2_scale(E)
    rn, rs = ref.given_norms(E)
    run = Run(E, Q, rn, rs)
    d, bd = ref.d_exact(E, Q), ref.dot_bound(E, Q, s)
    for metric in ("raw", "cosine", "l2"):
        base = run(metric, 3, s)
        want, bound = ref.score_ref(d, metric, Q, rn, rs), ref.score_bound(d, bd, metric, Q, rn, rs)
        _log(error_log, f"image_groups_dim{dim}", f"kernel3 {metric}", scan_ref.assert_within(base, want, bound, f"kernel 3 {metric}"))
        for grid in ref.IMAGE_GRIDS:
            assert _same_bits(run(metric, 3, s, grid=grid), base), f"{metric}: {grid} workgroups change the bits of the default grid"
    assert _same_bits(run("raw", 3, s)[:32], Run(E, Q[:32])("raw", 3, s)), "a group's scores depend on the batch it comes in"


def test_host_arrays_and_an_output_of_its_own(torch_cuda):
    """NumPy arrays take the staged route: the same bits as device tensors, and what lies between the rows of a strided host output stays."""
    E, Q = ref.uniform(61, 130, 96), ref.uniform(62, 97, 96)  # noqa: N806
    rn, rs = ref.given_norms(E)
    s = ref.pow2_scale(E)
    want = Run(E, Q, rn, rs)("l2", 2, s)
    assert _same_bits(score_gemm(E, Q, "l2", row_sumsq=rs, split_scale=s, kernel=2), want)
    flat = np.full(97 * 135, SENTINEL, dtype=np.float32)
    out = flat.reshape(97, 135)[:, :130]
    got, qss, qsc = score_gemm(E, Q, "l2", row_sumsq=rs, split_scale=s, kernel=2, out=out, readback=True)
    assert got is out and _same_bits(out, want) and np.all(flat.reshape(97, 135)[:, 130:] == SENTINEL)
    assert np.array_equal(qsc.astype(np.float64), ref.query_scale(Q)) and qss.shape == (97,)
