"""The four kernels of partition_sim.hip (`rl_partition_similarity`, and `rl_split_chunks` through its `cost_out`) against the float64
statement of the operation in tests/partition_sim_ref.py: every `ps_pairs_kernel<NV>` at both ends of its range of widths, widths off
a multiple of 64, the three branches (`no_selection`, `degenerate`, `mod`) side by side in one batch, the per-document flag on reused
scratch, the grid-stride loops past 16 384 rows, and the one-selected-row rule.

Inputs (`make_batch`): a row is a Gaussian plus a component shared by its document, so that ||X_mod row|| stays near 0.6; the last
column carries at least 0.2 of the row norm, and the first and last column of every group of 64 carry extra weight, so a dropped,
duplicated or misplaced column moves a similarity by 1e-2 or more.  Every `mod` document has a float64 min ||X_mod row|| >= 0.5 and
every `degenerate` document is degenerate exactly (its selected rows are one axis e_j, or there is one selected row: the rule); `checked`
asserts both, so no branch of these tests is decided by rounding.

Tolerance (`partition_sim_ref.tolerance`, derived, not tuned): (ceil(dim / 64) + 16) * 2^-24 on the plain branches, 4 times that over
min(na, nb)^2 on `mod`.  scripts/partition_sim_error.py prints the measured error against it (profiles/partition_sim_error.txt)."""

import numpy as np
import pytest

import raglite_amd
from raglite_amd import _ops
from raglite_amd._abi import check, lib
from raglite_amd._chunking import _nonoutlying
from tests import partition_sim_ref as ref

pytestmark = pytest.mark.gpu

WIDTHS = [32, 63, 64, 65, 100, 128, 129, 256, 257, 384, 512, 513, 1024, 1025, 2048, 2049, 4095, 4096]
SQRT_EPS = float(ref.SQRT_EPS32)


def similarity(X, off, sel, torch=None):
    """`rl_partition_similarity` through the call frame, with explicit `sel` (or None) and `off` (or None): host pointers, or CUDA
    tensors on torch's current stream where `torch` is given.  The output starts as -7 everywhere."""
    a = _ops._Args()  # noqa: SLF001
    x, p_x = a.inp(X if torch is None else torch.as_tensor(X, device="cuda"), np.float32)
    n, dim = int(x.shape[0]), int(x.shape[1])
    p_off = None if off is None else a.same_side(off, np.int64)[1]
    p_sel = None if sel is None else a.same_side(sel, np.uint8)[1]
    out, p_out = a.inp(np.full(n, -7.0, np.float32) if torch is None else torch.full((n,), -7.0, device="cuda"), np.float32)
    a.ensure_device()
    check(lib().rl_partition_similarity(p_x, n, dim, p_off, 1 if off is None else len(off) - 1, p_sel, p_out, a.mem, a.stream))
    return out if torch is None else out.cpu().numpy()


def edge_columns(dim):
    """The first and last column of every group of 64, without the last column of the row."""
    return sorted({c for g in range(0, dim, 64) for c in (g, min(g + 63, dim - 1))} - {dim - 1})


def make_rows(rng, n, dim):
    """n rows of one document (float64): shared component + Gaussian + weighted edge columns, the last column set to 0.25 .. 0.35 of
    the rest of the row, each row then scaled by 2^-2 .. 2^2."""
    def unit(v):
        return v / np.linalg.norm(v, axis=-1, keepdims=True)

    x = np.sqrt(0.35) * unit(rng.standard_normal(dim)) + np.sqrt(0.53) * unit(rng.standard_normal((n, dim)))
    edges = edge_columns(dim)
    if edges:
        x[:, edges] += rng.choice([-1.0, 1.0], size=(n, len(edges))) * np.sqrt(0.06 / len(edges))
    x[:, -1] = 0.0
    x[:, -1] = rng.choice([-1.0, 1.0], size=n) * rng.uniform(0.25, 0.35, size=n) * np.linalg.norm(x, axis=1)
    return x * np.exp2(rng.uniform(-2, 2, size=(n, 1)))


def make_batch(rng, dim, specs):
    """specs: ("mod", n) two or more selected rows (one where n == 1); ("none", n) no selected row; ("axis", n, positions, j) the rows at
    `positions` are multiples of e_j and the only selected ones.  -> X float32 (N, dim), off int64, sel uint8, the branch each document
    must take."""
    rows, sels, want = [], [], []
    for spec in specs:
        kind, n = spec[0], spec[1]
        x = make_rows(rng, n, dim)
        s = np.zeros(n, np.uint8)
        if kind == "mod":
            while n and s.sum() < min(n, 2):
                s = (rng.random(n) < 0.6).astype(np.uint8)
            while n >= 2 and ref.document(x.astype(np.float32), s)[2] < 0.52:  # (rare, at small dim: draw the rows again)
                x = make_rows(rng, n, dim)
            want.append("mod" if n >= 2 else "degenerate" if n else "no_selection")
        elif kind == "axis":
            for p in spec[2]:
                x[p] = 0.0
                x[p, spec[3]] = rng.choice([0.5, 1.0, 2.0, -4.0])
                s[p] = 1
            if len(spec[2]) > 1:
                x[spec[2][1:], spec[3]] = np.abs(x[spec[2][1:], spec[3]]) * np.sign(x[spec[2][0], spec[3]])  # the same axis, the same sense
            want.append("degenerate")
        else:
            want.append("no_selection")
        rows.append(x)
        sels.append(s)
    off = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int64)
    return np.concatenate(rows).astype(np.float32), off, np.concatenate(sels), want


def checked(X, off, sel, want_branches=None):
    """The float64 statement of a batch, with the conditions on the inputs asserted -> (sim, tol, branches)."""
    sim, branches, smallest, norms = ref.batch(X, off, sel)
    if want_branches is not None:
        assert branches == want_branches
    for d, branch in enumerate(branches):
        if branch == "mod":
            assert smallest[d] >= 0.5, (d, smallest[d])
        elif branch == "degenerate":
            assert smallest[d] == 0.0, (d, smallest[d])
    Xd = np.asarray(X, np.float64)
    made = np.count_nonzero(Xd, axis=1) > 1  # (not the one-axis rows)
    assert np.all(np.abs(Xd[made, -1]) >= 0.2 * np.linalg.norm(Xd[made], axis=1))
    return sim, ref.tolerance(X.shape[1], branches, off, norms), branches


def assert_close(got, sim, tol, off, what=""):
    assert got.dtype == np.float32 and np.all(np.isfinite(got)), what
    ratio = np.abs(got.astype(np.float64) - sim) / tol
    assert np.all(ratio <= 1.0), (what, int(np.argmax(ratio)), float(ratio.max()), int((ratio > 1).sum()))
    last = off[1:][off[1:] > off[:-1]] - 1
    assert np.all(got[last].view(np.uint32) == 0), what  # +0.0 at every document's last row
    return float(ratio.max())


def widths_batch(dim):
    rng = np.random.default_rng(1000 + dim)
    long = [int(v) for v in rng.integers(5, 41, size=3)]
    specs = [("mod", 0), ("mod", 0), ("mod", 1), ("mod", 2), ("none", 2), ("mod", 3), ("mod", long[0]), ("mod", 0), ("none", long[1]),
             ("mod", long[2]), ("mod", 0)]
    return make_batch(rng, dim, specs)


@pytest.mark.parametrize("dim", WIDTHS)
def test_every_width_against_float64(torch_cuda, dim):
    """Both ends of every `ps_pairs_kernel<NV>`'s range and the `k < dim` tails of the three kernels: values, the exact zero at every
    last row, a document alone == in the batch, host pointers == CUDA tensors, run to run."""
    X, off, sel, want = widths_batch(dim)
    sim, tol, _ = checked(X, off, sel, want)
    got = similarity(X, off, sel)
    worst = assert_close(got, sim, tol, off, "host")
    print(f"dim {dim}: max |error| / bound = {worst:.3f}")
    dev = similarity(X, off, sel, torch_cuda)
    assert dev.tobytes() == got.tobytes()
    assert similarity(X, off, sel).tobytes() == got.tobytes() and similarity(X, off, sel, torch_cuda).tobytes() == got.tobytes()
    for d in range(len(off) - 1):
        b, e = int(off[d]), int(off[d + 1])
        if e > b:
            alone = similarity(X[b:e], np.asarray([0, e - b]), sel[b:e])
            assert alone.tobytes() == got[b:e].tobytes(), d


def test_dim_one_is_exact(torch_cuda):
    """One column: every normalised row is +-1, d is +-1, every X_mod is exactly 0, so every document is plain: 1.0 or sqrt(eps)."""
    rng = np.random.default_rng(1)
    counts = [0, 1, 2, 3, 17, 0, 0, 40, 5]
    off = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    X = (rng.choice([-1.0, 1.0], size=(off[-1], 1)) * rng.choice([0.5, 1.0, 2.0, 4.0], size=(off[-1], 1))).astype(np.float32)
    sel = (X[:, 0] > 0).astype(np.uint8)  # selected rows of one sign: their mean is exactly 1
    sel[off[4]:off[5]] = 0
    want = np.where(np.sign(X[:-1, 0]) == np.sign(X[1:, 0]), np.float32(1.0), ref.SQRT_EPS32)
    want = np.concatenate((want, [0])).astype(np.float32)
    want[off[1:][np.diff(off) > 0] - 1] = 0.0
    assert np.array_equal(ref.batch(X, off, sel)[0].astype(np.float32), want)
    for torch in (None, torch_cuda):
        assert similarity(X, off, sel, torch).tobytes() == want.tobytes()
        assert similarity(X, off, None, torch).tobytes() == want.tobytes()


def branches_batch(dim):
    rng = np.random.default_rng(2000 + dim)
    specs = [("mod", 9), ("none", 6), ("axis", 7, [0], dim - 1), ("mod", 12), ("axis", 9, [4], 0), ("none", 1), ("axis", 8, [7], 64),
             ("mod", 0), ("axis", 11, [0, 10], dim // 2), ("mod", 31), ("axis", 6, [2, 3], dim - 1), ("none", 14), ("axis", 3, [0, 1, 2], 1),
             ("mod", 5), ("axis", 2, [1], 63)]
    return make_batch(rng, dim, specs)


@pytest.mark.parametrize("dim", [100, 1024])
def test_branches_side_by_side_in_one_batch(torch_cuda, dim):
    """`mod`, `no_selection` and exactly degenerate documents interleaved (the one-hot row first, in the middle and last -- the last
    row's wave must still raise the flag): each document takes its own branch, whatever its neighbours take."""
    X, off, sel, want = branches_batch(dim)
    sim, tol, _ = checked(X, off, sel, want)
    plain, plain_tol, _ = checked(X, off, None, ["no_selection"] * len(want))
    n_mod = sum(int(off[d + 1] - off[d] - 1) for d, w in enumerate(want) if w == "mod" and off[d + 1] > off[d])
    assert np.sum(np.abs(sim - plain) > 1e-2) > n_mod // 2  # the branches are far apart: taking the wrong one cannot pass
    for torch in (None, torch_cuda):
        got = similarity(X, off, sel, torch)
        assert_close(got, sim, tol, off, "sel")
        for d in range(len(off) - 1):
            b, e = int(off[d]), int(off[d + 1])
            if e > b:
                assert similarity(X[b:e], np.asarray([0, e - b]), sel[b:e], torch).tobytes() == got[b:e].tobytes(), d
        got_plain = similarity(X, off, None, torch)  # nonoutlying = NULL: everything plain
        assert_close(got_plain, plain, plain_tol, off, "sel = NULL")
        assert similarity(X, off, np.zeros_like(sel), torch).tobytes() == got_plain.tobytes()
    # doc_offsets = NULL: one document
    b, e = int(off[9]), int(off[10])
    one, one_tol, _ = checked(X[b:e], [0, e - b], sel[b:e], ["mod"])
    for torch in (None, torch_cuda):
        assert_close(similarity(X[b:e], None, sel[b:e], torch), one, one_tol, np.asarray([0, e - b]), "off = NULL")
        assert_close(similarity(X[b:e], None, None, torch), plain[b:e], plain_tol[b:e], np.asarray([0, e - b]), "off = sel = NULL")


@pytest.mark.parametrize("dim", [100, 1024])
def test_degenerate_flag_is_cleared_between_calls_on_one_stream(torch_cuda, dim):
    """A batch whose documents 2 and 5 are exactly degenerate, then a batch of the same shape where they are not, on one CUDA stream: the
    second call gives the `mod` values, so the flags of the first do not survive in reused scratch.  `rl_partition_similarity` twice,
    then the same pair through `rl_split_chunks` and its `cost_out`."""
    torch = torch_cuda
    rng = np.random.default_rng(3000 + dim)
    specs = [("mod", 7), ("mod", 4), ("axis", 9, [0, 8], dim - 1), ("mod", 3), ("none", 5), ("axis", 6, [2, 3], 0), ("mod", 10)]
    XA, off, sel, want_a = make_batch(rng, dim, specs)
    XB = XA.copy()
    for d in (2, 5):
        b, e = int(off[d]), int(off[d + 1])
        XB[b:e] = make_rows(rng, e - b, dim).astype(np.float32)
    want_b = ["mod" if w == "degenerate" else w for w in want_a]
    sim_a, tol_a, _ = checked(XA, off, sel, want_a)
    sim_b, tol_b, _ = checked(XB, off, sel, want_b)
    sizes = np.ones(len(XA), np.int64)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        tA, tB = torch.as_tensor(XA, device="cuda"), torch.as_tensor(XB, device="cuda")
        for _ in range(2):
            assert_close(similarity(tA, off, sel, torch), sim_a, tol_a, off, "A")
            assert_close(similarity(tB, off, sel, torch), sim_b, tol_b, off, "B after A")
        for x, sim, tol in ((tA, sim_a, tol_a), (tB, sim_b, tol_b), (tA, sim_a, tol_a)):
            _cut, cost, _obj, status = _ops.split_chunks_call(x, off, sel, None, sizes, 4, want_cost=True)
            assert np.all(status.cpu().numpy() == 0)
            assert_close(cost.cpu().numpy(), sim, tol, off, "rl_split_chunks cost_out")
    stream.synchronize()


def one_selected_batch(dim, n_docs=200):
    rng = np.random.default_rng(4000 + dim)
    X = np.concatenate([make_rows(rng, 3, dim) for _ in range(n_docs)]).astype(np.float32)
    off = np.arange(0, 3 * n_docs + 1, 3, dtype=np.int64)
    sel = np.tile(np.asarray([0, 1, 0], np.uint8), n_docs)
    return X, off, sel


def documents_off_the_plain_values(got, plain, dim, off):
    bad = np.abs(got.astype(np.float64) - plain) > ref.tol_plain(dim)
    return int(np.sum(np.add.reduceat(bad, off[:-1]) > 0))


@pytest.mark.parametrize("dim", [64, 128, 256, 1024])
def test_one_selected_row_takes_the_plain_branch(torch_cuda, dim):
    """d equals the one selected row, so that row's X_mod is zero in exact arithmetic and rounding noise in float32: such a document is
    degenerate by rule (partition_sim.hip), and its similarities are the plain ones.  Decided by rounding, as
    before the rule, 25 / 23 / 20 / 9 of these 200 documents at dim 64 / 128 / 256 / 1024 came out up to 0.30 off on the device
    (profiles/partition_sim_error.txt)."""
    X, off, sel = one_selected_batch(dim)
    sim, tol, branches = checked(X, off, sel, ["degenerate"] * 200)
    plain = ref.batch(X, off, None)[0]
    assert np.array_equal(sim, plain)
    got = similarity(X, off, sel)
    print(f"dim {dim}: {documents_off_the_plain_values(got, plain, dim, off)} of 200 one-selected-row documents differ from the plain values")
    assert_close(got, sim, tol, off, "sel = [0, 1, 0]")
    assert similarity(X, off, sel, torch_cuda).tobytes() == got.tobytes()
    # the same through the wrapper: the quantile step selects the middle of three distinct lengths
    assert _nonoutlying(np.asarray([1, 2, 50])).tolist() == [0, 1, 0]
    wrapped = raglite_amd.partition_similarities(X, off, np.tile([1, 2, 50], 200))
    assert wrapped.tobytes() == got.tobytes()


@pytest.fixture(scope="module")
def stride_batch():
    rng = np.random.default_rng(16384)
    n = 16384 + 700
    counts = []
    while sum(counts) < n:
        counts.append(min(int(rng.integers(0, 41)), n - sum(counts)))
    specs = [("none" if d % 7 == 3 else "mod", c) for d, c in enumerate(counts)]
    X, off, sel, want = make_batch(rng, 64, specs)
    return X, off, sel, checked(X, off, sel, want)


def test_more_rows_than_waves_in_the_grid(torch_cuda, stride_batch):
    """The grid is capped at 4 096 blocks of four waves: past 16 384 rows a wave takes row `r + 16 384` next, in the norms kernel and in
    the pairs kernel; ~850 documents for `doc_of`'s binary search.  Rows of the second round, and the document that straddles row
    16 384, agree like the rest."""
    X, off, sel, (sim, tol, branches) = stride_batch
    assert len(X) == 16384 + 700 and 800 < len(branches) < 1000
    d = int(np.searchsorted(off, 16384, side="right")) - 1
    assert off[d] < 16384 < off[d + 1] - 1 and branches[d] == "mod"  # a document straddles the row, as `mod`
    late = sim[16384:]
    assert np.sum(late > 0) > 600 and {"mod", "no_selection"} <= set(branches[d:])
    for torch in (None, torch_cuda):
        got = similarity(X, off, sel, torch)
        assert_close(got[16384:], late, tol[16384:], np.asarray([0, 0]), "rows past 16 384")
        assert_close(got, sim, tol, off, "all rows")


def test_a_zero_row_spoils_its_own_document_only(torch_cuda):
    rng = np.random.default_rng(5)
    specs = [("mod", 6), ("none", 4), ("mod", 8), ("mod", 5), ("axis", 7, [1, 5], 3), ("mod", 3)]
    X, off, sel, want = make_batch(rng, 100, specs)
    b, e = int(off[2]), int(off[3])
    X[b + 3] = 0.0
    sel[b + 3] = 1
    keep = np.concatenate((np.arange(0, b), np.arange(e, len(X))))
    off_without = np.concatenate((off[:3], off[4:] - (e - b)))
    sim, tol, _ = checked(X[keep], off_without, sel[keep], want[:2] + want[3:])
    for torch in (None, torch_cuda):
        got = similarity(X, off, sel, torch)
        without = similarity(X[keep], off_without, sel[keep], torch)
        assert got[keep].tobytes() == without.tobytes()
        assert_close(without, sim, tol, off_without)
        assert got[e - 1] == 0.0  # (the rest of the spoiled document: NaN or anything else)
