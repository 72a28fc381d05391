"""`raglite_amd._chunklets` on the host: the two mirrors of `_split_chunklets.py:11-71` against the reference's stored arrays, and
`chunklet_dp` -- the single host statement of the recurrence `chunklet_dp.hip` runs -- against the reference's stored cuts, a literal
scalar restatement of the reference's loop, and enumeration of all partitions.  Plus the argument checks of
`rl_partition_chunklets` that return before any HIP call."""

import itertools
import math

import numpy as np
import pytest

from raglite_amd import _abi
from raglite_amd._chunklets import chunklet_dp, compute_num_statements, markdown_chunklet_boundaries, split_chunklets
from tests.chunklets_ref import MAX_SIZES, golden_cases, numeric_document


@pytest.fixture(scope="module")
def cases():
    return golden_cases()


def test_statement_mirror_equals_the_reference_bit_for_bit(cases):
    for sentences, _, statements, _, _ in cases:
        assert compute_num_statements(sentences).tobytes() == statements.tobytes()


def test_markdown_mirror_equals_the_reference_bit_for_bit(cases):
    pytest.importorskip("markdown_it")
    for sentences, boundary, _, _, _ in cases:
        got = markdown_chunklet_boundaries(sentences)
        assert got.dtype == np.float64 and got.tobytes() == boundary.tobytes()
    assert sum(float(b.sum()) for _, b, _, _, _ in cases) > 50  # the fixture does hold boundaries


def test_chunklet_dp_reproduces_the_reference_cuts(cases):
    """Every stored case, over-long sentences included (at max_size 64 most sentences are; documents 8 and 9 hold one in the middle,
    at position 0 and at the end under 512): the partition is the reference's, the status says whether a sentence was too long."""
    seen_long = 0
    for _, boundary, statements, lengths, cuts in cases:
        for max_size in MAX_SIZES:
            got, objective, status = chunklet_dp(boundary, statements, lengths, max_size)
            assert got == cuts[max_size], (len(lengths), max_size)
            assert status == int(lengths.max() > max_size)
            assert math.isinf(objective) if lengths[-1] > max_size else not math.isnan(objective)
            assert status == 1 or math.isfinite(objective)
            seen_long += status
    assert seen_long >= 10  # the fixture does hold such cases: most documents at 64, documents 8 and 9 at 512


def test_split_chunklets_host_default_returns_the_reference_chunklets(cases):
    pytest.importorskip("markdown_it")
    for sentences, _, _, _, cuts in cases[:6]:
        bounds = [0, *cuts[512], len(sentences)]
        assert split_chunklets(sentences, max_size=512) == ["".join(sentences[i:j]) for i, j in zip(bounds[:-1], bounds[1:])]
    with pytest.raises(ValueError, match="partition"):
        split_chunklets(["a. "], partition="gpu")
    with pytest.raises(ValueError, match="custom cost"):
        split_chunklets(["a. "], statement_cost=lambda s: s, partition="device")
    # a custom cost takes the general loop; the default costs spelled out as callables give the default's chunklets
    sentences = cases[4][0]
    assert split_chunklets(sentences, boundary_cost=lambda p: (1.0 - p[0]) + np.sum(p[1:]), max_size=512) == split_chunklets(sentences, max_size=512)


def cost(p, pb, ps, j, i):
    """cost(j, i) of the issue, scalar float64, x * x for the square."""
    s = float(ps[i]) - float(ps[j])
    d = s - 3.0
    return ((1.0 - float(p[j])) + (float(pb[i]) - float(pb[j + 1]))) + d * d / math.sqrt(1e-6 if 1e-6 > s else s) / 2.0


def literal_loop(boundary, statements, lengths, max_size):
    """`_split_chunklets.py:138-178` restated literally -- backward iteration, early break, `<=` -- with x * x for `** 2`."""
    n = len(lengths)
    pc = np.concatenate(([0], np.cumsum(lengths)))
    pb = np.concatenate(([0.0], np.cumsum(boundary)))
    ps = np.concatenate(([0.0], np.cumsum(statements)))
    dp = [math.inf] * (n + 1)
    dp[0] = 0.0
    back = [-1] * (n + 1)
    for i in range(1, n + 1):
        for j in range(i - 1, -1, -1):
            if pc[i] - pc[j] > max_size:
                break
            total = dp[j] + cost(boundary, pb, ps, j, i)
            if total <= dp[i]:
                dp[i], back[i] = total, j
    cuts, i = [], back[n]
    while i > 0:
        cuts.append(i)
        i = back[i]
    return cuts[::-1], dp[n]


def test_chunklet_dp_equals_the_literal_loop_bit_for_bit():
    """Random documents, documents of identical sentences and documents with over-long sentences: same cuts, same objective bits."""
    rng = np.random.default_rng(3)
    for trial in range(120):
        n = int(rng.integers(1, 90))
        boundary, statements, lengths = numeric_document(rng, n, same=trial % 5 == 0)
        max_size = int(rng.choice([64, 300, 512, 2048]))
        if trial % 7 == 0:
            lengths[rng.integers(0, n, size=2)] = max_size + 1 + int(rng.integers(0, 50))
        cuts, objective, status = chunklet_dp(boundary, statements, lengths, max_size)
        want_cuts, want_objective = literal_loop(boundary, statements, lengths, max_size)
        assert cuts == want_cuts and status == int(lengths.max() > max_size)
        assert np.float64(objective).view(np.uint64) == np.float64(want_objective).view(np.uint64)


def test_chunklet_dp_against_enumeration():
    """n <= 12: all 2^(n - 1) partitions under the same cost formula.  Objectives within 1e-12 relative (four orders of magnitude
    above the rounding of 12 additions, far below any real cost gap); the cuts agree wherever the optimum is unique."""
    rng = np.random.default_rng(12)
    unique = 0
    for n in list(range(1, 13)) * 3:
        boundary, statements, lengths = numeric_document(rng, n, max_len=100)
        max_size = int(rng.choice([100, 250, 2048]))
        pc = np.concatenate(([0], np.cumsum(lengths)))
        pb = np.concatenate(([0.0], np.cumsum(boundary)))
        ps = np.concatenate(([0.0], np.cumsum(statements)))
        totals = []
        for mask in itertools.product((0, 1), repeat=n - 1):
            bounds = [0, *[k + 1 for k in range(n - 1) if mask[k]], n]
            if any(pc[i] - pc[j] > max_size for j, i in zip(bounds[:-1], bounds[1:])):
                continue
            total = 0.0
            for j, i in zip(bounds[:-1], bounds[1:]):
                total = total + cost(boundary, pb, ps, j, i)
            totals.append((total, bounds[1:-1]))
        totals.sort(key=lambda t: t[0])
        cuts, objective, status = chunklet_dp(boundary, statements, lengths, max_size)
        assert status == 0 and abs(objective - totals[0][0]) <= 1e-12 * abs(totals[0][0])
        if len(totals) == 1 or totals[1][0] - totals[0][0] > 1e-9 * abs(totals[0][0]):
            assert cuts == totals[0][1]
            unique += 1
    assert unique >= 30


def test_exact_ties_take_the_smallest_position():
    """Seven identical sentences (boundary 0, one statement each): a chunklet of 3 costs 1, of 4 costs 1.25, and 3 + 4 = 4 + 3 =
    2.25 exactly.  At i = 7 the predecessors j = 3 and j = 4 tie; the smallest wins, so the cut is after sentence 3."""
    cuts, objective, status = chunklet_dp(np.zeros(7), np.ones(7), np.full(7, 10), 2048)
    assert (cuts, objective, status) == ([3], 2.25, 0)
    # nine: 3 + 3 + 3 is the unique optimum; ten: 3 + 3 + 4, 3 + 4 + 3 and 4 + 3 + 3 tie, and the smallest j at every step gives 3 + 3 + 4
    assert chunklet_dp(np.zeros(9), np.ones(9), np.full(9, 10), 2048)[0] == [3, 6]
    assert chunklet_dp(np.zeros(10), np.ones(10), np.full(10, 10), 2048)[0] == [3, 6]
    # the window cuts the choice: at most two sentences per chunklet, 2 + 2 + 2 + 1 against 1 + 2 + 2 + 2 and the like (all equal)
    cuts, _, _ = chunklet_dp(np.zeros(7), np.ones(7), np.full(7, 10), 20)
    assert cuts == literal_loop(np.zeros(7), np.ones(7), np.full(7, 10), 20)[0] and len(cuts) == 3


def test_over_long_sentence_follows_the_inf_rules():
    """Sentence 1 alone exceeds max_size: dp[2] = inf with back -1 (an empty window); dp[3] and dp[4] stay inf and, because inf <= inf
    holds in the reference, point to their window's FIRST position, 2.  The backtrack 4 -> 2 -> -1 cuts before sentence 2 only."""
    boundary, statements, lengths = np.zeros(4), np.ones(4), np.asarray([10, 100, 10, 10])
    cuts, objective, status = chunklet_dp(boundary, statements, lengths, 50)
    assert (cuts, status) == ([2], 1) and objective == math.inf
    assert literal_loop(boundary, statements, lengths, 50) == ([2], math.inf)
    # at the end: dp[n] = inf, back[n] = -1, no cut at all; at position 0: everything behind it is inf, one cut before sentence 1
    assert chunklet_dp(boundary, statements, np.asarray([10, 10, 10, 100]), 50) == ([], math.inf, 1)
    assert chunklet_dp(boundary, statements, np.asarray([100, 10, 10, 10]), 50) == ([1], math.inf, 1)


def test_non_finite_input_and_bad_arguments():
    for bad in (np.nan, np.inf, -np.inf):
        boundary, statements = np.zeros(5), np.ones(5)
        statements[2] = bad
        cuts, objective, status = chunklet_dp(boundary, statements, np.full(5, 100), 50)  # over-long too: status 2 wins
        assert cuts == [] and math.isnan(objective) and status == 2
        assert chunklet_dp(np.asarray([0.0, 0.0, 0.0, 0.0, bad]), np.ones(5), np.full(5, 10), 50)[2] == 2
    assert chunklet_dp(np.zeros(0), np.zeros(0), np.zeros(0, np.int64), 5) == ([], 0.0, 0)
    for args in ((np.zeros(2), np.ones(2), [1, 1], 0), (np.zeros(2), np.ones(2), [1, -1], 5), (np.zeros(3), np.ones(2), [1, 1], 5)):
        with pytest.raises(ValueError):
            chunklet_dp(*args)


def test_c_entry_rejects_bad_arguments_without_a_gpu():
    """`rl_partition_chunklets` returns RL_ERR_INVALID before any HIP call for every listed argument error; n == 0 is RL_OK."""
    lib = _abi.lib()
    b, s = np.zeros(4), np.ones(4)
    ln = np.asarray([1, 2, 3, 4], np.int64)
    off = np.asarray([0, 2, 4], np.int64)
    cut, obj, st = np.zeros(4, np.uint8), np.zeros(2), np.zeros(2, np.int32)

    def call(boundary=b, statements=s, lengths=ln, offsets=off, n=4, n_docs=2, max_size=10, cut_=cut, status=st, mem=_abi.MEM_HOST):
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return lib.rl_partition_chunklets(ptr(boundary), ptr(statements), ptr(lengths), ptr(offsets), n, n_docs, max_size, ptr(cut_),
                                          obj.ctypes.data, ptr(status), mem, None)

    assert call(n=-1) == _abi.RL_ERR_INVALID and "rl_partition_chunklets" in _abi.last_error()
    assert call(max_size=0) == _abi.RL_ERR_INVALID
    assert call(n_docs=0) == _abi.RL_ERR_INVALID
    assert call(mem=7) == _abi.RL_ERR_INVALID
    for name in ("boundary", "statements", "lengths", "offsets", "cut_", "status"):
        assert call(**{name: None}) == _abi.RL_ERR_INVALID, name
    assert call(offsets=np.asarray([1, 2, 4], np.int64)) == _abi.RL_ERR_INVALID and "start at 0" in _abi.last_error()
    assert call(offsets=np.asarray([0, 3, 2], np.int64)) == _abi.RL_ERR_INVALID and "ascending" in _abi.last_error()
    assert call(offsets=np.asarray([0, 2, 3], np.int64)) == _abi.RL_ERR_INVALID and "end at n" in _abi.last_error()
    assert call(lengths=np.asarray([1, -2, 3, 4], np.int64)) == _abi.RL_ERR_INVALID
    assert call(n=0, boundary=None, statements=None, lengths=None, offsets=None, cut_=None, status=None) == _abi.RL_OK
    assert cut.sum() == 0 and st.sum() == 0  # nothing was written by any of these
