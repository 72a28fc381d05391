"""`raglite_amd._chunking.partition_dp` / `solve_partition_dp`: the chunk partition of `_split_chunks.py:87-113` as a shortest path
(DESIGN.md section 4.14).  It is the single host statement of the recurrence `partition_dp.hip` runs and the reference of
tests/test_gpu_partition_dp.py, so here it is held against exhaustive enumeration, the MILP mirror, the reference's own chunks
and the tie rule.  Also: the elementwise heading rule, and the argument checks of the two C entries that return before any HIP call."""

import itertools

import numpy as np
import pytest

from raglite_amd import _abi
from raglite_amd._chunking import (
    _apply_headings,
    _heading_flags,
    _solve_partition,
    apply_headings_elementwise,
    partition_dp,
    solve_partition_dp,
)
from tests.test_oracle_golden import _split_cases

SQRT_EPS = np.float32(np.sqrt(np.finfo(np.float32).eps))


def random_document(rng, n, max_len=59):
    """Costs uniform float32 floored at sqrt(eps) (what rl_partition_similarity can emit), sizes U{1 .. max_len}."""
    cost = np.maximum(rng.random(max(n - 1, 0), dtype=np.float32), SQRT_EPS)
    sizes = rng.integers(1, max_len + 1, size=n).astype(np.int64)
    return cost, sizes


def windows(sizes, max_size):
    """The constraint rows of `_solve_partition`: (i, end_i) for i < W."""
    n = len(sizes)
    csum = np.cumsum(sizes)
    starts = np.concatenate(([0], csum[:-1]))
    ends = np.searchsorted(csum, starts[: n - 1] + max_size, side="right")
    w = int(np.argmax(ends == n)) if np.any(ends == n) else n - 1
    return [(i, int(ends[i])) for i in range(w)]


def feasible(cuts, sizes, max_size):
    """`cuts` in `_solve_partition`'s convention (split after chunklet c - 1) satisfy every window, and no chunk overflows."""
    splits = {c - 1 for c in cuts}
    if not all(any(j in splits for j in range(i, e)) for i, e in windows(sizes, max_size)):
        return False
    bounds = [0, *cuts, len(sizes)]
    return all(int(np.sum(sizes[i:j])) <= max_size for i, j in zip(bounds[:-1], bounds[1:]))


def objective_of(cuts, cost):
    return float(np.sum(cost.astype(np.float64)[[c - 1 for c in cuts]])) if cuts else 0.0


def brute_force(cost, sizes, max_size):
    n, win = len(sizes), windows(sizes, max_size)
    best = np.inf
    for r in range(n):
        for splits in itertools.combinations(range(n - 1), r):
            s = set(splits)
            if all(any(j in s for j in range(i, e)) for i, e in win):
                best = min(best, float(np.sum(cost.astype(np.float64)[list(splits)])))
    return best


def test_equals_exhaustive_enumeration():
    rng = np.random.default_rng(0)
    for case in range(150):
        n = 2 + case % 11  # 2 .. 12
        cost, sizes = random_document(rng, n, max_len=40)
        max_size = int(rng.integers(40, 160))
        cuts, obj, status = partition_dp(cost, sizes, max_size)
        assert status == 0 and feasible(cuts, sizes, max_size), (case, cuts)
        want = brute_force(cost, sizes, max_size)
        assert abs(obj - want) <= 1e-12 and abs(objective_of(cuts, cost) - want) <= 1e-12, (case, obj, want)
        assert cuts == sorted(set(cuts)) and all(1 <= c <= n - 1 for c in cuts)


def test_no_worse_than_the_milp_and_the_same_cuts_where_the_optimum_is_unique():
    rng = np.random.default_rng(0)
    differed = 0
    for case in range(200):
        n = int(rng.integers(2, 401))
        cost, sizes = random_document(rng, n)
        cuts = solve_partition_dp(cost, sizes, 100)
        milp = _solve_partition(cost, sizes, 100)
        assert feasible(cuts, sizes, 100), case
        o_dp, o_milp = objective_of(cuts, cost), objective_of(milp, cost)
        assert o_dp <= o_milp * (1 + 1e-9), (case, o_dp, o_milp)  # not the converse: HiGHS stops at a relative gap
        if cuts != milp:
            differed += 1
            assert abs(o_dp - o_milp) <= 1e-9 * abs(o_milp), (case, o_dp, o_milp)
    print(f"documents whose cuts differ from the MILP's: {differed} of 200")


def test_reference_chunks_on_the_golden_cases():
    seen = 0
    for chunklets, _X, max_size, cost, sizes, chunks in _split_cases():
        if len(cost) == 0:
            continue
        seen += 1
        lens = np.asarray([len(c) for c in chunklets])
        cuts = solve_partition_dp(cost.astype(np.float32), lens, max_size)
        bounds = [0, *cuts, len(chunklets)]
        assert [j - i for i, j in zip(bounds[:-1], bounds[1:])] == sizes.tolist()
        assert ["".join(chunklets[i:j]) for i, j in zip(bounds[:-1], bounds[1:])] == chunks
    assert seen == 4


def tie_documents():
    """(cost, sizes, max_size) with planted ties: equal costs everywhere, or free splits, so only the tie rule decides."""
    docs = []
    for value in (np.float32(1.0), SQRT_EPS):
        for n, size, max_size in ((7, 1, 3), (12, 1, 4), (30, 2, 9), (200, 3, 20), (131, 1, 64), (300, 1, 65)):
            docs.append((np.full(n - 1, value, np.float32), np.full(n, size, np.int64), max_size))
    # ties between "no predecessor" and a predecessor need a zero: a free split
    docs.append((np.asarray([0.0, 1.0, 0.0, 0.0, 1.0], np.float32), np.ones(6, np.int64), 2))
    docs.append((np.zeros(9, np.float32), np.ones(10, np.int64), 3))
    docs.append((np.asarray([0.0, 1.0, 7.0], np.float32), np.ones(4, np.int64), 2))  # the tie sits ON the optimal path
    docs.append((np.asarray([0.0, 0.0, 2.0, 9.0, 9.0], np.float32), np.ones(6, np.int64), 3))
    return docs


def test_planted_ties_follow_the_tie_rule():
    # 7 chunklets of size 1, max_size 3: chunks of <= 3 need >= 2 splits; {1, 4}, {2, 4}, {2, 5}, {3, 5}, {3, 6}... cost 2 each.
    # Last cut: the smallest p >= W - 1; its predecessor: "none" if admissible, else the smallest admissible p.
    cuts, obj, _ = partition_dp(np.ones(6, np.float32), np.ones(7, np.int64), 3)
    assert obj == 2.0 and cuts == [1, 4]
    for cost, sizes, max_size in tie_documents():
        cuts, obj, status = partition_dp(cost, sizes, max_size)
        assert status == 0 and feasible(cuts, sizes, max_size)
        n = len(sizes)
        if len(cost) and np.all(cost == cost[0]) and cost[0] > 0:
            size = int(sizes[0])
            per = max_size // size  # chunklets per chunk at most
            k = -(-n // per) - 1   # fewest splits
            assert len(cuts) == k and obj == float(np.sum(np.full(k, cost[0], np.float64)))
            # the last split is the earliest that lets the tail fit; walking back, every earlier split is the smallest admissible one
            assert cuts[-1] == n - per
    # free splits: the optimum costs nothing ("no predecessor" ties with a predecessor here, but off the backtracked path)
    cuts, obj, _ = partition_dp(np.asarray([0.0, 1.0, 0.0, 0.0, 1.0], np.float32), np.ones(6, np.int64), 2)
    assert obj == 0.0 and feasible(cuts, np.ones(6, np.int64), 2)
    # ... and pinned where it decides the cuts: 4 chunklets of size 1, max_size 2, windows [0, 2) and [1, 3).  The optimum ends in the
    # split at 1 (cost 1; the split at 2 costs 7).  Its predecessor is "none" (0.0, window 0 reaches past 1) or the free split at 0
    # (g[0] = 0.0): a tie on the path.  "None" wins, so the split at 0 is NOT taken although it is free.
    assert partition_dp(np.asarray([0.0, 1.0, 7.0], np.float32), np.ones(4, np.int64), 2) == ([2], 1.0, 0)
    # 6 chunklets, max_size 3, windows [0, 3), [1, 4), [2, 5): the last split is 2 (cost 2, the first p >= W - 1); before it "none"
    # ties with the free splits at 0 and 1 and wins
    assert partition_dp(np.asarray([0.0, 0.0, 2.0, 9.0, 9.0], np.float32), np.ones(6, np.int64), 3) == ([3], 2.0, 0)
    cuts0, obj0, _ = partition_dp(np.zeros(9, np.float32), np.ones(10, np.int64), 3)
    assert obj0 == 0.0 and cuts0 == [1, 4, 7]  # last = smallest p >= W - 1 = 6; then the smallest admissible predecessors, none first


def test_degenerate_shapes():
    assert partition_dp(np.zeros(0, np.float32), np.zeros(0, np.int64), 10) == ([], 0.0, 0)
    assert partition_dp(np.zeros(0, np.float32), np.asarray([7]), 10) == ([], 0.0, 0)
    assert partition_dp(np.asarray([0.5], np.float32), np.asarray([5, 5]), 10) == ([], 0.0, 0)  # n = 2, fits
    assert partition_dp(np.asarray([0.5], np.float32), np.asarray([5, 6]), 10) == ([1], 0.5, 0)  # n = 2, does not
    cost, sizes = random_document(np.random.default_rng(3), 40)
    assert partition_dp(cost, sizes, int(sizes.sum())) == ([], 0.0, 0)  # everything fits: the reference's early exit
    assert partition_dp(cost, sizes, int(sizes.sum()) - 1)[0] != []
    # a chunklet of exactly max_size stands alone: forced cuts on both sides
    sizes = np.asarray([3, 4, 10, 2, 5], np.int64)
    cuts, obj, status = partition_dp(np.asarray([0.9, 0.8, 0.7, 0.1], np.float32), sizes, 10)
    assert status == 0 and 2 in cuts and 3 in cuts and feasible(cuts, sizes, 10)
    assert cuts == [2, 3] and obj == float(np.float64(np.float32(0.8)) + np.float64(np.float32(0.7)))
    # a chunklet over max_size: status 1, no cuts, NaN; the reference's message from solve_partition_dp
    cuts, obj, status = partition_dp(np.ones(2, np.float32), np.asarray([3, 11, 3]), 10)
    assert (cuts, status) == ([], 1) and np.isnan(obj)
    with pytest.raises(ValueError, match="Chunklet larger than chunk max_size detected."):
        solve_partition_dp(np.ones(2, np.float32), np.asarray([3, 11, 3]), 10)
    assert partition_dp(np.zeros(0, np.float32), np.asarray([11]), 10)[2] == 1  # also for a single chunklet
    for bad in (np.nan, np.inf, -np.inf):
        cuts, obj, status = partition_dp(np.asarray([0.5, bad, 0.5], np.float32), np.asarray([6, 6, 6, 6]), 10)
        assert (cuts, status) == ([], 2) and np.isnan(obj)
    # the ignored entry of the batched layout (cost[n - 1]) may hold anything
    assert partition_dp(np.asarray([0.5, np.nan], np.float32), np.asarray([5, 6]), 10) == ([1], 0.5, 0)
    # zero-length chunklets: windows grow over them, ends stay ascending
    sizes = np.asarray([0, 4, 0, 0, 4, 4, 0, 4, 0], np.int64)
    cost = np.asarray([0.3, 0.2, 0.9, 0.1, 0.5, 0.6, 0.05, 0.4], np.float32)
    cuts, obj, status = partition_dp(cost, sizes, 8)
    assert status == 0 and feasible(cuts, sizes, 8) and abs(obj - brute_force(cost, sizes, 8)) <= 1e-12
    cuts, obj, status = partition_dp(np.ones(5, np.float32), np.zeros(6, np.int64), 1)
    assert (cuts, obj, status) == ([], 0.0, 0)
    with pytest.raises(ValueError):
        partition_dp(np.ones(1, np.float32), np.asarray([1, -1]), 10)
    with pytest.raises(ValueError):
        partition_dp(np.ones(1, np.float32), np.asarray([1, 1]), 0)


def _headings_by_loop(sim, flags):
    chunklets = ["# heading\n" if f else "plain text\n" for f in flags]
    return _apply_headings(sim.copy(), chunklets)


def test_elementwise_heading_rule_equals_the_sequential_loop():
    rng = np.random.default_rng(5)
    patterns = [[1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0], [1, 1, 1, 0, 0], [0, 1, 1, 1, 0], [0, 0, 1, 1], [1, 1, 1, 1], [0, 1, 0, 1, 0, 1],
                [1, 0], [0, 1], [1, 1], [0, 0], [1], [0]]
    patterns += [rng.integers(0, 2, size=int(rng.integers(2, 40))).tolist() for _ in range(200)]
    for flags in patterns:
        sim = np.maximum(rng.random(len(flags) - 1, dtype=np.float32), SQRT_EPS)
        want = _headings_by_loop(sim, flags)
        got = apply_headings_elementwise(sim, np.asarray(flags, np.uint8))
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), flags
    texts = ["# Title\n", "body. ", "  ## Sub \n", "#nospace", "\n# late\n", "text #"]
    assert _heading_flags(texts).tolist() == [1, 0, 1, 0, 1, 0]


def test_c_entries_reject_bad_arguments_before_any_hip_call():
    lib = _abi.lib()
    n, dim = 4, 8
    cost = np.ones(n, np.float32)
    sizes = np.ones(n, np.int64)
    off = np.asarray([0, 2, 4], np.int64)
    cut = np.zeros(n, np.uint8)
    obj = np.zeros(2, np.float64)
    status = np.zeros(2, np.int32)
    X = np.ones((n, dim), np.float32)
    sel = np.ones(n, np.uint8)
    p = lambda a: a.ctypes.data  # noqa: E731

    def part(cost=cost, sizes=sizes, off=off, n=n, n_docs=2, max_size=10, cut=cut, obj=obj, status=status):
        return lib.rl_partition_chunks(*(None if a is None else p(a) for a in (cost, sizes, off)), n, n_docs, max_size,
                                       *(None if a is None else p(a) for a in (cut, obj, status)), _abi.MEM_HOST, None)

    def split(X=X, off=off, sizes=sizes, n=n, dim=dim, n_docs=2, max_size=10, cut=cut, status=status):
        return lib.rl_split_chunks(None if X is None else p(X), n, dim, None if off is None else p(off), n_docs, p(sel), None,
                                   None if sizes is None else p(sizes), max_size, None if cut is None else p(cut), None, None,
                                   None if status is None else p(status), _abi.MEM_HOST, None)

    for call, name in ((part, "rl_partition_chunks"), (split, "rl_split_chunks")):
        for kwargs, word in (({"n": -1}, "n"), ({"n_docs": 0}, "n_docs"), ({"max_size": 0}, "max_size"), ({"sizes": None}, "sizes"),
                             ({"off": None}, "doc_offsets"), ({"cut": None}, "cut"), ({"status": None}, "status"),
                             ({"off": np.asarray([1, 2, 4], np.int64)}, "start at 0"),
                             ({"off": np.asarray([0, 3, 2], np.int64)}, "ascending"),
                             ({"off": np.asarray([0, 2, 3], np.int64)}, "end at n"),
                             ({"sizes": np.asarray([1, 1, -1, 1], np.int64)}, "sizes")):
            assert call(**kwargs) == _abi.RL_ERR_INVALID, (name, kwargs)
            err = _abi.last_error()
            assert name in err and word in err, (name, kwargs, err)
        assert call(n=0) == _abi.RL_OK  # nothing to do, nothing written
    assert part(cost=None) == _abi.RL_ERR_INVALID and "cost" in _abi.last_error()
    assert split(X=None) == _abi.RL_ERR_INVALID and "X" in _abi.last_error()
    assert split(dim=0) == _abi.RL_ERR_INVALID
    assert split(X=np.ones((n, 4097), np.float32), dim=4097) == _abi.RL_ERR_UNSUPPORTED
    sim_out = np.zeros(n, np.float32)
    for bad_off, word in ((np.asarray([1, 2, 4], np.int64), "start at 0"), (np.asarray([0, 3, 2], np.int64), "ascending"),
                          (np.asarray([0, 2, 3], np.int64), "end at n")):
        assert lib.rl_partition_similarity(p(X), n, dim, p(bad_off), 2, p(sel), p(sim_out), _abi.MEM_HOST, None) == _abi.RL_ERR_INVALID, word
        err = _abi.last_error()
        assert "rl_partition_similarity" in err and word in err, (word, err)
    assert np.all(cut == 0) and np.all(status == 0) and np.all(sim_out == 0)
