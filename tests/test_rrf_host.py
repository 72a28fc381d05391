"""The weighted RRF contract that rl_rrf_fuse implements (tests/rrf_ref.py) against the package's reciprocal_rank_fusion, the
host restatement of the reference's `_search.py:233-252`: the same ids in the same order and the same float64 scores, bit for bit."""

import numpy as np
import pytest

import raglite_amd
from tests import rrf_ref as ref

WEIGHTS = [(0.75, 0.25), (1.0, 1.0), (1.0, -0.5), (0.0, 1.0), (-0.0, 0.3), (-0.0, -0.0), (2.5, 0.0, -1.25), (0.1, 0.2, 0.3, 0.4)]


def _python(rows, weights, rrf_k):
    rankings = [[int(x) for x in row if x >= 0] for row in rows]
    return raglite_amd.reciprocal_rank_fusion(rankings, k=rrf_k, weights=list(weights))


def _same(rows, weights, rrf_k):
    ids, scores = ref.fuse_one(rows, weights, rrf_k)
    want_ids, want_scores = _python(rows, weights, rrf_k)
    assert ids.tolist() == want_ids
    assert np.array_equal(np.asarray(scores, np.float64).view(np.uint64), np.asarray(want_scores, np.float64).view(np.uint64))


@pytest.mark.parametrize("rrf_k", [1, 60])
@pytest.mark.parametrize("weights", WEIGHTS)
def test_restatement_matches_reciprocal_rank_fusion(weights, rrf_k):
    rng = np.random.default_rng(hash((weights, rrf_k)) & 0xFFFF)
    R = len(weights)
    for L in (1, 2, 6, 20, 64):
        lists = ref.random_lists(rng, R, 12, L)  # overlaps, repeats within a list, padding anywhere
        for b in range(lists.shape[1]):
            _same(lists[:, b], weights, rrf_k)


@pytest.mark.parametrize("rrf_k", [1, 60])
def test_exact_ties_go_by_first_occurrence(rrf_k):
    lists = ref.tie_lists(1, 9)
    ids, scores = ref.fuse_one(lists[:, 0], (1.0, 1.0), rrf_k)
    _same(lists[:, 0], (1.0, 1.0), rrf_k)
    # list 0's entry at rank i and list 1's entry at rank i tie: list 0's comes first
    assert ids.tolist() == [x for i in range(9) for x in (i, 9 + i)]
    assert all(scores[2 * i] == scores[2 * i + 1] for i in range(9))


def test_sum_starts_from_positive_zero():
    # an ordinal that only meets -0.0 weights scores +0.0 (Python: 0.0 + -0.0 == +0.0), and ties with +0.0 ones by first occurrence
    rows = np.array([[3, 1, -1], [2, 3, 4]])
    ids, scores = ref.fuse_one(rows, (-0.0, 0.0), 60)
    assert np.all(np.signbit(scores) == False)  # noqa: E712
    assert ids.tolist() == [3, 1, 2, 4]
    _same(rows, (-0.0, 0.0), 60)


def test_repeats_within_a_list_add_every_time():
    rows = np.array([[5, 5, 7, 5]])
    ids, scores = ref.fuse_one(rows, (1.0,), 60)
    assert ids.tolist() == [5, 7]
    assert scores[0] == ((0.0 + 1.0 / 60) + 1.0 / 61) + 1.0 / 63
    _same(rows, (1.0,), 60)


def test_batch_layout_and_padding():
    rng = np.random.default_rng(3)
    lists = ref.random_lists(rng, 3, 5, 7, pad=0.5)
    lists[:, 2] = -1  # a query with no result at all
    scores, ids, counts = ref.fuse(lists, (0.5, 0.25, 1.0), 60, 10)
    assert counts[2] == 0 and np.all(ids[2] == -1) and np.all(scores[2] == -np.inf)
    for b in range(5):
        want_ids, want_scores = _python(lists[:, b], (0.5, 0.25, 1.0), 60)
        n = int(counts[b])
        assert n == min(10, len(want_ids)) and ids[b, :n].tolist() == want_ids[:n] and scores[b, :n].tolist() == want_scores[:n]
        assert np.all(ids[b, n:] == -1)
