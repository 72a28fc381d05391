"""`raglite_amd._keyword.Vocabulary`: the stable term ids of the device token store and their ranks in the sorted vocabulary (host only)."""

import numpy as np

from raglite_amd import _keyword


def _argsort_of_argsort(stems):
    return np.argsort(np.argsort(np.asarray(stems, dtype=object), kind="stable"), kind="stable").astype(np.int32)


def test_ids_are_stable_under_growth_and_follow_first_appearance():
    v = _keyword.Vocabulary()
    first = v.add(["pear", "apple", "pear", "zebra"])
    assert first.dtype == np.int32 and first.tolist() == [0, 1, 0, 2] and len(v) == 3
    second = v.add(["aardvark", "apple", "mango", "aardvark"])
    assert second.tolist() == [3, 1, 4, 3] and len(v) == 5
    assert v.add(["pear", "apple", "zebra"]).tolist() == [0, 1, 2]  # what was stored keeps its id
    assert v.stems == ["pear", "apple", "zebra", "aardvark", "mango"] and "mango" in v and "kiwi" not in v
    assert v.add([]).tolist() == [] and len(v) == 5


def test_ranks_are_the_argsort_of_the_argsort_of_the_stems():
    rng = np.random.default_rng(3)
    stems = ["".join(rng.choice(list("abcxyz"), size=int(rng.integers(1, 6)))) for _ in range(400)]
    v = _keyword.Vocabulary()
    v.add(stems)
    r = v.ranks()
    assert r.dtype == np.int32 and np.array_equal(r, _argsort_of_argsort(v.stems))
    assert sorted(v.stems) == [s for _, s in sorted(zip(r.tolist(), v.stems))]
    assert v.ranks() is r  # recomputed only after growth
    assert _keyword.Vocabulary().ranks().size == 0


def test_ranks_change_when_a_stem_that_sorts_earlier_arrives():
    v = _keyword.Vocabulary()
    v.add(["mango", "pear"])
    assert v.ranks().tolist() == [0, 1]
    v.add(["zebra"])  # sorts last: the others keep their ranks
    assert v.ranks().tolist() == [0, 1, 2]
    v.add(["apple"])  # sorts first: every rank moves up, the ids stay
    assert v.ranks().tolist() == [1, 2, 3, 0] and v.add(["mango"]).tolist() == [0]


def test_a_query_maps_to_sorted_ranks_and_drops_unknown_stems():
    v = _keyword.Vocabulary()
    v.add(["pear", "apple", "zebra", "mango"])
    assert v.query_ranks(["zebra", "kiwi", "apple", "zebra"]) == [0, 3]
    assert v.query_ranks(["kiwi"]) == [] and v.query_ranks([]) == []
    assert len(v) == 4  # a query adds nothing


def test_a_vocabulary_grown_in_pieces_ranks_like_one_built_at_once():
    rng = np.random.default_rng(11)
    stems = [f"s{int(x)}" for x in rng.integers(0, 300, size=2000)]
    whole, pieces = _keyword.Vocabulary(), _keyword.Vocabulary()
    ids_whole = whole.add(stems)
    ids_pieces = np.concatenate([pieces.add(stems[a:b]) for a, b in ((0, 1), (1, 700), (700, 700), (700, 2000))])
    assert np.array_equal(ids_whole, ids_pieces) and whole.stems == pieces.stems
    assert np.array_equal(whole.ranks(), pieces.ranks())
    # the rank of a stored token is the term id the sorted vocabulary of build_from_stems gives its stem
    vocab = sorted(set(stems))
    assert [vocab[r] for r in whole.ranks()[ids_whole]] == stems


def test_stems_to_store_ids_marks_the_dead_chunks():
    v = _keyword.Vocabulary()
    flat, off, dead = _keyword.stems_to_store_ids([["b", "a", "b"], None, [], ["c"]], v)
    assert flat.tolist() == [0, 1, 0, 2] and off.tolist() == [0, 3, 3, 3, 4] and dead.tolist() == [1]
    assert flat.dtype == np.int32 and off.dtype == np.int64 and dead.dtype == np.int64


def test_a_query_can_be_numbered_by_the_ranks_of_an_earlier_build():
    """An index keeps the numbering it was built with: stems added since are unknown to it, and the old ranks are not touched by growth."""
    v = _keyword.Vocabulary()
    v.add(["mango", "pear"])
    built = v.ranks()
    v.add(["apple"])  # sorts first: the current ranks move, the built ones stay
    assert built.tolist() == [0, 1] and v.ranks().tolist() == [1, 2, 0]
    assert v.query_ranks(["pear", "apple", "mango"], built) == [0, 1]
    assert v.query_ranks(["pear", "apple", "mango"]) == [0, 1, 2]
    assert v.query_ranks(["apple"], built) == []
