"""The host statement of the sentence partition (`raglite_amd._sentences`) against the reference's stored results
(`tests/golden/split_sentences.npz`, written by scripts/make_golden_sentences.py from the reference's own module), its mirrors, its tie
rules and the argument checks of `rl_partition_sentences`.  No GPU."""

import numpy as np
import pytest

import raglite_amd
from raglite_amd import _abi
from raglite_amd._sentences import (
    SENTENCES_NO_SPLIT,
    SENTENCES_NOT_FINITE,
    SENTENCES_OK,
    SENTENCES_TOO_LONG,
    markdown_sentence_boundaries,
    propagate_whitespace,
    sentence_dp,
    sentence_partition,
    split_sentences,
    whitespace_mask,
)
from tests.sentences_ref import CASES, GOLDEN, golden_cases


def sentences_of(doc, bounds):
    edges = [0, *[b + 1 for b in bounds], len(doc)]
    return [doc[i:j] for i, j in zip(edges[:-1], edges[1:])]


def lengths_of(n, bounds):
    return np.diff([0, *[b + 1 for b in bounds], n]).tolist()


@pytest.fixture(scope="module")
def cases():
    return golden_cases()


def test_statement_gives_the_reference_sentences(cases):
    """Every stored case: float32 and float64 predictions, five (min_len, max_len) each; phase 2 adds boundaries in some of them."""
    assert len(cases) >= 12 and {c[1].dtype for c in cases} == {np.dtype(np.float32), np.dtype(np.float64)}
    phase2 = 0
    for doc, predictions, known, starts in cases:
        space = whitespace_mask(doc)
        free = len(sentence_partition(predictions, space, 4, None, known)[0])
        for min_len, max_len in CASES:
            bounds, objective, status = sentence_partition(predictions, space, min_len, max_len, known)
            want = starts[(min_len, max_len)]
            if want is None:
                assert status == SENTENCES_NO_SPLIT and not bounds
                continue
            assert [b + 1 for b in bounds] == want and np.isfinite(objective)
            longest = max(lengths_of(len(doc), bounds))
            assert status == int(max_len is not None and longest > max_len) and min(lengths_of(len(doc), bounds)) >= min_len
            phase2 += min_len == 4 and max_len is not None and len(bounds) > free
    assert phase2 >= 6


def test_split_sentences_on_the_host(cases):
    for doc, predictions, known, starts in cases:
        for min_len, max_len in CASES:
            want = sentences_of(doc, [s - 1 for s in starts[(min_len, max_len)]])
            assert split_sentences(doc, min_len, max_len, known, predicted_probas=predictions) == want
            assert split_sentences(doc, min_len, max_len, lambda d: known, predicted_probas=lambda d: predictions) == want


def test_markdown_mirror_equals_the_stored_array(cases):
    pytest.importorskip("markdown_it")
    seen = 0
    for doc, _, known, _ in cases:
        mine = markdown_sentence_boundaries(doc)
        assert mine.dtype == np.float64 and mine.tobytes() == known.tobytes()
        seen += int(np.isfinite(known).any())
    assert seen >= 3
    assert markdown_sentence_boundaries("").shape == (0,)
    assert markdown_sentence_boundaries("# T").tolist() == [0.0, 0.0, 0.0]  # the heading's end lies behind the document
    got = markdown_sentence_boundaries("ab\n\n# T\ncd")  # the heading's range reaches one character into the next line
    assert got[3] == 1 and got[4:8].tolist() == [0, 0, 0, 0] and got[8] == 1 and np.isnan(got[[0, 1, 2, 9]]).all()


def test_whitespace_class_is_str_isspace_for_every_code_point():
    cp = np.arange(0x110000, dtype=np.uint32)
    mask = whitespace_mask(cp)
    want = np.fromiter((chr(c).isspace() for c in range(0x110000)), dtype=np.uint8, count=0x110000)
    assert mask.dtype == np.uint8 and np.array_equal(mask, want) and int(mask.sum()) == 29
    assert not mask[0x200B] and not mask[0x180E] and mask[0x85] and mask[0x3000]
    text = "a\u00a0b\u2003c\u200bd\n\ud800\u3000e"  # a lone surrogate passes through the encoder
    assert whitespace_mask(text).tolist() == [int(c.isspace()) for c in text]


def reference_propagation(probas, is_space):
    """The loop of `_split_sentences.py:189-196` over the ranges as the docstring of `propagate_whitespace` defines them."""
    p = probas.copy()
    n = len(p)
    i = 0
    while i < n - 1:
        if not is_space[i] and is_space[i + 1]:
            j = i + 1
            while j < n and is_space[j]:
                j += 1
            if j < n:
                lo, hi = p[i:j].min(), p[i:j].max()
                p[i:j - 1] = lo
                p[j - 1] = hi
            i = j
        else:
            i += 1
    return p


def test_propagation_mirror():
    rng = np.random.default_rng(0)
    for n in (0, 1, 2, 3, 10, 500, 5000):
        for rate in (0.0, 0.3, 0.9, 1.0):
            for dtype in (np.float32, np.float64):
                space = rng.random(n) < rate
                probas = rng.random(n).astype(dtype)
                got = propagate_whitespace(probas, space)
                assert got.dtype == dtype and got.tobytes() == reference_propagation(probas, space).tobytes()
    p = np.asarray([0.1, 0.9, 0.5, 0.2, 0.7, 0.3, 0.6, 0.4])
    #               sp   a    sp   sp   b    c    sp   sp      a leading run, "a" + 2, "c" + a trailing run
    got = propagate_whitespace(p, np.asarray([1, 0, 1, 1, 0, 0, 1, 1]))
    assert got.tolist() == [0.1, 0.2, 0.2, 0.9, 0.7, 0.3, 0.6, 0.4]


def test_both_tie_rules_on_constant_probabilities():
    """Without max_len the earliest of equal predecessors wins, with max_len the latest in the window; the golden file holds what the
    reference's own programme gave for these two inputs."""
    stored = np.load(GOLDEN)
    assert stored["ties_earliest"].tolist() == [4] * 10 and stored["ties_latest"].tolist() == [12, 4, 4, 4, 4, 12]
    for dtype in (np.float32, np.float64):
        bounds, best, status = sentence_dp(np.full(40, 0.5, dtype), 4)
        assert lengths_of(40, bounds) == [4] * 10 and best == 2.25 and status == SENTENCES_OK
        bounds, best, status = sentence_dp(np.full(40, 0.25, dtype), 4, 12)
        assert lengths_of(40, bounds) == [12, 4, 4, 4, 4, 12] and best == 0.0 and status == SENTENCES_OK
        assert sentence_dp(np.full(40, 0.25, dtype), 4) == ([], 0.0, SENTENCES_OK)  # nothing is above 0.0: no boundary
        # both phases in one call: phase 1 finds nothing, phase 2 gets the whole document
        assert lengths_of(40, sentence_partition(np.full(40, 0.25, dtype), np.zeros(40), 4, 12)[0]) == [12, 4, 4, 4, 4, 12]
    # the same values under the other rule: at 0.5 with max_len the chain of ten is still the only optimum
    assert lengths_of(40, sentence_dp(np.full(40, 0.5), 4, 12)[0]) == [4] * 10


def test_phase_two_cases():
    zeros10, zeros11, half11 = np.zeros(10), np.zeros(11), np.full(11, 0.5)
    assert sentence_dp(zeros10, 4, 5) == ([4], -0.25, SENTENCES_OK)
    assert lengths_of(10, sentence_partition(zeros10, np.zeros(10), 4, 5)[0]) == [5, 5]
    bounds, best, status = sentence_dp(zeros11, 4, 5)
    assert (bounds, status) == ([], SENTENCES_NO_SPLIT) and best == -np.inf
    assert sentence_partition(zeros11, np.zeros(11), 4, 5) == ([], 0.0, SENTENCES_NO_SPLIT)
    doc = "abcdefghijk"
    nothing = np.full(11, np.nan)
    with pytest.raises(ValueError, match="Sentence partition failed: no valid split satisfies the constraints."):
        split_sentences(doc, 4, 5, nothing, predicted_probas=zeros11)
    assert split_sentences(doc[:10], 4, 5, nothing[:10], predicted_probas=zeros10) == ["abcde", "fghij"]
    # at 0.5 phase 1 gives abcd + efghijk; 7 characters are longer than max_len and shorter than 2 min_len: unsplit, nothing raised
    assert sentence_partition(half11, np.zeros(11), 4, 5) == ([3], 0.25, SENTENCES_TOO_LONG)
    assert split_sentences(doc, 4, 5, nothing, predicted_probas=half11) == ["abcd", "efghijk"]
    assert sentence_dp(np.full(7, 0.5), 4, 5) == ([], 0.0, SENTENCES_TOO_LONG)
    # the early exit never looks at the probabilities
    assert split_sentences("abcd", predicted_probas=None) == ["abcd"]
    with pytest.raises(ValueError, match="10 probabilities"):
        split_sentences(doc, predicted_probas=zeros10)


def test_score_dtype_is_the_input_dtype():
    """`probas - 0.25` is rounded to float32 for float32 input (0.001 - 0.25 needs more bits than float32 has), and dp follows."""
    small = np.float32(1e-3)
    p32 = np.full(10, small)
    b32, best32, _ = sentence_dp(p32, 4, 5)
    b64, best64, _ = sentence_dp(p32.astype(np.float64), 4, 5)
    assert b32 == b64 == [4]
    assert best32 == float(small - np.float32(0.25)) and best64 == float(small) - 0.25 and best32 != best64


def test_non_finite_input():
    for bad in (np.nan, np.inf, -np.inf):
        p = np.full(20, 0.5)
        p[7] = bad
        bounds, best, status = sentence_dp(p, 4)
        assert bounds == [] and np.isnan(best) and status == SENTENCES_NOT_FINITE
        assert sentence_partition(p, np.zeros(20), 4, 8)[2] == SENTENCES_NOT_FINITE
        with pytest.raises(ValueError, match="Non-finite"):
            split_sentences("x" * 20, 4, None, np.full(20, np.nan), predicted_probas=p)
    p = np.full(20, np.nan)
    known = np.full(20, 0.5)
    assert sentence_partition(p, np.zeros(20), 4, None, known)[2] == SENTENCES_OK  # the override repairs it
    known[3] = np.inf  # not finite: the prediction stays
    assert sentence_partition(p, np.zeros(20), 4, None, known)[2] == SENTENCES_NOT_FINITE
    huge = np.where(np.arange(20) == 3, 1e300, np.nan)  # finite in float64 only
    assert sentence_partition(np.full(20, 0.5), np.zeros(20), 4, None, huge)[2] == SENTENCES_OK
    assert sentence_partition(np.full(20, 0.5, np.float32), np.zeros(20), 4, None, huge)[2] == SENTENCES_NOT_FINITE


def test_c_entry_argument_validation_without_gpu():
    lib = _abi.lib()
    n = 8
    cp = np.full(n, 0x61, np.uint32)
    p = np.zeros(n, np.float32)
    cut = np.zeros(n, np.uint8)
    status = np.zeros(2, np.int32)
    good = np.asarray([0, 3, 8], np.int64)

    def call(n=n, n_docs=2, min_len=4, max_len=0, cp=cp, p=p, off=good, cut=cut, status=status, mem=_abi.MEM_HOST):
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return lib.rl_partition_sentences(ptr(cp), ptr(p), 0, None, ptr(off), n, n_docs, min_len, max_len, ptr(cut), None, ptr(status),
                                          mem, None)

    for kwargs, word in (({"n": -1}, "n must"), ({"min_len": 0}, "min_len"), ({"max_len": -1}, "max_len"), ({"n_docs": 0}, "n_docs"),
                         ({"cp": None}, "codepoints"), ({"p": None}, "probas"), ({"off": None}, "doc_offsets"), ({"cut": None}, "cut"),
                         ({"status": None}, "status"), ({"mem": 7}, "mem"),
                         ({"off": np.asarray([1, 3, 8], np.int64)}, "start at 0"),
                         ({"off": np.asarray([0, 9, 8], np.int64)}, "ascending"),
                         ({"off": np.asarray([0, 3, 7], np.int64)}, "end at n"),
                         ({"n": 1 << 31, "n_docs": 1, "off": np.asarray([0, 1 << 31], np.int64)}, "2\\^31"),
                         ({"n": 1 << 31, "n_docs": 1, "mem": _abi.MEM_DEVICE}, "2\\^31"),
                         ({"n": (1 << 31) + 3, "off": np.asarray([0, 3, (1 << 31) + 3], np.int64)}, "2\\^31")):
        assert call(**kwargs) == _abi.RL_ERR_INVALID, kwargs
        assert "rl_partition_sentences" in _abi.last_error() and __import__("re").search(word, _abi.last_error()), (kwargs, _abi.last_error())
    assert call(n=0, n_docs=0, cp=None, p=None, off=None, cut=None, status=None) == _abi.RL_OK  # nothing to do, nothing written
    assert not cut.any()


def test_wrapper_checks_without_gpu():
    with pytest.raises(ValueError, match="min_len"):
        raglite_amd.partition_sentences(np.zeros(4, np.uint32), np.zeros(4), np.asarray([0, 4]), min_len=0)
    with pytest.raises(ValueError, match="differ in length"):
        raglite_amd.partition_sentences(np.zeros(5, np.uint32), np.zeros(4), np.asarray([0, 4]))
    cut, objective, status = raglite_amd.partition_sentences(np.zeros(0, np.uint32), np.zeros(0), np.asarray([0, 0, 0]))
    assert cut.shape == (0,) and objective.tolist() == [0.0, 0.0] and status.tolist() == [0, 0]
    assert raglite_amd.split_sentences_batch(["", "abc", "abcd"], predicted_probas=None) == [[""], ["abc"], ["abcd"]]
    with pytest.raises(ValueError, match="share a dtype"):
        raglite_amd.split_sentences_batch(["abcdefgh", "abcdefgh"], predicted_probas=[np.zeros(8, np.float32), np.zeros(8)],
                                          boundary_probas=lambda doc: np.full(len(doc), np.nan))
    with pytest.raises(ValueError, match="one predicted_probas array per document"):
        raglite_amd.split_sentences_batch(["abcdefgh"], predicted_probas=[])
