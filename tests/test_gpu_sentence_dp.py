"""`rl_partition_sentences` / `split_sentences_batch` / `split_texts_batch` on the device against the host statement
(`raglite_amd._sentences.sentence_partition`: `sentence_dp` plus the mirrors, themselves held against the reference's stored sentences
in tests/test_sentences_host.py).  `cut` is compared as bytes, `objective` as uint64 bits, `status` as integers, for host and for
device pointers.  Neither markdown-it nor the reference is needed (where a test goes through the Markdown parse and markdown-it is
missing, a stand-in replaces the parse on both sides of the comparison)."""

import numpy as np
import pytest

import raglite_amd
from raglite_amd import _chunklets, _sentences
from oracle.fake_embedder import FakeLlama
from tests.sentences_ref import CASES, golden_cases, host_batch, numeric_document, pack, text_document

pytestmark = pytest.mark.gpu


def check_call(torch, cp, probas, known, off, min_len, max_len, want=None, sides=("host", "device")):
    want = want or host_batch(cp, probas, known, off, min_len, max_len)
    for side in sides:
        if side == "host":
            cut, obj, status = raglite_amd.partition_sentences(cp, probas, off, min_len, max_len, known)
        else:
            dev = lambda a: None if a is None else torch.as_tensor(a, device="cuda")  # noqa: E731
            t = raglite_amd.partition_sentences(dev(cp.view(np.int32)), dev(probas), dev(off), min_len, max_len, dev(known))
            assert all(x.is_cuda for x in t)
            cut, obj, status = (x.cpu().numpy() for x in t)
        assert cut.dtype == np.uint8 and obj.dtype == np.float64 and status.dtype == np.int32
        assert np.array_equal(status, want[2]), (side, np.flatnonzero(status != want[2])[:8])
        assert cut.tobytes() == want[0].tobytes(), (side, np.flatnonzero(cut != want[0])[:8])
        assert np.array_equal(obj.view(np.uint64), want[1].view(np.uint64)), (side, np.flatnonzero(obj.view(np.uint64) != want[1].view(np.uint64))[:8])
    return want


def letters(n, proba, dtype=np.float64):
    return text_document("abcdefghijklmnopqrstuvwxyz"[:n] if n <= 26 else "x" * n, proba, dtype)


def lengths_of(cut_of_one_document):
    return np.diff(np.concatenate(([0], np.flatnonzero(cut_of_one_document) + 1, [len(cut_of_one_document)]))).tolist()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_documents_around_min_len(torch_cuda, dtype):
    """0, 1, min_len, min_len + 1, 2 min_len - 1 and 2 min_len characters at probability 0.5, with empty documents first, last and in
    a row: only the last length can hold a boundary.  Under max_len 5 the documents of 7 characters come back unsplit (status 1)."""
    docs = [letters(k, 0.5, dtype) for k in (0, 0, 1, 4, 5, 0, 0, 7, 8, 3, 0)]
    want = check_call(torch_cuda, *pack(docs), 4, None)
    assert np.flatnonzero(want[0]).tolist() == [17 + 3] and want[2].tolist() == [0] * 11
    assert want[1].tolist() == [0.0] * 8 + [0.25, 0.0, 0.0]
    want = check_call(torch_cuda, *pack(docs), 4, 5)
    assert np.flatnonzero(want[0]).tolist() == [17 + 3] and want[2].tolist() == [0] * 7 + [1, 0, 0, 0]
    only_empty = check_call(torch_cuda, *pack([letters(0, 0.5, dtype)] * 2), 4, 5)  # n == 0: the call writes nothing
    assert only_empty[1].tolist() == [0.0, 0.0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("min_len", [1, 4, 64, 70])
def test_lengths_around_the_block_of_64(torch_cuda, dtype, min_len):
    """Phase 1 walks 64 positions per block from position min_len - 1: documents of 63 to 129 characters (and these plus
    2 min_len - 1, so that the walked range itself has those lengths); min_len 64 and 70 take every predecessor from the block's
    load, min_len 1 and 4 from the block's own lanes."""
    rng = np.random.default_rng(64 + min_len)
    sizes = [63, 64, 65, 127, 128, 129]
    docs = [numeric_document(rng, n + extra, dtype, levels=8) for extra in (0, 2 * min_len - 1) for n in sizes]
    want = check_call(torch_cuda, *pack(docs), min_len, None)
    assert want[0].sum() >= len(docs) // 2 and not want[2].any()


def test_constant_probabilities_show_both_tie_rules(torch_cuda):
    """40 characters at 0.5, min_len 4: every position is worth the same, the EARLIEST of equal predecessors wins and the chain of
    ten sentences of 4 is the best.  At 0.25 every score is 0, phase 1 finds nothing above 0.0 and the whole document goes to phase 2
    under max_len 12, where the LATEST of equal predecessors in the window wins: 12, 4, 4, 4, 4, 12."""
    for dtype in (np.float32, np.float64):
        want = check_call(torch_cuda, *pack([letters(40, 0.5, dtype)]), 4, None)
        assert lengths_of(want[0]) == [4] * 10 and want[1][0] == 9 * 0.25
        want = check_call(torch_cuda, *pack([letters(40, 0.25, dtype), letters(40, 0.5, dtype)]), 4, 12)
        assert lengths_of(want[0][:40]) == [12, 4, 4, 4, 4, 12] and lengths_of(want[0][40:]) == [4] * 10
        assert want[1].tolist() == [0.0, 9 * 0.25] and want[2].tolist() == [0, 0]


@pytest.mark.parametrize("min_len,max_len", [(4, 34), (4, 68), (4, 69), (6, 206)])
def test_windows_narrower_and_wider_than_a_wave(torch_cuda, min_len, max_len):
    """max_len - min_len of 30, 64, 65 and 200.  Probabilities of at most 0.25 in 17 steps: no score is positive, so phase 1 leaves
    every document whole and phase 2 solves all of it, with equal window values in different lanes and rounds."""
    rng = np.random.default_rng(max_len)
    docs = []
    for n in (max_len + 1, 2 * max_len, 700, 1501):
        cp, p, _ = numeric_document(rng, n, np.float64, levels=16)
        docs.append((cp, p / 4.0, None))
    docs.append(letters(900, 0.25))
    want = check_call(torch_cuda, *pack(docs), min_len, max_len)
    assert not want[2].any() and not want[1].any() and max(lengths_of(want[0][:max_len + 1])) <= max_len
    assert max(lengths_of(want[0][-900:])) <= max_len


def test_white_space_runs(torch_cuda):
    """Runs at the very start and end of a document (no range), a run of 5 000 characters, runs straddling multiples of 64, a document
    of white space only and one without any, and the Unicode spaces next to U+200B (which is none).  Probabilities in 9 steps, so the
    minimum and the maximum of a run differ from what the positions held."""
    rng = np.random.default_rng(5000)
    texts = [
        "  \n\t leading and trailing.  Second one here?   \n\n",
        "word" + " " * 5000 + "after the long run. And more text follows here.",
        "a" * 60 + " " * 10 + "b" * 50 + "\n" * 20 + "c" * 53 + " \t" * 40 + "d" * 30,
        " \n\t \u00a0\u2003\u3000\u0085" * 30,
        "nowhitespaceatallinthisdocument" * 10,
        "one\u00a0two\u2003three\u3000four\u0085five\u200bsix\u200b seven \u200beight\u180enine. " * 12,
        " ",
        "x ",
        " x",
        "ab  \n",
    ]
    for dtype in (np.float32, np.float64):
        docs = [text_document(t, rng.integers(0, 9, size=len(t)) / 8.0, dtype) for t in texts]
        cp, probas, known, off = pack(docs)
        want = check_call(torch_cuda, cp, probas, known, off, 4, 64)
        flat = host_batch(np.full(len(cp), 0x61, np.uint32), probas, known, off, 4, 64)  # the same without any white space
        for d in (0, 1, 2, 5):
            assert want[0][off[d]:off[d + 1]].tobytes() != flat[0][off[d]:off[d + 1]].tobytes(), d
        for d in (3, 4):
            assert want[0][off[d]:off[d + 1]].tobytes() == flat[0][off[d]:off[d + 1]].tobytes(), d
        free = check_call(torch_cuda, cp, probas, known, off, 4, None)
        assert not free[0][off[1] + 3:off[1] + 5003].any(), "a boundary inside the long run: its probabilities are the run's minimum"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_known_boundaries_override_the_predictions(torch_cuda, dtype):
    """NaN keeps the prediction, 0 / 1 / 0.5 replace it; an infinite known value keeps it too (`np.isfinite`); a value that is finite
    in float64 and not in float32 makes the float32 document non-finite."""
    rng = np.random.default_rng(7)
    docs = [numeric_document(rng, n, dtype, known_rate=r) for n, r in ((300, 0.1), (1000, 0.3), (50, 0.0), (777, 0.05))]
    docs[1][2][5], docs[1][2][6] = np.inf, -np.inf
    docs.append((docs[0][0], docs[0][1], np.where(np.arange(300) == 7, 1e300, np.nan)))
    cp, probas, known, off = pack(docs)
    want = check_call(torch_cuda, cp, probas, known, off, 4, 100)
    plain = host_batch(cp, probas, None, off, 4, 100)
    assert want[2].tolist() == [0, 0, 0, 0, 2 if dtype == np.float32 else 0]
    assert want[0][:300].tobytes() != plain[0][:300].tobytes() and want[0][1300:1350].tobytes() == plain[0][1300:1350].tobytes()


def test_failing_documents_between_clean_ones(torch_cuda):
    """Status 2 (NaN, +inf), status 3 (11 characters of probability 0 cannot be cut into pieces of 4 to 5) and status 1 (at 0.5 phase 1
    gives 4 + 7, and 7 is longer than max_len 5 but shorter than 2 min_len): the clean documents around them keep their results."""
    rng = np.random.default_rng(3)
    clean = [numeric_document(rng, 90, np.float64) for _ in range(5)]
    nan_doc = numeric_document(rng, 90, np.float64)
    nan_doc[1][33] = np.nan
    inf_doc = numeric_document(rng, 200, np.float64)
    inf_doc[1][199] = np.inf
    docs = [clean[0], nan_doc, clean[1], letters(11, 0.0), clean[2], letters(11, 0.5), clean[3], inf_doc, letters(10, 0.0), clean[4]]
    cp, probas, known, off = pack(docs)
    want = check_call(torch_cuda, cp, probas, known, off, 4, 5)
    assert want[2][[1, 3, 5, 7, 8]].tolist() == [2, 3, 1, 2, 0] and np.isnan(want[1][[1, 7]]).all()
    for d in (1, 3, 7):
        assert not want[0][off[d]:off[d + 1]].any()
    assert lengths_of(want[0][off[5]:off[6]]) == [4, 7] and lengths_of(want[0][off[8]:off[9]]) == [5, 5]
    alone = host_batch(*pack(clean), 4, 5)
    assert np.array_equal(want[1][[0, 2, 4, 6, 9]], alone[1]) and want[0][off[9]:].tobytes() == alone[0][-90:].tobytes()
    assert np.array_equal(want[2][[0, 2, 4, 6, 9]], alone[2])
    # a long document whose phase-2 failure comes after a sentence that phase 2 did cut: none of the cuts stay
    cp2, p2, _ = numeric_document(rng, 400, np.float64, space_rate=0.0, levels=16)
    p2 = p2 / 4.0
    p2[200], p2[211] = 1.0, 1.0  # phase 1: [0, 200], [201, 211] (11 characters of probability 0 inside), [212, 400)
    p2[201:211] = 0.0
    late = check_call(torch_cuda, cp2, p2, None, np.asarray([0, 400]), 4, 5)
    assert late[2].tolist() == [3] and not late[0].any() and late[1][0] == 1.5


def test_more_documents_than_waves_in_the_grid(torch_cuda):
    """The launch caps its grid at 4 096 blocks of four waves: past 16 384 documents a wave takes document `doc + 16 384` next.
    20 000 documents of 0 to 12 characters, so the second round holds cut and uncut, empty, failing and non-finite documents."""
    rng = np.random.default_rng(16384)
    counts = rng.integers(0, 13, size=20000)
    counts[[0, 16383, 16384, 16385, 17000, 17001, 19999]] = [0, 12, 0, 12, 11, 9, 12]
    docs = [numeric_document(rng, int(c), np.float32, levels=4) for c in counts]
    docs[16385][1][:] = 0.5
    docs[17000][1][:] = 0.0          # status 3 in the second round
    docs[17001][1][4] = np.nan       # status 2 in the second round
    cp, probas, known, off = pack(docs)
    want = check_call(torch_cuda, cp, probas, known, off, 4, 5, sides=("device",))
    assert want[0][int(off[16384]):].sum() > 500 and want[2][17000] == 3 and want[2][17001] == 2
    assert lengths_of(want[0][off[16385]:off[16386]]) == [4, 4, 4]


def test_one_document_of_two_hundred_thousand_characters(torch_cuda):
    """No limit on a document's length: 3 125 blocks of 64 in phase 1 for one wave; a stretch of 6 000 characters without a positive
    score, which phase 2 cuts under max_len 2 048 (a window of 2 045 positions, 32 rounds of the lanes)."""
    rng = np.random.default_rng(200000)
    cp, probas, _ = numeric_document(rng, 200000, np.float32)
    probas[100000:106000] /= 4.0
    want = check_call(torch_cuda, cp, probas, None, np.asarray([0, 200000]), 4, 2048, sides=("device",))
    assert want[0].sum() > 20000 and want[0][100100:105900].sum() >= 2 and want[2].tolist() == [0]
    assert max(lengths_of(want[0])) <= 2048


@pytest.fixture(scope="module")
def many_documents():
    rng = np.random.default_rng(11)
    counts = rng.integers(0, 3001, size=2000)
    counts[[0, 1, 2, 500, 501, 502, 503, 1998, 1999]] = 0  # empty documents at both ends and in a row
    counts[[3, 700, 701, 1997]] = [1, 4, 7, 8]
    docs = []
    for d, c in enumerate(counts):
        cp, p, known = numeric_document(rng, int(c), np.float32, known_rate=0.02 if d % 3 == 0 else 0.0)
        if d % 5 == 0:
            p[len(p) // 3:2 * len(p) // 3] /= 4  # a stretch for phase 2
        docs.append((cp, p, known))
    cp, probas, known, off = pack(docs)
    return cp, probas, known, off, host_batch(cp, probas, known, off, 4, 100)


@pytest.mark.parametrize("side", ["host", "device"])
def test_two_thousand_documents_in_one_call(torch_cuda, many_documents, side):
    cp, probas, known, off, want = many_documents
    assert want[0].sum() > 100000 and not want[2].any()
    check_call(torch_cuda, cp, probas, known, off, 4, 100, want=want, sides=(side,))
    if side == "device":  # same bits run to run
        check_call(torch_cuda, cp, probas, known, off, 4, 100, want=want, sides=(side,))


def test_split_sentences_batch_returns_the_reference_sentences(torch_cuda):
    """The golden file's predictions and Markdown boundaries in, the reference's sentences out, for every stored (min_len, max_len),
    float32 and float64 documents in calls of their own, with a document too short to be split in the batch."""
    cases = golden_cases()
    for dtype in (np.float32, np.float64):
        group = [c for c in cases if c[1].dtype == dtype]
        assert len(group) >= 4
        for min_len, max_len in CASES:
            got = raglite_amd.split_sentences_batch([c[0] for c in group] + ["a"], min_len, max_len,
                                                    predicted_probas=[c[1] for c in group] + [np.zeros(1)],
                                                    boundary_probas=[c[2] for c in group] + [None])
            assert got[-1] == ["a"]
            for (doc, _, _, starts), sentences in zip(group, got):
                edges = [0, *starts[(min_len, max_len)], len(doc)]
                assert sentences == [doc[i:j] for i, j in zip(edges[:-1], edges[1:])]
    with pytest.raises(ValueError, match="no valid split.*document 1"):
        raglite_amd.split_sentences_batch(["abcdefgh", "abcdefghijk"], 4, 5, predicted_probas=lambda doc: np.zeros(len(doc)),
                                          boundary_probas=lambda doc: np.full(len(doc), np.nan))
    with pytest.raises(ValueError, match="Non-finite.*document 0"):
        raglite_amd.split_sentences_batch(["abcdefgh"], predicted_probas=[np.full(8, np.nan)], boundary_probas=[np.full(8, np.nan)])
    with pytest.raises(ValueError, match="7 probabilities"):
        raglite_amd.split_sentences_batch(["abcdefgh"], predicted_probas=[np.zeros(7)], boundary_probas=[np.full(8, np.nan)])


@pytest.fixture
def markdown_parse(monkeypatch):
    """The real Markdown parse where markdown-it is installed; else a stand-in on both sides of the comparison."""
    try:
        import markdown_it  # noqa: F401
    except ImportError:
        monkeypatch.setattr(_sentences, "markdown_sentence_boundaries", lambda doc: np.full(len(doc), np.nan))
        monkeypatch.setattr(_chunklets, "markdown_chunklet_boundaries",
                            lambda sentences: np.asarray([1.0 if s.startswith("#") else 0.0 for s in sentences]))


def test_split_sentences_on_the_device_equals_the_host_default(torch_cuda, markdown_parse):
    for doc, predictions, known, _ in golden_cases()[:6]:
        for min_len, max_len in ((4, None), (4, 64), (12, 40)):
            host = raglite_amd.split_sentences(doc, min_len, max_len, predicted_probas=predictions)
            assert len(host) > 3 and "".join(host) == doc
            assert raglite_amd.split_sentences(doc, min_len, max_len, predicted_probas=predictions, partition="device") == host
            assert raglite_amd.split_sentences(doc, min_len, max_len, known, predicted_probas=lambda d: predictions, partition="device") == \
                raglite_amd.split_sentences(doc, min_len, max_len, known, predicted_probas=predictions)
    assert raglite_amd.split_sentences("abcd", predicted_probas=None, partition="device") == ["abcd"]


def test_split_texts_batch_chains_its_two_steps(torch_cuda, markdown_parse):
    """Per text what `split_documents_batch` returns when fed the sentences of `split_sentences_batch` under
    `max_len=config.chunk_max_size`."""
    config = raglite_amd.HotPathConfig(embedder="llama-cpp-python/fake/sentences", chunk_max_size=400)
    cases = golden_cases()[1:5]
    predictions = {c[0]: c[1].astype(np.float64) for c in cases}
    texts = [c[0] for c in cases]
    raglite_amd.set_embedder_factory(lambda cfg: FakeLlama(dim=64))
    try:
        got = raglite_amd.split_texts_batch(texts, predicted_probas=predictions.__getitem__, config=config)
        sentences = raglite_amd.split_sentences_batch(texts, max_len=400, predicted_probas=predictions.__getitem__)
        want = raglite_amd.split_documents_batch(sentences, config=config)
    finally:
        raglite_amd.set_embedder_factory(None)
    assert len(got) == len(texts) and all(max(len(s) for s in doc) <= 400 for doc in sentences)
    for (chunks, mats), (want_chunks, want_mats) in zip(got, want):
        assert chunks == want_chunks and len(chunks) >= 1 and len(mats) == len(want_mats)
        assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(mats, want_mats))
