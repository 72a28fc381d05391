"""`rl_partition_chunklets` / `split_chunklets_batch` / `split_documents_batch` on the device against the host statement of the
recurrence (`raglite_amd._chunklets.chunklet_dp`, itself held against the reference's stored cuts, its literal loop and enumeration in
tests/test_chunklets_host.py).  `cut` is compared as bytes, `objective` as uint64 bits, `status` as integers, for host and for device
pointers.  Numeric inputs only: neither markdown-it nor the reference is needed (where a test goes through the Markdown parse and
markdown-it is missing, a stand-in replaces the parse on both sides of the comparison)."""

import math

import numpy as np
import pytest

import raglite_amd
from raglite_amd import _chunklets
from oracle.fake_embedder import FakeLlama
from tests.chunklets_ref import MAX_SIZES, golden_cases, host_batch, numeric_document, pack

pytestmark = pytest.mark.gpu


def check_call(torch, boundary, statements, lengths, off, max_size, want=None, sides=("host", "device")):
    want = want or host_batch(boundary, statements, lengths, off, max_size)
    for side in sides:
        if side == "host":
            cut, obj, status = raglite_amd.partition_chunklets(boundary, statements, lengths, off, max_size)
        else:
            t = raglite_amd.partition_chunklets(*(torch.as_tensor(a, device="cuda") for a in (boundary, statements, lengths, off)), max_size)
            assert all(x.is_cuda for x in t)
            cut, obj, status = (x.cpu().numpy() for x in t)
        assert cut.dtype == np.uint8 and obj.dtype == np.float64 and status.dtype == np.int32
        assert np.array_equal(status, want[2]), (side, np.flatnonzero(status != want[2])[:8])
        assert cut.tobytes() == want[0].tobytes(), (side, np.flatnonzero(cut != want[0])[:8])
        assert np.array_equal(obj.view(np.uint64), want[1].view(np.uint64)), (side, np.flatnonzero(obj.view(np.uint64) != want[1].view(np.uint64))[:8])
    return want


def doc(lengths, boundary=None, statements=None):
    n = len(lengths)
    return (np.zeros(n) if boundary is None else np.asarray(boundary, np.float64),
            np.ones(n) if statements is None else np.asarray(statements, np.float64), np.asarray(lengths, np.int64))


def test_documents_of_zero_one_and_two_sentences(torch_cuda):
    """Empty documents first, last and in a row; one sentence; a pair that fits max_size (one chunklet of two: 1 + 1 / (2 sqrt 2),
    against 3 + 3 for two of one) and a pair that does not (the window forces the cut)."""
    docs = [doc([]), doc([]), doc([7]), doc([5, 5]), doc([]), doc([]), doc([5, 6]), doc([3], [1.0], [3.0]), doc([])]
    want = check_call(torch_cuda, *pack(docs), 10)
    assert want[0].tolist() == [0, 0, 0, 1, 0, 0] and want[2].tolist() == [0] * 9
    assert want[1].tolist() == [0.0, 0.0, 3.0, 1.0 + 1.0 / math.sqrt(2.0) / 2.0, 0.0, 0.0, 6.0, 0.0, 0.0]
    only_empty = check_call(torch_cuda, *pack([doc([]), doc([])]), 10)  # n == 0: the call writes nothing, the wrapper fills in
    assert only_empty[1].tolist() == [0.0, 0.0]


def test_window_wider_than_a_wave(torch_cuda):
    """Sentences of 1 to 4 characters under max_size 512: windows of 128 to 512 positions, two to eight 64-lane rounds per step.  Runs
    of identical sentences (and two documents of nothing else) make exact ties that span lanes and rounds; the smallest j must win."""
    rng = np.random.default_rng(512)
    b, s, ln = numeric_document(rng, 1500, max_len=4)
    for begin in (100, 700, 1200):
        b[begin:begin + 200], s[begin:begin + 200], ln[begin:begin + 200] = 0.0, 1.0, 2
    same1, same4 = numeric_document(rng, 700, max_len=1, same=True), (np.zeros(900), np.full(900, 0.5), np.full(900, 4, np.int64))
    flat = (np.zeros(600), np.zeros(600), np.ones(600, np.int64))  # s = 0 everywhere: max(s, 1e-6), and every cost of a step equal
    want = check_call(torch_cuda, *pack([(b, s, ln), same1, same4, flat]), 512)
    assert want[0].sum() > 400 and not want[2].any()


def test_over_long_sentences_next_to_clean_documents(torch_cuda):
    """Status 1 and the propagation of +inf: an over-long sentence in the middle, at position 0 and at the end; the clean documents
    around them keep their results."""
    rng = np.random.default_rng(1)
    docs = [numeric_document(rng, 90) for _ in range(7)]
    healthy = host_batch(*pack(docs), 300)
    docs[1][2][40] = 301
    docs[3][2][0] = 5000
    docs[5][2][89] = 301
    docs[5][2][88] = 302
    b, s, ln, off = pack(docs)
    want = check_call(torch_cuda, b, s, ln, off, 300)
    assert want[2].tolist() == [0, 1, 0, 1, 0, 1, 0]
    assert np.isinf(want[1][[1, 3, 5]]).all() and want[0][off[1]:off[2]].sum() >= 1
    for d in (0, 2, 4, 6):
        assert want[1][d] == healthy[1][d] and np.array_equal(want[0][off[d]:off[d + 1]], healthy[0][off[d]:off[d + 1]])
    tiny = check_call(torch_cuda, *pack([doc([10, 100, 10, 10]), doc([10, 10, 10, 100]), doc([100, 10, 10, 10]), doc([100])]), 50)
    assert tiny[0].tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0]


def test_non_finite_input_next_to_clean_documents(torch_cuda):
    rng = np.random.default_rng(2)
    docs = [numeric_document(rng, 70) for _ in range(6)]
    healthy = host_batch(*pack(docs), 300)
    docs[1][0][33] = np.nan
    docs[2][1][0] = np.inf
    docs[4][1][69] = -np.inf
    docs[4][2][5] = 999  # over-long too: status 2 wins
    b, s, ln, off = pack(docs)
    want = check_call(torch_cuda, b, s, ln, off, 300)
    assert want[2].tolist() == [0, 2, 2, 0, 2, 0] and np.isnan(want[1][[1, 2, 4]]).all()
    for d in (1, 2, 4):
        assert not want[0][off[d]:off[d + 1]].any()
    for d in (0, 3, 5):
        assert want[1][d] == healthy[1][d] and np.array_equal(want[0][off[d]:off[d + 1]], healthy[0][off[d]:off[d + 1]])


def test_more_documents_than_waves_in_the_grid(torch_cuda):
    """The launch caps its grid at 4 096 blocks of four waves: past 16 384 documents a wave takes document `doc + 16 384` next, in
    the prefix kernel and in the recurrence.  20 000 documents of 0 to 4 sentences, so the second round holds cut and uncut, empty,
    over-long and non-finite documents."""
    rng = np.random.default_rng(16384)
    counts = rng.integers(0, 5, size=20000)
    counts[[0, 16383, 16384, 16385, 17000, 17001, 19999]] = [0, 4, 0, 4, 3, 2, 4]
    docs = [numeric_document(rng, int(c), max_len=60) for c in counts]
    docs[16385][2][:] = 59                       # must be cut three times
    docs[17000][2][1] = 101                      # status 1 in the second round
    docs[17001][0][1] = np.nan                   # status 2 in the second round
    b, s, ln, off = pack(docs)
    want = check_call(torch_cuda, b, s, ln, off, 100, sides=("device",))
    late = slice(int(off[16384]), None)
    assert want[0][late].sum() > 500 and want[2][17000] == 1 and want[2][17001] == 2
    assert want[0][off[16385]:off[16386]].tolist() == [1, 1, 1, 0]


def test_one_document_of_five_thousand_sentences(torch_cuda):
    """No limit on a document's length: 79 blocks of 64 in the prefix phase, one wave for the whole recurrence."""
    want = check_call(torch_cuda, *pack([numeric_document(np.random.default_rng(5000), 5000)]), 2048)
    assert want[0].sum() > 500


@pytest.fixture(scope="module")
def many_documents():
    rng = np.random.default_rng(11)
    counts = rng.integers(0, 301, size=3000)
    counts[[0, 1, 2, 500, 501, 502, 503, 2998, 2999]] = 0  # empty documents at both ends and in a row
    counts[[3, 700, 701, 2997]] = 1
    counts[[4, 702]] = 2
    docs = [numeric_document(rng, int(c), same=(d % 97 == 5)) for d, c in enumerate(counts)]
    b, s, ln, off = pack(docs)
    return b, s, ln, off, host_batch(b, s, ln, off, 512)


@pytest.mark.parametrize("side", ["host", "device"])
def test_three_thousand_documents_in_one_call(torch_cuda, many_documents, side):
    b, s, ln, off, want = many_documents
    assert want[0].sum() > 50000 and not want[2].any()
    check_call(torch_cuda, b, s, ln, off, 512, want=want, sides=(side,))
    if side == "device":  # same bits run to run
        again = raglite_amd.partition_chunklets(*(torch_cuda.as_tensor(a, device="cuda") for a in (b, s, ln, off)), 512)
        assert again[0].cpu().numpy().tobytes() == want[0].tobytes()
        assert np.array_equal(again[1].cpu().numpy().view(np.uint64), want[1].view(np.uint64))


def test_split_chunklets_batch_returns_the_reference_chunklets(torch_cuda):
    """`boundary_probas=` from the golden file replaces the Markdown parse; the strings are the reference's, for every stored
    max_size, with an empty document in the batch (`[""]`, the reference's "".join([]))."""
    cases = golden_cases()
    for max_size in MAX_SIZES:
        got = raglite_amd.split_chunklets_batch([c[0] for c in cases] + [[]], max_size,
                                                boundary_probas=[c[1] for c in cases] + [np.zeros(0)])
        assert got[-1] == [""]
        for (sentences, _, _, _, cuts), chunklets in zip(cases, got):
            bounds = [0, *cuts[max_size], len(sentences)]
            assert chunklets == ["".join(sentences[i:j]) for i, j in zip(bounds[:-1], bounds[1:])]
    with pytest.raises(ValueError, match="document 1"):
        raglite_amd.split_chunklets_batch([["a. "], ["b. ", "c. "]], 10, boundary_probas=[np.zeros(1), np.asarray([0.0, np.nan])])
    with pytest.raises(ValueError, match="do not match"):
        raglite_amd.split_chunklets_batch([["a. "], ["b. ", "c. "]], 10, boundary_probas=[np.zeros(1), np.zeros(3)])


@pytest.fixture
def markdown_parse(monkeypatch):
    """The real Markdown parse where markdown-it is installed; else a stand-in on both sides of the comparison."""
    try:
        import markdown_it  # noqa: F401
    except ImportError:
        monkeypatch.setattr(_chunklets, "markdown_chunklet_boundaries",
                            lambda sentences: np.asarray([1.0 if s.startswith("#") else 0.25 if s.startswith("- ") else 0.0 for s in sentences]))


def test_split_chunklets_on_the_device_equals_the_host_default(torch_cuda, markdown_parse):
    for sentences, _, _, _, _ in golden_cases():
        for max_size in (300, 2048):
            assert raglite_amd.split_chunklets(sentences, max_size=max_size, partition="device") == raglite_amd.split_chunklets(sentences, max_size=max_size)
    assert raglite_amd.split_chunklets([], partition="device") == raglite_amd.split_chunklets([]) == [""]


def test_split_documents_batch_chains_the_three_steps(torch_cuda, markdown_parse):
    """Per document what `split_chunks_batch` returns when fed the host-split chunklets of the same sentences and their embeddings."""
    config = raglite_amd.HotPathConfig(embedder="llama-cpp-python/fake/chunklets", chunk_max_size=400)
    documents = [c[0] for c in golden_cases()[2:6]]
    raglite_amd.set_embedder_factory(lambda cfg: FakeLlama(dim=64))
    try:
        got = raglite_amd.split_documents_batch(documents, config=config)
        chunklets = [raglite_amd.split_chunklets(s, max_size=400) for s in documents]
        embeddings = [raglite_amd.embed_strings(c, config=config) for c in chunklets]
        want = raglite_amd.split_chunks_batch(chunklets, embeddings, max_size=400)
    finally:
        raglite_amd.set_embedder_factory(None)
    assert len(got) == len(documents) and sum(len(g[0]) for g in got) > len(documents)
    for (chunks, mats), (want_chunks, want_mats) in zip(got, want):
        assert chunks == want_chunks and len(mats) == len(want_mats)
        assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(mats, want_mats))
