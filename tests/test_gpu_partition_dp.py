"""`rl_partition_chunks` / `rl_split_chunks` / `split_chunks_batch` on the device against the host statement of the recurrence
(`raglite_amd._chunking.partition_dp`, itself held against enumeration and the MILP in tests/test_partition_dp_host.py).
`cut` is compared as bytes, `objective` as uint64 bits, `status` as integers."""

import numpy as np
import pytest

import raglite_amd
from raglite_amd import _ops
from raglite_amd._chunking import _apply_headings, _heading_flags, _nonoutlying, partition_dp
from tests.test_oracle_golden import _split_cases
from tests.test_partition_dp_host import SQRT_EPS, random_document, tie_documents

pytestmark = pytest.mark.gpu


def host_batch(cost, sizes, off, max_size):
    """The reference of one call: `partition_dp` per document, in the layout of the C entry."""
    n, n_docs = int(off[-1]), len(off) - 1
    cut = np.zeros(n, np.uint8)
    obj = np.zeros(n_docs, np.float64)
    status = np.zeros(n_docs, np.int32)
    for d in range(n_docs):
        b, e = int(off[d]), int(off[d + 1])
        cuts, obj[d], status[d] = partition_dp(cost[b:e], sizes[b:e], max_size)
        cut[[b + c - 1 for c in cuts]] = 1
    return cut, obj, status


def pack(docs):
    """[(cost[n_d - 1], sizes[n_d])] -> cost[n] (a poison value at every document's ignored last entry), sizes[n], off."""
    off = np.concatenate(([0], np.cumsum([len(s) for _, s in docs]))).astype(np.int64)
    cost = np.full(int(off[-1]), np.float32(-7.0))
    sizes = np.zeros(int(off[-1]), np.int64)
    for d, (c, s) in enumerate(docs):
        b, e = int(off[d]), int(off[d + 1])
        sizes[b:e] = s
        cost[b:max(e - 1, b)] = c[: max(e - b - 1, 0)]
    return cost, sizes, off


def check_call(torch, cost, sizes, off, max_size, want=None, sides=("host", "device")):
    want = want or host_batch(cost, sizes, off, max_size)
    for side in sides:
        if side == "host":
            cut, obj, status = raglite_amd.partition_chunks(cost, sizes, off, max_size)
        else:
            t = raglite_amd.partition_chunks(torch.as_tensor(cost, device="cuda"), torch.as_tensor(sizes, device="cuda"),
                                             torch.as_tensor(off, device="cuda"), max_size)
            assert all(x.is_cuda for x in t)
            cut, obj, status = (x.cpu().numpy() for x in t)
        assert cut.dtype == np.uint8 and obj.dtype == np.float64 and status.dtype == np.int32
        assert np.array_equal(status, want[2]), side
        assert cut.tobytes() == want[0].tobytes(), (side, np.flatnonzero(cut != want[0])[:8])
        assert np.array_equal(obj.view(np.uint64), want[1].view(np.uint64)), (side, np.flatnonzero(obj != want[1])[:8])
    return want


def test_one_document_of_two_chunklets(torch_cuda):
    for sizes, max_size, cuts in (([5, 6], 10, [1]), ([5, 5], 10, [0])):
        cost, sz, off = pack([(np.asarray([0.5], np.float32), np.asarray(sizes))])
        want = check_call(torch_cuda, cost, sz, off, max_size)
        assert want[0].tolist() == cuts + [0] and want[1][0] == (0.5 if cuts[0] else 0.0)


@pytest.fixture(scope="module")
def many_documents():
    rng = np.random.default_rng(11)
    counts = rng.integers(0, 301, size=3000)
    counts[[0, 1, 2, 500, 501, 502, 503, 2998, 2999]] = 0  # empty documents at both ends and in a row
    counts[[3, 700, 701, 2997]] = 1
    counts[[4, 702]] = 2
    docs = [random_document(rng, int(c)) for c in counts]
    cost, sizes, off = pack(docs)
    return cost, sizes, off, host_batch(cost, sizes, off, 100)


@pytest.mark.parametrize("side", ["host", "device"])
def test_three_thousand_documents_in_one_call(torch_cuda, many_documents, side):
    """One wave per document (750 blocks of four): empty documents at both ends and in a row, single-chunklet documents."""
    cost, sizes, off, want = many_documents
    assert want[0].sum() > 10000 and np.all(want[2] == 0)
    check_call(torch_cuda, cost, sizes, off, 100, want=want, sides=(side,))


def test_more_documents_than_waves_in_the_grid(torch_cuda):
    """The launch caps its grid at 4 096 blocks of four waves: past 16 384 documents a wave takes document `doc + 16 384` next, in
    the prefix kernel and in the DP kernel.  20 000 documents of 0 to 4 chunklets, so the second round holds cut and uncut, empty
    and failed documents."""
    rng = np.random.default_rng(16384)
    counts = rng.integers(0, 5, size=20000)
    counts[[0, 16383, 16384, 16385, 19999]] = [0, 4, 0, 4, 4]
    docs = [random_document(rng, int(c)) for c in counts]
    docs[16385][1][:] = 59       # must be cut three times
    docs[17000] = (np.ones(2, np.float32), np.asarray([3, 101, 3]))  # status 1 in the second round
    cost, sizes, off = pack(docs)
    want = check_call(torch_cuda, cost, sizes, off, 100, sides=("device",))
    late = slice(int(off[16384]), None)
    assert want[0][late].sum() > 500 and want[2][17000] == 1 and want[0][off[16385]:off[16386]].tolist() == [1, 1, 1, 0]


@pytest.mark.parametrize("max_size", [1, 2, 63, 64, 65, 66, 2047, 2048])
def test_predecessor_ranges_around_the_wave_width(torch_cuda, max_size):
    """Size-1 chunklets: step j scans g[j - max_size .. j - 1], a range of max_size entries -- below, at and above one 64-lane
    round, and 32 rounds."""
    rng = np.random.default_rng(max_size)
    n = 3 * max_size + 131
    docs = [(np.maximum(rng.random(n - 1, dtype=np.float32), SQRT_EPS), np.ones(n, np.int64)),
            (np.maximum(rng.random(max_size, dtype=np.float32), SQRT_EPS), np.ones(max_size + 1, np.int64))]
    want = check_call(torch_cuda, *pack(docs), max_size)
    assert want[0].sum() >= 3


def test_one_document_of_twenty_thousand_chunklets(torch_cuda):
    cost, sizes = random_document(np.random.default_rng(20), 20000)
    c, s, off = pack([(cost, sizes)])
    want = check_call(torch_cuda, c, s, off, 2048, sides=("device",))
    assert want[0].sum() > 250


def test_failed_documents_leave_their_neighbours_alone(torch_cuda):
    rng = np.random.default_rng(7)
    docs = [random_document(rng, 50) for _ in range(7)]
    healthy = host_batch(*pack(docs), 100)
    docs[2][1][17] = 101                     # a chunklet over max_size: status 1
    docs[4][0][30] = np.nan                  # a non-finite cost: status 2
    docs[5][0][0] = np.inf
    docs[5][1][49] = 500                     # both: the size wins
    cost, sizes, off = pack(docs)
    want = check_call(torch_cuda, cost, sizes, off, 100)
    assert want[2].tolist() == [0, 0, 1, 0, 2, 1, 0] and np.isnan(want[1][[2, 4, 5]]).all()
    for d in (0, 1, 3, 6):
        assert want[1][d] == healthy[1][d] and np.array_equal(want[0][off[d]:off[d + 1]], healthy[0][off[d]:off[d + 1]])
    for d in (2, 4, 5):
        assert not want[0][off[d]:off[d + 1]].any()


def test_planted_ties(torch_cuda):
    by_max = {}
    for cost, sizes, max_size in tie_documents():
        by_max.setdefault(max_size, []).append((cost, sizes))
    for max_size, docs in by_max.items():
        check_call(torch_cuda, *pack(docs), max_size)


def make_texts(rng, n):
    """n chunklets of 5 .. 120 characters, some of them Markdown headings (runs, first and last included)."""
    out = []
    for i in range(n):
        body = "".join(rng.choice(list("abcdefgh ")) for _ in range(int(rng.integers(5, 121))))
        out.append(("# " + body + "\n") if rng.random() < 0.25 else body + ". ")
    return out


def make_corpus(seed, dim, n_docs=24):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 60, size=n_docs)
    counts[0] = 40
    counts[[1, 5]] = 0
    counts[2] = 1
    counts[3] = 2
    docs = [make_texts(rng, int(c)) for c in counts]
    docs[0][0] = "# first\n"
    docs[0][-1] = "## last\n"
    embs = [rng.standard_normal((len(d), dim)).astype(np.float32) for d in docs]
    return docs, embs


@pytest.mark.parametrize("dim", [32, 1024])
def test_split_chunks_call_equals_its_three_steps(torch_cuda, dim):
    """`rl_split_chunks` == partition_similarities -> _apply_headings -> partition_dp, the costs bit for bit."""
    docs, embs = make_corpus(dim, dim)
    off = np.concatenate(([0], np.cumsum([len(d) for d in docs]))).astype(np.int64)
    X = np.concatenate(embs)
    sizes = np.asarray([len(c) for d in docs for c in d], np.int64)
    sel = np.concatenate([_nonoutlying(sizes[off[d]:off[d + 1]]) for d in range(len(docs)) if len(docs[d])])
    head = np.concatenate([_heading_flags(d) for d in docs])
    sim = raglite_amd.partition_similarities(X, off, sizes)
    want_cost = sim.copy()
    for d, chunklets in enumerate(docs):
        b, e = int(off[d]), int(off[d + 1])
        if e - b >= 2:
            want_cost[b:e - 1] = _apply_headings(sim[b:e - 1].copy(), chunklets)
    assert (want_cost == 1.0).sum() > 20 and not np.array_equal(want_cost, sim)
    want = host_batch(want_cost, sizes, off, 300)
    assert want[0].sum() > 40
    for side in ("host", "device"):
        x = X if side == "host" else torch_cuda.as_tensor(X, device="cuda")
        cut, cost, obj, status = _ops.split_chunks_call(x, off, sel, head, sizes, 300, want_cost=True)
        if side == "device":
            assert cut.is_cuda and cost.is_cuda
            cut, cost, obj, status = (t.cpu().numpy() for t in (cut, cost, obj, status))
        assert cost.tobytes() == want_cost.tobytes(), side
        assert np.array_equal(status, want[2]) and cut.tobytes() == want[0].tobytes()
        assert np.array_equal(obj.view(np.uint64), want[1].view(np.uint64))


def test_split_chunks_batch_equals_a_loop_over_documents(torch_cuda):
    torch = torch_cuda
    docs, embs = make_corpus(3, 64)
    loop = [raglite_amd.split_chunks(d, e, max_size=300, partition="device") for d, e in zip(docs, embs)]
    assert sum(len(c) for c, _ in loop) > len(docs) + 20
    for variant in ("numpy list", "numpy concatenated", "cuda list", "cuda concatenated"):
        conv = (lambda a: torch.as_tensor(a, device="cuda")) if "cuda" in variant else (lambda a: a)
        arg = [conv(e) for e in embs] if "list" in variant else conv(np.concatenate(embs))
        got = raglite_amd.split_chunks_batch(docs, arg, max_size=300)
        assert len(got) == len(docs)
        for d, ((chunks, parts), (want_chunks, want_parts)) in enumerate(zip(got, loop)):
            assert chunks == want_chunks and len(parts) == len(want_parts), (variant, d)
            assert all(len(c) <= 300 for c in chunks) and "".join(chunks) == "".join(docs[d])
            for part, want_part in zip(parts, want_parts):
                if "cuda" in variant:
                    assert part.is_cuda
                    part = part.cpu().numpy()
                assert np.array_equal(part, want_part), (variant, d)
    assert got[1][0] == [] and got[2][0] == ["".join(docs[2])]  # no chunklets; one chunklet
    # views, not copies: a chunk's embeddings alias the caller's tensor
    t = torch.as_tensor(np.concatenate(embs), device="cuda")
    parts = raglite_amd.split_chunks_batch(docs, t, max_size=300)[0][1]
    assert parts[0].data_ptr() == t.data_ptr()
    with pytest.raises(ValueError, match="partition"):
        raglite_amd.split_chunks(docs[0], embs[0], partition="simplex")


def test_split_chunks_batch_reproduces_the_reference_chunks(torch_cuda):
    cases = _split_cases()
    for dim in sorted({c[1].shape[1] for c in cases}):
        for max_size in sorted({c[2] for c in cases if c[1].shape[1] == dim}):
            group = [c for c in cases if c[1].shape[1] == dim and c[2] == max_size]
            got = raglite_amd.split_chunks_batch([c[0] for c in group], [c[1] for c in group], max_size=max_size)
            for (chunks, parts), c in zip(got, group):
                assert chunks == c[5] and [len(p) for p in parts] == c[4].tolist()
                assert np.array_equal(np.vstack(parts), c[1])
    for c in cases:
        chunks, parts = raglite_amd.split_chunks(c[0], c[1], max_size=c[2], partition="device")
        assert chunks == c[5] and [len(p) for p in parts] == c[4].tolist()


def test_the_two_value_errors(torch_cuda):
    good = (["x" * 9, "y" * 9, "z" * 9], np.ones((3, 8), np.float32) + np.eye(3, 8, dtype=np.float32))
    big = (["x" * 50, "y"], np.ones((2, 8), np.float32))
    zero = (["x" * 9, "y" * 9], np.zeros((2, 8), np.float32))
    one_zero = (["x" * 9], np.zeros((1, 8), np.float32))
    with pytest.raises(ValueError, match=r"Chunklet larger than chunk max_size detected\. \(document 1\)"):
        raglite_amd.split_chunks_batch([good[0], big[0], zero[0]], [good[1], big[1], zero[1]], max_size=10)
    with pytest.raises(ValueError, match=r"Chunklet embeddings with zero norm detected\. \(document 2\)"):
        raglite_amd.split_chunks_batch([good[0], good[0], zero[0]], [good[1], good[1], zero[1]], max_size=10)
    with pytest.raises(ValueError, match=r"zero norm detected\. \(document 0\)"):
        raglite_amd.split_chunks_batch([one_zero[0], good[0]], [one_zero[1], good[1]], max_size=10)
    with pytest.raises(ValueError, match=r"max_size detected\.$"):
        raglite_amd.split_chunks(big[0], big[1], max_size=10, partition="device")
    with pytest.raises(ValueError, match=r"zero norm detected\.$"):
        raglite_amd.split_chunks(zero[0], torch_cuda.as_tensor(zero[1], device="cuda"), max_size=10, partition="device")
    assert raglite_amd.split_chunks([], np.zeros((0, 8), np.float16), partition="device")[0] == []
    assert len(raglite_amd.split_chunks_batch([good[0]], [good[1]], max_size=10)[0][0]) == 3
