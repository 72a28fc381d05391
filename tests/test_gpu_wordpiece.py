"""The device WordPiece tokenizer on the GPU (raglite_amd/csrc/wordpiece.hip), through the C ABI: `rl_wordpiece_encode`
must leave, for every text that carries no flagged code point, ids equal with `==` to the `tokenizers` library's own, and for ALL texts
the bytes of the host statement (`WordPieceTables.encode_tables`: ids, offsets, status, the five counts); `rl_wordpiece_pairs` the arrays
of `pairs_host`; and `TorchCrossEncoderRanker(forward="native")` with the device tokenizer the same doc ids, order and score BITS as with
the same tokenizer wrapped as `encode(str) -> list[int]`.

The tiles named below are the kernels': WP_THREADS = 256 items per block of the element-wise kernels, WP_MATCH_THREADS = 64 words per
block of the match kernel, KB_SCAN_TILE = 2048 items per block of the scans between them."""

import ctypes as C

import numpy as np
import pytest
import torch

from raglite_amd import _abi
from raglite_amd._cross_encoder import CrossEncoderShape, TorchCrossEncoderRanker
from raglite_amd._torch_embedder import pack_runs
from raglite_amd._wordpiece import DeviceWordPiece, pairs_arrays, pairs_host, text_codepoints
from tests import wordpiece_ref as ref

pytestmark = pytest.mark.gpu

WP_THREADS, WP_MATCH_THREADS, KB_SCAN_TILE = 256, 64, 2048


@pytest.fixture(scope="module")
def toks(torch_cuda):
    made = {}

    def get(lowercase=True, hash_bits=0):
        if (lowercase, hash_bits) not in made:
            made[lowercase, hash_bits] = DeviceWordPiece(ref.tables(lowercase), hash_bits=hash_bits)
        return made[lowercase, hash_bits]

    yield get
    for t in made.values():
        t.close()


def encode_c(tok, texts, mem=_abi.MEM_HOST):
    """(ids, offsets, status, counts) of `rl_wordpiece_encode` + `rl_wordpiece_result`, with host or device pointers."""
    lib = _abi.lib()
    cp, off = text_codepoints(texts)
    counts = (C.c_int64 * 5)()
    h = tok._handle  # noqa: SLF001
    if mem == _abi.MEM_HOST:
        _abi.check(lib.rl_wordpiece_encode(h, cp.ctypes.data if len(cp) else None, off.ctypes.data, len(cp), len(texts), counts, mem, None))
        ids, offsets, status = np.full(counts[0], -1, np.int32), np.full(len(texts) + 1, -1, np.int64), np.full(len(texts), 9, np.uint8)
        _abi.check(lib.rl_wordpiece_result(h, ids.ctypes.data if len(ids) else None, offsets.ctypes.data, status.ctypes.data if len(status) else None, mem, None))
        return ids, offsets, status, tuple(counts)
    d_cp, d_off = torch.from_numpy(cp.view(np.int32).copy()).cuda(), torch.from_numpy(off).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    _abi.check(lib.rl_wordpiece_encode(h, d_cp.data_ptr() if len(cp) else None, d_off.data_ptr(), len(cp), len(texts), counts, mem, stream))
    ids = torch.full((counts[0],), -1, dtype=torch.int32, device="cuda")
    offsets = torch.full((len(texts) + 1,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((len(texts),), 9, dtype=torch.uint8, device="cuda")
    _abi.check(lib.rl_wordpiece_result(h, ids.data_ptr() if counts[0] else None, offsets.data_ptr(), status.data_ptr() if len(texts) else None, mem, stream))
    p_ids, p_off, p_st = C.c_void_p(), C.c_void_p(), C.c_void_p()
    _abi.check(lib.rl_wordpiece_device(h, C.byref(p_ids), C.byref(p_off), C.byref(p_st)))
    assert p_ids.value and p_off.value and p_st.value
    return ids.cpu().numpy(), offsets.cpu().numpy(), status.cpu().numpy(), tuple(counts)


def check(tok, texts, lowercase=True, mem=_abi.MEM_HOST, want=None):
    """The call against the host statement (every byte and count; `want`: computed before) and, text by text, against the yardstick
    where no code point is flagged."""
    ids, offsets, status, counts = encode_c(tok, texts, mem)
    want = want or ref.tables(lowercase).encode_tables(texts)
    print(f"texts {len(texts)} counts (tokens, words, unk, flagged, symbols) {counts} want {want['counts']}")
    assert counts == want["counts"]
    assert np.array_equal(offsets, want["offsets"]) and np.array_equal(status, want["status"])
    assert np.array_equal(ids, want["ids"])
    for i, (text, w) in enumerate(zip(texts, ref.yardstick(texts, lowercase))):
        if not status[i]:
            assert ids[offsets[i]: offsets[i + 1]].tolist() == w, repr(text)
    return ids, offsets, status, counts


def test_one_text(toks):
    ids, offsets, _, counts = check(toks(), ["Hello, World: the quick brown fox!"])
    assert offsets.tolist() == [0, len(ids)] and counts[0] == len(ids) > 8


def test_empty_texts_first_in_the_middle_and_last(toks):
    texts = ["", "", "ab cd", "", ref.WHITE_SPACE_ONLY, "", "ef.", "", ""]
    _, offsets, _, _ = check(toks(), texts)
    lens = np.diff(offsets)
    assert all(lens[i] == 0 for i in (0, 1, 3, 4, 5, 7, 8)) and lens[2] > 0 and lens[6] > 0
    check(toks(), [""])
    check(toks(), [])
    check(toks(), ["", ""], mem=_abi.MEM_DEVICE)


def test_two_texts_without_white_space_between_them_do_not_join(toks):
    head, cont = ref.HEAD_ONLY, ref.CONT_ONLY
    v = ref.vocabulary()
    ids, offsets, _, _ = check(toks(), [head, cont, head + cont])
    assert ids[offsets[2]:].tolist() == [v[head], v["##" + cont]], "one word: the continuation piece matches"
    assert ids[: offsets[1]].tolist() == [v[head]] and v["##" + cont] not in ids[offsets[1]: offsets[2]].tolist(), "two texts: two words"


@pytest.mark.parametrize("lowercase", [True, False], ids=["lowercase", "cased"])
def test_edge_texts_and_word_lengths(toks, lowercase):
    words = ["a" * n for n in (1, 63, 64, 65, 100, 101)] + ["q" * 100, "q" * 101, "É" * 100, "É" * 101]
    texts = [*ref.EDGE_TEXTS, ref.FLAGGED_TEXT, *words, " ".join(words)]
    ids, offsets, status, counts = check(toks(lowercase), texts, lowercase)
    assert status[len(ref.EDGE_TEXTS)] == 1 and counts[3] >= 1, "the flagged text is found"
    base = len(ref.EDGE_TEXTS) + 1
    unk = ref.tables(lowercase).unk_id
    assert [int(offsets[base + i + 1] - offsets[base + i]) for i in range(6)] == [1, 63, 64, 65, 100, 1]
    assert ids[offsets[base + 5]] == unk and ids[offsets[base + 6]] == ref.vocabulary()["q" * 100] and ids[offsets[base + 7]] == unk


def _letters(n):
    """A text of exactly n normalised symbols: words of 1 .. 9 letters."""
    rng = np.random.default_rng(n)
    out = []
    while sum(map(len, out)) + len(out) < n - 9:
        out.append("".join(rng.choice(list(ref.LETTERS), size=int(rng.integers(1, 10)))))
    rest = n - sum(map(len, out)) - len(out)
    out.append("x" * rest)
    text = " ".join(out)
    assert len(text) == n
    return text


@pytest.mark.parametrize("tile", [WP_THREADS, KB_SCAN_TILE], ids=["WP_THREADS", "KB_SCAN_TILE"])
def test_an_expansion_that_ends_at_a_tile_edge(toks, tile):
    for d in (-1, 0, 1):
        # alone; behind a text that ends exactly on the edge (the next text's first word starts a block); and with the expansion, not
        # the input, on the edge: every CJK character is three symbols
        check(toks(), [_letters(tile + d)])
        check(toks(), [_letters(tile), _letters(tile + d), "ab"])
        cjk = "中" * ((tile + d) // 3) + "a" * ((tile + d) % 3)
        _, _, _, counts = check(toks(), [cjk])
        assert counts[4] == tile + d


def test_word_counts_around_the_match_tile(toks):
    for n_words in (WP_MATCH_THREADS - 1, WP_MATCH_THREADS, WP_MATCH_THREADS + 1, 2 * WP_MATCH_THREADS):
        _, _, _, counts = check(toks(), [" ".join(["ab"] * n_words)])
        assert counts[1] == n_words
        _, _, _, counts = check(toks(), ["."] * n_words)  # one punctuation word per text
        assert counts[1] == n_words


@pytest.fixture(scope="module")
def many():
    """About 19 000 words and 150 000 symbols, and their host statement (computed once).  The kernels have no grid-stride loop -- every
    item has its own lane -- so the second round is the second BLOCK of each (hundreds here), and the second level of the scans, which
    starts behind KB_SCAN_TILE items."""
    texts = ref.random_texts(77, 1000, 30)
    return texts, ref.tables(True).encode_tables(texts)


def test_many_words_host_against_device_pointers_and_two_runs(toks, many):
    texts, want = many
    a = check(toks(), texts, want=want)
    assert a[3][1] > 4 * KB_SCAN_TILE and a[3][4] > 40 * KB_SCAN_TILE and a[3][2] > 0
    b = encode_c(toks(), texts, _abi.MEM_HOST)
    c = encode_c(toks(), texts, _abi.MEM_DEVICE)
    for x, y, z in zip(a[:3], b[:3], c[:3]):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    assert a[3] == b[3] == c[3]


def test_every_lookup_collides_with_four_hash_bits(toks, many):
    texts = many[0][:8] + ref.EDGE_TEXTS[:5] + ref.EDGE_TEXTS[11:]  # (every miss walks the whole cluster: few words)
    a = check(toks(True, 4), texts)
    b = encode_c(toks(), texts)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    assert toks(True, 4).info()["slots"] == toks().info()["slots"] >= 2 * toks().info()["pieces"]


def test_cased_tables(toks, many):
    texts = many[0][:200] + ["Hello World HELLO", "É é", "ΟΔΟΣ οδοσ"]
    check(toks(False), texts, lowercase=False, mem=_abi.MEM_DEVICE)


def test_the_python_object_splices_flagged_texts(toks, many):
    tok = toks()
    many = many[0]
    texts = [many[1], ref.FLAGGED_TEXT, "", many[2], ref.FLAGGED_TEXT + " tail", many[3]]
    ids, offsets, counts = tok.encode_batch(texts)
    assert ids.is_cuda and ids.dtype == torch.int32 and offsets.dtype == torch.int64 and counts["flagged"] == 2
    off = offsets.cpu().tolist()
    got = [ids[off[i]: off[i + 1]].cpu().tolist() for i in range(len(texts))]
    assert got == ref.yardstick(texts) and counts["tokens"] == off[-1]
    assert tok.encode(texts[3]) == got[3] and tok.encode("") == []


# ---- pair assembly ------------------------------------------------------------------------------------------------------------------
def _pair_case(n_pairs, seed):
    """Token lists whose pairs meet every branch of the truncation at max_length 24: no cut, query longer, doc longer, a tie, empty texts."""
    rng = np.random.default_rng(seed)
    lens = [0, 1, 5, 10, 11, 21, 22, 40, 3, 10]
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    ids = rng.integers(103, 30000, size=int(off[-1])).astype(np.int32)
    if n_pairs == 1:
        q, d = np.asarray([7], np.int32), np.asarray([5], np.int32)
    else:
        q, d = rng.integers(0, len(lens), size=n_pairs).astype(np.int32), rng.integers(0, len(lens), size=n_pairs).astype(np.int32)
        q[:6], d[:6] = [2, 7, 2, 3, 5, 0], [3, 2, 7, 9, 6, 0]  # no cut, query longer, doc longer, a tie (10, 10), both over, both empty
    return ids, off, q, d


@pytest.mark.parametrize("n_pairs", [1, 1300])
@pytest.mark.parametrize("max_length", [24, 3, 512])
def test_pairs_equal_the_host_statement(torch_cuda, n_pairs, max_length):
    ids, off, q, d = _pair_case(n_pairs, n_pairs)
    want = pairs_host(ids, off, q, d, max_length, 101, 102, 2)
    got = pairs_arrays(ids, off, q, d, max_length, 101, 102, 2)
    for name, g, w in zip(("ids", "positions", "type_ids", "seq_offsets"), got, want):
        assert g.dtype == np.int32 and np.array_equal(g, w), name
    assert int(np.diff(want[3]).max()) <= max(max_length, 3) and (n_pairs == 1 or len(want[0]) > KB_SCAN_TILE or max_length == 3)
    # device pointers: the same bytes, and nothing written behind the totals
    lib = _abi.lib()
    t = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    d_ids, d_off, d_q, d_d = t(ids), t(off), t(q), t(d)
    n = len(want[0])
    out = torch.full((3, n + 8), -7, dtype=torch.int32, device="cuda")
    seq = torch.full((n_pairs + 9,), -7, dtype=torch.int32, device="cuda")
    total = C.c_int64()
    stream = torch.cuda.current_stream().cuda_stream
    args = (d_ids.data_ptr(), d_off.data_ptr(), len(off) - 1, d_q.data_ptr(), d_d.data_ptr(), n_pairs, max_length, 101, 102, 2)
    _abi.check(lib.rl_wordpiece_pairs(*args, None, None, None, seq.data_ptr(), C.byref(total), _abi.MEM_DEVICE, stream))
    assert total.value == n and np.array_equal(seq[: n_pairs + 1].cpu().numpy(), want[3])
    _abi.check(lib.rl_wordpiece_pairs(*args, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), seq.data_ptr(), C.byref(total), _abi.MEM_DEVICE, stream))
    torch.cuda.synchronize()
    for r in range(3):
        assert np.array_equal(out[r, :n].cpu().numpy(), want[r]) and bool((out[r, n:] == -7).all())
    assert bool((seq[n_pairs + 1:] == -7).all())


# ---- end to end: text -> logits with no id list in between --------------------------------------------------------------------------
class Wrapped:
    """The same tokenizer as `encode(str) -> list[int]`: the host route of the ranker."""

    def __init__(self, lowercase=True):
        self.lowercase = lowercase

    def encode(self, text):
        return ref.yardstick([text], self.lowercase)[0]


def _same_results(got, want):
    assert got.query == want.query and len(got.results) == len(want.results)
    for g, w in zip(got.results, want.results):
        assert (g.doc_id, g.rank, g.text) == (w.doc_id, w.rank, w.text)
        assert np.float32(g.score).tobytes() == np.float32(w.score).tobytes()


def test_rank_batch_with_the_device_tokenizer_equals_the_wrapped_host_one(toks):
    shape = CrossEncoderShape(vocab_size=len(ref.vocabulary()) + 8, hidden=64, layers=2, heads=2, ffn=128, max_positions=512, n_ctx=512,
                              bos_id=ref.vocabulary()["[CLS]"], eos_id=ref.vocabulary()["[SEP]"])
    kw = dict(device="cuda", dtype=torch.bfloat16, forward="native", seed=3, max_length=96)
    dev = TorchCrossEncoderRanker(shape, tokenizer=toks(), **kw)
    host = TorchCrossEncoderRanker(shape, tokenizer=Wrapped(), **kw)
    try:
        rng = np.random.default_rng(9)
        queries = [ref.random_text(rng, int(rng.integers(1, 8))) for _ in range(5)]
        docs = [[ref.random_text(rng, int(rng.integers(1, 40))) for _ in range(n)] for n in (4, 0, 9, 1, 6)]  # ragged candidate lists
        docs[2][3] = ref.random_text(rng, 150)  # longer than max_length: the device truncates it
        docs[2][5] = docs[2][0]  # a duplicate: equal scores keep input order; and a string tokenized once
        docs[4][2] = ref.FLAGGED_TEXT  # answered by the mirrored tokenizer, spliced in
        docs[0][1] = ""
        ids = [None, None, [100 + 3 * i for i in range(9)], None, None]
        assert dev._device_pairs_apply() and not host._device_pairs_apply()  # noqa: SLF001
        got = dev.rank_batch(queries, docs, ids)
        want = host.rank_batch(queries, docs, ids)
        for g, w in zip(got, want):
            _same_results(g, w)
        lens = [len(p[0]) for q, d in zip(queries, docs) for p in host.encode_pairs(q, d)]
        assert max(lens) == 96 and dev.native.pack_forwards == host.native.pack_forwards == len(pack_runs(lens, 8192)) == 1
        # rank and logits of one query go the same way; the score bits are the batch's
        _same_results(dev.rank(queries[2], docs[2], ids[2]), want[2])
        z_dev, z_host = dev.logits(queries[0], docs[0]), host.logits(queries[0], docs[0])
        assert torch.equal(z_dev.view(torch.int32), z_host.view(torch.int32))
        # more than one pack: the slices and the rebased offsets
        dev.pack_tokens = host.pack_tokens = 300
        n0 = dev.native.pack_forwards
        for g, w in zip(dev.rank_batch(queries, docs, ids), want):
            _same_results(g, w)
        assert dev.native.pack_forwards - n0 == len(pack_runs(lens, 300)) > 3
    finally:
        for r in (dev, host):
            if r.native is not None:
                r.native.close()
