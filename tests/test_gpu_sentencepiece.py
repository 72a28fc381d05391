"""The device SentencePiece Unigram tokenizer on the GPU (raglite_amd/csrc/sentencepiece.hip), through the C ABI:
`rl_sentencepiece_encode` must leave, for ALL texts, the bytes of the host statement (`UnigramTables.encode_tables`: ids, offsets, status,
the normalised symbols, the five counts), for every recorded case the library's recorded ids, and where the library imports its own
ids for every text that carries no flagged code point; `rl_sentencepiece_rows` the arrays of `rows_host`; and a `TorchTokenEmbedder`
with the device tokenizer the same bits as with `SentencePieceTokenizer` on the same model.

The tiles named below are the kernels': SP_THREADS = 256 items per block of the element-wise kernels, KB_SCAN_TILE = 2048 items per
block of the scans between them, one text per 64-lane wave in the search."""

import ctypes as C

import numpy as np
import pytest
import torch

import raglite_amd
from raglite_amd import _abi
from raglite_amd._sentencepiece import DeviceSentencePiece, rows_arrays, rows_host, text_codepoints
from raglite_amd._torch_embedder import EncoderShape, SentencePieceTokenizer, TorchTokenEmbedder
from tests import sentencepiece_ref as ref

pytestmark = pytest.mark.gpu

SP_THREADS, KB_SCAN_TILE, WAVE = 256, 2048, 64


@pytest.fixture(scope="module")
def toks(torch_cuda):
    made = {}

    def get(hash_bits=0):
        if hash_bits not in made:
            made[hash_bits] = DeviceSentencePiece(ref.tables(), hash_bits=hash_bits)
        return made[hash_bits]

    yield get
    for t in made.values():
        t.close()


def encode_c(tok, texts, mem=_abi.MEM_HOST, raw=True):
    """(ids, offsets, status, symbols, sym_off, counts) of `rl_sentencepiece_encode` + `_result` + `_device`, with host or device pointers."""
    lib = _abi.lib()
    cp, off = text_codepoints(texts)
    counts = (C.c_int64 * 5)()
    h = tok._handle  # noqa: SLF001
    n_texts = len(texts)
    if mem == _abi.MEM_HOST:
        _abi.check(lib.rl_sentencepiece_encode(h, cp.ctypes.data if len(cp) else None, off.ctypes.data, len(cp), n_texts, int(raw), counts, mem, None))
        ids, offsets, status = np.full(counts[0], -1, np.int32), np.full(n_texts + 1, -1, np.int64), np.full(n_texts, 9, np.uint8)
        _abi.check(lib.rl_sentencepiece_result(h, ids.ctypes.data if len(ids) else None, offsets.ctypes.data, status.ctypes.data if n_texts else None, mem, None))
    else:
        d_cp, d_off = torch.from_numpy(cp.view(np.int32).copy()).cuda(), torch.from_numpy(off).cuda()
        stream = torch.cuda.current_stream().cuda_stream
        _abi.check(lib.rl_sentencepiece_encode(h, d_cp.data_ptr() if len(cp) else None, d_off.data_ptr(), len(cp), n_texts, int(raw), counts, mem, stream))
        t_ids = torch.full((counts[0],), -1, dtype=torch.int32, device="cuda")
        t_off = torch.full((n_texts + 1,), -1, dtype=torch.int64, device="cuda")
        t_st = torch.full((n_texts,), 9, dtype=torch.uint8, device="cuda")
        _abi.check(lib.rl_sentencepiece_result(h, t_ids.data_ptr() if counts[0] else None, t_off.data_ptr(), t_st.data_ptr() if n_texts else None, mem, stream))
        ids, offsets, status = t_ids.cpu().numpy(), t_off.cpu().numpy(), t_st.cpu().numpy()
    p = [C.c_void_p() for _ in range(5)]
    _abi.check(lib.rl_sentencepiece_device(h, *(C.byref(x) for x in p)))
    assert all(x.value for x in p)
    symbols, sym_off = np.full(counts[1], 0xFFFFFFFF, np.uint32), np.full(n_texts + 1, -1, np.int64)
    if counts[1]:
        _abi.check(lib.rl_memcpy_d2h(symbols.ctypes.data, p[3], symbols.nbytes, None))
    _abi.check(lib.rl_memcpy_d2h(sym_off.ctypes.data, p[4], sym_off.nbytes, None))
    return ids, offsets, status, symbols, sym_off, tuple(counts)


def check(tok, texts, mem=_abi.MEM_HOST, want=None, recorded=None, raw=True):
    """The call against the host statement (every byte and count; `want`: computed before), against the recorded ids where there are
    some, and text by text against the library where it imports and no code point is flagged."""
    got = encode_c(tok, texts, mem, raw)
    ids, offsets, status, symbols, sym_off, counts = got
    want = want or ref.tables().encode_tables(texts, xlmr=not raw)
    print(f"texts {len(texts)} counts (tokens, symbols, unk, flagged, longest) {counts} want {want['counts']}")
    assert counts == want["counts"]
    assert np.array_equal(sym_off, want["sym_off"]) and np.array_equal(symbols, want["symbols"])
    assert np.array_equal(offsets, want["offsets"]) and np.array_equal(status, want["status"])
    assert np.array_equal(ids, want["ids"])
    sp = ref.library()
    layout = (lambda x: x) if raw else (lambda x: ref.tables().layout(x, True))
    for i, text in enumerate(texts):
        mine = ids[offsets[i]: offsets[i + 1]].tolist()
        if recorded is not None and not status[i]:
            assert mine == layout(recorded[i]), repr(text[:80])
        if sp is not None and not status[i]:
            assert mine == layout(sp.encode(text)), repr(text[:80])
    return got


def recorded(names):
    c = ref.cases()
    return [c["texts"][c["names"].index(n)] for n in names], [c["ids"][c["names"].index(n)] for n in names]


def test_one_text(toks):
    texts, ids = recorded(["ascii"])
    got = check(toks(), texts, recorded=ids)
    assert got[1].tolist() == [0, len(got[0])] and got[5][0] == len(got[0]) > 8


def test_empty_texts_first_in_the_middle_and_last(toks):
    texts = ["", "", "ab cd", "", ref.case("space_only"), "", "ef.", "", ""]
    _, offsets, *_ = check(toks(), texts)
    lens = np.diff(offsets)
    assert all(lens[i] == 0 for i in (0, 1, 3, 4, 5, 7, 8)) and lens[2] > 0 and lens[6] > 0
    check(toks(), [""])
    check(toks(), [])
    check(toks(), ["", ""], mem=_abi.MEM_DEVICE)


def test_two_texts_without_a_space_between_them_do_not_join(toks):
    ids, offsets, _, symbols, sym_off, _ = check(toks(), ["kern", "el", "kernel"])
    assert symbols[sym_off[1]] == 0x2581 and symbols[sym_off[2]] == 0x2581, "every text has its own dummy prefix"
    assert ids[: offsets[2]].tolist() != ids[offsets[2]:].tolist()


def test_every_recorded_case(toks):
    c = ref.cases()
    names = [n for n in c["names"] if n != "words_3000"]
    texts, ids = recorded(names)
    _, offsets, status, _, sym_off, counts = check(toks(), texts, recorded=ids)
    assert not status.any() and counts[2] > 0, "no recorded case is flagged, and some hold unknown runs"
    by = dict(zip(names, np.diff(sym_off).tolist()))
    L = c["longest_piece"]  # noqa: N806
    assert [by[f"symbols_{n}"] for n in (L - 1, L, L + 1, 63, 64, 65)] == [L - 1, L, L + 1, 63, 64, 65]
    assert by["one_letter"] == 2, "the shortest text that is not empty: the dummy prefix and one symbol"
    assert by["run_L"] == L and by["run_L_plus_1"] == L + 1 and by["run_long"] == 3 * L + 6
    assert by["empty"] == by["space_only"] == by["empty_images_only"] == 0
    toks_of = dict(zip(names, np.diff(offsets).tolist()))
    assert toks_of["oov_only"] == 2, "the dummy prefix and ONE unknown for the whole run"


def test_expansions_that_end_at_a_block_and_a_scan_tile(toks):
    for n in (SP_THREADS, KB_SCAN_TILE):
        names = [f"expanded_{n + d}" for d in (-1, 0, 1)]
        texts, ids = recorded(names)
        for text, want in zip(texts, ids):  # each alone: the stream ends where the block or the tile does
            check(toks(), [text], recorded=[want])
        check(toks(), texts, recorded=ids, mem=_abi.MEM_DEVICE)


def test_the_3000_word_text_where_the_carry_matters(toks):
    texts, ids = recorded(["words_3000"])
    got = check(toks(), texts, recorded=ids)
    assert got[5][0] == len(ids[0]) > 10_000 and got[5][4] == got[5][1] > 20_000


@pytest.fixture(scope="module")
def batch():
    texts = list(ref.batch_texts())
    return texts, ref.tables().encode_tables(texts, xlmr=False)


def test_many_texts_twice_and_from_host_and_device_pointers(toks, batch):
    texts, want = batch
    assert len(texts) == 300 and want["counts"][1] > 2 * KB_SCAN_TILE, "many blocks, two scan levels"
    first = check(toks(), texts, want=want)
    second = check(toks(), texts, want=want)
    device = check(toks(), texts, want=want, mem=_abi.MEM_DEVICE)
    for a, b, c in zip(first[:5], second[:5], device[:5]):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    assert first[5] == second[5] == device[5] and first[5][2] > 0
    ids, off = first[0], first[1]
    assert first[5][0] == ref.cases()["batch_tokens"], "the recorded token count"
    assert ref.digest([ids[off[i]: off[i + 1]].tolist() for i in range(len(texts))]) == ref.cases()["batch_sha256"], "the recorded ids, as their digest"


def test_forced_collisions_change_nothing(toks, batch):
    texts, _ = batch
    assert toks(4).info()["pieces"] == toks().info()["pieces"] > 1900 and toks().info()["longest_piece"] == ref.cases()["longest_piece"]
    short = sorted((t for t in texts if t), key=len)[:12]  # (every probe walks the whole table: keep the walk short)
    check(toks(4), short)
    e_texts, e_ids = recorded(["oov_across_space", "run_long", "fdfa_in_text", "symbols_64"])
    check(toks(4), e_texts, recorded=e_ids)


def test_xlmr_layout_and_counts(toks):
    texts, ids = recorded(["ascii", "oov_middle", "oov_across_space", "empty", "cjk"])
    texts = [*texts, *ref.FLAGGED_TEXTS]
    raw = check(toks(), texts, raw=True)
    xl = check(toks(), texts, raw=False)
    t = ref.tables()
    assert xl[0].tolist() == [i + 1 if i != t.unk_id else 3 for i in raw[0].tolist()] and 3 in xl[0].tolist()
    assert raw[2].tolist() == [0, 0, 0, 0, 0, 1, 1, 1] and raw[5][3] == 3, "the three flagged texts are found"
    assert raw[5][2] == int((raw[0] == t.unk_id).sum()) > 0
    tok_ids, off, counts = toks().encode_batch(texts)  # the Python route: flagged texts answered by the mirrored processor
    assert counts["flagged"] == 3
    off = off.cpu().tolist()
    want = SentencePieceTokenizer(model_proto=t.model_proto)
    assert [tok_ids[off[i]: off[i + 1]].cpu().tolist() for i in range(len(texts))] == [want.encode(x) for x in texts]
    assert toks().encode(texts[1]) == want.encode(texts[1]) and toks().vocab_size == want.vocab_size
    assert toks().decode(want.encode(texts[0])) == want.decode(want.encode(texts[0]))


@pytest.mark.parametrize("n_texts", [1, 1300])
def test_rows(toks, batch, n_texts):
    texts = (batch[0][1:] * 5)[:n_texts]  # (the first text of the batch is empty)
    ids, offsets, *_ = encode_c(toks(), texts, raw=False)
    lens = np.diff(offsets)
    longest = int(lens.max())
    for max_len in (longest + 2, longest + 1, 2):  # nothing cut, the longest text cut, everything cut to bos eos
        want = rows_host(ids, offsets, max_len, 0, 2, 2)
        got = rows_arrays(ids, offsets, max_len, 0, 2, 2)
        for g, w in zip(got, want):
            assert g.dtype == np.int32 and np.array_equal(g, w)
        if max_len == 2:
            assert got[0].tolist() == [0, 2] * n_texts
        if max_len == longest + 1:
            assert int((np.diff(got[2]) - 2 < lens).sum()) == int((lens == longest).sum()) >= 1
    shape = EncoderShape(vocab_size=2100, hidden=64, layers=1, heads=2, ffn=128, max_positions=40, n_ctx=32)
    d_ids, d_pos, d_seq, seq_host = toks().rows_device(texts, shape)
    want = rows_host(ids, offsets, shape.n_ctx, shape.bos_id, shape.eos_id, shape.position_offset)
    assert np.array_equal(d_ids.cpu().numpy(), want[0]) and np.array_equal(d_pos.cpu().numpy(), want[1])
    assert np.array_equal(d_seq.cpu().numpy(), want[2]) and np.array_equal(seq_host, want[2])


# ---- the embedder: the same bits through the device tokenizer as through SentencePieceTokenizer -------------------------------------------
SHAPE = EncoderShape(vocab_size=2100, hidden=64, layers=2, heads=2, ffn=128, max_positions=200, n_ctx=160)
RAGGED = ["kernel", "the wave writes one row per query and the tile holds the slab", "", "scan fuse rank 中 span", "a  b   c " * 60]


@pytest.fixture(scope="module")
def embedders(toks):
    host = SentencePieceTokenizer(model_proto=ref.tables().model_proto)
    return {(kind, mode): TorchTokenEmbedder(SHAPE, device="cuda", seed=3, tokenizer=toks() if kind == "device" else host, **kw)
            for kind in ("device", "host") for mode, kw in (("native", {"short_forward": "native"}), ("packed", {"batching": "packed"}), ("padded", {}))}


def test_embed_pack_and_embed_have_the_host_routes_bits(embedders):
    dev, host = embedders["device", "native"], embedders["host", "native"]
    got, want = dev.embed_pack(RAGGED), host.embed_pack(RAGGED)
    assert got is not None and len(got) == len(want) == 5
    for g, w in zip(got, want):
        assert g.shape == w.shape and torch.equal(g, w)
    assert got[2].shape[0] == 2 and got[4].shape[0] == SHAPE.n_ctx, "an empty text is <s> </s>; the long one is cut to n_ctx"
    for mode in ("native", "packed", "padded"):
        for texts in (RAGGED[1], RAGGED[:4]):
            g, w = embedders["device", mode].embed(texts), embedders["host", mode].embed(texts)
            g, w = ([g], [w]) if isinstance(texts, str) else (g, w)
            assert all(torch.equal(a, b) for a, b in zip(g, w)), mode


def test_hybrid_search_batch_of_strings_has_the_host_routes_ids_and_score_bits(embedders):
    rng = np.random.default_rng(5)
    words = "kernel wave tile slab chunk bias norm token query vector index store scan fuse rank span batch block lane stream".split()
    mats = [rng.standard_normal((int(rng.integers(1, 4)), 64)).astype(np.float32) for _ in range(40)]
    mats = [m / np.linalg.norm(m, axis=1, keepdims=True) for m in mats]
    docs = [" ".join(rng.choice(words, size=10).tolist()) + f" text {i}" for i in range(40)]
    gi = raglite_amd.GpuIndex([f"chunk-{i}" for i in range(40)], mats, docs=docs, keyword_texts=docs)
    queries = [" ".join(rng.choice(words, size=int(rng.integers(2, 6))).tolist()) for _ in range(6)]
    cfg = raglite_amd.HotPathConfig(vector_search_query_adapter=False)
    try:
        out = {}
        for kind in ("device", "host"):
            raglite_amd.set_embedder_factory(lambda config, k=kind: embedders[k, "native"])
            out[kind] = raglite_amd.hybrid_search_batch(queries, num_results=5, config=cfg, index=gi)
        assert out["device"] == out["host"] and all(len(ids) == 5 for ids, _ in out["device"])
        for (_, a), (_, b) in zip(out["device"], out["host"]):
            assert np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()
    finally:
        raglite_amd.set_embedder_factory(None)
        gi.close()
