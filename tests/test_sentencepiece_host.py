"""The device SentencePiece Unigram tokenizer on the host (no GPU): the walk of the normaliser's precompiled character
map, what `UnigramTables.from_model` refuses, the `.npz` round trip, the plain-Python statements of the kernels' algorithm
(`normalize_host`, `encode_host`) held with `==` to the `sentencepiece` library's own answers, every argument check of the C entries
(all return before the first HIP call) and the tables' header under the host compiler's sanitizers."""

import ctypes as C
import shutil
import subprocess
import unicodedata
from pathlib import Path

import numpy as np
import pytest

from raglite_amd import _abi
from raglite_amd._sentencepiece import BYTE, CONTROL, MARK, NORMAL, USER_DEFINED, UnigramTables, charsmap_summary, rows_host
from raglite_amd._torch_embedder import SentencePieceTokenizer

from tests import sentencepiece_ref as ref

ROOT = Path(__file__).resolve().parent.parent
INVALID, UNSUPPORTED = _abi.RL_ERR_INVALID, _abi.RL_ERR_UNSUPPORTED


def _proto():
    from sentencepiece import sentencepiece_model_pb2 as pb

    m = pb.ModelProto()
    m.ParseFromString(ref.MODEL.read_bytes())
    return m


# ---- the character map and the tables -------------------------------------------------------------------------------------------------
def test_the_charsmap_walk_reproduces_the_counts():
    s = charsmap_summary(_proto().normalizer_spec.precompiled_charsmap)
    assert (s["units"], s["keys"], s["single"], s["multi"], s["longest_key"], s["longest_value"]) == (44_800, 225_275, 5_008, 220_267, 4, 18)
    assert len(s["trailing"]) == 185 and sum(1 for c in s["trailing"] if unicodedata.combining(chr(c)) == 0) == 143
    assert s["images"][0xFDFA] == unicodedata.normalize("NFKC", "ﷺ") and len(s["images"][0xFDFA]) == 18
    assert {0x1161, 0x11A8, 0x3099, 0xFF9E, 0x0301} <= s["trailing"], "Hangul medial and final jamo, kana voicing marks, a combining accent"
    assert any(0x0900 <= c < 0x0E00 and unicodedata.category(chr(c)) == "Mc" for c in s["trailing"]), "an Indic vowel sign"


def test_the_tables_are_what_the_model_holds():
    t, m = ref.tables(), _proto()
    assert t.image_off.dtype == np.int32 and t.image_len.dtype == np.uint8 and len(t.image_off) == len(t.image_len) == 0x110000
    assert int((t.image_off >= 0).sum()) == 5_008 and int((t.image_len & t.FLAG != 0).sum()) == 185
    assert t.expand("ﬁ") == [ord("f"), ord("i")] and t.expand("\x7f") == [] and t.expand("a") == [ord("a")] and t.expand("　") == [0x20]
    normal = [(i, p) for i, p in enumerate(m.pieces) if p.type == NORMAL]
    assert t.piece_ids.tolist() == [i for i, _ in normal] and t.vocab_size == len(m.pieces) == 2000 and t.unk_id == 0
    assert t.piece_scores.dtype == np.float32 and t.piece_scores.tolist() == [np.float32(p.score) for _, p in normal]
    assert t.longest_piece == max(len(p.piece) for _, p in normal) == ref.cases()["longest_piece"]
    assert np.float32(t.unk_score) == np.float32(min(p.score for _, p in normal)) - np.float32(10)
    joined = t.piece_cp.astype("<u4").tobytes().decode("utf-32-le")
    assert [joined[t.piece_off[k]: t.piece_off[k + 1]] for k in range(len(normal))] == [p.piece for _, p in normal]
    assert "<unk>" not in t._piece_dict() and "<s>" not in t._piece_dict()  # noqa: SLF001 - CONTROL and UNKNOWN pieces never match


def test_the_bpe_fixture_is_refused_by_name():
    with pytest.raises(ValueError, match=r"trainer_spec\.model_type is BPE"):
        UnigramTables.from_model(ref.BPE_MODEL)
    with pytest.raises(ValueError, match="exactly one of"):
        UnigramTables.from_model()


def _edited(edit):
    m = _proto()
    edit(m)
    return m.SerializeToString()


def _first_normal(m, start=10):
    return next(i for i in range(start, len(m.pieces)) if m.pieces[i].type == NORMAL and len(m.pieces[i].piece) > 1)


def _set(path, value):
    def edit(m):
        obj = m
        for name in path[:-1]:
            obj = getattr(obj, name)
        setattr(obj, path[-1], value)
    return edit


def _piece(field, value, mark=False):
    def edit(m):
        i = next(k for k, p in enumerate(m.pieces) if p.piece == chr(MARK)) if mark else _first_normal(m)
        setattr(m.pieces[i], field, value)
    return edit


def _move_unk(m):
    m.pieces[0].type, m.pieces[1].type = CONTROL, 2


REFUSALS = [
    (_set(("trainer_spec", "model_type"), 3), r"trainer_spec\.model_type is WORD"),
    (_set(("trainer_spec", "byte_fallback"), True), r"trainer_spec\.byte_fallback"),
    (_set(("trainer_spec", "treat_whitespace_as_suffix"), True), r"trainer_spec\.treat_whitespace_as_suffix"),
    (_piece("type", USER_DEFINED), r"pieces\[\d+\]\.type is USER_DEFINED"),
    (_piece("type", BYTE), r"pieces\[\d+\]\.type is BYTE"),
    (_piece("piece", "ab▁c"), r"pieces\[\d+\]\.piece has U\+2581 after its first code point"),
    (_piece("type", CONTROL, mark=True), "U\\+2581 itself must be a NORMAL piece"),
    (_set(("normalizer_spec", "precompiled_charsmap"), b""), r"normalizer_spec\.precompiled_charsmap is empty"),
    (_set(("normalizer_spec", "add_dummy_prefix"), False), r"normalizer_spec\.add_dummy_prefix must be true"),
    (_set(("normalizer_spec", "remove_extra_whitespaces"), False), r"normalizer_spec\.remove_extra_whitespaces must be true"),
    (_set(("normalizer_spec", "escape_whitespaces"), False), r"normalizer_spec\.escape_whitespaces must be true"),
    (_move_unk, r"trainer_spec\.unk_id is 1, the XLM-R layout needs 0"),
]


@pytest.mark.parametrize("edit,text", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_what_the_builder_refuses(edit, text):
    with pytest.raises(ValueError, match=text):
        UnigramTables.from_model(model_proto=_edited(edit))


def test_unk_elsewhere_is_fine_in_the_raw_layout():
    t = UnigramTables.from_model(model_proto=_edited(_move_unk), xlmr=False)
    assert t.unk_id == 1 and not t.xlmr


def test_npz_round_trip(tmp_path):
    t = ref.tables()
    t.save(tmp_path / "tables.npz")
    back = UnigramTables.load(tmp_path / "tables.npz")
    for name in ("image_off", "image_len", "image_pool", "piece_cp", "piece_off", "piece_ids", "piece_scores"):
        a, b = getattr(t, name), getattr(back, name)
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    assert (back.unk_id, back.vocab_size, back.xlmr, back.model_proto) == (t.unk_id, t.vocab_size, t.xlmr, t.model_proto)
    assert np.float32(back.unk_score) == np.float32(t.unk_score)
    texts = ["a round trip", ref.FLAGGED_TEXTS[0]]
    assert back.encode_host(texts) == t.encode_host(texts) == [SentencePieceTokenizer(model_proto=t.model_proto).encode(x) for x in texts]


# ---- normalize_host and encode_host against the library ---------------------------------------------------------------------------------
def test_every_recorded_case_equals_the_library():
    t, c, sp = ref.tables(), ref.cases(), ref.library()
    want = {"ascii", "runs_of_space", "leading_only", "trailing_only", "nbsp_ideographic_zwsp", "empty_images_last", "ligature_circled", "fdfa",
            "full_width", "cjk", "hangul_precomposed", "run_L", "run_L_plus_1", "oov_start", "oov_middle", "oov_end", "oov_across_space", "empty",
            "space_only", "words_3000"}
    assert want <= set(c["names"])
    for name, text, ids, norm in zip(c["names"], c["texts"], c["ids"], c["normalized"]):
        assert not t.flagged(text), name  # (asserted: the fallback cannot hide a failure)
        assert t.normalize_host(text) == norm == sp.normalize(text), name
        assert t.viterbi(norm) == ids == sp.encode(text), name
    by = dict(zip(c["names"], c["ids"]))
    L = c["longest_piece"]  # noqa: N806
    assert len(t.normalize_host(ref.case("run_L"))) == L and len(t.normalize_host(ref.case("run_L_plus_1"))) == L + 1
    assert by["empty"] == by["space_only"] == by["empty_images_only"] == []
    assert by["oov_only"] == [sp.piece_to_id(chr(MARK)), 0], "a run of unknowns is one"
    assert by["oov_across_space"].count(0) == 2 and by["oov_start"][1] == 0 and by["oov_end"][-1] == 0
    assert t.normalize_host(ref.case("empty_images_last")).endswith("end") and t.normalize_host(ref.case("space_then_empty_images")) == "▁word"
    assert len(by["words_3000"]) > 10_000


def test_the_batch_equals_the_library_in_both_layouts():
    t, c = ref.tables(), ref.cases()
    batch = list(ref.batch_texts())
    got = t.encode_host(batch, xlmr=False)
    assert len(batch) == 300 and not any(t.needs_mirror(x) for x in batch)
    assert sum(map(len, got)) == c["batch_tokens"] and ref.digest(got) == c["batch_sha256"], "the recorded ids, as their digest"
    texts = batch[:60]
    assert got[:60] == ref.library().encode(texts)
    wrapped = SentencePieceTokenizer(model_proto=t.model_proto)
    assert t.encode_host(texts[:20]) == [wrapped.encode(x) for x in texts[:20]]
    r = t.encode_tables([*texts[:20], ref.case("oov_across_space")], xlmr=False)
    assert r["counts"][0] == len(r["ids"]) and r["counts"][2] == int((r["ids"] == 0).sum()) > 0 and r["counts"][4] == int(np.diff(r["sym_off"]).max())


def test_random_sweep_equals_the_library_with_no_text_flagged():
    t, sp = ref.tables(), ref.library()
    texts = ref.random_texts(7, 2000)
    assert not any(t.needs_mirror(x) for x in texts), "no generated text may reach the fallback: it would hide a failure"
    tokens = 0
    for text, ids in zip(texts, sp.encode(texts)):
        norm = t.normalize_host(text)
        assert norm == sp.normalize(text), repr(text)
        assert t.viterbi(norm) == ids, repr(text)
        tokens += len(ids)
    assert tokens > 30_000 and sum(ids.count(0) for ids in sp.encode(texts)) > 1000, "enough tokens, and many unknown runs"


def test_the_flagged_cases_are_found_and_answered_by_the_mirror():
    t, sp = ref.tables(), ref.library()
    assert [unicodedata.normalize("NFC", x) != x for x in ref.FLAGGED_TEXTS[:1]] == [True], "the e-acute is decomposed"
    texts = ["plain text", *ref.FLAGGED_TEXTS, "more plain text", "lone \ud800 surrogate"]
    r = t.encode_tables(texts)
    assert r["status"].tolist() == [0, 1, 1, 1, 0, 0] and r["counts"][3] == 3
    assert [t.needs_mirror(x) for x in texts] == [False, True, True, True, False, True]
    assert t.encode_host(texts[:5], xlmr=False) == sp.encode(texts[:5])
    assert t.encode_host(texts[5:], xlmr=False) == [sp.encode("lone ? surrogate")]
    # the tables alone would have been wrong on at least one of them: that is what the flag is for
    assert any(t.viterbi(t.normalize_host(x)) != sp.encode(x) for x in ref.FLAGGED_TEXTS)


def test_rows_host():
    ids = np.arange(10, 22, dtype=np.int32)
    off = np.asarray([0, 5, 5, 12], dtype=np.int64)
    rows, pos, seq = rows_host(ids, off, 6, 0, 2, 2)
    assert rows.tolist() == [0, 10, 11, 12, 13, 2, 0, 2, 0, 15, 16, 17, 18, 2] and seq.tolist() == [0, 6, 8, 14]
    assert pos.tolist() == [2, 3, 4, 5, 6, 7, 2, 3, 2, 3, 4, 5, 6, 7]


# ---- the C entries' argument checks (none reaches a HIP call) -----------------------------------------------------------------------------
def _create_args(**over):
    a = dict(image_off=np.asarray([-1, 0, 2, -1], dtype=np.int32), image_len=np.asarray([1, 2, 0, 0x81], dtype=np.uint8), n_table=4,
             image_pool=np.asarray([97, 98], dtype=np.uint32), n_pool=2, piece_cp=np.asarray([97, 98, 99], dtype=np.uint32),
             piece_off=np.asarray([0, 1, 3], dtype=np.int64), piece_ids=np.asarray([5, 6], dtype=np.int32),
             piece_scores=np.asarray([-1.0, -2.0], dtype=np.float32), n_pieces=2, unk_id=0, unk_score=-12.0, hash_bits=0)
    a.update(over)
    return a


def _create(h, a):
    ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731
    return _abi.lib().rl_sentencepiece_create(h, ptr(a["image_off"]), ptr(a["image_len"]), a["n_table"], ptr(a["image_pool"]), a["n_pool"], ptr(a["piece_cp"]),
                                              ptr(a["piece_off"]), ptr(a["piece_ids"]), ptr(a["piece_scores"]), a["n_pieces"], a["unk_id"],
                                              C.c_float(a["unk_score"]), a["hash_bits"])


def _bad(field, value, at):
    x = _create_args()[field].copy()
    x[at] = value
    return {field: x}


_LONG = dict(piece_cp=np.full(65, 97, dtype=np.uint32), piece_off=np.asarray([0, 65], dtype=np.int64), piece_ids=np.asarray([5], dtype=np.int32),
             piece_scores=np.asarray([-1.0], dtype=np.float32), n_pieces=1)
CREATE_CASES = [
    ({"image_off": None}, INVALID, "image_off is null"), ({"image_len": None}, INVALID, "image_len is null"), ({"n_table": 0}, INVALID, "n_table"),
    ({"n_table": 0x110001}, INVALID, "n_table must be in [1, 0x110000]"), ({"n_pool": -1}, INVALID, "n_pool"), ({"image_pool": None}, INVALID, "image_pool is null"),
    ({"piece_off": None}, INVALID, "piece_off is null"), ({"piece_cp": None}, INVALID, "piece_cp"), ({"piece_ids": None}, INVALID, "piece_ids"),
    ({"piece_scores": None}, INVALID, "piece_scores"), ({"n_pieces": -1}, INVALID, "n_pieces"), ({"unk_id": -1}, INVALID, "unk_id"),
    ({"unk_score": float("nan")}, INVALID, "unk_score must be finite"), ({"hash_bits": 65}, INVALID, "hash_bits"), ({"hash_bits": -1}, INVALID, "hash_bits"),
    (_bad("piece_off", 1, 0), INVALID, "piece_off must start at 0"), (_bad("piece_off", 0, 2), INVALID, "piece_off must be ascending"),
    (_bad("piece_ids", -2, 1), INVALID, "piece_ids must be >= 0"), (_bad("piece_scores", float("inf"), 1), INVALID, "piece_scores must be finite"),
    (_bad("image_off", 1, 1), INVALID, "malformed image entry"), (_bad("image_pool", 0x110000, 1), INVALID, "malformed image_pool entry"),
    (_LONG, UNSUPPORTED, "at most 64 code points"),
]


@pytest.mark.parametrize("over,status,text", CREATE_CASES, ids=[f"{i}-" + "-".join(c[0]) for i, c in enumerate(CREATE_CASES)])
def test_create_rejects_before_any_hip_call(over, status, text):
    h = C.c_void_p(7)
    assert _create(C.byref(h), _create_args(**over)) == status
    assert _abi.last_error().startswith("rl_sentencepiece_create: ") and text in _abi.last_error()
    assert not h.value, "the handle is cleared"


def test_the_other_entries_reject_before_any_hip_call():
    lib = _abi.lib()
    assert _create(None, _create_args()) == INVALID and _abi.last_error() == "rl_sentencepiece_create: out is null"
    counts = (C.c_int64 * 5)()
    for call, text in [
        (lambda: lib.rl_sentencepiece_encode(None, None, None, 0, 0, 0, counts, 0, None), "rl_sentencepiece_encode: null handle"),
        (lambda: lib.rl_sentencepiece_result(None, None, None, None, 0, None), "rl_sentencepiece_result: null handle"),
        (lambda: lib.rl_sentencepiece_device(None, None, None, None, None, None), "rl_sentencepiece_device: null handle"),
        (lambda: lib.rl_sentencepiece_info(None, None), "rl_sentencepiece_info: null handle"),
    ]:
        assert call() == INVALID and _abi.last_error() == text
    assert lib.rl_sentencepiece_destroy(None) == _abi.RL_OK
    # the checks of rl_sentencepiece_encode behind the handle need one, and making one needs a device: a fake non-null pointer is never
    # dereferenced by the checks in front of the first HIP call
    fake = C.c_void_p(0x1000)
    cp = np.zeros(4, dtype=np.uint32)
    off = lambda *v: np.asarray(v, dtype=np.int64)  # noqa: E731
    enc = lambda cp_, off_, n, n_texts, cnt=counts, mem=0, raw=0: lib.rl_sentencepiece_encode(  # noqa: E731
        fake, None if cp_ is None else cp_.ctypes.data, None if off_ is None else off_.ctypes.data, n, n_texts, raw, cnt, mem, None)
    for call, status, text in [
        (lambda: enc(cp, off(0, 4), -1, 1), INVALID, "negative size"), (lambda: enc(cp, off(0, 4), 4, -1), INVALID, "negative size"),
        (lambda: enc(cp, off(0, 4), 4, 1, mem=7), INVALID, "bad mem"), (lambda: enc(cp, off(0, 4), 4, 1, raw=2), INVALID, "raw_ids must be 0 or 1"),
        (lambda: enc(cp, None, 4, 1), INVALID, "text_off is null"), (lambda: enc(cp, off(0, 4), 4, 1, cnt=None), INVALID, "out_counts is null"),
        (lambda: enc(None, off(0, 4), 4, 1), INVALID, "codepoints is null"), (lambda: enc(cp, off(0), 4, 0), INVALID, "code points without a text"),
        (lambda: enc(cp, off(0, 4), 1 << 25, 1), UNSUPPORTED, "2^25"), (lambda: enc(cp, off(1, 4), 4, 1), INVALID, "text_off must start at 0"),
        (lambda: enc(cp, off(0, 3, 2, 4), 4, 3), INVALID, "text_off must be ascending"), (lambda: enc(cp, off(0, 2, 3), 4, 2), INVALID, "text_off must end at n"),
    ]:
        assert call() == status and _abi.last_error().startswith("rl_sentencepiece_encode: ") and text in _abi.last_error(), text


def test_rows_rejects_before_any_hip_call():
    lib = _abi.lib()
    ids = np.arange(6, dtype=np.int32)
    off = np.asarray([0, 2, 6], dtype=np.int64)
    out = np.zeros((2, 16), dtype=np.int32)
    seq = np.zeros(3, dtype=np.int32)
    total = C.c_int64()
    base = dict(ids=ids, tok_off=off, n_texts=2, max_len=16, out_ids=out[0], out_positions=out[1], out_seq_offsets=seq, out_total=C.byref(total), mem=0)

    def call(**over):
        a = {**base, **over}
        ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        return lib.rl_sentencepiece_rows(ptr(a["ids"]), ptr(a["tok_off"]), a["n_texts"], a["max_len"], 0, 2, 2, ptr(a["out_ids"]), ptr(a["out_positions"]),
                                         ptr(a["out_seq_offsets"]), a["out_total"], a["mem"], None)

    bad_off = lambda *v: np.asarray(v, dtype=np.int64)  # noqa: E731
    for over, status, text in [
        ({"mem": 5}, INVALID, "bad mem"), ({"n_texts": -1}, INVALID, "negative size"), ({"n_texts": 1 << 30}, UNSUPPORTED, "fewer than 2^31 tokens"),
        ({"max_len": 1}, INVALID, "max_len must be >= 2"), ({"tok_off": None}, INVALID, "tok_off is null"),
        ({"out_seq_offsets": None}, INVALID, "out_seq_offsets is null"), ({"out_total": None}, INVALID, "out_total is null"),
        ({"out_positions": None}, INVALID, "give out_ids and out_positions"), ({"out_ids": None}, INVALID, "give out_ids and out_positions"),
        ({"ids": None}, INVALID, "ids is null"), ({"tok_off": bad_off(1, 2, 6)}, INVALID, "tok_off must start at 0"),
        ({"tok_off": bad_off(0, 7, 6)}, INVALID, "tok_off must be ascending"),
    ]:
        assert call(**over) == status, text
        assert _abi.last_error().startswith("rl_sentencepiece_rows: ") and text in _abi.last_error(), text


# ---- the tables' header under the host compiler's sanitizers ------------------------------------------------------------------------------
_DRIVER = r"""
#include <cstdio>
#include <string>
#include <vector>
#include "sentencepiece_table.h"
using namespace rl;

// the white-space rule stated the long way: images in, leading and trailing spaces dropped, runs collapsed, one mark in front
static std::vector<uint32_t> slow(const std::vector<uint32_t>& raw) {
    std::vector<uint32_t> out;
    size_t b = 0, e = raw.size();
    while (b < e && raw[b] == SP_SPACE) ++b;
    while (e > b && raw[e - 1] == SP_SPACE) --e;
    if (b == e) return out;
    out.push_back(SP_MARK);
    for (size_t p = b; p < e; ++p) {
        if (raw[p] == SP_SPACE) {
            if (raw[p - 1] != SP_SPACE) out.push_back(SP_MARK);
        } else out.push_back(raw[p]);
    }
    return out;
}

int main() {
    int failures = 0;
    // 1. images: own image, a replacement, an empty one, the flag, a code point beyond the table, an image that leaves the pool
    const int32_t off[] = {-1, 0, 2, -1, 1};
    const uint8_t len[] = {1, 2, 0, (uint8_t)(1 | SP_FLAG), 5};
    const uint32_t pool[] = {'x', 'y', 'z'};
    const SpImage im{off, len, pool, 5, 3};
    int32_t first; bool flagged;
    failures += sp_image_len(im, 0, &first, &flagged) != 1 || first != -1 || flagged;
    failures += sp_image_len(im, 1, &first, &flagged) != 2 || first != 0 || flagged;
    failures += sp_image_len(im, 2, &first, &flagged) != 0 || flagged;
    failures += sp_image_len(im, 3, &first, &flagged) != 1 || first != -1 || !flagged;
    failures += sp_image_len(im, 4, &first, &flagged) != 0;
    failures += sp_image_len(im, 0x10FFFF, &first, &flagged) != 1 || first != -1 || flagged;
    // 2. the white-space rule against the long statement, over every stream of up to 9 symbols of {space, a, mark}
    const uint32_t alphabet[] = {SP_SPACE, 'a', SP_MARK};
    for (int n = 0; n <= 9; ++n) {
        int total = 1;
        for (int j = 0; j < n; ++j) total *= 3;
        for (int code = 0; code < total; ++code) {
            std::vector<uint32_t> raw;
            for (int j = 0, c = code; j < n; ++j, c /= 3) raw.push_back(alphabet[c % 3]);
            std::vector<uint32_t> got;
            for (int p = 0; p < n; ++p) {
                const bool next = p + 1 < n;
                const int k = sp_keep_count(raw[p] == SP_SPACE, p == 0, next, next && raw[p + 1] == SP_SPACE);
                if (k == 2) got.push_back(SP_MARK);
                if (k >= 1) got.push_back(raw[p] == SP_SPACE ? SP_MARK : raw[p]);
            }
            // (leading spaces: the long statement drops them and adds a mark, the rule keeps the last of them as the mark)
            failures += got != slow(raw);
        }
    }
    // 3. the vocabulary: every piece comes back with its score and id, at every hash width; a prefix that is no piece does not
    for (int hash_bits : {0, 4, 64}) {
        std::vector<uint32_t> cp;
        std::vector<int32_t> poff{0}, ids;
        std::vector<float> score;
        uint32_t x = 12345;
        for (int i = 0; i < 700; ++i) {
            for (int v = i + 1; v; v /= 26) cp.push_back('a' + v % 26);
            cp.push_back('A');
            const int tail = (i % 7 == 0) ? SP_MAX_PIECE - 4 : (int)(i % 5);
            for (int j = 0; j < tail; ++j) cp.push_back(0x4E00 + (x = x * 1664525u + 1013904223u) % 5000);
            poff.push_back((int32_t)cp.size());
            ids.push_back(3 + i);
            score.push_back(-1.f - i);
        }
        const int32_t n = (int32_t)ids.size();
        const int64_t n_slots = wp_table_slots(n);
        std::vector<uint8_t> flags((size_t)n, 0);
        std::vector<int32_t> slots((size_t)n_slots, WP_EMPTY);
        const SpTable t{{cp.data(), poff.data(), flags.data(), slots.data(), n_slots, hash_bits == 64 ? 0 : hash_bits}, score.data(), ids.data()};
        for (int32_t i = 0; i < n; ++i) failures += wp_table_insert(t.pieces, slots.data(), i) < 0;
        for (int32_t i = 0; i < n; ++i) {
            const uint32_t* p = cp.data() + poff[i];
            const int32_t l = poff[i + 1] - poff[i];
            failures += l > SP_MAX_PIECE;
            const int32_t at = wp_table_find(t.pieces, p, l, 0u, wp_poly(p, l));
            failures += at != i || t.id[at] != 3 + i || t.score[at] != -1.f - i;
            failures += wp_table_find(t.pieces, p, l - 1, 0u, wp_poly(p, l - 1)) != WP_EMPTY;
        }
    }
    // 4. the order of candidates: greater first, then the smaller start; never both ways
    failures += !sp_better(-1.f, 5, -2.f, 1) || sp_better(-2.f, 1, -1.f, 5) || !sp_better(-1.f, 1, -1.f, 5) || sp_better(-1.f, 5, -1.f, 1);
    failures += sp_better(-1.f, 3, -1.f, 3);
    std::printf("failures %d\n", failures);
    return failures != 0;
}
"""


def test_the_table_header_builds_and_holds_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    (tmp_path / "drv.cpp").write_text(_DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    f"-I{ROOT / 'raglite_amd' / 'csrc'}", str(tmp_path / "drv.cpp"), "-o", str(tmp_path / "drv")], check=True)
    run = subprocess.run([str(tmp_path / "drv")], capture_output=True, text=True)  # (an ordinary child, the environment as it is)
    assert run.returncode == 0 and run.stdout.strip() == "failures 0", (run.stdout + run.stderr)[-4000:]
