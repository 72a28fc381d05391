"""The device WordPiece tokenizer on the host (no GPU): the tables probed from the `tokenizers` library, the plain-Python
statement of the kernels' algorithm (`WordPieceTables.encode_tables` / `encode_host`) held with `==` to that library's own ids, the host
statement of the pair assembly against `TorchCrossEncoderRanker.encode_pairs`, every argument check of the C entries (all return before
the first HIP call) and the vocabulary table's header under the host compiler's sanitizers."""

import ctypes as C
import shutil
import subprocess
import unicodedata
from pathlib import Path

import numpy as np
import pytest

from raglite_amd import _abi
from raglite_amd._cross_encoder import CrossEncoderShape, TorchCrossEncoderRanker, truncate_pair
from raglite_amd._wordpiece import CLS_CONTEXT, CLS_PUNCT, CLS_SPACE, WordPieceTables, pairs_host

from tests import wordpiece_ref as ref

ROOT = Path(__file__).resolve().parent.parent
INVALID, UNSUPPORTED = _abi.RL_ERR_INVALID, _abi.RL_ERR_UNSUPPORTED
BOTH = pytest.mark.parametrize("lowercase", [True, False], ids=["lowercase", "cased"])


# ---- the tables ---------------------------------------------------------------------------------------------------------------------
def test_the_tables_are_what_the_probe_of_this_library_gives():
    t = ref.tables(True)
    assert t.image.dtype == np.uint64 and t.cls.dtype == np.uint8 and len(t.image) == len(t.cls) == 0x110000
    assert int(((t.cls & 3) == CLS_SPACE).sum()) == 25 and int(((t.cls & 3) == CLS_PUNCT).sum()) == 726  # the classes the issue measured
    assert not t.image[0xD800:0xE000].any(), "surrogates have the empty image"
    assert int(t.image[ord("A")]) == ord("a") + 1 and int(t.image[ord("É")]) == ord("e") + 1
    assert int(t.image[ord("中")]) == (ord(" ") + 1) | ((ord("中") + 1) << 21) | ((ord(" ") + 1) << 42), "an image of three"
    assert t.image[0] == 0 and t.image[0xFFFD] == 0 and t.image[0x0301] == 0, "NUL, U+FFFD and stripped accents vanish"
    flagged = np.flatnonzero(t.cls & CLS_CONTEXT)
    assert len(flagged) > 0 and all(unicodedata.combining(chr(c)) != 0 and t.image[c] != 0 for c in flagged)
    assert {0x1D165, 0x1D16D} <= set(flagged.tolist())
    cased = ref.tables(False)
    assert int(cased.image[ord("A")]) == ord("A") + 1 and int(cased.image[ord("É")]) == ord("É") + 1
    assert t.unk_id == ref.vocabulary()["[UNK]"] and t.max_input_chars_per_word == ref.LONGEST


def test_npz_round_trip(tmp_path):
    t = ref.tables(True)
    t.save(tmp_path / "tables.npz")
    back = WordPieceTables.load(tmp_path / "tables.npz")
    for name in ("image", "cls", "piece_cp", "piece_off", "piece_flags", "piece_ids"):
        a, b = getattr(t, name), getattr(back, name)
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    assert (back.unk_id, back.max_input_chars_per_word, back.tokenizer_json, back.added_tokens) == \
           (t.unk_id, t.max_input_chars_per_word, t.tokenizer_json, t.added_tokens)
    texts = ref.EDGE_TEXTS[:4] + [ref.FLAGGED_TEXT]
    assert back.encode_host(texts) == t.encode_host(texts) == ref.yardstick(texts)  # (the mirrored tokenizer came back with them)


def test_from_vocab_builds_the_same_tables():
    small = {t: i for i, t in enumerate(["[UNK]", "a", "##b", "ab", "!"])}
    t = WordPieceTables.from_vocab(small, lowercase=False)
    assert np.array_equal(t.image, ref.tables(False).image) and np.array_equal(t.cls, ref.tables(False).cls)
    assert t.encode_host(["ab abb! b A"]) == [[3, 3, 2, 4, 0, 0]]


# ---- encode_host against the yardstick ----------------------------------------------------------------------------------------------
@BOTH
def test_edge_texts_equal_the_yardstick(lowercase):
    t = ref.tables(lowercase)
    want = ref.yardstick(ref.EDGE_TEXTS, lowercase)
    got = t.encode_host(ref.EDGE_TEXTS)
    for text, g, w in zip(ref.EDGE_TEXTS, got, want):
        assert g == w, repr(text)
    unk = t.unk_id
    by = dict(zip(ref.EDGE_TEXTS, got))
    assert by[""] == [] and by[ref.WHITE_SPACE_ONLY] == []
    assert len(by["a" * ref.LONGEST]) == ref.LONGEST and by["a" * (ref.LONGEST + 1)] == [unk]
    v = ref.vocabulary()
    assert by["q" * ref.LONGEST + " " + "q" * (ref.LONGEST + 1)] == [v["q" * ref.LONGEST], unk], "the longest piece, and one symbol too many"
    if lowercase:
        e = by["É" * ref.LONGEST + " " + "É" * (ref.LONGEST + 1)]
        assert e[-1] == unk and e.count(unk) == 1 and len(e) > 1, "the limit counts NORMALISED symbols: 100 matches, 101 is one [UNK]"
    head, cont = v[ref.HEAD_ONLY], v["##" + ref.CONT_ONLY]
    hc = by[f"{ref.HEAD_ONLY} a{ref.HEAD_ONLY} {ref.CONT_ONLY} a{ref.CONT_ONLY} {ref.HEAD_ONLY}{ref.CONT_ONLY}"]
    assert hc[0] == head and hc[-2:] == [head, cont] and hc.count(head) == 2, "never the head-only piece behind a word's first piece"
    assert by["ab中cd abc§def xy\U0001f600z"].count(unk) == 2, "the section sign, and the word with an emoji in its middle as ONE [UNK]"


@BOTH
def test_random_sweep_equals_the_yardstick_with_no_text_flagged(lowercase):
    t = ref.tables(lowercase)
    texts = ref.random_texts(11 + lowercase, 300)
    r = t.encode_tables(texts)
    assert not r["status"].any() and r["counts"][3] == 0, "no generated text may reach the fallback: it would hide a failure"
    assert not any(t.holds_added_token(x) for x in texts)
    want = ref.yardstick(texts, lowercase)
    off = r["offsets"]
    for i, text in enumerate(texts):
        assert r["ids"][off[i]: off[i + 1]].tolist() == want[i], repr(text)
    assert r["counts"][0] == len(r["ids"]) == sum(map(len, want)) > 5000 and r["counts"][2] > 0, "enough tokens, and some [UNK]"


@BOTH
def test_the_flagged_case_is_found_and_answered_by_the_mirrored_tokenizer(lowercase):
    t = ref.tables(lowercase)
    texts = ["plain text", ref.FLAGGED_TEXT, "more plain text"]
    r = t.encode_tables(texts)
    assert r["status"].tolist() == [0, 1, 0] and r["counts"][3] == 1
    assert t.encode_host(texts) == ref.yardstick(texts, lowercase)


def test_a_text_that_spells_an_added_token_goes_to_the_host():
    from tokenizers import Tokenizer

    tok = Tokenizer.from_str(ref.tokenizer(True).to_str())
    tok.add_special_tokens(["[SEP]"])
    t = WordPieceTables(**{**{k: getattr(ref.tables(True), k) for k in ("image", "cls", "piece_cp", "piece_off", "piece_flags", "piece_ids", "unk_id",
                                                                        "max_input_chars_per_word")},
                           "tokenizer_json": tok.to_str(), "added_tokens": ("[SEP]",)})
    texts = ["a [SEP] b", "a [ SEP ] b"]
    want = [tok.encode(x, add_special_tokens=False).ids for x in texts]
    assert want[0] == [ref.vocabulary()[k] for k in ("a", "[SEP]", "b")]
    assert t.encode_host(texts) == want and t.holds_added_token(texts[0]) and not t.holds_added_token(texts[1])


# ---- pair assembly ------------------------------------------------------------------------------------------------------------------
class _Lookup:
    """`encode(str) -> list[int]` from a dict."""

    def __init__(self, table):
        self.table = table

    def encode(self, text):
        return self.table[text]


def test_pairs_host_equals_encode_pairs():
    shape = CrossEncoderShape(vocab_size=500, hidden=32, layers=1, heads=1, ffn=32, max_positions=64, n_ctx=64, position_offset=0)
    rng = np.random.default_rng(5)
    # (n_query, n_doc, max_length): no cut, query longer, doc longer, a tie, an empty doc, an empty query, the smallest budget
    sweep = [(4, 9, 64), (30, 5, 20), (5, 30, 20), (20, 20, 21), (20, 20, 22), (7, 0, 64), (0, 7, 5), (9, 9, 3), (40, 3, 10), (3, 40, 10), (1, 1, 4)]
    for nq, nd, max_length in sweep:
        texts = {"q": rng.integers(103, 500, size=nq).tolist(), "d": rng.integers(103, 500, size=nd).tolist(), "e": rng.integers(103, 500, size=3).tolist()}
        ranker = TorchCrossEncoderRanker(shape, tokenizer=_Lookup(texts), device="cpu", max_length=max_length)
        want = ranker.encode_pairs("q", ["d", "e", "d"])
        ids = np.asarray(texts["q"] + texts["d"] + texts["e"], dtype=np.int32)
        off = np.asarray([0, nq, nq + nd, nq + nd + 3], dtype=np.int64)
        rows, pos, typ, seq = pairs_host(ids, off, [0, 0, 0], [1, 2, 1], max_length, shape.bos_id, shape.eos_id, 2)
        assert seq.tolist() == [0, *np.cumsum([len(r) for r, _ in want]).tolist()]
        for p, (row, first) in enumerate(want):
            lo, hi = seq[p], seq[p + 1]
            assert rows[lo:hi].tolist() == row and len(row) <= max(max_length, 3)
            assert typ[lo:hi].tolist() == [0] * first + [1] * (len(row) - first)
            assert pos[lo:hi].tolist() == list(range(2, 2 + len(row)))
        kq, kd = truncate_pair(nq, nd, max_length - 3)
        assert seq[1] == kq + kd + 3


# ---- the C entries' argument checks (none reaches a HIP call) -----------------------------------------------------------------------
def _create_args(**over):
    image = np.zeros(64, dtype=np.uint64)
    image[40] = (0x110000) | (5 << 21)
    cls = np.zeros(64, dtype=np.uint8)
    cp = np.asarray([97, 98, 99], dtype=np.uint32)
    off = np.asarray([0, 1, 3], dtype=np.int64)
    flags = np.zeros(2, dtype=np.uint8)
    ids = np.asarray([5, 6], dtype=np.int32)
    a = dict(image=image, cls=cls, n_table=64, piece_cp=cp, piece_off=off, piece_flags=flags, piece_ids=ids, n_pieces=2, unk_id=1, max_word_chars=100,
             hash_bits=0)
    a.update(over)
    return a


def _create(h, a):
    ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731
    return _abi.lib().rl_wordpiece_create(h, ptr(a["image"]), ptr(a["cls"]), a["n_table"], ptr(a["piece_cp"]), ptr(a["piece_off"]), ptr(a["piece_flags"]),
                                          ptr(a["piece_ids"]), a["n_pieces"], a["unk_id"], a["max_word_chars"], a["hash_bits"])


def _bad(field, value, at=None):
    a = _create_args()
    x = a[field].copy()
    x[at] = value
    return {field: x}


CREATE_CASES = [
    ({"image": None}, INVALID, "image is null"), ({"cls": None}, INVALID, "cls is null"), ({"n_table": 0}, INVALID, "n_table"),
    ({"n_table": 0x110001}, INVALID, "n_table must be in [1, 0x110000]"), ({"piece_off": None}, INVALID, "piece_off is null"),
    ({"piece_cp": None}, INVALID, "piece_cp"), ({"piece_flags": None}, INVALID, "piece_flags"), ({"piece_ids": None}, INVALID, "piece_ids"),
    ({"n_pieces": -1}, INVALID, "n_pieces"), ({"unk_id": -1}, INVALID, "unk_id"), ({"max_word_chars": 0}, INVALID, "max_word_chars"),
    ({"max_word_chars": 201}, UNSUPPORTED, "max_word_chars must be <= 200"), ({"hash_bits": 65}, INVALID, "hash_bits"),
    ({"hash_bits": -1}, INVALID, "hash_bits"), (_bad("piece_off", 1, 0), INVALID, "piece_off must start at 0"),
    (_bad("piece_off", 0, 2), INVALID, "piece_off must be ascending"), (_bad("piece_ids", -2, 1), INVALID, "piece_ids must be >= 0"),
    (_bad("image", 0x110001, 3), INVALID, "malformed image entry"), (_bad("image", 7 << 21, 3), INVALID, "malformed image entry"),
    (_bad("image", 1 << 63, 3), INVALID, "malformed image entry"), (_bad("cls", 3, 9), INVALID, "malformed cls entry"),
    (_bad("cls", 8, 9), INVALID, "malformed cls entry"),
]


@pytest.mark.parametrize("over,status,text", CREATE_CASES, ids=[f"{i}-" + "-".join(c[0]) for i, c in enumerate(CREATE_CASES)])
def test_create_rejects_before_any_hip_call(over, status, text):
    h = C.c_void_p(7)
    assert _create(C.byref(h), _create_args(**over)) == status
    assert _abi.last_error().startswith("rl_wordpiece_create: ") and text in _abi.last_error()
    assert not h.value, "the handle is cleared"


def test_the_other_entries_reject_before_any_hip_call():
    lib = _abi.lib()
    assert _create(None, _create_args()) == INVALID and _abi.last_error() == "rl_wordpiece_create: out is null"
    counts = (C.c_int64 * 5)()
    for call, text in [
        (lambda: lib.rl_wordpiece_encode(None, None, None, 0, 0, counts, 0, None), "rl_wordpiece_encode: null handle"),
        (lambda: lib.rl_wordpiece_result(None, None, None, None, 0, None), "rl_wordpiece_result: null handle"),
        (lambda: lib.rl_wordpiece_device(None, None, None, None), "rl_wordpiece_device: null handle"),
        (lambda: lib.rl_wordpiece_info(None, None), "rl_wordpiece_info: null handle"),
    ]:
        assert call() == INVALID and _abi.last_error() == text
    assert lib.rl_wordpiece_destroy(None) == _abi.RL_OK
    # the checks of rl_wordpiece_encode behind the handle need one, and making one needs a device: a fake non-null pointer is never
    # dereferenced by the checks in front of the first HIP call
    fake = C.c_void_p(0x1000)
    cp = np.zeros(4, dtype=np.uint32)
    off = lambda *v: np.asarray(v, dtype=np.int64)  # noqa: E731
    enc = lambda cp_, off_, n, n_texts, cnt=counts, mem=0: lib.rl_wordpiece_encode(fake, None if cp_ is None else cp_.ctypes.data,  # noqa: E731
                                                                                   None if off_ is None else off_.ctypes.data, n, n_texts, cnt, mem, None)
    for call, status, text in [
        (lambda: enc(cp, off(0, 4), -1, 1), INVALID, "negative size"), (lambda: enc(cp, off(0, 4), 4, -1), INVALID, "negative size"),
        (lambda: enc(cp, off(0, 4), 4, 1, mem=7), INVALID, "bad mem"), (lambda: enc(cp, None, 4, 1), INVALID, "text_off is null"),
        (lambda: enc(cp, off(0, 4), 4, 1, cnt=None), INVALID, "out_counts is null"), (lambda: enc(None, off(0, 4), 4, 1), INVALID, "codepoints is null"),
        (lambda: enc(cp, off(0), 4, 0), INVALID, "code points without a text"), (lambda: enc(cp, off(0, 4), 1 << 28, 1), UNSUPPORTED, "2^28"),
        (lambda: enc(cp, off(1, 4), 4, 1), INVALID, "text_off must start at 0"), (lambda: enc(cp, off(0, 3, 2, 4), 4, 3), INVALID, "text_off must be ascending"),
        (lambda: enc(cp, off(0, 2, 3), 4, 2), INVALID, "text_off must end at n"),
    ]:
        assert call() == status and _abi.last_error().startswith("rl_wordpiece_encode: ") and text in _abi.last_error(), text


def test_pairs_rejects_before_any_hip_call():
    lib = _abi.lib()
    ids = np.arange(6, dtype=np.int32)
    off = np.asarray([0, 2, 6], dtype=np.int64)
    q, d = np.asarray([0], dtype=np.int32), np.asarray([1], dtype=np.int32)
    out = np.zeros((3, 16), dtype=np.int32)
    seq = np.zeros(2, dtype=np.int32)
    total = C.c_int64()
    base = dict(ids=ids, tok_off=off, n_texts=2, query_text=q, doc_text=d, n_pairs=1, max_length=16, out_ids=out[0], out_positions=out[1],
                out_type_ids=out[2], out_seq_offsets=seq, out_total=C.byref(total), mem=0)

    def call(**over):
        a = {**base, **over}
        ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        return lib.rl_wordpiece_pairs(ptr(a["ids"]), ptr(a["tok_off"]), a["n_texts"], ptr(a["query_text"]), ptr(a["doc_text"]), a["n_pairs"], a["max_length"],
                                      101, 102, 0, ptr(a["out_ids"]), ptr(a["out_positions"]), ptr(a["out_type_ids"]), ptr(a["out_seq_offsets"]),
                                      a["out_total"], a["mem"], None)

    bad_off = lambda *v: np.asarray(v, dtype=np.int64)  # noqa: E731
    i32 = lambda *v: np.asarray(v, dtype=np.int32)  # noqa: E731
    for over, status, text in [
        ({"mem": 5}, INVALID, "bad mem"), ({"n_texts": -1}, INVALID, "negative size"), ({"n_pairs": -1}, INVALID, "negative size"),
        ({"n_pairs": 1 << 30}, UNSUPPORTED, "fewer than 2^31 tokens"), ({"max_length": 2}, INVALID, "max_length must be >= 3"),
        ({"tok_off": None}, INVALID, "tok_off is null"), ({"out_seq_offsets": None}, INVALID, "out_seq_offsets is null"),
        ({"out_total": None}, INVALID, "out_total is null"), ({"query_text": None}, INVALID, "query_text is null"),
        ({"doc_text": None}, INVALID, "doc_text is null"), ({"out_positions": None}, INVALID, "give out_ids, out_positions and out_type_ids"),
        ({"out_ids": None, "out_type_ids": None}, INVALID, "give out_ids, out_positions and out_type_ids"), ({"ids": None}, INVALID, "ids is null"),
        ({"tok_off": bad_off(1, 2, 6)}, INVALID, "tok_off must start at 0"), ({"tok_off": bad_off(0, 7, 6)}, INVALID, "tok_off must be ascending"),
        ({"query_text": i32(2)}, INVALID, "query_text holds an index outside [0, n_texts)"), ({"query_text": i32(-1)}, INVALID, "query_text holds an index"),
        ({"doc_text": i32(2)}, INVALID, "doc_text holds an index outside [0, n_texts)"),
    ]:
        assert call(**over) == status, text
        assert _abi.last_error().startswith("rl_wordpiece_pairs: ") and text in _abi.last_error(), text


# ---- the table's header under the host compiler's sanitizers ------------------------------------------------------------------------
_DRIVER = r"""
#include <cstdio>
#include <vector>
#include "wordpiece_table.h"
using namespace rl;
int main() {
    static_assert(WP_B * WP_B_INV == 1u, "");
    int failures = 0;
    for (int hash_bits : {0, 4, 64}) {
        std::vector<uint32_t> cp;
        std::vector<int32_t> off{0};
        std::vector<uint8_t> flags;
        uint32_t x = 12345;
        for (int i = 0; i < 700; ++i) {  // distinct pieces: the number i in base 26 plus a random tail, each as head and as continuation
            for (int f = 0; f < 2; ++f) {
                for (int v = i + 1; v; v /= 26) cp.push_back('a' + v % 26);
                cp.push_back('A' + f);
                const int tail = (i % 7 == 0) ? 95 : (int)(i % 5);
                for (int j = 0; j < tail; ++j) cp.push_back(0x4E00 + (x = x * 1664525u + 1013904223u) % 5000);
                off.push_back((int32_t)cp.size());
                flags.push_back((uint8_t)f);
            }
        }
        const int32_t n = (int32_t)flags.size();
        const int64_t n_slots = wp_table_slots(n);
        std::vector<int32_t> slots((size_t)n_slots, WP_EMPTY);
        const WpTable t{cp.data(), off.data(), flags.data(), slots.data(), n_slots, hash_bits == 64 ? 0 : hash_bits};
        for (int32_t i = 0; i < n; ++i) failures += wp_table_insert(t, slots.data(), i) < 0;
        failures += wp_table_insert(t, slots.data(), 3) != -1;  // an equal piece: the first stays
        for (int32_t i = 0; i < n; ++i) {
            const uint32_t* p = cp.data() + off[i];
            const int32_t len = off[i + 1] - off[i];
            failures += wp_table_find(t, p, len, flags[i], wp_poly(p, len)) != i;               // every piece comes back ...
            failures += wp_table_find(t, p, len - 1, flags[i], wp_poly(p, len - 1)) != WP_EMPTY;  // ... its prefix does not (no piece is one)
            // the kernel's way to the same polynomial: prefix sums over a longer word, the piece at [at, at + len)
            std::vector<uint32_t> word{1, 2, 3};
            word.insert(word.end(), p, p + len);
            std::vector<uint32_t> prefix(word.size() + 1, 0);
            uint32_t pw = 1, inv = 1;
            for (size_t j = 0; j < word.size(); ++j, pw *= WP_B) prefix[j + 1] = wp_poly_add(prefix[j], word[j], pw);
            for (int j = 0; j < 3; ++j) inv *= WP_B_INV;
            failures += (prefix[3 + len] - prefix[3]) * inv != wp_poly(p, len);
        }
    }
    std::printf("failures %d\n", failures);
    return failures != 0;
}
"""


def test_the_table_header_builds_and_probes_every_piece_back_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    (tmp_path / "drv.cpp").write_text(_DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    f"-I{ROOT / 'raglite_amd' / 'csrc'}", str(tmp_path / "drv.cpp"), "-o", str(tmp_path / "drv")], check=True)
    run = subprocess.run([str(tmp_path / "drv")], capture_output=True, text=True)  # (an ordinary child, the environment as it is)
    assert run.returncode == 0 and run.stdout.strip() == "failures 0", (run.stdout + run.stderr)[-4000:]
