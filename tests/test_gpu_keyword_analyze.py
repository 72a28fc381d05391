"""The BM25 index analyzer on the device (raglite_amd/csrc/keyword_analyze.hip): `analyze_texts_batch` against its
specification, `_keyword.index_stems` + `stems_to_store_ids` on a fresh `Vocabulary`.  Everything is compared with `==`: the flat int32
term ids, the offsets, the vocabulary's stems in id order and the ordinals of the dead chunks."""

import random

import numpy as np
import pytest

import raglite_amd
from oracle.fake_embedder import FakeLlama
from raglite_amd import _keyword, _ops

pytestmark = pytest.mark.gpu

# the launch geometry of keyword_analyze.hip and of the scan it shares with keyword_build.hip
WAVE = 64
KA_THREADS = 256    # lanes per workgroup of every kernel: one per code point, symbol, token or text
SCAN_TILE = 2048    # KB_SCAN_TILE: items per workgroup of the exclusive scans
BOUNDARIES = (WAVE, KA_THREADS, SCAN_TILE, 2 * SCAN_TILE)

CLASSIC = ("caresses ponies ties caress cats feed agreed plastered bled motoring sing conflated troubled sized hopping tanned falling "
           "hissing fizzed failing filing happy sky relational conditional rational probate rate cease controll roll generalizations "
           "oscillators").split()


def _reference(texts, vocab):
    return _keyword.stems_to_store_ids([None if t is None else _keyword.index_stems(t) for t in texts], vocab)


def _check(texts, *, analyzer=None, what="", **kwargs):
    """One batch through the device and through the specification, each on a fresh vocabulary; returns the device side."""
    v_dev, v_ref = _keyword.Vocabulary(), _keyword.Vocabulary()
    want_flat, want_off, want_dead = _reference(texts, v_ref)
    flat, off, dead = raglite_amd.analyze_texts_batch(texts, v_dev, analyzer=analyzer, return_dead=True, **kwargs)
    assert flat.dtype == np.int32 and off.dtype == np.int64 and dead.dtype == np.int64, what
    assert off.tolist() == want_off.tolist(), what
    assert flat.tolist() == want_flat.tolist(), what
    assert dead.tolist() == want_dead.tolist(), what
    assert v_dev.stems == v_ref.stems, what
    return flat, off, v_dev


@pytest.fixture(scope="module")
def no_stopwords(torch_cuda):
    """An analyzer with an empty stopword list: every token's stem comes back."""
    analyzer = _ops.KeywordAnalyzer(_keyword.fold_table(), [])
    yield analyzer
    analyzer.close()


def _words(rng, n, lo=2, hi=9):
    return ["".join(rng.choice("abcdefghilmnoprstuy") for _ in range(rng.randint(lo, hi))) for _ in range(n)]


@pytest.fixture(scope="module")
def corpus():
    """600 bodies over ~1 500 words with suffixes, stopwords, accents and escapes: the batch of the id tests."""
    rng = random.Random(18)
    heads = _words(rng, 500, 3, 7)
    suffixes = ["", "s", "ed", "ing", "ation", "ational", "ness", "ful", "ize", "ly", "ement", "ies"]
    stop = sorted(_keyword.STOPWORDS)
    texts = []
    for _ in range(600):
        parts = []
        for _ in range(rng.randint(0, 40)):
            r = rng.random()
            if r < 0.6:
                parts.append(rng.choice(heads) + rng.choice(suffixes))
            elif r < 0.85:
                parts.append(rng.choice(stop))
            elif r < 0.9:
                parts.append("Él\\n über﹨x ﬁnal")
            else:
                parts.append(rng.choice(heads).upper())
        texts.append(rng.choice([" ", ", ", "\n", " - "]).join(parts))
    return texts


# ---- degenerate texts and text boundaries --------------------------------------------------------------------------------------
def test_degenerate_texts(torch_cuda):
    for texts in ([], [""], ["a"], ["q"], ["kernel"], ["ox"], [" "], ["\\"], ["́"], [None], [None, None], ["", "", ""],
                  ["x", None, "", None, "y z"], [None, "kernel"], ["kernel", None], ["́", "q", "\\", " ", "q"]):
        flat, off, _ = _check(texts, what=repr(texts))
        assert off.size == len(texts) + 1


def test_nothing_crosses_a_text_boundary(torch_cuda):
    flat, off, vocab = _check(["ab", "cd"])
    assert off.tolist() == [0, 1, 2] and vocab.stems == ["ab", "cd"]
    _, off, vocab = _check(["ab\\", "cd"])  # the backslash ends its text: nothing is consumed
    assert vocab.stems == ["ab", "cd"]
    _, off, vocab = _check(["kernel\\", "\\", "\\kernel", "xo\\\\\\", "bcd"])
    assert off.tolist() == [0, 1, 1, 2, 3, 4] and vocab.stems == ["kernel", "ernel", "xo", "bcd"]
    _check(["graﬁ", "x", "ﬁ", "ﬁ", "aﬃ", "", "ne"])  # texts that end in a letter image of several letters
    _check(["a\\", None, "\nb", "\\", "", "b\\", "Ⅷ"])


# ---- escapes -------------------------------------------------------------------------------------------------------------------
def test_backslash_runs_of_every_length(torch_cuda):
    texts = []
    for r in list(range(1, 10)) + [4097]:
        for slash in ("\\", "﹨", "＼"):
            for nxt in ("a", "\n", " ", "́a", "Ⅷ", "ﬁx", "\r", "."):
                texts.append(f"left{slash * r}{nxt}bc right")
        mixed = "".join(("\\", "﹨", "＼")[i % 3] for i in range(r))
        texts.append(f"left{mixed}abc")
        texts.append(mixed)           # a text of backslashes alone
        texts.append(mixed + "abc")   # ... and a run at the start of a text
    _check(texts)


# ---- launch geometry -----------------------------------------------------------------------------------------------------------
def test_tokens_and_texts_straddle_every_boundary(torch_cuda):
    rng = random.Random(5)
    for b in BOUNDARIES:
        for d in (-1, 0, 1):
            # one text whose token `straddling` lies across folded position b + d, behind one-letter tokens
            filler = ("q " * b)[: b + d - 4]
            _check([filler + "straddling tail"], what=f"token across {b}+{d}")
            # a text boundary at code point b + d, with a token on each side of it and an escape in front of it
            _check(["w" * (b + d), "kernel"], what=f"text boundary at {b}+{d}")
            _check([("zz " * b)[: b + d - 1] + "\\", "kernel"], what=f"escape at {b}+{d}")
            # b + d texts, some empty or dead; b + d tokens in one text; an image of several letters across the boundary
            many = [rng.choice(["kernel", "", None, "two words", "the"]) for _ in range(b + d)]
            _check(many, what=f"{b}+{d} texts")
            _check([" ".join(_words(rng, b + d))], what=f"{b}+{d} tokens")
            _check(["e" * (b + d - 2) + "Ⅷ kernel"], what=f"image across {b}+{d}")


def test_one_long_text(torch_cuda):
    rng = random.Random(6)
    words = _words(rng, 3000) + sorted(_keyword.STOPWORDS)[:100] + ["Él", "über\\x", "ﬁnal", "Ⅷ", "naïve"]
    parts, size = [], 0
    while size < 300_000:
        w = rng.choice(words)
        parts.append(w)
        size += len(w) + 1
    text = " ".join(parts)
    assert len(text) >= 300_000
    _check([text])
    _check(["front", text, None, "back"])


# ---- the stemmer ---------------------------------------------------------------------------------------------------------------
def _stemmer_words():
    rng = random.Random(7)
    cons, vowels = "bcdfghjklmnpqrstvwxzy", "aeiouy"

    def head(m):  # [C](VC)^m[V], y in both roles
        s = rng.choice(["", rng.choice(cons), rng.choice(cons) + rng.choice(cons)])
        for _ in range(m):
            s += rng.choice(vowels) + rng.choice(cons) + (rng.choice(cons) if rng.random() < 0.3 else "")
        return s + (rng.choice(vowels) if rng.random() < 0.4 else "")

    suffixes = (["sses", "ies", "ss", "s", "eed", "ed", "ing", "at", "bl", "iz", "y", "e", "l", "ll", "ated", "bling", "izing"]
                + list(_keyword._STEP2) + list(_keyword._STEP3) + list(_keyword._STEP4))  # noqa: SLF001
    words = set(CLASSIC)
    for m in range(4):
        for _ in range(5):
            h = head(m)
            words.add(h)
            for s in suffixes:
                words.add(h + s)
                for s2 in ("s", "ed", "ing", "e", "ly", "ness", "al", "ion", "es"):
                    words.add(h + s + s2)
    words |= {"y" * 100, "s", "yyed", "ying", "x" * 40 + "ationalizationalities"}
    words.discard("")
    return sorted(words)


def test_every_rule_of_the_stemmer(torch_cuda, no_stopwords):
    words = _stemmer_words()
    assert len(words) > 5000
    flat, off, vocab = _check_no_stop(words, no_stopwords)
    assert off.tolist() == list(range(len(words) + 1))  # one token per word
    stems = vocab.stems
    for i, w in enumerate(words):
        assert stems[flat[i]] == _keyword.stem(w), w


def _check_no_stop(texts, analyzer):
    """As `_check`, against the specification without the stopword removal."""
    v_dev, v_ref = _keyword.Vocabulary(), _keyword.Vocabulary()
    want_flat, want_off, _ = _keyword.stems_to_store_ids([[_keyword.stem(t) for t in _keyword.tokenize(x)] for x in texts], v_ref)
    flat, off = raglite_amd.analyze_texts_batch(texts, v_dev, analyzer=analyzer)
    assert off.tolist() == want_off.tolist() and flat.tolist() == want_flat.tolist() and v_dev.stems == v_ref.stems
    return flat, off, v_dev


def test_long_tokens(torch_cuda):
    rng = random.Random(8)
    long_ization = "".join(rng.choice("abcdefgy") for _ in range(5000 - 7)) + "ization"
    flat, off, vocab = _check([long_ization, "a" * 5000, "x " + "y" * 5000 + " z", long_ization + "s " + "a" * 5000])
    assert len(long_ization) == 5000 and vocab.stems[0] == _keyword.stem(long_ization) and vocab.stems[1] == "a" * 5000
    assert off.tolist() == [0, 1, 2, 3, 5]  # (x and z are stopwords)


# ---- stopwords -----------------------------------------------------------------------------------------------------------------
def test_stopwords(torch_cuda):
    stop = sorted(_keyword.STOPWORDS)
    assert len(stop) == 570 and max(map(len, stop)) == 13
    plain = [w for w in stop if w.isalpha()]  # (the others, such as `ain't`, split into tokens that are no stopwords)
    assert len(plain) > 500 and all(len(w) == 1 for w in "abcxyz" if w in _keyword.STOPWORDS)
    flat, off, vocab = _check([" ".join(plain), "The AND of", "kernel " + " kernel ".join(stop) + " zebra"])
    assert off[:3].tolist() == [0, 0, 0] and vocab.stems[0] == "kernel" and vocab.stems[-1] == "zebra"
    assert int(np.count_nonzero(flat == 0)) == len(stop)  # `kernel` in front of every stopword
    plural = [w + "s" for w in plain if w + "s" not in _keyword.STOPWORDS]
    assert len(plural) > 400
    _, off, _ = _check([" ".join(plural)] + [w + "s" for w in stop] + [w[:-1] for w in stop if len(w) > 1])
    assert int(off[1]) == len(plural)  # none of them is dropped


# ---- term ids ------------------------------------------------------------------------------------------------------------------
def test_vocabulary_carries_across_calls(torch_cuda, corpus):
    v_dev, v_ref = _keyword.Vocabulary(), _keyword.Vocabulary()
    for part in (corpus[:200], corpus[150:450], corpus[400:]):  # overlapping: known stems keep their ids, new ones go on counting
        want_flat, want_off, _ = _reference(part, v_ref)
        flat, off = raglite_amd.analyze_texts_batch(part, v_dev)
        assert flat.tolist() == want_flat.tolist() and off.tolist() == want_off.tolist() and v_dev.stems == v_ref.stems


def test_split_into_calls_and_forced_collisions(torch_cuda, corpus):
    flat, off, vocab = _check(corpus)
    assert len(vocab) >= 200
    total = sum(map(len, corpus))
    calls = []
    v = _keyword.Vocabulary()
    for result in _keyword.analyze_texts_device(corpus, v, max_chars_per_call=total // 3 - 1):
        calls.append(result.n_chunks)
    assert len(calls) >= 3 and sum(calls) == len(corpus)
    flat3, off3, vocab3 = _check(corpus, max_chars_per_call=total // 3 - 1)
    assert flat3.tobytes() == flat.tobytes() and off3.tobytes() == off.tobytes() and vocab3.stems == vocab.stems
    _check(corpus, max_chars_per_call=1)  # every text alone
    colliding = _ops.KeywordAnalyzer(_keyword.fold_table(), sorted(_keyword.STOPWORDS), hash_bits=4)  # 16 hash values, >= 200 stems
    try:
        flat4, off4, vocab4 = _check(corpus, analyzer=colliding)
        assert flat4.tobytes() == flat.tobytes() and off4.tobytes() == off.tobytes() and vocab4.stems == vocab.stems
    finally:
        colliding.close()


def test_same_call_twice_gives_the_same_bytes(torch_cuda, corpus):
    analyzer = _keyword.default_analyzer()
    sizes = np.asarray([len(t) for t in corpus], dtype=np.int64)
    text_off = np.concatenate(([0], np.cumsum(sizes)))
    codepoints = np.frombuffer("".join(corpus).encode("utf-32-le"), dtype=np.uint32)
    runs = []
    for _ in range(2):
        n_tokens, stems, first_pos = analyzer.begin(codepoints, text_off)
        result = analyzer.finish(np.arange(len(stems), dtype=np.int32))
        flat, off = result.read()
        runs.append((n_tokens, stems, first_pos.tobytes(), flat.tobytes(), off.tobytes()))
    assert runs[0] == runs[1]
    n_tokens, stems, first_pos, _, _ = runs[0]
    first_pos = np.frombuffer(first_pos, dtype=np.int64)
    assert len(set(stems)) == len(stems) and np.all(np.diff(first_pos) > 0) and first_pos[0] == 0 and first_pos[-1] < n_tokens
    with pytest.raises(ValueError):
        analyzer.begin(codepoints, text_off)  # a new call ...
        result.read()                         # ... and the earlier result is gone


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def test_device_and_host_analyzed_indexes_are_twins(torch_cuda):
    rng = np.random.default_rng(62)
    prng = random.Random(62)
    dim, n = 32, 2000
    raglite_amd.set_embedder_factory(lambda config: FakeLlama(dim=dim))
    vocab_words = _words(prng, 400, 3, 8)
    suffixes = ["", "s", "ed", "ing", "ation", "ness", "ly"]
    stop = sorted(_keyword.STOPWORDS)

    def bodies(count):
        out = []
        for _ in range(count):
            words = [prng.choice(vocab_words) + prng.choice(suffixes) if prng.random() < 0.8 else prng.choice(stop)
                     for _ in range(prng.randint(0, 30))]
            out.append(" ".join(words) + prng.choice(["", " café\\x", " Ⅷ"]))
        return out

    def chunks(prefix, count):
        mats = [rng.standard_normal((int(rng.integers(1, 3)), dim)).astype(np.float32) for _ in range(count)]
        return [f"{prefix}-{i:05d}" for i in range(count)], mats, bodies(count)

    ids, mats, texts = chunks("base", n)
    dev = raglite_amd.GpuIndex(ids, mats, keyword_texts=texts, keyword_analyzer="device")
    host = raglite_amd.GpuIndex(ids, mats, keyword_texts=texts, keyword_analyzer="host")
    queries = [" ".join(prng.choice(vocab_words) + prng.choice(suffixes) for _ in range(prng.randint(1, 4))) for _ in range(32)]

    def twins():
        assert dev._kw_vocabulary.stems == host._kw_vocabulary.stems  # noqa: SLF001
        got = raglite_amd.keyword_search_batch(queries, num_results=10, index=dev)
        want = raglite_amd.keyword_search_batch(queries, num_results=10, index=host)
        assert len(got) == len(want) == 32
        for g, w in zip(got, want):
            assert g[0] == w[0] and g[1] == w[1] and len(g[0]) == len(w[0])

    try:
        assert dev.keyword_analyzer == "device" and host.keyword_analyzer == "host"
        assert all(isinstance(x, np.ndarray) and x.dtype == np.int32 for x in dev._kw_stems)  # noqa: SLF001
        twins()
        ids2, mats2, texts2 = chunks("new", 100)
        for gi in (dev, host):
            gi.insert_chunks(ids2, mats2, keyword_texts=texts2)
        twins()
        gone = [ids[int(i)] for i in rng.choice(n, size=60, replace=False)] + ids2[:3]
        for gi in (dev, host):
            assert gi.delete_chunks(gone) == 63
        twins()
        for gi in (dev, host):
            gi.compact()
        assert dev.index.n_chunks == n + 100 - 63
        got = raglite_amd.keyword_search_batch(queries, num_results=10, index=dev)
        want = raglite_amd.keyword_search_batch(queries, num_results=10, index=host)
        for g, w in zip(got, want):  # (the vocabularies differ now: the device one keeps the dropped chunks' stems, with df = 0)
            assert g[0] == w[0] and g[1] == w[1]
        with pytest.raises(ValueError):
            raglite_amd.GpuIndex(ids[:2], mats[:2], keyword_texts=texts[:2], keyword_analyzer="device", keyword_build="host")
    finally:
        raglite_amd.set_embedder_factory(None)
        dev.close()
        host.close()
