"""The yardstick, the synthetic vocabulary and the text generators of the device WordPiece tokenizer (raglite_amd/csrc/wordpiece.hip,
DESIGN.md 4.24), shared by tests/test_wordpiece_host.py and tests/test_gpu_wordpiece.py.

The yardstick is the `tokenizers` library itself: a BERT pipeline (BertNormalizer, BertPreTokenizer, WordPiece) over a vocabulary made
here, no file fetched.  `tables(lowercase)` probes it once per process (a few seconds) and both test files share the result."""

import functools

import numpy as np

from raglite_amd._wordpiece import WordPieceTables, bert_tokenizer

LETTERS = "abcdefghijklmnopqrstuvwxyz"
PUNCT = "!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~"
SPECIAL = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]
LONGEST = 100  # the model's max_input_chars_per_word: a longer piece can match nothing
HEAD_ONLY, CONT_ONLY = "zqxjv", "kzqxw"  # one piece present only as a head, one only as a continuation


@functools.lru_cache(maxsize=None)
def vocabulary() -> dict:
    rng = np.random.default_rng(20240)
    vocab: dict = {}

    def add(token):
        vocab.setdefault(token, len(vocab))

    for t in SPECIAL:
        add(t)
    for ch in LETTERS + "0123456789":
        add(ch)
        add("##" + ch)
    for ch in PUNCT:
        add(ch)
    for i in range(3000):  # random 2-7 letter pieces, half of them continuations
        w = "".join(rng.choice(list(LETTERS), size=int(rng.integers(2, 8))))
        if w in (HEAD_ONLY, CONT_ONLY):
            continue
        add("##" + w if i % 2 else w)
    for t in ("中", "é", "ß", "ss", "σ", "ς", "##ß", "##σ", "İ", "##é"):
        add(t)
    add(HEAD_ONLY)
    add("##" + CONT_ONLY)
    add("q" * LONGEST)  # one piece of the longest length a word can have
    add("##" + "q" * (LONGEST - 1))
    return vocab


@functools.lru_cache(maxsize=None)
def tokenizer(lowercase: bool = True):
    return bert_tokenizer(vocabulary(), lowercase=lowercase)


@functools.lru_cache(maxsize=None)
def tables(lowercase: bool = True) -> WordPieceTables:
    return WordPieceTables.from_tokenizer(tokenizer(lowercase))


def yardstick(texts, lowercase: bool = True) -> list:
    return [e.ids for e in tokenizer(lowercase).encode_batch(list(texts), add_special_tokens=False)]


@functools.lru_cache(maxsize=None)
def _pieces() -> tuple:
    heads = [t for t in vocabulary() if t[0] in LETTERS and len(t) > 1]
    conts = [t[2:] for t in vocabulary() if t.startswith("##") and len(t) > 3 and t[2] in LETTERS]
    return tuple(heads), tuple(conts)


# code points of the sweep beside the words: none is a combining mark, so no generated text is flagged (the tests assert it)
EXTRA = (" \t\n\u00a0\u3000" + PUNCT + "\u00e9\u00fc\u00df\u00c9\u0130\u03a3\u03c3\u03c2\u4e2d\u6587\u65e5\u672c\u8a9e\ud55c\uad6d\uc5b4\uac00\U0001f600\u00e6"
         "\ufffd\x00\x01\u200b\u00ad\u039f\u0394\u0391\u00c5\u00a7\u00ab\u00bb\u2014\u2026")


def random_word(rng) -> str:
    """A word that mostly matches: a head piece and a few continuations, sometimes random letters, sometimes upper case."""
    heads, conts = _pieces()
    kind = rng.integers(0, 10)
    if kind < 6:
        w = str(rng.choice(heads)) + "".join(str(rng.choice(conts)) for _ in range(int(rng.integers(0, 4))))
    elif kind < 9:
        w = "".join(rng.choice(list(LETTERS + "0123456789"), size=int(rng.integers(1, 12))))
    else:
        w = "".join(rng.choice(list(EXTRA), size=int(rng.integers(1, 4))))
    return w.upper() if rng.integers(0, 8) == 0 else w


def random_text(rng, n_words: int) -> str:
    seps = [" ", " ", " ", "  ", ", ", ".", "-", "\n", ""]
    return "".join(random_word(rng) + str(rng.choice(seps)) for _ in range(n_words))


def random_texts(seed: int, n_texts: int, max_words: int = 30) -> list:
    rng = np.random.default_rng(seed)
    return [random_text(rng, int(rng.integers(0, max_words + 1))) for _ in range(n_texts)]


WHITE_SPACE_ONLY = " \t\n\u00a0\u3000  "
EDGE_TEXTS = [
    "The quick brown fox jumps over the lazy dog, doesn't it? Yes: 42 times.",  # ASCII prose
    "İstanbul ạ́b straße ΟΔΟΣ Ünïcödé",  # accents (ạ́b holds combining marks: flagged, answered by the mirrored tokenizer)
    "中文字 한국어 가각 日本語のテキスト",  # CJK (images of 3) and Hangul
    "...!!!???---((()))[[]]{}<<>>@#$%^&*",  # runs of punctuation
    "a\x00b\x01c\ufffdd\x7fe\u200bf\u00adg",  # control characters, U+FFFD, NUL, a zero-width space, a soft hyphen
    "",  # an empty text
    WHITE_SPACE_ONLY,
    "a" * LONGEST,  # a word of exactly 100 normalised symbols
    "a" * (LONGEST + 1),  # ... and of 101
    "q" * LONGEST + " " + "q" * (LONGEST + 1),
    "É" * LONGEST + " " + "É" * (LONGEST + 1),  # 100 / 101 symbols AFTER normalisation (lowercase: each É is one e)
    "ab中cd abc§def xy\U0001f600z",  # a word with no match in the middle
    f"{HEAD_ONLY} a{HEAD_ONLY} {CONT_ONLY} a{CONT_ONLY} {HEAD_ONLY}{CONT_ONLY}",  # head-only and continuation-only pieces
    "straße STRASSE ß ss σς ΣΣ",
]
FLAGGED_TEXT = "a\U0001d16d\U0001d165b \U0001d165\U0001d16d c"  # the two musical marks whose order normalisation may change
