"""What the SentencePiece tests share (tests/test_sentencepiece_host.py, tests/test_gpu_sentencepiece.py): the committed Unigram fixture
(tests/golden/unigram_2k.model, made by scripts/make_unigram_fixture.py and never retrained here), its tables, the recorded cases
and the random texts of the sweeps.  Everything is computed once per process and left unchanged."""

import functools
import hashlib
import json
import random
from pathlib import Path

from raglite_amd._sentencepiece import UnigramTables

GOLDEN = Path(__file__).resolve().parent / "golden"
MODEL = GOLDEN / "unigram_2k.model"
BPE_MODEL = GOLDEN / "spm_2k.model"

# decomposed e-acute, half-width katakana with its voicing mark, a Hangul jamo sequence: each holds a code point of the trailing set
FLAGGED_TEXTS = ["café au lait", "ｶﾞｷﾞ", "한글"]


@functools.lru_cache(maxsize=None)
def tables(xlmr: bool = True) -> UnigramTables:
    return UnigramTables.from_model(MODEL, xlmr=xlmr)


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    return json.loads((GOLDEN / "unigram_2k_cases.json").read_text(encoding="utf-8"))


def case(name: str) -> str:
    c = cases()
    return c["texts"][c["names"].index(name)]


def batch_of(words: list, oov: str) -> list:
    """About 20 000 words over 300 texts, by arithmetic alone (the same on every machine): 1 .. 130 words per text, one or two spaces
    between them, every 37th text empty, and in every tenth text some words replaced by out-of-vocabulary runs."""
    out = []
    for i in range(300):
        if i % 37 == 0:
            out.append("")
            continue
        parts = []
        for j in range(1 + (i * 37) % 130):
            k = i * 7919 + j * 104729
            if i % 10 == 0 and k % 17 == 0:
                parts.append("".join(oov[(k + r) % len(oov)] for r in range(1 + k % 3)))
            else:
                parts.append(words[k % len(words)])
            parts.append("  " if k % 4 == 0 else " ")
        out.append("".join(parts))
    return out


def digest(ids_per_text: list) -> str:
    """One SHA-256 over the token counts and the ids of many texts: what the fixture records of the batch instead of some 80 000 ids."""
    h = hashlib.sha256()
    for ids in ids_per_text:
        h.update(len(ids).to_bytes(4, "little"))
        h.update(b"".join(int(i).to_bytes(4, "little") for i in ids))
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def batch_texts() -> tuple:
    return tuple(batch_of(sorted(set(case("words_3000").split())), cases()["oov"]))


def library():
    """The mirrored processor, or None where the library does not import."""
    try:
        import sentencepiece  # noqa: F401
    except ImportError:
        return None
    return tables().processor()


@functools.lru_cache(maxsize=None)
def trailing() -> frozenset:
    t = tables()
    return frozenset(int(c) for c in (t.image_len & t.FLAG).nonzero()[0])


# ASCII, Latin-1 / Extended, Greek, Cyrillic, kana, full-width forms, CJK, ligatures, circled digits, controls and exotic spaces
_POOLS = [(0x20, 0x7F), (0xA0, 0x250), (0x370, 0x400), (0x400, 0x500), (0x3041, 0x3100), (0xFF01, 0xFF60), (0x4E00, 0x4F00), (0xFB00, 0xFB07),
          (0x2460, 0x2474), (0x00, 0x20), (0x2000, 0x2010), (0x3000, 0x3001), (0xAC00, 0xAC40)]


def random_texts(seed: int, count: int) -> list[str]:
    """Random texts over the pools above WITHOUT the trailing set: none may be flagged."""
    rng = random.Random(seed)
    bad = trailing()
    out = []
    for _ in range(count):
        n = rng.randint(0, 60)
        chars = []
        while len(chars) < n:
            if rng.random() < 0.55:
                c = rng.choice((0x20, 0x20, rng.randint(0x61, 0x7A), rng.randint(0x61, 0x7A), rng.randint(0x41, 0x5A)))
            else:
                lo, hi = rng.choice(_POOLS)
                c = rng.randrange(lo, hi)
            if c not in bad and not 0xD800 <= c < 0xE000:
                chars.append(chr(c))
        out.append("".join(chars))
    return out
