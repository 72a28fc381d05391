"""Shared inputs of the sentence tests: a deterministic text generator (the documents of `tests/golden/split_sentences.npz` are
described by its parameters, not stored), numeric documents for the device tests, and the layout helpers of
`rl_partition_sentences`.  The texts come from the 64-bit LCG of `tests/chunklets_ref.py`, so they never drift."""

import json
from pathlib import Path

import numpy as np

from tests.chunklets_ref import Lcg, _phrase

GOLDEN = Path(__file__).resolve().parent / "golden" / "split_sentences.npz"
CASES = ((4, None), (4, 64), (4, 2048), (1, None), (12, 40))  # (min_len, max_len)

_SEPARATORS = (". ", ". ", ". ", "?\n\n", ".  \t", "! ", ".\n")
_UNICODE_SPACES = ("\u00a0", "\u2003", "\u3000", "\u0085", "\u200b", " \u00a0", "\u200b ")  # U+200B is NOT white space

# seed, blocks, kind, dtype of the predictions -- kind "prose": paragraphs; "markdown": headings between paragraphs; "unicode": prose
# whose words are joined by Unicode spaces (and by U+200B, which is none); "table": prose around table-like lines of several hundred
# characters without sentence punctuation (phase 2 runs on them); lead / trail: white space around the document
DOCUMENTS = (
    {"seed": 1, "blocks": 3, "kind": "prose", "dtype": "float32"},
    {"seed": 2, "blocks": 6, "kind": "markdown", "dtype": "float32"},
    {"seed": 3, "blocks": 5, "kind": "unicode", "dtype": "float64"},
    {"seed": 4, "blocks": 4, "kind": "table", "dtype": "float32"},
    {"seed": 5, "blocks": 8, "kind": "markdown", "dtype": "float64", "lead": " \n\t ", "trail": "  \n\n"},
    {"seed": 6, "blocks": 6, "kind": "table", "dtype": "float64", "lead": "\n"},
    {"seed": 7, "blocks": 20, "kind": "markdown", "dtype": "float32"},
    {"seed": 8, "blocks": 12, "kind": "prose", "dtype": "float64", "trail": " "},
    {"seed": 9, "blocks": 9, "kind": "unicode", "dtype": "float32", "lead": "\u3000", "trail": " \u200b"},
    {"seed": 10, "blocks": 1, "kind": "table", "dtype": "float32"},
    {"seed": 11, "blocks": 2, "kind": "markdown", "dtype": "float64"},
    {"seed": 12, "blocks": 30, "kind": "prose", "dtype": "float32"},
)


def make_document(seed: int, blocks: int, kind: str = "prose", lead: str = "", trail: str = "") -> str:
    rng = Lcg(seed)
    out = [lead]
    for block in range(blocks):
        if kind == "markdown" and (block == 0 or rng.below(3) == 0):
            out.append("#" * (1 + rng.below(3)) + " " + _phrase(rng, 1, 5).capitalize() + "\n\n")
        if kind == "table" and (block % 2 == 0):
            cells = 40 + rng.below(60)
            out.append("| " + " | ".join(_phrase(rng, 1, 2) for _ in range(cells)) + " |\n")
        count = 1 + rng.below(6)
        for k in range(count):
            sentence = _phrase(rng, 3, 24).capitalize()
            if kind == "unicode":
                sentence = "".join(c if c != " " or rng.below(3) else _UNICODE_SPACES[rng.below(len(_UNICODE_SPACES))] for c in sentence)
            out.append(sentence + ("\n\n" if k == count - 1 and rng.below(2) else _SEPARATORS[rng.below(len(_SEPARATORS))]))
    out.append(trail)
    return "".join(out)


def make_predictions(doc: str, seed: int, dtype: str) -> np.ndarray:
    """Synthetic model output: high at sentence punctuation, low elsewhere, in steps of 1 / 256 (exact in float32; equal values are
    frequent, so the tie rules matter).  The golden file stores the result; this is how it was made."""
    rng = Lcg(seed + 1000)
    p = np.asarray([(128 + rng.below(120)) / 256.0 if c in ".?!" else rng.below(24) / 256.0 for c in doc], dtype=np.float64)
    return p.astype(dtype)


def golden_cases():
    """[(doc, predictions, known, {(min_len, max_len): sentence starts, or None where the reference raised})] of the golden file."""
    z = np.load(GOLDEN)
    meta = json.loads(str(z["meta_json"]))
    cases = []
    for d, m in enumerate(meta):
        doc = make_document(m["seed"], m["blocks"], m["kind"], m.get("lead", ""), m.get("trail", ""))
        predictions = z[f"doc{d}_predictions"]
        assert len(doc) == len(predictions) == int(z[f"doc{d}_length"]), "the text generator drifted from the golden file"
        starts = {}
        for min_len, max_len in CASES:
            key = f"doc{d}_starts_{min_len}_{max_len or 0}"
            starts[(min_len, max_len)] = None if bool(z[key + "_raised"]) else z[key].tolist()
        cases.append((doc, predictions, z[f"doc{d}_known"], starts))
    return cases


# ---- numeric documents ---------------------------------------------------------------------------------------------------------
_SPACES = np.asarray([0x20, 0x20, 0x20, 0x0A, 0x09, 0xA0, 0x2003, 0x3000, 0x85], dtype=np.uint32)
_OTHERS = np.asarray([0x61, 0x62, 0x7A, 0x2E, 0x200B, 0x180E, 0xE9, 0x4E2D, 0x1F600], dtype=np.uint32)


def numeric_document(rng: np.random.Generator, n: int, dtype=np.float64, space_rate: float = 0.2, known_rate: float = 0.0,
                     levels: int = 64):
    """(codepoints, probas, known or None) of n characters: white space at `space_rate`, probabilities in `levels` steps (ties are
    frequent), and with known_rate > 0 overrides of 0, 1 and 0.5 at that rate (NaN elsewhere)."""
    space = rng.random(n) < space_rate
    cp = np.where(space, rng.choice(_SPACES, size=n), rng.choice(_OTHERS, size=n)).astype(np.uint32)
    probas = (rng.integers(0, levels + 1, size=n) / levels).astype(dtype)
    known = None
    if known_rate > 0:
        known = np.where(rng.random(n) < known_rate, rng.choice(np.asarray([0.0, 1.0, 0.5]), size=n), np.nan)
    return cp, probas, known


def text_document(text: str, probas, dtype=np.float64, known=None):
    cp = np.frombuffer(text.encode("utf-32-le", "surrogatepass"), dtype=np.uint32)
    p = np.full(len(cp), probas, dtype=dtype) if np.isscalar(probas) else np.asarray(probas, dtype=dtype)
    assert len(p) == len(cp)
    return cp, p, known


def pack(docs):
    """[(codepoints, probas, known or None)] -> the concatenated arrays (known: None if no document has one) and doc_offsets."""
    off = np.concatenate(([0], np.cumsum([len(d[0]) for d in docs]))).astype(np.int64)
    dtype = docs[0][1].dtype if docs else np.float64
    assert all(d[1].dtype == dtype for d in docs)
    cp = np.concatenate([d[0] for d in docs]) if docs else np.zeros(0, np.uint32)
    probas = np.concatenate([d[1] for d in docs]) if docs else np.zeros(0, dtype)
    known = None
    if any(d[2] is not None for d in docs):
        known = np.concatenate([np.full(len(d[0]), np.nan) if d[2] is None else np.asarray(d[2], np.float64) for d in docs])
    return cp, probas, known, off


def host_batch(cp, probas, known, off, min_len, max_len):
    """The reference of one call: `sentence_partition` per document, in the layout of the C entry."""
    from raglite_amd._sentences import sentence_partition, whitespace_mask

    n_docs = len(off) - 1
    space = whitespace_mask(cp)
    cut = np.zeros(int(off[-1]), np.uint8)
    obj = np.zeros(n_docs, np.float64)
    status = np.zeros(n_docs, np.int32)
    for d in range(n_docs):
        b, e = int(off[d]), int(off[d + 1])
        bounds, obj[d], status[d] = sentence_partition(probas[b:e], space[b:e], min_len, max_len, None if known is None else known[b:e])
        cut[[b + k for k in bounds]] = 1
    return cut, obj, status
