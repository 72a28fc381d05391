"""Shared inputs of the chunklet tests: a deterministic Markdown text generator (the documents of `tests/golden/split_chunklets.npz`
are described by its parameters, not stored), numeric documents for the device tests, and the layout helpers of
`rl_partition_chunklets`.  Uses no random-number library: the generator is a 64-bit LCG, so the texts never drift."""

import json
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden" / "split_chunklets.npz"
MAX_SIZES = (64, 512, 2048)

_WORDS = ("kernel", "wave", "tile", "memory", "bandwidth", "retrieval", "index", "vector", "query", "chunk", "of", "the", "a", "and",
          "to", "in", "is", "for", "with", "latency", "throughput", "cache", "segment", "document")

# seed, sentences, kind -- kind "mixed": headings, paragraphs, lists, quotes; "prose": paragraphs only; "lists": mostly list items of
# one to three words; "same": identical sentences in one paragraph (exact ties); long_at: sentences padded to 600+ characters
DOCUMENTS = (
    {"seed": 1, "n": 1, "kind": "mixed"},
    {"seed": 2, "n": 2, "kind": "mixed"},
    {"seed": 3, "n": 5, "kind": "mixed"},
    {"seed": 4, "n": 30, "kind": "mixed"},
    {"seed": 5, "n": 80, "kind": "mixed"},
    {"seed": 6, "n": 150, "kind": "mixed"},
    {"seed": 7, "n": 300, "kind": "mixed"},
    {"seed": 8, "n": 60, "kind": "same"},
    {"seed": 9, "n": 40, "kind": "mixed", "long_at": [20]},
    {"seed": 10, "n": 40, "kind": "prose", "long_at": [0, 39]},
    {"seed": 11, "n": 120, "kind": "lists"},
    {"seed": 12, "n": 200, "kind": "prose"},
)


class Lcg:
    """Knuth's 64-bit linear congruential generator; `below(k)` takes the high bits."""

    def __init__(self, seed: int) -> None:
        self.x = (seed * 0x9E3779B97F4A7C15 + 1) & 0xFFFFFFFFFFFFFFFF

    def below(self, k: int) -> int:
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        return (self.x >> 33) % k


def _phrase(rng: Lcg, lo: int, hi: int) -> str:
    return " ".join(_WORDS[rng.below(len(_WORDS))] for _ in range(lo + rng.below(hi - lo + 1)))


def make_sentences(seed: int, n: int, kind: str = "mixed", long_at=()) -> list[str]:
    """n non-empty sentences whose concatenation is a Markdown document; a sentence keeps its trailing white space, and a paragraph's
    sentences share lines, so sentence and line boundaries differ."""
    rng = Lcg(seed)
    out: list[str] = []
    if kind == "same":
        out = ["The same words again. "] * n
    while len(out) < n:
        block = rng.below(10) if kind == "mixed" else (9 if kind == "prose" else rng.below(4))
        if kind == "lists":
            items = 2 + rng.below(5)
            mark = rng.below(2)
            for k in range(items):
                out.append((f"{k + 1}. " if mark else "- ") + _phrase(rng, 1, 3) + ("\n\n" if k == items - 1 else "\n"))
            if block == 0:
                out.append(_phrase(rng, 2, 6).capitalize() + ".\n\n")
        elif block == 0:
            out.append("#" * (1 + rng.below(3)) + " " + _phrase(rng, 1, 4).capitalize() + "\n\n")
        elif block == 1:
            items = 2 + rng.below(4)
            for k in range(items):
                out.append("- " + _phrase(rng, 2, 9) + ("\n\n" if k == items - 1 else "\n"))
        elif block == 2:
            items = 2 + rng.below(3)
            for k in range(items):
                out.append(f"{k + 1}. " + _phrase(rng, 2, 9) + ("\n\n" if k == items - 1 else "\n"))
        elif block == 3:
            out.append("> " + _phrase(rng, 4, 14).capitalize() + ".\n\n")
        else:
            count = 1 + rng.below(6)
            for k in range(count):
                out.append(_phrase(rng, 3, 28).capitalize() + (".\n\n" if k == count - 1 else ". "))
    out = out[:n]
    for i in long_at:
        out[i] = _phrase(rng, 110, 120).capitalize() + " " + out[i]
    return out


def golden_cases():
    """[(sentences, boundary, statements, lengths, {max_size: cuts})] of the golden file, the texts regenerated."""
    z = np.load(GOLDEN)
    meta = json.loads(str(z["meta_json"]))
    cases = []
    for d, m in enumerate(meta):
        sentences = make_sentences(m["seed"], m["n"], m["kind"], m.get("long_at", ()))
        lengths = z[f"doc{d}_lengths"]
        assert [len(s) for s in sentences] == lengths.tolist(), "the text generator drifted from the golden file"
        cases.append((sentences, z[f"doc{d}_boundary"], z[f"doc{d}_statements"], lengths,
                      {ms: z[f"doc{d}_cuts_{ms}"].tolist() for ms in MAX_SIZES}))
    return cases


# ---- numeric documents ---------------------------------------------------------------------------------------------------------
def numeric_document(rng: np.random.Generator, n: int, max_len: int = 200, same: bool = False):
    """(boundary, statements, lengths) of n sentences in the value ranges of the two host mirrors; same: identical sentences."""
    if same:
        return np.zeros(n), np.full(n, 1.0), np.full(n, int(rng.integers(1, max_len + 1)), np.int64)
    boundary = rng.choice(np.asarray([0.0, 0.0, 0.0, 0.25, 0.5, 0.75, 1.0]), size=n)
    statements = np.round(rng.random(n) * 2.0, 3)
    return boundary, statements, rng.integers(1, max_len + 1, size=n).astype(np.int64)


def pack(docs):
    """[(boundary, statements, lengths)] -> the concatenated arrays and doc_offsets of one call."""
    off = np.concatenate(([0], np.cumsum([len(d[2]) for d in docs]))).astype(np.int64)
    cat = lambda k, dt: np.concatenate([np.asarray(d[k], dt) for d in docs]) if docs else np.zeros(0, dt)  # noqa: E731
    return cat(0, np.float64), cat(1, np.float64), cat(2, np.int64), off


def host_batch(boundary, statements, lengths, off, max_size):
    """The reference of one call: `chunklet_dp` per document, in the layout of the C entry."""
    from raglite_amd._chunklets import chunklet_dp

    n_docs = len(off) - 1
    cut = np.zeros(int(off[-1]), np.uint8)
    obj = np.zeros(n_docs, np.float64)
    status = np.zeros(n_docs, np.int32)
    for d in range(n_docs):
        b, e = int(off[d]), int(off[d + 1])
        cuts, obj[d], status[d] = chunklet_dp(boundary[b:e], statements[b:e], lengths[b:e], max_size)
        cut[[b + c - 1 for c in cuts]] = 1
    return cut, obj, status
