"""What the tests of the Markdown block parser share: the fixture, the reduction of markdown-it's tokens to the two per-line arrays the
device writes, the host statements of the two derived arrays on top of those arrays, and the predicate that allows UNDECIDED."""

from __future__ import annotations

import functools
import json
import struct
from pathlib import Path
from typing import Sequence

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden" / "markdown_blocks.json"
FIRST_OPEN = {"heading_open": 1, "blockquote_open": 2, "paragraph_open": 3, "bullet_list_open": 4, "ordered_list_open": 5}
PROBA = {0: 0.0, 1: 1.0, 2: 0.75, 3: 0.5, 4: 0.25, 5: 0.25}
OK, UNDECIDED = 0, 1
_TRIGGERS = "<[\t\x0b\x0c\x1c\x1d\x1e\x85\u2028\u2029"


@functools.lru_cache(maxsize=1)
def fixture() -> dict:
    return json.loads(GOLDEN.read_text())


def cases(group: str | None = None) -> list[dict]:
    data = fixture()
    return [c for g in (("hand", "edges", "fuzz_a", "fuzz_b") if group is None else (group,)) for c in data[g]]


def may_be_undecided(text: str) -> bool:
    return any(ch in text for ch in _TRIGGERS)


def line_starts(text: str) -> list[int]:
    """The start of every `str.splitlines` line, and len(text) behind the last."""
    out = [0]
    for line in text.splitlines(keepends=True):
        out.append(out[-1] + len(line))
    return out


def reduce_tokens(tokens: Sequence[Sequence], n_lines: int) -> tuple[np.ndarray, np.ndarray]:
    """(first_open uint8[n_lines], heading_end int32[n_lines]) of a token list of [type, map0, map1] in markdown-it's order."""
    first_open = np.zeros(n_lines, np.uint8)
    heading_end = np.zeros(n_lines, np.int32)
    for kind, begin, end in tokens:
        code = FIRST_OPEN.get(kind)
        if code is None:
            continue
        if first_open[begin] == 0:
            first_open[begin] = code
        if code == 1:
            assert heading_end[begin] == 0, "two headings start on one line"
            heading_end[begin] = end
    return first_open, heading_end


def known_from_lines(text: str, heading_end: np.ndarray) -> np.ndarray:
    """`markdown_sentence_boundaries` from heading_end alone."""
    start_of = line_starts(text)
    probas = np.full(len(text), np.nan)
    for line in np.flatnonzero(heading_end).tolist():
        start, end = start_of[line], start_of[int(heading_end[line])] + 1
        if 0 <= start - 1 < len(probas):
            probas[start - 1] = 1
        probas[start:end - 1] = 0
        if 0 <= end - 1 < len(probas):
            probas[end - 1] = 1
    return probas


def boundaries_from_lines(sentences: Sequence[str], first_open: np.ndarray) -> np.ndarray:
    """`markdown_chunklet_boundaries` from first_open alone."""
    n = len(sentences)
    probas = np.zeros(n)
    if n == 0:
        return probas
    text = "".join(sentences)
    start_of = np.asarray(line_starts(text)[:-1], np.int64) if text else np.zeros(0, np.int64)
    sentence_start = np.concatenate(([0], np.cumsum([len(s) for s in sentences], dtype=np.int64))).astype(np.int64)
    line_sentence = np.searchsorted(sentence_start, start_of, side="right") - 1
    seen = set()
    for line in np.flatnonzero(first_open[:len(start_of)]).tolist():
        i = int(line_sentence[line])
        if i not in seen:
            seen.add(i)
            probas[i] = PROBA[int(first_open[line])]
    marked = np.concatenate(([False], probas != 0.0, [False]))
    edges = np.flatnonzero(marked[1:] != marked[:-1])
    for begin, end in zip(edges[0::2].tolist(), edges[1::2].tolist()):
        if end - begin > 1:
            keep = begin + int(np.argmax(probas[begin:end]))
            value = probas[keep]
            probas[begin:end] = 0.0
            probas[keep] = value
    return probas


def random_sentences(text: str, rng: np.random.Generator) -> list[str]:
    """The text cut at random positions (most of them inside lines); some cuts repeat, which gives empty sentences."""
    if not text:
        return []
    cuts = np.sort(rng.integers(0, len(text) + 1, size=int(rng.integers(0, max(2, len(text) // 6)))))
    edges = [0, *cuts.tolist(), len(text)]
    return [text[a:b] for a, b in zip(edges[:-1], edges[1:])]


def write_driver_input(path: Path, texts: Sequence[str]) -> None:
    """The input file of tests/c/markdown_blocks_main.cpp."""
    offsets = np.concatenate(([0], np.cumsum([len(t) for t in texts]))).astype(np.int64)
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(texts)))
        f.write(offsets.tobytes())
        f.write("".join(texts).encode("utf-32-le", "surrogatepass"))


def read_driver_output(out: str) -> list[tuple[int, np.ndarray, np.ndarray]]:
    lines = out.split("\n")
    docs = []
    for k in range(0, len(lines) - 1, 3):
        status, n_lines = (int(v) for v in lines[k].split())
        first_open = np.asarray(lines[k + 1].split(), dtype=np.int64).astype(np.uint8)
        heading_end = np.asarray(lines[k + 2].split(), dtype=np.int64).astype(np.int32)
        assert len(first_open) == n_lines and len(heading_end) == n_lines
        docs.append((status, first_open, heading_end))
    return docs
