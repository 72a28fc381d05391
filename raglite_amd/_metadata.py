"""Host encoding of chunk metadata for the device filters.

The reference's metadata filter is JSON containment (`src/raglite/_search.py:82-94`, `_search._matches` here): a chunk matches when,
for every key of the filter, every wanted value occurs among the chunk's values for that key, a scalar chunk value counting as a
one-element list.  A (key, value) pair is a *tag*; a chunk becomes the ascending, duplicate-free list of its tag ids, a filter the
distinct tag ids of its (key, wanted) pairs, and containment is "the chunk's list holds every tag of the filter" -- what
`rl_metadata_filters` evaluates on the device and `filter_bits_host` restates in NumPy.

Tag ids come from a dict, which gives the `==` of `in`: `1`, `1.0` and `True` are one tag, as they match each other in `_matches`.
Only values of type str, int, bool and non-NaN float are encoded.  A key under which some chunk holds anything else (None, NaN, a dict,
a nested list) is *host-only*: a filter that touches it, or that wants a value outside the four types, is not encodable and its call
takes the host path.
"""

from __future__ import annotations

import math
from typing import Any, Iterable, Sequence

import numpy as np

NO_TAG = np.iinfo(np.int32).max  # the id of a wanted value the vocabulary has never seen: no chunk carries it

_SEQUENCES = (list, tuple, set)  # what `_matches` takes as a list of values


def _encodable(value: Any) -> bool:
    t = type(value)
    return t is str or t is int or t is bool or (t is float and not math.isnan(value))


class TagVocabulary:
    """(key, value) -> int32 tag id, stable and in first-seen order (as `_keyword.Vocabulary` numbers stems), and the host-only keys."""

    def __init__(self) -> None:
        self.ids: dict[tuple, int] = {}
        self.host_only: set = set()

    def __len__(self) -> int:
        return len(self.ids)

    def add(self, key: Any, value: Any) -> int:
        tag = (key, value)
        i = self.ids.get(tag)
        if i is None:
            i = len(self.ids)
            if i >= NO_TAG:
                raise ValueError("metadata: more than 2^31-1 distinct (key, value) pairs")
            self.ids[tag] = i
        return i

    def encode_chunks(self, metadata: Iterable[dict]) -> tuple[np.ndarray, np.ndarray]:
        """The CSR of the chunks' tags: (tag_off int64 [C + 1] from 0, tags int32 [nnz]), each chunk's ids ascending and free of
        duplicates.  New pairs get the next ids (earlier ids never change); keys with a value that cannot be a tag become host-only."""
        offsets = [0]
        flat: list[int] = []
        for meta in metadata:
            ids = set()
            for key, have in (meta or {}).items():
                for value in (have if isinstance(have, _SEQUENCES) else (have,)):
                    if _encodable(value):
                        ids.add(self.add(key, value))
                    else:
                        self.host_only.add(key)
            flat.extend(sorted(ids))
            offsets.append(len(flat))
        return np.asarray(offsets, dtype=np.int64), np.asarray(flat, dtype=np.int32)

    def encode_filter(self, flt: dict) -> list[int] | None:
        """A normalised filter (`_search._adapt_metadata`: every value a list) as its distinct tag ids, ascending; a wanted value never
        seen is NO_TAG, a filter whose lists are all empty has no tags (it matches every chunk).  None: not encodable."""
        ids = set()
        for key, wanted in flt.items():
            if key in self.host_only:
                return None
            for value in wanted:
                if not _encodable(value):
                    return None
                ids.add(self.ids.get((key, value), NO_TAG))
        return sorted(ids)

    def encode_filters(self, filters: Sequence[dict]) -> tuple[np.ndarray, np.ndarray] | None:
        """The CSR of a call's distinct filters: (f_off int64 [F + 1], f_tags int32); None if one of them is not encodable."""
        offsets = [0]
        flat: list[int] = []
        for flt in filters:
            ids = self.encode_filter(flt)
            if ids is None:
                return None
            flat.extend(ids)
            offsets.append(len(flat))
        return np.asarray(offsets, dtype=np.int64), np.asarray(flat, dtype=np.int32)


def filter_bits_host(tag_off, tags, f_off, f_tags) -> np.ndarray:
    """What `rl_metadata_filters` computes, in NumPy: uint32 [F x (C + 31) // 32], bit c of row j set iff chunk c's tags hold every tag
    of filter j (the layout of `chunk_filters`; the bits past C are zero)."""
    tag_off = np.asarray(tag_off, dtype=np.int64)
    tags = np.asarray(tags, dtype=np.int32)
    f_off = np.asarray(f_off, dtype=np.int64)
    f_tags = np.asarray(f_tags, dtype=np.int32)
    C, F = tag_off.size - 1, f_off.size - 1
    chunk_of = np.repeat(np.arange(C, dtype=np.int64), np.diff(tag_off))
    words = (C + 31) // 32
    out = np.zeros((F, words), dtype=np.uint32)
    for j in range(F):
        match = np.ones(C, dtype=bool)
        for t in f_tags[f_off[j] : f_off[j + 1]]:
            match &= np.bincount(chunk_of[tags == t], minlength=C) > 0
        padded = np.zeros(words * 32, dtype=np.uint8)
        padded[:C] = match
        out[j] = np.packbits(padded, bitorder="little").view(np.uint32)
    return out


def filter_counts_host(bits: np.ndarray, rows_per_chunk) -> tuple[np.ndarray, np.ndarray]:
    """(matching chunks int64 [F], their embedding rows int64 [F]) of `filter_bits_host`'s table: `rl_metadata_filters`' two counts."""
    rows = np.asarray(rows_per_chunk, dtype=np.int64)
    on = np.unpackbits(np.ascontiguousarray(bits).view(np.uint8), axis=1, bitorder="little")[:, : rows.size].astype(bool)
    return on.sum(axis=1).astype(np.int64), (on * rows[None, :]).sum(axis=1).astype(np.int64)
