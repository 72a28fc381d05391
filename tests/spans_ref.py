"""`retrieve_chunk_spans` restated on plain Python values: the yardstick of tests/test_spans_host.py and
tests/test_gpu_spans.py.

The reference function (`src/raglite/_search.py:302-361`) works on ORM objects and SQL.  Here a stored chunk is any hashable key
(a chunk id, or a chunk ordinal) and the store is a `Table`: key -> (document_id, index).  The rules, each with the line it restates:

  R1 (`:314-315`)  an empty input gives no spans.
  R2 (`:318-322`, `retrieve_chunks` `:282-299`)  a list of ids is first resolved: the store returns each chunk whose id is in the
     list once, and they are put in the order of the id's FIRST place in the list (`chunk_ids.index`); ids the store does not
     hold are not there.  A list of chunk objects is taken as it comes, duplicates included.
  R3 (`:324`)  chunk number i of that list (from 0) scores 1 / (i + 1); the scores go into a dict in list order, so of a chunk that
     comes twice the LAST score stands.
  R4 (`:327-340`)  with neighbours, every chunk of the list asks, per offset, for the chunk at (its document_id, its index + offset);
     the store returns each chunk that some condition names, once.  They are appended to the list.  They are not scored.
  R5 (`:342`)  the chunks are de-duplicated and sorted by (document_id, index): Python's tuple order, strings by code point.
  R6 (`:344-353`)  within a document, a chunk whose index is the previous chunk's index + 1 continues its span; any other starts one.
  R7 (`:356-358`)  a span's score is `sum()` over its chunks, in span order, of the chunk's score, 0.0 where it has none.  On
     CPython before 3.12 `sum()` adds left to right in IEEE doubles, which is what `left_to_right` spells out (3.12 and later
     compensate the sum; the project's contract is the plain one).
  R8 (`:355-360`)  the spans are sorted by score with `reverse=True`, which is stable: equal scores keep the (document_id, index)
     order of R5.

A span comes back as (keys in ascending index, document_id, score)."""

from __future__ import annotations

from typing import Hashable, Iterable, Sequence


class Table:
    """key -> (document_id, index) of the stored chunks, and the way back."""

    def __init__(self, positions: dict) -> None:
        self.pos = dict(positions)
        self.at = {p: key for key, p in self.pos.items()}
        assert len(self.at) == len(self.pos), "two chunks share a (document_id, index)"

    def __contains__(self, key: Hashable) -> bool:
        return key in self.pos


def left_to_right(values: Iterable[float]) -> float:
    total = 0.0
    for v in values:
        total = total + v
    return total


def resolve_ids(table: Table, ids: Sequence[Hashable]) -> list:
    """R2 for a list of ids."""
    return [key for key in dict.fromkeys(ids) if key in table]


def spans_of_chunks(table: Table, chunks: Sequence[Hashable], neighbors: Sequence[int] | None = (-1, 1)) -> list[tuple[list, str, float]]:
    """R1, R3-R8 for a list of stored chunks (the object branch; every key is in the table)."""
    if not chunks:
        return []
    score = {}
    for i, key in enumerate(chunks):
        score[key] = 1 / (i + 1)
    members = list(chunks)
    if neighbors:
        asked = {(table.pos[key][0], table.pos[key][1] + offset) for key in chunks for offset in neighbors}
        members += [table.at[p] for p in asked if p in table.at]
    ordered = sorted(set(members), key=lambda key: table.pos[key])
    spans: list[list] = []
    for key in ordered:
        document_id, index = table.pos[key]
        if spans and table.pos[spans[-1][-1]] == (document_id, index - 1):
            spans[-1].append(key)
        else:
            spans.append([key])
    scored = [(span, table.pos[span[0]][0], left_to_right(score.get(key, 0.0) for key in span)) for span in spans]
    scored.sort(key=lambda s: s[2], reverse=True)
    return scored


def spans_of_ids(table: Table, ids: Sequence[Hashable], neighbors: Sequence[int] | None = (-1, 1)) -> list[tuple[list, str, float]]:
    """The id branch: R2, then the rest."""
    return spans_of_chunks(table, resolve_ids(table, ids), neighbors)


def spans_of_entries(table: Table, entries: Sequence[Hashable], neighbors: Sequence[int] | None = (-1, 1)) -> list[tuple[list, str, float]]:
    """What rl_chunk_spans is handed: a list that may hold entries the table does not know (padding, tombstoned or out-of-range
    ordinals).  They are skipped and take no rank -- R2's "ids the store does not hold are not there" -- and the rest is taken as it
    comes (the object branch: duplicates stay)."""
    return spans_of_chunks(table, [key for key in entries if key in table], neighbors)
