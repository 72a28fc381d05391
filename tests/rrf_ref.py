"""NumPy restatement of the weighted RRF contract (include/raglite_hip.h `rl_rrf_fuse`, DESIGN.md "Batched hybrid search").

Per query: R ranked lists of chunk ordinals padded with entries < 0.  Rank i of an entry = the results before it in its list.  An
ordinal's score = float64 sum of w_r / (rrf_k + i) over its occurrences in concatenation order, from +0.0; order = score descending,
ties by first occurrence in list 0 || list 1 || ...
"""

from __future__ import annotations

import numpy as np


def fuse_one(rows: np.ndarray, weights, rrf_k: int) -> tuple[np.ndarray, np.ndarray]:
    """rows (R, len) int -> (ordinals, float64 scores), the whole fused list of one query."""
    rows = np.asarray(rows, dtype=np.int64)
    R, L = rows.shape
    valid = rows >= 0
    rank = np.cumsum(valid, axis=1) - valid  # results before each entry in its list
    w = np.asarray(weights, dtype=np.float64)
    terms = w[:, None] / (np.float64(rrf_k) + rank)  # one IEEE division per entry
    flat_ord, flat_term = rows.ravel()[valid.ravel()], terms.ravel()[valid.ravel()]
    pos = np.arange(R * L)[valid.ravel()]
    order = np.lexsort((pos, flat_ord))  # occurrences of an ordinal together, in concatenation order
    ords, first, scores = [], [], []
    for j in order:
        if not ords or ords[-1] != flat_ord[j]:
            ords.append(int(flat_ord[j]))
            first.append(int(pos[j]))
            scores.append(np.float64(0.0))
        scores[-1] = scores[-1] + flat_term[j]  # sequential, from +0.0
    if not ords:
        return np.zeros(0, np.int64), np.zeros(0, np.float64)
    sc = np.asarray(scores, dtype=np.float64)
    out = np.lexsort((np.asarray(first), -sc))  # score descending, then first occurrence
    return np.asarray(ords, dtype=np.int64)[out], sc[out]


def fuse(lists: np.ndarray, weights, rrf_k: int, k: int):
    """lists (R, B, len) -> (scores (B, k) float64, ordinals (B, k) int32, counts (B,)), unfilled slots (-inf, -1)."""
    lists = np.asarray(lists)
    R, B, L = lists.shape
    scores = np.full((B, k), -np.inf)
    ids = np.full((B, k), -1, dtype=np.int32)
    counts = np.zeros(B, dtype=np.int32)
    for b in range(B):
        o, s = fuse_one(lists[:, b, :], weights, rrf_k)
        n = min(k, o.size)
        ids[b, :n], scores[b, :n], counts[b] = o[:n], s[:n], n
    return scores, ids, counts


def random_lists(rng, R: int, B: int, L: int, *, universe: int | None = None, pad: float = 0.2, repeats: bool = True) -> np.ndarray:
    """(R, B, len) ordinals drawn from a small universe (so that the lists overlap), padding anywhere in a list."""
    universe = universe or max(2, (R * L) // 2)
    lists = rng.integers(0, universe, size=(R, B, L)).astype(np.int32)
    if not repeats:
        for r in range(R):
            for b in range(B):
                lists[r, b] = rng.permutation(max(universe, L))[:L]
    lists[rng.random(lists.shape) < pad] = -1
    return lists


def tie_lists(B: int, L: int) -> np.ndarray:
    """Two lists with disjoint ordinals at the same ranks: with equal weights every pair of scores ties exactly."""
    a = np.tile(np.arange(L, dtype=np.int32), (B, 1))
    return np.stack([a, a + L])
