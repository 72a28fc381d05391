"""Tests-only restatements of BM25 keyword search (DESIGN.md "Keyword search"): what the device must return, in NumPy.

- `impacts_f32` / `scores_f32` / `topk_f32`: the float32 arithmetic of raglite_amd/csrc/keyword.hip, step by step (every NumPy
  float32 operation is one IEEE rounding, as `__fmul_rn` / `__fdiv_rn` / `__fadd_rn` on the device), so results compare bitwise.
- `bm25_f64`: BM25 from dictionaries in float64, straight from the formula, with no postings at all: the check of the restatement.
- `zipf_corpus` / `zipf_queries`: seeded pre-tokenised corpora (term ids) for the GPU tests and scripts/bench_keyword.py.
Nothing under raglite_amd/ imports this module.
"""

from __future__ import annotations

import math
from collections import Counter

import numpy as np

from raglite_amd import _keyword

NEG_INF = np.float32(-np.inf)


def impacts_f32(p: _keyword.Postings) -> np.ndarray:
    tf = p.post_tf.astype(np.float32)
    k1p1 = np.float32(_keyword.K1) + np.float32(1.0)
    return p.idf[p.post_term] * ((tf * k1p1) / (tf + p.nrm[p.post_chunk]))


def scores_f32(p: _keyword.Postings, impacts: np.ndarray, query_ids) -> np.ndarray:
    """Chunk scores of one query: impacts summed in ascending term id order from the first one; -inf where no term occurs."""
    s = np.full(p.n_chunks, NEG_INF, dtype=np.float32)
    for t in sorted(set(int(t) for t in query_ids)):
        if not 0 <= t < p.n_terms:
            continue
        a, b = int(p.term_off[t]), int(p.term_off[t + 1])
        c, v = p.post_chunk[a:b], impacts[a:b]
        cur = s[c]
        s[c] = np.where(cur == NEG_INF, v, cur + v)
    return s


def topk_f32(scores: np.ndarray, k: int, allowed: np.ndarray | None = None) -> tuple[np.ndarray, np.ndarray]:
    """(scores, chunk ordinals) of the best k finite scores by (score desc, ordinal asc)."""
    s = scores if allowed is None else np.where(allowed, scores, NEG_INF)
    order = np.lexsort((np.arange(s.size), -s))
    order = order[np.isfinite(s[order])][:k]
    return s[order], order.astype(np.int32)


def bm25_f64(chunk_stems, query: list[str]) -> dict[int, float]:
    """ordinal -> score for every live chunk (stems not None) containing a query stem; float64 from the formula."""
    live = [i for i, st in enumerate(chunk_stems) if st is not None]
    n = len(live)
    avgdl = sum(len(chunk_stems[i]) for i in live) / n if n else 0.0
    df: Counter = Counter()
    for i in live:
        df.update(set(chunk_stems[i]))
    out: dict[int, float] = {}
    for i in live:
        tf = Counter(chunk_stems[i])
        nrm = _keyword.K1 * (1 - _keyword.B + _keyword.B * (len(chunk_stems[i]) / avgdl if avgdl else 0.0))
        terms = [t for t in set(query) if t in tf]
        if terms:
            out[i] = sum(math.log(1 + (n - df[t] + 0.5) / (df[t] + 0.5)) * tf[t] * (_keyword.K1 + 1) / (tf[t] + nrm) for t in terms)
    return out


def zipf_corpus(rng: np.random.Generator, n_chunks: int, n_terms: int, mean_len: int, a: float = 1.1):
    """(flat term ids, offsets): chunk lengths uniform in [0, 2 mean_len] (so some chunks are empty), term ids Zipf(a) ranks
    folded into the vocabulary (term 0 is the most frequent)."""
    lengths = rng.integers(0, 2 * mean_len + 1, size=n_chunks)
    offsets = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    return ((rng.zipf(a, size=int(offsets[-1])) - 1) % n_terms).astype(np.int64), offsets


def zipf_queries(rng: np.random.Generator, n_queries: int, n_terms: int, lo: int = 1, hi: int = 12, a: float = 1.1) -> list[np.ndarray]:
    """Queries of lo..hi term ids: half Zipf-drawn like the corpus (common terms, long postings), half uniform (mostly rare terms,
    some absent from the corpus); repeats are allowed (the search drops them)."""
    out = []
    for _ in range(n_queries):
        m = int(rng.integers(lo, hi + 1))
        common = (rng.zipf(a, size=m - m // 2) - 1) % n_terms
        rare = rng.integers(0, n_terms, size=m // 2)
        out.append(np.concatenate([common, rare]).astype(np.int32))
    return out
