"""NumPy restatement of the rerank order (include/raglite_hip.h `rl_rerank_order`).

Per query: n_cand (score, candidate) pairs, a candidate < 0 being padding.  The real candidates are ordered as `MaxSimRanker.rank`
orders its docs -- `np.lexsort((arange, -key))`, key = where(isnan(s), -inf, s): score descending, NaN as -inf, -0.0 equal to +0.0,
equal keys by position -- and padding comes last, uncounted.  The first k are returned with the score's own bits.
"""

from __future__ import annotations

import numpy as np

NAN_A, NAN_B = 0x7FC00000, 0xFFC00001  # two quiet NaNs: different sign and payload


def score_pool() -> np.ndarray:
    """The values the adversarial lists draw from: ties are common, and every special case of the order is in it."""
    bits = np.array([NAN_A, NAN_B], dtype=np.uint32).view(np.float32)
    tiny = np.array([1, 0x80000001], dtype=np.uint32).view(np.float32)  # +/- the smallest denormal: not zero
    vals = np.array([np.inf, -np.inf, 0.0, -0.0, -1.5, -0.25, 0.25, 1.0, 1.0000001, 3.0], dtype=np.float32)
    return np.concatenate([bits, tiny, vals])


def order_one(scores: np.ndarray, candidates: np.ndarray) -> np.ndarray:
    """The positions of one query's real candidates, best first."""
    scores = np.asarray(scores, dtype=np.float32)
    pos = np.nonzero(np.asarray(candidates) >= 0)[0]
    s = scores[pos]
    key = np.where(np.isnan(s), -np.inf, s)
    return pos[np.lexsort((np.arange(len(pos)), -key))]


def order(scores: np.ndarray, candidates: np.ndarray, k: int):
    """scores / candidates (B, n_cand) -> (scores (B, k) float32, candidates (B, k) int32, positions (B, k) int32, counts (B,) int32);
    unfilled slots (-inf, -1, -1)."""
    scores = np.asarray(scores, dtype=np.float32)
    candidates = np.asarray(candidates, dtype=np.int32)
    B = scores.shape[0]
    out_s = np.full((B, k), -np.inf, dtype=np.float32)
    out_c = np.full((B, k), -1, dtype=np.int32)
    out_p = np.full((B, k), -1, dtype=np.int32)
    counts = np.zeros(B, dtype=np.int32)
    for b in range(B):
        p = order_one(scores[b], candidates[b])[:k]
        n = len(p)
        out_s[b, :n], out_c[b, :n], out_p[b, :n], counts[b] = scores[b, p], candidates[b, p], p, n
    return out_s, out_c, out_p, counts


def adversarial(rng, B: int, n_cand: int, *, pad: float = 0.3, universe: int = 1000):
    """(scores (B, n_cand) float32 from score_pool(), candidates (B, n_cand) int32 with padding anywhere at rate `pad`)."""
    pool = score_pool()
    scores = pool[rng.integers(0, len(pool), size=(B, n_cand))]
    candidates = rng.integers(0, universe, size=(B, n_cand)).astype(np.int32)
    candidates[rng.random((B, n_cand)) < pad] = -1
    return np.ascontiguousarray(scores), candidates


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)
