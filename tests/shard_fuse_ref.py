"""NumPy restatement of `rl_shard_hybrid_fuse` (include/raglite_hip.h), query by query, for the tests.

Records per query: every rank's num_hits rows (score f32 bits, global row, global chunk) and, with keywords, n_each keyword records
(score f32 bits, global chunk); an id < 0 is padding.  Rows merged by (score desc, row asc; NaN after -inf, -0.0 below +0.0: the
device's order-preserving float key), the first num_hits real ones; the first hit of each chunk among them, up to n_each; the keyword
records merged by (score desc, chunk asc), the first n_each; then weighted RRF (tests/rrf_ref.py).  A SHARD_MISSING record poisons the
query (NaN, -1, count 0).
"""

from __future__ import annotations

import numpy as np

from tests import rrf_ref

SHARD_MISSING = -2


def _desc_key(score: np.float32) -> int:
    """Larger = better: the device's score_key (every NaN ranks below -inf)."""
    u = int(np.asarray(score, np.float32).view(np.uint32))
    if (u & 0x7FFFFFFF) > 0x7F800000:
        return 0
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def _ranked(scores: np.ndarray, ids: np.ndarray, extra: np.ndarray | None = None) -> list[tuple]:
    out = [(-_desc_key(s), int(i), None if extra is None else int(x))
           for s, i, x in zip(scores, ids, extra if extra is not None else ids) if int(i) >= 0]
    return sorted(out)


def fuse(gathered, *, num_hits: int, n_each: int, keywords: bool, weights, rrf_k: int = 60, k: int):
    g = np.asarray(gathered, dtype=np.int32)
    world, B, W = g.shape
    assert W == 3 * num_hits + (2 * n_each if keywords else 0)
    R = 2 if keywords else 1
    w = list(np.asarray(weights, np.float64).ravel()[:R])
    scores = np.full((B, k), -np.inf)
    ids = np.full((B, k), -1, np.int32)
    counts = np.zeros(B, np.int32)
    for b in range(B):
        rows = g[:, b, : 3 * num_hits].reshape(world * num_hits, 3)
        kw = g[:, b, 3 * num_hits :].reshape(world * n_each, 2) if keywords else np.zeros((0, 2), np.int32)
        if (rows[:, 1:] == SHARD_MISSING).any() or (kw[:, 1] == SHARD_MISSING).any():
            scores[b], ids[b], counts[b] = np.nan, -1, 0
            continue
        top = _ranked(rows[:, 0].view(np.float32), rows[:, 1], rows[:, 2])[:num_hits]
        seen, vec = set(), []
        for _, _, c in top:
            if c >= 0 and c not in seen:
                seen.add(c)
                vec.append(c)
        vec = vec[:n_each]
        lists = [vec + [-1] * (n_each - len(vec))]
        if keywords:
            kl = [i for _, i, _ in _ranked(kw[:, 0].view(np.float32), kw[:, 1])[:n_each]]
            lists.append(kl + [-1] * (n_each - len(kl)))
        o, s = rrf_ref.fuse_one(np.asarray(lists), w, rrf_k)
        n = min(k, o.size)
        ids[b, :n], scores[b, :n], counts[b] = o[:n], s[:n], n
    return scores, ids, counts


def random_records(rng: np.random.Generator, world: int, B: int, num_hits: int, n_each: int, keywords: bool, *, pad: float = 0.15,
                   rows_per_chunk: int = 3) -> np.ndarray:
    """(world, B, W) records: integer-valued scores (ties within and across ranks), distinct rows per query spread over the ranks, several
    rows (on several ranks) per chunk, a few NaN scores, padding (-1) anywhere."""
    W = 3 * num_hits + (2 * n_each if keywords else 0)
    g = np.zeros((world, B, W), np.int32)
    n = world * num_hits
    for b in range(B):
        rows = rng.permutation(4 * n)[:n].reshape(world, num_hits)
        sc = rng.integers(-4, 5, size=(world, num_hits)).astype(np.float32)
        sc[rng.random(sc.shape) < 0.02] = np.nan
        chunk = rows // rows_per_chunk
        dead = rng.random(rows.shape) < pad
        rows, chunk = np.where(dead, -1, rows), np.where(dead, -1, chunk)
        sc = np.where(dead, np.float32(-np.inf), sc).astype(np.float32)
        rec = np.stack([sc.view(np.int32), rows, chunk], axis=-1).reshape(world, 3 * num_hits)
        g[:, b, : 3 * num_hits] = rec
        if keywords:
            kc = rng.permutation(max(2 * world * n_each, 8))[: world * n_each].reshape(world, n_each)
            ks = rng.integers(0, 6, size=kc.shape).astype(np.float32) * np.float32(0.5)
            kdead = rng.random(kc.shape) < pad
            kc = np.where(kdead, -1, kc)
            ks = np.where(kdead, np.float32(-np.inf), ks).astype(np.float32)
            g[:, b, 3 * num_hits :] = np.stack([ks.view(np.int32), kc], axis=-1).reshape(world, 2 * n_each)
    return g
