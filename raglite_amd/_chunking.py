"""Host mirror of `src/raglite/_split_chunks.py` with the arithmetic on the GPU.

    split_chunks(chunklets, chunklet_embeddings, max_size=2048) -> (chunks, chunk_embeddings)   (`_split_chunks.py:13-122`)
    split_chunks_batch(documents, embeddings, max_size=2048) -> the same per document, all documents in ONE device call

This is the step between a1-a3 (pooled chunklet embeddings) and a4 (the contiguous row spans that make a chunk a
multi-vector object, `np.split(chunklet_embeddings, partition_indices)`).  What runs on the device: row normalisation,
discourse-vector removal and the similarity of consecutive chunklets (`:54-72`, `rl_partition_similarity`), and -- through
`rl_split_chunks` / `rl_partition_chunks` -- the Markdown-heading adjustments (`:73-86`) and the partition itself (`:87-113`),
solved exactly as a shortest path instead of a MILP (`partition_dp` below is the host statement of that recurrence).  What stays
on the host: string lengths and their 15 % / 85 % quantiles, the heading regex, joining the strings -- and, for the default
`split_chunks(partition="milp")`, the binary integer programme with scipy's HiGHS, as in the reference.
"""

from __future__ import annotations

import ctypes as C
import re
from typing import Any, Sequence

import numpy as np

from raglite_amd import _ops
from raglite_amd._abi import check, lib

_HEADING = re.compile(r"^#+\s")


def _nonoutlying(sizes: np.ndarray) -> np.ndarray:
    q15, q85 = np.quantile(sizes, [0.15, 0.85])  # `_split_chunks.py:57-58`
    return ((q15 <= sizes) & (sizes <= q85)).astype(np.uint8)


def partition_similarities(embeddings: Any, doc_offsets: np.ndarray, chunklet_sizes: np.ndarray) -> Any:
    """Similarities of consecutive chunklets for MANY documents in one launch.

    embeddings: (N, dim) NumPy array or CUDA tensor, the documents' chunklet embeddings concatenated;
    doc_offsets: int64[n_docs + 1]; chunklet_sizes: int64[N] string lengths.  Returns float32[N] on the same side as
    `embeddings` (entry i = chunklets i and i+1 of one document; 0 at every document's last chunklet)."""
    off = np.ascontiguousarray(doc_offsets, dtype=np.int64)
    sizes = np.asarray(chunklet_sizes)
    sel = np.concatenate([_nonoutlying(sizes[off[d] : off[d + 1]]) if off[d + 1] > off[d] else np.zeros(0, np.uint8)
                          for d in range(len(off) - 1)]) if len(off) > 1 else np.zeros(0, np.uint8)
    a = _ops._Args()  # noqa: SLF001
    x, p_x = a.inp(embeddings, np.float32)
    n, dim = int(x.shape[0]), int(x.shape[1])
    if n != int(off[-1]) or len(sel) != n:
        raise ValueError("doc_offsets / chunklet_sizes do not match the embedding rows")
    _, p_off = a.same_side(off, np.int64)
    _, p_sel = a.same_side(sel, np.uint8)
    out, p_out = a.out((n,), np.float32)
    a.ensure_device()
    check(lib().rl_partition_similarity(p_x, n, dim, p_off, len(off) - 1, p_sel, p_out, a.mem, a.stream))
    return out


def _apply_headings(sim: np.ndarray, chunklets: Sequence[str]) -> np.ndarray:
    """`_split_chunks.py:73-86`."""
    prev_is_heading = True
    for i, chunklet in enumerate(chunklets[:-1]):
        is_heading = bool(_HEADING.match(chunklet.replace("\n", "").strip()))
        if is_heading:
            if not prev_is_heading:
                sim[i - 1] = sim[i - 1] / 4  # encourage a split before the heading
            sim[i] = 1.0  # never split right after it
        prev_is_heading = is_heading
    return sim


def _solve_partition(cost: np.ndarray, sizes: np.ndarray, max_size: int) -> list[int]:
    """`_split_chunks.py:87-113`: minimise cost . x over binary x (x[i] = split after chunklet i) such that every
    window of chunklets that overflows `max_size` contains a split."""
    from scipy.optimize import linprog
    from scipy.sparse import coo_matrix

    csum = np.cumsum(sizes)
    starts = np.concatenate(([0], csum[:-1]))
    n = len(sizes)
    # first chunklet index (exclusive end) whose inclusion overflows a chunk starting at i
    ends = np.searchsorted(csum, starts[: n - 1] + max_size, side="right")
    rows_needed = int(np.argmax(ends == n)) if np.any(ends == n) else n - 1  # the reference stops at the first fit
    rows, cols = [], []
    for i in range(rows_needed):
        span = np.arange(i, ends[i])
        rows.append(np.full(len(span), i))
        cols.append(span)
    if not rows:
        return []
    A = coo_matrix((np.ones(sum(len(r) for r in rows), np.float32), (np.concatenate(rows), np.concatenate(cols))),  # noqa: N806
                   shape=(rows_needed, n - 1), dtype=np.float32)
    res = linprog(cost, A_ub=-A, b_ub=-np.ones(A.shape[0], np.float32), bounds=(0, 1), integrality=[1] * A.shape[1])
    if not res.success:
        raise ValueError("Optimization of chunk partitions failed.")
    return (np.where(res.x)[0] + 1).tolist()


def _heading_flags(chunklets: Sequence[str]) -> np.ndarray:
    """uint8[n]: chunklet i is a Markdown heading (the test of `_apply_headings`, `_split_chunks.py:76`)."""
    return np.fromiter((bool(_HEADING.match(c.replace("\n", "").strip())) for c in chunklets), dtype=np.uint8, count=len(chunklets))


def apply_headings_elementwise(sim: np.ndarray, is_heading: np.ndarray) -> np.ndarray:
    """`_apply_headings` without its loop-carried state, as `ps_headings_kernel` computes it.  sim float32[n - 1] of one document,
    is_heading uint8[n] (the last chunklet's flag is never read).  Entry i becomes 1 if chunklet i is a heading (the later division
    needs "previous is no heading"), sim[i] / 4 if it is none and chunklet i + 1 <= n - 2 is one, and stays otherwise."""
    sim = np.asarray(sim, dtype=np.float32)
    m = len(sim)
    head = np.asarray(is_heading[:m]).astype(bool)
    next_head = np.concatenate((head[1:], [False]))
    return np.where(head, np.float32(1.0), np.where(next_head, sim / np.float32(4), sim)).astype(np.float32)


_I64_MAX = np.iinfo(np.int64).max
PARTITION_OK, PARTITION_TOO_LARGE, PARTITION_NOT_FINITE = 0, 1, 2


def partition_dp(cost: np.ndarray, sizes: np.ndarray, max_size: int) -> tuple[list[int], float, int]:
    """The optimal partition of ONE document as a shortest path: the host statement of `partition_dp.hip`, same bits.

    `_solve_partition`'s programme has a window [i, end[i]) for every i < W that must hold a split; the ends ascend, so with
    g[j] = cost of the cheapest feasible set of splits whose last one is j,
        g[j] = float64(cost[j]) + min(g[p] for the admissible p < j; 0.0 for "no predecessor" when end[0] > j)
    where p is admissible when no window lies between p and j (p + 1 >= W or end[p + 1] > j): the range [lo(j), j - 1], lo
    non-decreasing.  The last split is the cheapest p >= W - 1.  Ties: "no predecessor" before an equal p, then the smallest p.
    Returns (split indices as `_solve_partition` returns them, objective, status); status 1: a size > max_size, 2: a non-finite
    cost (then no splits and objective NaN)."""
    s = np.asarray(sizes, dtype=np.int64).reshape(-1)
    n = len(s)
    m = max(n - 1, 0)
    c = np.asarray(cost, dtype=np.float32).reshape(-1)
    if max_size < 1 or np.any(s < 0) or len(c) < m:
        raise ValueError("partition_dp: max_size >= 1, sizes >= 0 and len(cost) >= len(sizes) - 1 are required")
    c = c[:m]
    if np.any(s > max_size):
        return [], float("nan"), PARTITION_TOO_LARGE
    if not np.all(np.isfinite(c)):
        return [], float("nan"), PARTITION_NOT_FINITE
    if n <= 1:
        return [], 0.0, PARTITION_OK
    csum = np.cumsum(s)
    starts = np.concatenate(([0], csum[:-1]))[:m]
    room = min(int(max_size), _I64_MAX)
    ends = np.searchsorted(csum, np.where(starts > _I64_MAX - room, _I64_MAX, starts + room), side="right")
    W = int(np.argmax(ends == n)) if np.any(ends == n) else m  # noqa: N806  the reference stops at the first fit
    if W == 0:
        return [], 0.0, PARTITION_OK
    ends = ends.tolist()
    cd = c.astype(np.float64)
    g = np.empty(m, np.float64)
    prev = np.full(m, -1, np.int64)
    lo = 0
    for j in range(m):
        while lo < j - 1 and lo + 1 < W and ends[lo + 1] <= j:
            lo += 1
        pv, pp = np.inf, -1
        if j > 0 and (lo + 1 >= W or ends[lo + 1] > j):
            pp = lo + int(np.argmin(g[lo:j]))  # the first minimum: the smallest p
            pv = g[pp]
        if ends[0] > j and not pv < 0.0:  # "no predecessor" wins a tie
            pv, pp = 0.0, -1
        g[j] = cd[j] + pv
        prev[j] = pp
    last = W - 1 + int(np.argmin(g[W - 1:m]))
    cuts, p = [], last
    while p >= 0:
        cuts.append(p + 1)
        p = int(prev[p])
    return cuts[::-1], float(g[last]), PARTITION_OK


# What `split_chunks_batch` raises for a status of `rl_split_chunks`.  There status 2 means a row of zero or NaN norm OR a non-finite
# cost, which an embedding with an infinite value also produces (its norm overflows, the similarity is NaN): the reference does not
# raise for such a row, it hands NaN costs to its solver; here the document is reported with the zero-norm message.
_STATUS_MESSAGES = {PARTITION_TOO_LARGE: "Chunklet larger than chunk max_size detected.",
                    PARTITION_NOT_FINITE: "Chunklet embeddings with zero norm detected."}


def solve_partition_dp(cost: np.ndarray, sizes: np.ndarray, max_size: int) -> list[int]:
    """`_solve_partition` without the solver: the same split indices wherever the optimum is unique (see `partition_dp`)."""
    cuts, _, status = partition_dp(cost, sizes, max_size)
    if status == PARTITION_TOO_LARGE:
        raise ValueError(_STATUS_MESSAGES[status])
    if status != PARTITION_OK:
        raise ValueError("Non-finite partition cost detected.")
    return cuts


def partition_chunks(cost: Any, sizes: Any, doc_offsets: Any, max_size: int) -> tuple[Any, Any, Any]:
    """The optimal partitions of MANY documents in one device call (`rl_partition_chunks`).

    cost: float32[N] NumPy array or CUDA tensor in the layout `partition_similarities` returns (the entry at every document's last
    chunklet is ignored); sizes int64[N]; doc_offsets int64[n_docs + 1].  Returns (cut uint8[N] with 1 = a split after chunklet i,
    objective float64[n_docs], status int32[n_docs]) on the side of `cost`; per document the bits of `partition_dp`."""
    return _ops.partition_chunks(cost, sizes, doc_offsets, max_size)


def _split_chunks_batch(documents: Sequence[Sequence[str]], embeddings: Any, max_size: int, name_document: bool) -> list[tuple[list[str], list[Any]]]:
    docs = [d if isinstance(d, list) else list(d) for d in documents]
    counts = np.fromiter((len(d) for d in docs), dtype=np.int64, count=len(docs))
    off = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    n = int(off[-1])
    if isinstance(embeddings, (list, tuple)):
        if len(embeddings) != len(docs):
            raise ValueError("split_chunks_batch: one embedding array per document is required")
        per_doc = list(embeddings)
        if any(int(e.shape[0]) != int(c) for e, c in zip(per_doc, counts)):
            raise ValueError("split_chunks_batch: a document's embeddings do not match its chunklets")
        full = [e for e in per_doc if int(e.shape[0]) > 0]
        if any(hasattr(e, "cpu") for e in full):
            x = _ops._torch().cat(full) if len(full) > 1 else (full[0] if full else None)  # noqa: SLF001
        else:
            x = np.concatenate([np.asarray(e) for e in full]) if len(full) > 1 else (np.asarray(full[0]) if full else None)
    else:
        x = embeddings
        if int(x.shape[0]) != n:
            raise ValueError("split_chunks_batch: the concatenated embeddings do not match the chunklets")
        per_doc = [x[off[d]:off[d + 1]] for d in range(len(docs))]
    if n > 0:
        sizes = np.fromiter((len(c) for d in docs for c in d), dtype=np.int64, count=n)
        sel = np.concatenate([_nonoutlying(sizes[off[d]:off[d + 1]]) for d in range(len(docs)) if counts[d] > 0])
        head = np.concatenate([_heading_flags(d) for d in docs])
        cut, _, _, status = _ops.split_chunks_call(x, off, sel, head, sizes, max_size)
        if hasattr(cut, "cpu"):  # the one read-back: a byte per chunklet, a word per document
            cut, status = cut.cpu().numpy(), status.cpu().numpy()
        bad = np.flatnonzero(status)
        if len(bad):
            d = int(bad[0])
            raise ValueError(_STATUS_MESSAGES[int(status[d])] + (f" (document {d})" if name_document else ""))
    out = []
    for d, chunklets in enumerate(docs):
        emb = per_doc[d]
        if not chunklets:
            out.append((chunklets, [emb]))  # the reference's early exit: `_split_chunks.py:43-44`
            continue
        cuts = (np.flatnonzero(cut[off[d]:off[d + 1]]) + 1).tolist()
        if not cuts:
            out.append((["".join(chunklets)], [emb]))
            continue
        bounds = [0, *cuts, len(chunklets)]
        chunks = ["".join(chunklets[i:j]) for i, j in zip(bounds[:-1], bounds[1:])]
        if hasattr(emb, "cpu"):
            parts = [emb[i:j] for i, j in zip(bounds[:-1], bounds[1:])]  # views: the tensor stays on the device
        else:
            parts = np.split(np.asarray(emb), cuts)  # `_split_chunks.py:121`
        out.append((chunks, list(parts)))
    return out


def split_chunks_batch(documents: Sequence[Sequence[str]], embeddings: Any, max_size: int = 2048) -> list[tuple[list[str], list[Any]]]:
    """`split_chunks` for MANY documents in one `rl_split_chunks` call: similarities, heading adjustments and the partition run on
    the device; the host derives string lengths, their quantiles and the heading flags, and joins the strings.

    documents: a sequence of chunklet lists; embeddings: one (n_d, dim) array / CUDA tensor per document, or ONE array / tensor of
    all documents' rows concatenated.  Returns per document what `split_chunks` returns (including `([], [emb])` for no chunklets
    and one chunk when everything fits); CUDA tensors stay on the device and the per-chunk embeddings are views.  Raises the
    reference's two `ValueError`s with " (document i)" appended for the first offending document; the zero-norm one also for a
    document whose embeddings hold an infinite value (a non-finite cost), which the reference passes on to its solver."""
    return _split_chunks_batch(documents, embeddings, max_size, name_document=True)


def partition_cost(chunklets: Sequence[str], chunklet_embeddings: Any) -> np.ndarray:
    """The MILP's cost vector for one document: device similarities + host heading adjustments (float32[n - 1])."""
    sizes = np.asarray([len(c) for c in chunklets])
    sim = partition_similarities(chunklet_embeddings, np.asarray([0, len(chunklets)], np.int64), sizes)
    sim = sim.cpu().numpy() if hasattr(sim, "cpu") else np.asarray(sim)
    return _apply_headings(sim[:-1].astype(np.float32), chunklets)


def split_chunks(chunklets: list[str], chunklet_embeddings: Any, max_size: int = 2048,
                 partition: str = "milp") -> tuple[list[str], list[Any]]:
    """Split chunklets into optimal semantic chunks (same contract and error messages as the reference).

    partition="milp" (default): device similarities, host MILP as in the reference.  partition="device": the whole document
    through `rl_split_chunks` (the one-document case of `split_chunks_batch`)."""
    if partition == "device":
        return _split_chunks_batch([chunklets], [chunklet_embeddings], max_size, name_document=False)[0]
    if partition != "milp":
        raise ValueError('partition must be "milp" or "device"')
    sizes = np.asarray([len(c) for c in chunklets])
    if not np.all(sizes <= max_size):
        raise ValueError("Chunklet larger than chunk max_size detected.")
    emb_host = chunklet_embeddings.float().cpu().numpy() if hasattr(chunklet_embeddings, "cpu") else np.asarray(chunklet_embeddings)
    if not np.all(np.linalg.norm(emb_host.astype(np.float32), axis=1) > 0.0):
        raise ValueError("Chunklet embeddings with zero norm detected.")
    if len(chunklets) <= 1 or int(sizes.sum()) <= max_size:
        return ["".join(chunklets)] if chunklets else chunklets, [chunklet_embeddings]
    cost = partition_cost(chunklets, chunklet_embeddings)
    cuts = _solve_partition(cost, sizes, max_size)
    bounds = [0, *cuts, len(chunklets)]
    chunks = ["".join(chunklets[i:j]) for i, j in zip(bounds[:-1], bounds[1:])]
    if hasattr(chunklet_embeddings, "cpu"):
        parts = [chunklet_embeddings[i:j] for i, j in zip(bounds[:-1], bounds[1:])]
    else:
        parts = np.split(np.asarray(chunklet_embeddings), cuts)  # `_split_chunks.py:121`
    return chunks, list(parts)
