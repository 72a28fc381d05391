"""Host mirror of `src/raglite/_split_chunklets.py` with the partition on the GPU.

    split_chunklets(sentences, boundary_cost=None, statement_cost=None, max_size=2048) -> chunklets   (`_split_chunklets.py:74-184`)
    split_chunklets_batch(documents, max_size=2048) -> the same per document, all documents in ONE device call
    split_documents_batch(documents) -> (chunks, chunk_embeddings) per document: chunklets -> embeddings -> chunks (`_insert.py:95-101`)

This is step 2 of the reference's indexing path (sentences -> chunklets -> embeddings -> chunks).  What runs on the device: the
partition itself (`:136-178`), an exact shortest path over split positions in float64 (`rl_partition_chunklets`; `chunklet_dp` below
is the host statement of that recurrence).  What stays on the host: the Markdown parse (`markdown_chunklet_boundaries`, needs
markdown-it), the word counts and their quantiles (`compute_num_statements`), string lengths and the joins.

One known difference from the reference: it squares `(s - 3.0)` with a NumPy scalar `** 2`, which calls libm `pow`; for about one
value in a thousand that differs from `x * x` in the last bit.  The statement and the kernel use `x * x`.  Objective bits are therefore
pinned between kernel and statement, not against the reference; against the reference the partitions are pinned
(`scripts/make_golden_chunklets.py` asserts it for every stored case).
"""

from __future__ import annotations

from typing import Any, Callable, Sequence

import numpy as np

from raglite_amd import _ops

CHUNKLETS_OK, CHUNKLETS_LONG_SENTENCE, CHUNKLETS_NOT_FINITE = 0, 1, 2

# `_split_chunklets.py:29-35`: how likely a Markdown block of this kind starts a chunklet
_BOUNDARY_PROBA = {"blockquote_open": 0.75, "bullet_list_open": 0.25, "heading_open": 1.0, "paragraph_open": 0.5,
                   "ordered_list_open": 0.25}


def markdown_chunklet_boundaries(sentences: Sequence[str]) -> np.ndarray:
    """`_split_chunklets.py:11-55`, same bits: float64[n], the probability that sentence i starts a chunklet, from the Markdown block
    that opens in it; of a run of consecutive boundary sentences only the (first) largest keeps its value.  No sentences: an empty
    array (the reference raises there, in `np.argmax` of an empty segment)."""
    from markdown_it import MarkdownIt  # lazily: only this function needs it

    n = len(sentences)
    probas = np.zeros(n)
    if n == 0:
        return probas
    doc = "".join(sentences)
    line_lengths = [len(line) for line in doc.splitlines(keepends=True)]
    line_start = np.concatenate(([0], np.cumsum(line_lengths[:-1], dtype=np.int64))).astype(np.int64)
    sentence_start = np.concatenate(([0], np.cumsum([len(s) for s in sentences], dtype=np.int64))).astype(np.int64)
    line_sentence = np.searchsorted(sentence_start, line_start, side="right") - 1
    last = -1
    for token in MarkdownIt().parse(doc):
        proba = _BOUNDARY_PROBA.get(token.type)
        if proba is None:
            continue
        i = int(line_sentence[token.map[0]])
        if i != last:
            probas[i] = proba
            last = i
    # runs of consecutive boundary sentences: the largest stays (np.argmax: the first of equals), the others become 0
    marked = np.concatenate(([False], probas != 0.0, [False]))
    edges = np.flatnonzero(marked[1:] != marked[:-1])
    for begin, end in zip(edges[0::2].tolist(), edges[1::2].tolist()):
        if end - begin > 1:
            keep = begin + int(np.argmax(probas[begin:end]))
            value = probas[keep]
            probas[begin:end] = 0.0
            probas[keep] = value
    return probas


def compute_num_statements(sentences: Sequence[str]) -> np.ndarray:
    """`_split_chunklets.py:58-71`, same bits: float64[n], a sentence's information content in statements -- 0.75 at the document's
    first word-count quartile, 1.25 at the third, linear below and above.  No sentences: an empty array."""
    words = np.asarray([len(s.split()) for s in sentences], dtype=np.float64)
    if len(words) == 0:
        return words
    tiny = np.sqrt(np.finfo(np.float64).eps)
    q25, q75 = np.quantile(words, [0.25, 0.75])
    q25 = max(q25, tiny)
    q75 = max(q75, q25 + tiny)
    with np.errstate(all="ignore"):
        return np.where(words <= q25, 0.75 * words / q25, 0.75 + 0.5 * (words - q25) / (q75 - q25))


def chunklet_dp(boundary: np.ndarray, statements: np.ndarray, lengths: np.ndarray, max_size: int) -> tuple[list[int], float, int]:
    """The chunklet partition of ONE document (`_split_chunklets.py:136-178`): the host statement of `chunklet_dp.hip`, same bits.

    boundary / statements float64[n], lengths int64[n] (the sentences' characters).  With pb, ps, pc the prefix sums (np.cumsum's
    order, a leading 0),
        dp[0] = 0,   dp[i] = min over j in [lo(i), i) of dp[j] + cost(j, i),   lo(i) = the smallest j with pc[i] - pc[j] <= max_size
        cost(j, i) = ((1.0 - p[j]) + (pb[i] - pb[j + 1])) + (s - 3.0) * (s - 3.0) / sqrt(max(s, 1e-6)) / 2.0,   s = ps[i] - ps[j]
    The smallest j wins a tie (the reference's `<=` under backward iteration).  +inf takes part in ties: behind a sentence longer than
    max_size the back-pointers go to the window's first position, and an empty window leaves dp[i] = inf, back[i] = -1.  NaN never wins.
    The backtrack is `i = back[n]; while i > 0`.  The square is x * x where the reference calls `pow` (see the module docstring).
    Returns (the positions where a new chunklet starts, as the reference's `partition_indices`; dp[n]; status) with status 0: ok,
    1: some sentence is longer than max_size (the partition is still the reference's, which does not raise there), 2: a non-finite
    boundary or statements value (no cuts, objective NaN; it wins over 1)."""
    p = np.asarray(boundary, dtype=np.float64).reshape(-1)
    st = np.asarray(statements, dtype=np.float64).reshape(-1)
    ln = np.asarray(lengths, dtype=np.int64).reshape(-1)
    n = len(ln)
    if max_size < 1 or len(p) != n or len(st) != n or np.any(ln < 0):
        raise ValueError("chunklet_dp: max_size >= 1, lengths >= 0 and one boundary / statements value per sentence are required")
    if not (np.all(np.isfinite(p)) and np.all(np.isfinite(st))):
        return [], float("nan"), CHUNKLETS_NOT_FINITE
    status = CHUNKLETS_LONG_SENTENCE if np.any(ln > max_size) else CHUNKLETS_OK
    pc = np.concatenate(([0], np.cumsum(ln))).astype(np.int64)
    pb = np.concatenate(([0.0], np.cumsum(p)))
    ps = np.concatenate(([0.0], np.cumsum(st)))
    lo = np.searchsorted(pc, pc - min(int(max_size), int(np.iinfo(np.int64).max)), side="left")  # pc[j] >= pc[i] - max_size
    head = 1.0 - p
    dp = np.full(n + 1, np.inf)
    dp[0] = 0.0
    back = np.full(n + 1, -1, np.int64)
    width = int((np.arange(n + 1) - lo).max()) if n else 0  # the widest window
    ks = np.arange(width)
    rows = max(1, (1 << 20) // max(width, 1))  # cost(j, i) for a block of rows i at once (elementwise: the bits of the scalar formula)
    with np.errstate(all="ignore"):
        for r0 in range(1, n + 1, rows):
            r1 = min(n + 1, r0 + rows)
            jj = np.minimum(lo[r0:r1, None] + ks[None, :], n - 1)  # j = lo(i) + k; entries with j >= i are never read
            s = ps[r0:r1, None] - ps[jj]
            d = s - 3.0
            cost = (head[jj] + (pb[r0:r1, None] - pb[jj + 1])) + d * d / np.sqrt(np.maximum(s, 1e-6)) / 2.0
            for i in range(r0, r1):
                a = int(lo[i])
                if a >= i:
                    continue  # an empty window: sentence i - 1 alone is longer than max_size
                v = dp[a:i] + cost[i - r0, :i - a]
                k = int(np.argmin(v))  # the first minimum: the smallest j; all +inf: the window's first position; a NaN if there is one
                if v[k] != v[k]:
                    ok = ~np.isnan(v)
                    if not ok.any():
                        continue
                    k = int(np.flatnonzero(ok & (v == v[ok].min()))[0])
                dp[i] = v[k]
                back[i] = a + k
    cuts, i = [], int(back[n])
    while i > 0:
        cuts.append(i)
        i = int(back[i])
    return cuts[::-1], float(dp[n]), status


def partition_chunklets(boundary: Any, statements: Any, lengths: Any, doc_offsets: Any, max_size: int) -> tuple[Any, Any, Any]:
    """The chunklet partitions of MANY documents in one device call (`rl_partition_chunklets`).

    boundary / statements: float64[N] NumPy arrays or CUDA tensors, one value per sentence of the concatenated documents; lengths
    int64[N]; doc_offsets int64[n_docs + 1].  Returns (cut uint8[N] with 1 = a chunklet ends after sentence i, objective
    float64[n_docs], status int32[n_docs]) on the side of `boundary`; per document the bits of `chunklet_dp`."""
    return _ops.partition_chunklets(boundary, statements, lengths, doc_offsets, max_size)


def _join(sentences: Sequence[str], cuts: Sequence[int]) -> list[str]:
    bounds = [0, *cuts, len(sentences)]
    return ["".join(sentences[i:j]) for i, j in zip(bounds[:-1], bounds[1:])]  # no sentences: [""], the reference's "".join([])


def split_chunklets_batch(documents: Sequence[Sequence[str]], max_size: int = 2048, *,
                          boundary_probas: Sequence[Any] | None = None, markdown: str = "host") -> list[list[str]]:
    """`split_chunklets` for MANY documents in one `rl_partition_chunklets` call: the partition runs on the device; the host parses
    the Markdown, counts words and characters, and joins the strings.

    documents: a sequence of sentence lists; boundary_probas: optionally one float array per document that replaces the Markdown
    parse.  One device call and one read-back (a byte per sentence, a word per document).  markdown="host" (default):
    `markdown_chunklet_boundaries` per document, with markdown-it; markdown="device": the Markdown block parse of the joined sentences
    runs on the device too (`_markdown.py`), its boundary probabilities go to the partition on the device, and only the documents the
    device parser gives up are parsed by markdown-it -- the same chunklets; an explicit boundary_probas still wins.  Returns per
    document what the reference returns, `[""]` for a document without sentences."""
    if markdown not in ("host", "device"):
        raise ValueError('markdown must be "host" or "device"')
    docs = [d if isinstance(d, list) else list(d) for d in documents]
    if boundary_probas is not None and len(boundary_probas) != len(docs):
        raise ValueError("split_chunklets_batch: one boundary_probas array per document is required")
    counts = np.fromiter((len(d) for d in docs), dtype=np.int64, count=len(docs))
    off = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    n = int(off[-1])
    cut = np.zeros(0, np.uint8)
    if n > 0:
        full = [d for d in range(len(docs)) if counts[d] > 0]
        lengths = np.fromiter((len(s) for d in docs for s in d), dtype=np.int64, count=n)
        if boundary_probas is None and markdown == "device":
            from raglite_amd import _markdown

            boundary = _markdown.device_chunklet_boundary(docs, off, lengths, lambda d: markdown_chunklet_boundaries(docs[d]))
        elif boundary_probas is None:
            boundary = np.concatenate([markdown_chunklet_boundaries(docs[d]) for d in full])
        else:
            boundary = np.concatenate([np.asarray(boundary_probas[d], dtype=np.float64).reshape(-1) for d in full])
        if len(boundary) != n:
            raise ValueError("split_chunklets_batch: a document's boundary_probas do not match its sentences")
        statements = np.concatenate([compute_num_statements(docs[d]) for d in full])
        cut, _, status = _ops.partition_chunklets(boundary, statements, lengths, off, max_size, want_objective=False)
        if not isinstance(cut, np.ndarray):  # the device route: one read-back
            cut, status = cut.cpu().numpy(), status.cpu().numpy()
        bad = np.flatnonzero(status == CHUNKLETS_NOT_FINITE)
        if len(bad):
            raise ValueError(f"Non-finite chunklet boundary probabilities or statement counts detected. (document {int(bad[0])})")
    return [_join(d, (np.flatnonzero(cut[off[i]:off[i + 1]]) + 1).tolist()) for i, d in enumerate(docs)]


def _split_chunklets_general(sentences: Sequence[str], boundary_cost: Callable[[np.ndarray], float] | None,
                             statement_cost: Callable[[float], float] | None, max_size: int) -> list[int]:
    """The reference's loop for caller-supplied costs (`_split_chunklets.py:142-171`, the branch of `:158-163`)."""
    boundary_cost = boundary_cost or (lambda p: (1.0 - p[0]) + np.sum(p[1:]))
    statement_cost = statement_cost or (lambda s: ((s - 3) ** 2 / np.sqrt(max(s, 1e-6)) / 2))
    probas, counts = markdown_chunklet_boundaries(sentences), compute_num_statements(sentences)
    n = len(sentences)
    pc = np.concatenate(([0], np.cumsum([len(s) for s in sentences], dtype=np.int64))).astype(np.int64)
    dp = np.full(n + 1, np.inf)
    dp[0] = 0.0
    back = np.full(n + 1, -1, np.intp)
    for i in range(1, n + 1):
        j = i - 1
        while j >= 0 and pc[i] - pc[j] <= max_size:
            total = dp[j] + (boundary_cost(probas[j:i]) + statement_cost(np.sum(counts[j:i])))
            if total <= dp[i]:  # `<=` going backwards: the smallest j of equals
                dp[i], back[i] = total, j
            j -= 1
    cuts, i = [], int(back[n])
    while i > 0:
        cuts.append(i)
        i = int(back[i])
    return cuts[::-1]


def split_chunklets(sentences: list[str], boundary_cost: Callable[[np.ndarray], float] | None = None,
                    statement_cost: Callable[[float], float] | None = None, max_size: int = 2048,
                    partition: str = "host") -> list[str]:
    """Split sentences into optimal chunklets (the reference's contract, `_split_chunklets.py:74-184`).

    partition="host" (default): the recurrence on the host (`chunklet_dp`; with a custom cost callable the reference's general loop).
    partition="device": the one-document case of `split_chunklets_batch`; custom cost callables cannot run there (ValueError)."""
    if partition not in ("host", "device"):
        raise ValueError('partition must be "host" or "device"')
    custom = boundary_cost is not None or statement_cost is not None
    if partition == "device":
        if custom:
            raise ValueError('split_chunklets: custom cost callables need partition="host"')
        return split_chunklets_batch([sentences], max_size)[0]
    if custom:
        return _join(sentences, _split_chunklets_general(sentences, boundary_cost, statement_cost, max_size))
    if not sentences:
        return _join(sentences, [])
    cuts, _, status = chunklet_dp(markdown_chunklet_boundaries(sentences), compute_num_statements(sentences),
                                  [len(s) for s in sentences], max_size)
    if status == CHUNKLETS_NOT_FINITE:
        raise ValueError("Non-finite chunklet boundary probabilities or statement counts detected.")
    return _join(sentences, cuts)


def split_documents_batch(documents: Sequence[Sequence[str]], *, config: Any | None = None,
                          embedder: Any | None = None, embed: str = "loop", markdown: str = "host") -> list[tuple[list[str], list[Any]]]:
    """Sentences -> chunklets -> chunklet embeddings -> chunks for MANY documents (`_insert.py:95-101`): `split_chunklets_batch`,
    the chunklet embeddings, `split_chunks_batch`.  embed="loop" (default): `embed_strings` one document at a time (as `_insert.py:96`
    does); embed="batch": `embed_strings_batch`, which shares encoder forwards and the pooling launch across documents.  Returns per
    document (chunks, chunk_embeddings), ready for `GpuIndex.insert_chunks`.  markdown: where `split_chunklets_batch` parses the
    Markdown."""
    from raglite_amd._chunking import split_chunks_batch
    from raglite_amd._config import HotPathConfig
    from raglite_amd._embed import embed_strings, embed_strings_batch

    if embed not in ("loop", "batch"):
        raise ValueError('embed must be "loop" or "batch"')
    config = config or HotPathConfig()
    chunklets = split_chunklets_batch(documents, max_size=config.chunk_max_size, markdown=markdown)
    if embed == "batch":
        embeddings = embed_strings_batch(chunklets, config=config, embedder=embedder)
    else:
        embeddings = [embed_strings(c, config=config, embedder=embedder) for c in chunklets]
    return split_chunks_batch(chunklets, embeddings, max_size=config.chunk_max_size)
