"""Host mirror of `src/raglite/_split_sentences.py` with the partition on the GPU.

    split_sentences(doc, min_len=4, max_len=None, boundary_probas=..., *, predicted_probas) -> sentences   (`_split_sentences.py:146-219`)
    split_sentences_batch(documents, ...) -> the same per document, all documents in ONE device call
    split_texts_batch(texts, predicted_probas=...) -> (chunks, chunk_embeddings) per text: sentences -> chunklets -> embeddings -> chunks

This is step 1 of the reference's indexing path (`_insert.py:94`).  The reference takes one boundary probability per character from a
Segment-any-Text model (`wtpsplit-lite`); the package ships no such model, so the caller hands the probabilities in
(`predicted_probas`).  Everything after the model is arithmetic on that vector and runs on the device (`rl_partition_sentences`): the
white-space class of every code point, the override by known boundaries, the white-space propagation (`:188-196`), the dynamic
programme without a maximum length (`:79-94`) and, for every sentence longer than `max_len`, the programme with the sliding window
(`:95-114`).  What stays on the host: the Markdown parse (`markdown_sentence_boundaries`, needs markdown-it), the model, the UTF-32
encode and the string slices.  `sentence_dp` is the host statement of the programme and `sentence_partition` of the whole call; the
kernels give their bits.
"""

from __future__ import annotations

from typing import Any, Callable, Sequence

import numpy as np

from raglite_amd import _ops

SENTENCES_OK, SENTENCES_TOO_LONG, SENTENCES_NOT_FINITE, SENTENCES_NO_SPLIT = 0, 1, 2, 3
_NO_SPLIT_MESSAGE = "Sentence partition failed: no valid split satisfies the constraints."
_NOT_FINITE_MESSAGE = "Non-finite sentence boundary probabilities detected."

# `str.isspace`: 29 code points (U+200B and U+180E are not among them)
_SPACE_RANGES = ((0x0009, 0x000D), (0x001C, 0x0020), (0x0085, 0x0085), (0x00A0, 0x00A0), (0x1680, 0x1680), (0x2000, 0x200A),
                 (0x2028, 0x2029), (0x202F, 0x202F), (0x205F, 0x205F), (0x3000, 0x3000))


def markdown_sentence_boundaries(doc: str) -> np.ndarray:
    """`_split_sentences.py:23-53`, same bits: float64[len(doc)], NaN where nothing is known; the character before a Markdown heading
    and the heading's last character (its line break) end a sentence (1), the heading's body holds no boundary (0)."""
    from markdown_it import MarkdownIt  # lazily: only this function needs it

    line_start = [0]
    for line in doc.splitlines(keepends=True):
        line_start.append(line_start[-1] + len(line))
    probas = np.full(len(doc), np.nan)
    for token in MarkdownIt().parse(doc):
        if token.type != "heading_open":
            continue
        start, end = line_start[token.map[0]], line_start[token.map[1]] + 1
        if 0 <= start - 1 < len(probas):
            probas[start - 1] = 1
        probas[start:end - 1] = 0
        if 0 <= end - 1 < len(probas):
            probas[end - 1] = 1
    return probas


def codepoints_of(doc: str) -> np.ndarray:
    """uint32[len(doc)]: the document's code points (lone surrogates pass through)."""
    return np.frombuffer(doc.encode("utf-32-le", "surrogatepass"), dtype=np.uint32)


def whitespace_mask(doc: str | np.ndarray) -> np.ndarray:
    """uint8[len(doc)]: 1 where `str.isspace` holds for the character (`_split_sentences.py:188`), from the UTF-32 code points (a
    string, or the uint32 array itself); the class the kernel computes."""
    cp = codepoints_of(doc) if isinstance(doc, str) else np.asarray(doc, dtype=np.uint32).reshape(-1)
    mask = np.zeros(len(cp), dtype=bool)
    for lo, hi in _SPACE_RANGES:
        mask |= (cp >= lo) & (cp <= hi)
    return mask.astype(np.uint8)


def propagate_whitespace(probas: np.ndarray, is_space: np.ndarray) -> np.ndarray:
    """`_split_sentences.py:188-196` on a copy: white space always trails a sentence and never leads one.

    A range is [i, j): i is a non-space character followed by a space, j the first non-space character after that run.  Within it
    probas[i:j-1] = min(probas[i:j]) and probas[j-1] = max(probas[i:j]).  The reference's trimming (`start < max(end)`,
    `end > min(start)`) drops a leading run with no character before it and a trailing run with no character after it.  The ranges are
    disjoint (a range ends where the next may begin, and writes nothing at j), so the order of application does not matter: the kernel
    gives every range to a thread of its own.  Dtype of `probas` is kept."""
    probas = np.array(probas, copy=True).reshape(-1)
    space = np.asarray(is_space).reshape(-1).astype(bool)
    if len(space) != len(probas):
        raise ValueError("propagate_whitespace: one is_space flag per probability is required")
    if len(space) < 2:
        return probas
    start = np.flatnonzero(~space[:-1] & space[1:])
    end = np.flatnonzero(~space[1:] & space[:-1]) + 1
    start = start[start < np.max(end, initial=-1)]
    end = end[end > np.min(start, initial=len(space))]
    if len(start) == 0:
        return probas
    assert len(start) == len(end) and np.all(start < end)
    edges = np.column_stack((start, end)).reshape(-1)
    lo, hi = np.minimum.reduceat(probas, edges)[0::2], np.maximum.reduceat(probas, edges)[0::2]
    width = end - start
    inside = np.repeat(start - (np.cumsum(width) - width), width) + np.arange(int(width.sum()))
    probas[inside] = np.repeat(lo, width)
    probas[end - 1] = hi
    return probas


def sentence_dp(probas: np.ndarray, min_len: int, max_len: int | None = None) -> tuple[list[int], float, int]:
    """ONE run of the reference's dynamic programme (`_split_sentences.py:67-137`), in its order of operations; the tests' reference.

    probas: float32 or float64, one value per character.  `scores = probas - 0.25` is computed in that dtype; dp is float64 and every
    `best_prev + scores[i]` a float64 add of the widened score.  A boundary at i makes character i the last of a sentence.  Without
    max_len the predecessor is a running maximum under strict `>` (the EARLIEST of equal predecessors wins) and is taken only if
    `best_prev > -inf and best_prev + s > s`.  With max_len a monotonic deque pops while `dq[-1][0] <= dp[j]` (the LATEST of equal
    predecessors in the window [i - max_len, i - min_len] wins), only finite dp[j] enter, and the first boundary is allowed only if
    `i + 1 <= max_len`.  The final boundary is the earliest maximum over [answer_min, last_valid] under strict `>`, starting from 0.0
    when "no boundary" is admissible (`max_len is None or max_len >= n`) and from -inf otherwise.
    Returns (boundaries ascending, best_score, status): 0 ok; 1 the input is longer than max_len but shorter than 2 * min_len and
    comes back unsplit (the reference returns `[doc]` there and raises nothing); 2 a non-finite probability (no boundaries, NaN);
    3 no valid split under max_len (no boundaries, -inf; the reference raises ValueError)."""
    p = np.asarray(probas).reshape(-1)
    if p.dtype != np.float32:
        p = p.astype(np.float64, copy=False)
    if min_len < 1 or (max_len is not None and max_len < 1):
        raise ValueError("sentence_dp: min_len >= 1 and max_len >= 1 (or None) are required")
    if not np.all(np.isfinite(p)):
        return [], float("nan"), SENTENCES_NOT_FINITE
    n = len(p)
    first_valid = min_len - 1
    last_valid = n - min_len - 1
    if last_valid < first_valid:
        return [], 0.0, (SENTENCES_TOO_LONG if max_len is not None and n > max_len else SENTENCES_OK)
    scores = (p - p.dtype.type(0.25)).astype(np.float64).tolist()  # Python floats: every add below is an IEEE float64 add
    inf = float("inf")
    dp = [-inf] * n
    back = [-1] * n
    if max_len is None:
        best_prev, best_prev_idx = -inf, -1
        for i in range(first_valid, last_valid + 1):
            j = i - min_len
            if j >= first_valid and dp[j] > best_prev:
                best_prev, best_prev_idx = dp[j], j
            dp[i] = scores[i]
            if best_prev > -inf and best_prev + scores[i] > dp[i]:
                dp[i] = best_prev + scores[i]
                back[i] = best_prev_idx
    else:
        dq: list[tuple[float, int]] = []  # a deque by a list and a head index
        head = 0
        for i in range(first_valid, last_valid + 1):
            j = i - min_len
            if j >= first_valid and -inf < dp[j] < inf:
                while len(dq) > head and dq[-1][0] <= dp[j]:
                    dq.pop()
                dq.append((dp[j], j))
            while len(dq) > head and dq[head][1] < i - max_len:
                head += 1
            if i + 1 <= max_len:
                dp[i] = scores[i]
            if len(dq) > head and dq[head][0] + scores[i] > dp[i]:
                dp[i] = dq[head][0] + scores[i]
                back[i] = dq[head][1]
    answer_min = first_valid
    if max_len is not None:
        answer_min = max(answer_min, n - max_len - 1)
    no_boundary_valid = max_len is None or max_len >= n
    best_score = 0.0 if no_boundary_valid else -inf
    best_last = -1
    for i in range(answer_min, last_valid + 1):
        if dp[i] > best_score:
            best_score, best_last = dp[i], i
    if best_last == -1:
        return [], best_score, (SENTENCES_OK if no_boundary_valid else SENTENCES_NO_SPLIT)
    boundaries = []
    pos = best_last
    while pos >= 0:
        boundaries.append(pos)
        pos = back[pos]
    return boundaries[::-1], best_score, SENTENCES_OK


def sentence_partition(probas: np.ndarray, is_space: np.ndarray, min_len: int, max_len: int | None = None,
                       known: np.ndarray | None = None) -> tuple[list[int], float, int]:
    """What `rl_partition_sentences` computes for ONE document (`_split_sentences.py:183-218` after the model): the override by the
    finite entries of `known` (cast to the dtype of probas), the white-space propagation, phase 1 (`sentence_dp` without max_len) and
    phase 2 (`sentence_dp` with max_len on every phase-1 sentence longer than max_len, on its slice of the PROPAGATED probabilities).
    Returns (boundaries ascending, the phase-1 best score, status); status 2 wins over 3 and 3 over 1; 2 and 3 leave no boundaries."""
    p = np.array(probas, copy=True).reshape(-1)
    if p.dtype != np.float32:
        p = p.astype(np.float64)
    if known is not None:
        known = np.asarray(known, dtype=np.float64).reshape(-1)
        if len(known) != len(p):
            raise ValueError("sentence_partition: one known value per probability is required")
        keep = np.isfinite(known)
        with np.errstate(over="ignore"):
            p[keep] = known[keep]
    if not np.all(np.isfinite(p)):
        return [], float("nan"), SENTENCES_NOT_FINITE
    p = propagate_whitespace(p, is_space)
    bounds, objective, _ = sentence_dp(p, min_len)
    if max_len is None:
        return bounds, objective, SENTENCES_OK
    status = SENTENCES_OK
    out: list[int] = []
    edges = [0, *[b + 1 for b in bounds], len(p)]
    for begin, end in zip(edges[:-1], edges[1:]):
        if end - begin > max_len:
            inner, _, st = sentence_dp(p[begin:end], min_len, max_len)
            if st == SENTENCES_NO_SPLIT:
                return [], objective, SENTENCES_NO_SPLIT
            status = max(status, st)
            out.extend(begin + b for b in inner)
        if end < len(p):
            out.append(end - 1)
    return out, objective, status


def partition_sentences(codepoints: Any, probas: Any, doc_offsets: Any, min_len: int = 4, max_len: int | None = None,
                        known: Any | None = None) -> tuple[Any, Any, Any]:
    """The sentence partitions of MANY documents in one device call (`rl_partition_sentences`).

    codepoints uint32[N] and probas float32[N] or float64[N] (NumPy arrays or CUDA tensors; any other float dtype is widened to
    float64), one per character of the concatenated documents; doc_offsets int64[n_docs + 1]; known float64[N] or None.  Returns
    (cut uint8[N] with 1 = character i is the last of a sentence, never a document's final character; objective float64[n_docs];
    status int32[n_docs]) on the side of `probas`; per document the bits of `sentence_partition`."""
    return _ops.partition_sentences(codepoints, probas, doc_offsets, min_len, max_len, known)


def _slices(doc: str, bounds: Sequence[int]) -> list[str]:
    edges = [0, *[b + 1 for b in bounds], len(doc)]
    return [doc[i:j] for i, j in zip(edges[:-1], edges[1:])]


def _probas_of(source: Any, d: int, doc: str, what: str) -> np.ndarray:
    p = np.asarray(source(doc) if callable(source) else source[d]).reshape(-1)
    if len(p) != len(doc):
        raise ValueError(f"{what}: {len(p)} probabilities for a document of {len(doc)} characters (document {d})")
    return p


def _raise_for(status: int, d: int | None) -> None:
    where = "" if d is None else f" (document {d})"
    if status == SENTENCES_NOT_FINITE:
        raise ValueError(_NOT_FINITE_MESSAGE + where)
    if status == SENTENCES_NO_SPLIT:
        raise ValueError(_NO_SPLIT_MESSAGE + where)


def split_sentences_batch(documents: Sequence[str], min_len: int = 4, max_len: int | None = None, *, predicted_probas: Any,
                          boundary_probas: Any | None = None, markdown: str = "host") -> list[list[str]]:
    """`split_sentences` for MANY documents in one `rl_partition_sentences` call and one read-back (a byte per character, a word per
    document).

    predicted_probas: the model's boundary probability per character, one array per document or a callable `str -> array` (float32
    stays float32, as the reference keeps the model's dtype; all documents of one call share a dtype).  boundary_probas: known
    boundaries that override the prediction where finite -- one array per document, a callable, or None for
    `markdown_sentence_boundaries` (the reference's default).  A document with `len(doc) <= min_len` comes back as `[doc]` without a
    look at its probabilities (`_split_sentences.py:178`).  markdown="host" (default): `markdown_sentence_boundaries` per document,
    with markdown-it; markdown="device": the Markdown block parse runs on the device too (`_markdown.py`; the code points are uploaded
    once, the known boundaries go from `rl_markdown_sentence_known` to the partition on the device, and only the documents the
    device parser gives up are parsed by markdown-it) -- the same sentences; an explicit boundary_probas still wins.  ValueError: a
    probability array of the wrong length, non-finite probabilities, or no valid split under max_len (the reference's message), each
    naming the document."""
    if markdown not in ("host", "device"):
        raise ValueError('markdown must be "host" or "device"')
    docs = list(documents)
    for name, source in (("predicted_probas", predicted_probas), ("boundary_probas", boundary_probas)):
        if source is not None and not callable(source) and len(source) != len(docs):
            raise ValueError(f"split_sentences_batch: one {name} array per document is required")
    if min_len < 1 or (max_len is not None and max_len < 1):
        raise ValueError("split_sentences_batch: min_len >= 1 and max_len >= 1 (or None) are required")
    known_source = markdown_sentence_boundaries if boundary_probas is None else boundary_probas
    full = [d for d, doc in enumerate(docs) if len(doc) > min_len]
    out: list[list[str]] = [[doc] for doc in docs]
    if not full:
        return out
    predicted = [_probas_of(predicted_probas, d, docs[d], "predicted_probas") for d in full]
    dtypes = {np.dtype(np.float32) if p.dtype == np.float32 else np.dtype(np.float64) for p in predicted}
    if len(dtypes) != 1:
        raise ValueError("split_sentences_batch: the predicted_probas of one call must share a dtype (float32 or float64)")
    dtype = dtypes.pop()
    codepoints = codepoints_of("".join(docs[d] for d in full))
    off = np.concatenate(([0], np.cumsum([len(docs[d]) for d in full]))).astype(np.int64)
    probas = np.concatenate(predicted).astype(dtype, copy=False)
    if markdown == "device" and boundary_probas is None:
        from raglite_amd import _markdown

        cp, known = _markdown.device_sentence_known(codepoints, off, lambda k: markdown_sentence_boundaries(docs[full[k]]))
        cut, _, status = (x.cpu().numpy() if x is not None else None for x in _ops.partition_sentences(
            cp, _markdown._upload(probas), off, min_len, max_len, known, want_objective=False))
    else:
        known = np.concatenate([_probas_of(known_source, d, docs[d], "boundary_probas").astype(np.float64, copy=False) for d in full])
        cut, _, status = _ops.partition_sentences(codepoints, probas, off, min_len, max_len, known, want_objective=False)
    for k in np.flatnonzero(status >= SENTENCES_NOT_FINITE).tolist()[:1]:
        _raise_for(int(status[k]), full[k])
    for k, d in enumerate(full):
        out[d] = _slices(docs[d], np.flatnonzero(cut[off[k]:off[k + 1]]).tolist())
    return out


def split_sentences(doc: str, min_len: int = 4, max_len: int | None = None,
                    boundary_probas: Any = markdown_sentence_boundaries, *, predicted_probas: Any,
                    partition: str = "host") -> list[str]:
    """Split a document into sentences (the reference's contract, `_split_sentences.py:146-219`, with the model's output handed in as
    `predicted_probas`: an array or a callable `str -> array`).

    partition="host" (default): the statement (`sentence_partition`).  partition="device": the one-document case of
    `split_sentences_batch`."""
    if partition not in ("host", "device"):
        raise ValueError('partition must be "host" or "device"')
    if partition == "device":
        one = (lambda source: source if callable(source) or source is None else [source])
        return split_sentences_batch([doc], min_len, max_len, predicted_probas=one(predicted_probas),
                                     boundary_probas=one(boundary_probas))[0]
    if len(doc) <= min_len:
        return [doc]
    predicted = _probas_of(predicted_probas if callable(predicted_probas) else [predicted_probas], 0, doc, "predicted_probas")
    boundary_probas = markdown_sentence_boundaries if boundary_probas is None else boundary_probas
    known = _probas_of(boundary_probas if callable(boundary_probas) else [boundary_probas], 0, doc, "boundary_probas")
    bounds, _, status = sentence_partition(predicted, whitespace_mask(doc), min_len, max_len, known)
    _raise_for(status, None)
    return _slices(doc, bounds)


def split_texts_batch(texts: Sequence[str], *, predicted_probas: Any, config: Any | None = None,
                      embedder: Any | None = None, markdown: str = "host") -> list[tuple[list[str], list[Any]]]:
    """Texts -> sentences -> chunklets -> chunklet embeddings -> chunks for MANY documents (`_insert.py:94-101`):
    `split_sentences_batch` with `max_len=config.chunk_max_size` (as `_insert.py:94` does), then `split_documents_batch`.  Returns per
    text (chunks, chunk_embeddings), ready for `GpuIndex.insert_chunks`.  markdown: where both splitters parse the Markdown
    (`split_sentences_batch`)."""
    from raglite_amd._chunklets import split_documents_batch
    from raglite_amd._config import HotPathConfig

    config = config or HotPathConfig()
    sentences = split_sentences_batch(texts, max_len=config.chunk_max_size, predicted_probas=predicted_probas, markdown=markdown)
    return split_documents_batch(sentences, config=config, embedder=embedder, markdown=markdown)
