"""The Markdown parse of the two splitters on the device.

    markdown_blocks_batch(documents) -> (first_open, heading_end, line_offsets, status)

`markdown_sentence_boundaries` and `markdown_chunklet_boundaries` read very little from `MarkdownIt().parse`: where headings begin and
end, and which block opens first on a line.  `rl_markdown_blocks` computes exactly that for many documents in one call, with
markdown-it-py's own block rules, and answers per document "these are the library's tokens" (MARKDOWN_OK) or "parse this one on the
host" (MARKDOWN_UNDECIDED: raw HTML blocks, link reference definitions, tabs where they count as indentation, line separators only
`str.splitlines` knows, nesting 16 deep).  Never an approximation.  The splitters' `markdown="device"` route is built from the three
functions at the bottom: the device arrays go from one library call to the next, and only the undecided documents see markdown-it.
"""

from __future__ import annotations

from typing import Any, Callable, Sequence

import numpy as np

from raglite_amd._abi import check, lib
from raglite_amd._ops_frame import _Args, _is_torch, _torch

MARKDOWN_OK, MARKDOWN_UNDECIDED = 0, 1
FIRST_OPEN_NONE, FIRST_OPEN_HEADING, FIRST_OPEN_BLOCKQUOTE, FIRST_OPEN_PARAGRAPH, FIRST_OPEN_BULLET_LIST, FIRST_OPEN_ORDERED_LIST = range(6)


def _codepoints(text: str) -> np.ndarray:
    return np.frombuffer(text.encode("utf-32-le", "surrogatepass"), dtype=np.uint32)


def _offsets(lengths: Sequence[int]) -> np.ndarray:
    return np.concatenate(([0], np.cumsum(np.asarray(lengths, dtype=np.int64)))).astype(np.int64)


# ---- the three C entries ----------------------------------------------------------------------------------------------------------------
def _codepoints_inp(a: _Args, codepoints: Any) -> tuple[Any, int]:
    """UTF-32 code points as the call's leading argument: a CUDA tensor (uint32 or int32, the same bits) or a NumPy array."""
    if _is_torch(codepoints):
        torch = _torch()
        if codepoints.dtype not in (torch.int32, torch.uint32):
            codepoints = codepoints.to(torch.int32)  # code points are below 2^21
        return a.inp(codepoints.view(torch.int32), np.int32)
    return a.inp(np.ascontiguousarray(codepoints, dtype=np.uint32).view(np.int32), np.int32)


def markdown_blocks(codepoints: Any, doc_offsets: Any) -> tuple[Any, Any, Any, Any, Any]:
    """`rl_markdown_blocks`: the Markdown block structure of many documents in one call.  codepoints uint32[n], doc_offsets
    int64[n_docs + 1] -> (first_open uint8[n + n_docs], heading_end int32[n + n_docs], line_start int64[n + n_docs], line_offsets
    int64[n_docs + 1], status int32[n_docs]) on the side of `codepoints`; the per-line arrays are used up to line_offsets[-1]."""
    a = _Args()
    cp, p_cp = _codepoints_inp(a, codepoints)
    n = int(cp.shape[0])
    off, p_off = a.same_side(doc_offsets, np.int64)
    n_docs = int(off.shape[0]) - 1
    rows = n + max(n_docs, 0)
    first_open, p_first = a.out((rows,), np.uint8)
    heading_end, p_end = a.out((rows,), np.int32)
    line_start, p_start = a.out((rows,), np.int64)
    line_offsets, p_loff = a.out((max(n_docs, 0) + 1,), np.int64)
    status, p_status = a.out((max(n_docs, 0),), np.int32)
    if n == 0 and n_docs >= 0:  # every document is empty: no lines, all decided; the call would write nothing
        for out in (first_open, heading_end, line_start, line_offsets, status):
            out[...] = 0
        return first_open, heading_end, line_start, line_offsets, status
    a.ensure_device()
    check(lib().rl_markdown_blocks(p_cp, p_off, n, n_docs, p_first, p_end, p_start, p_loff, p_status, a.mem, a.stream))
    return first_open, heading_end, line_start, line_offsets, status


def markdown_sentence_known(heading_end: Any, line_start: Any, line_offsets: Any, status: Any, doc_offsets: Any, n: int) -> Any:
    """`rl_markdown_sentence_known`: float64[n], the known sentence boundaries of the decided documents (NaN elsewhere), on the side of
    `heading_end`."""
    a = _Args()
    he, p_end = a.inp(heading_end, np.int32)
    n_lines = int(he.shape[0])
    ls, p_start = a.same_side(line_start, np.int64)
    lo, p_loff = a.same_side(line_offsets, np.int64)
    st, p_status = a.same_side(status, np.int32)
    off, p_off = a.same_side(doc_offsets, np.int64)
    n_docs = int(off.shape[0]) - 1
    if int(ls.shape[0]) != n_lines or int(lo.shape[0]) != n_docs + 1 or int(st.shape[0]) != n_docs:
        raise ValueError("markdown_sentence_known: the per-line arrays or the per-document arrays differ in length")
    known, p_known = a.out((int(n),), np.float64)
    if n > 0:
        a.ensure_device()
        check(lib().rl_markdown_sentence_known(p_end, p_start, p_loff, p_status, p_off, int(n), n_docs, n_lines, p_known, a.mem,
                                               a.stream))
    return known


def markdown_chunklet_boundary(first_open: Any, line_start: Any, line_offsets: Any, status: Any, sentence_offsets: Any,
                               doc_offsets: Any) -> Any:
    """`rl_markdown_chunklet_boundary`: float64[n_sentences], the boundary probabilities of the decided documents (0 elsewhere), on
    the side of `first_open`.  sentence_offsets int64[n_sentences + 1] over the characters, doc_offsets int64[n_docs + 1] over the
    sentences."""
    a = _Args()
    fo, p_first = a.inp(first_open, np.uint8)
    n_lines = int(fo.shape[0])
    ls, p_start = a.same_side(line_start, np.int64)
    lo, p_loff = a.same_side(line_offsets, np.int64)
    st, p_status = a.same_side(status, np.int32)
    so, p_soff = a.same_side(sentence_offsets, np.int64)
    off, p_off = a.same_side(doc_offsets, np.int64)
    n_sent, n_docs = int(so.shape[0]) - 1, int(off.shape[0]) - 1
    if int(ls.shape[0]) != n_lines or int(lo.shape[0]) != n_docs + 1 or int(st.shape[0]) != n_docs:
        raise ValueError("markdown_chunklet_boundary: the per-line arrays or the per-document arrays differ in length")
    boundary, p_out = a.out((max(n_sent, 0),), np.float64)
    if n_sent > 0:
        a.ensure_device()
        check(lib().rl_markdown_chunklet_boundary(p_first, p_start, p_loff, p_status, p_soff, p_off, n_sent, n_docs, n_lines, p_out,
                                                  a.mem, a.stream))
    return boundary


def markdown_blocks_batch(documents: Sequence[str]) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """The block structure of MANY documents in one `rl_markdown_blocks` call.

    Returns (first_open uint8[n_lines], heading_end int32[n_lines], line_offsets int64[n_docs + 1], status int32[n_docs]): document d
    owns the lines [line_offsets[d], line_offsets[d + 1]), its `str.splitlines` lines.  first_open: the first block token that starts
    on the line, of FIRST_OPEN_HEADING .. FIRST_OPEN_ORDERED_LIST (FIRST_OPEN_NONE: none of these starts there); heading_end: `map[1]`
    of the heading that starts on the line, else 0.  status MARKDOWN_OK: both are what markdown-it's tokens give; MARKDOWN_UNDECIDED:
    the document's lines are unspecified, parse it with markdown-it."""
    docs = list(documents)
    off = _offsets([len(d) for d in docs])
    first_open, heading_end, _, line_offsets, status = markdown_blocks(_codepoints("".join(docs)), off)
    n_lines = int(line_offsets[-1])
    return first_open[:n_lines].copy(), heading_end[:n_lines].copy(), line_offsets, status


# ---- the splitters' device route --------------------------------------------------------------------------------------------------------
def _device():
    import torch

    from raglite_amd._ops_frame import _current_device

    return torch.device("cuda", _current_device())


def _upload(array: np.ndarray) -> Any:
    import torch

    array = np.ascontiguousarray(array)
    return torch.from_numpy(array if array.flags.writeable else array.copy()).to(_device())  # (torch refuses read-only memory)


def _merge_host(values: Any, off: np.ndarray, status: Any, host_values: Callable[[int], np.ndarray]) -> None:
    """Overwrites, in the device array `values`, the rows [off[d], off[d + 1]) of every undecided document d with host_values(d): one
    read-back of the status words, one upload and one scatter for all of them."""
    undecided = np.flatnonzero(status.cpu().numpy() != MARKDOWN_OK)
    if len(undecided) == 0:
        return
    parts = [np.asarray(host_values(int(d)), dtype=np.float64).reshape(-1) for d in undecided]
    for d, part in zip(undecided, parts):
        if len(part) != off[d + 1] - off[d]:
            raise ValueError("markdown: the host parse of a document does not match its rows")
    rows = np.concatenate([np.arange(off[d], off[d + 1], dtype=np.int64) for d in undecided])
    if len(rows):
        values[_upload(rows)] = _upload(np.concatenate(parts))


def device_sentence_known(codepoints: np.ndarray, off: np.ndarray, host_known: Callable[[int], np.ndarray]) -> tuple[Any, Any]:
    """(the code points on the device, float64[n] known sentence boundaries on the device) of documents whose characters are
    `codepoints` under the CSR `off`: `rl_markdown_blocks`, `rl_markdown_sentence_known`, and host_known(d) for every undecided d."""
    cp = _upload(codepoints.view(np.int32))
    _, heading_end, line_start, line_offsets, status = markdown_blocks(cp, off)
    known = markdown_sentence_known(heading_end, line_start, line_offsets, status, off, len(codepoints))
    _merge_host(known, off, status, host_known)
    return cp, known


def device_chunklet_boundary(documents: Sequence[Sequence[str]], off: np.ndarray, lengths: np.ndarray,
                             host_boundary: Callable[[int], np.ndarray]) -> Any:
    """float64[n_sentences] on the device: the chunklet boundary probabilities of documents given as sentence lists (`off`: the CSR
    over the sentences, `lengths`: their characters): `rl_markdown_blocks` on the joined sentences, `rl_markdown_chunklet_boundary`,
    and host_boundary(d) for every undecided d."""
    sentence_offsets = _offsets(lengths)
    char_off = sentence_offsets[off]
    cp = _upload(_codepoints("".join(s for d in documents for s in d)).view(np.int32))
    first_open, _, line_start, line_offsets, status = markdown_blocks(cp, char_off)
    boundary = markdown_chunklet_boundary(first_open, line_start, line_offsets, status, sentence_offsets, off)
    _merge_host(boundary, off, status, host_boundary)
    return boundary
