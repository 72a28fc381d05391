"""Host mirror of `src/raglite/_embed.py` with the pooling arithmetic on the GPU.

Same entry points, argument meaning and return contract as the reference:

    embed_strings(strings, *, config=None)                         (`_embed.py:193-200`)
    embed_strings_with_late_chunking(sentences, *, config=None)    (`_embed.py:16-141`)
    embed_strings_without_late_chunking(strings, *, config=None)   (`_embed.py:168-184`)
    embedding_type(*, config=None)                                 (`_embed.py:187-190`)

all returning a float16 matrix with one row per input string (`tests/test_embed.py:19-26`); plus `embed_strings_batch(documents)`,
which the reference has no counterpart of: many documents per call, their late-chunking segments grouped across documents into
shared encoder forwards and pooled in one launch, one such matrix per document.

What stays on the host (integer bookkeeping, a few hundred values per document): sentinel-based
token counting, the 38.2 % / 61.8 % preamble/content segment plan, the largest-remainder split of a
segment's token rows over its sentences.  What moves to `rl_pool_norm` (one launch per document):
per-sentence mean over contiguous token rows, rowwise L2 normalisation, fp16 cast
(`_embed.py:131-140`, `:154-164`).  The token-level embedding model itself (llama.cpp in the
reference, `_embed.py:64-66,119`) is reached through `embedder_for(config)`.
"""

from __future__ import annotations

from typing import Any, Callable, Literal, Sequence

import numpy as np

from raglite_amd import _ops
from raglite_amd._config import HotPathConfig
from raglite_amd._torch_embedder import pack_runs

SENTINEL = "⊕"  # `_embed.py:70`
_BATCH = 96  # `_embed.py:173`

# ---- embedder plumbing ---------------------------------------------------------------------------
_embedder_factory: Callable[[Any], Any] | None = None


def set_embedder_factory(factory: Callable[[Any], Any] | None) -> None:
    """Install `factory(config) -> llama-like embedder` (needs tokenize/detokenize/embed/n_ctx/n_batch)."""
    global _embedder_factory  # noqa: PLW0603
    _embedder_factory = factory


def embedder_for(config: Any) -> Any:
    if _embedder_factory is not None:
        return _embedder_factory(config)
    try:  # the reference's own provider, when RAGLite + llama-cpp-python are installed
        from raglite._lazy_llama import LLAMA_POOLING_TYPE_NONE
        from raglite._litellm import LlamaCppPythonLLM
    except ImportError as e:  # pragma: no cover - depends on the environment
        msg = "No token-level embedder available: call raglite_amd.set_embedder_factory(...) first."
        raise ModuleNotFoundError(msg) from e
    return LlamaCppPythonLLM.llm(config.embedder, embedding=True, pooling_type=LLAMA_POOLING_TYPE_NONE)


def embedding_type(*, config: Any | None = None) -> Literal["late_chunking", "standard"]:
    config = config or HotPathConfig()
    return "late_chunking" if config.embedder.startswith("llama-cpp-python") else "standard"


# ---- host-side integer bookkeeping ------------------------------------------------------------------
def _sentinel_token_ids(embedder: Any) -> list[int]:
    probe = f"A{SENTINEL}B {SENTINEL} C.\n{SENTINEL}D"
    ids = [t for t in embedder.tokenize(probe.encode(), add_bos=False) if SENTINEL in embedder.detokenize([t]).decode()]
    assert ids, f"Sentinel `{SENTINEL}` not supported by embedder"
    return ids


def count_sentence_tokens(sentences: list[str], embedder: Any) -> np.ndarray:
    """Tokens per sentence, measured the reference's way (`_embed.py:21-36,79-93`): sentences are
    joined with a sentinel character in batches of > n_ctx // 2 characters, tokenised once per batch,
    and the gaps between sentinel tokens are the counts."""
    sentinels = _sentinel_token_ids(embedder)
    limit = embedder.n_ctx() // 2
    counts: list[int] = []
    group: list[str] = []
    chars = 0
    for pos, sentence in enumerate(sentences):
        group.append(sentence)
        chars += len(sentence)
        if pos == len(sentences) - 1 or chars > limit:
            toks = np.asarray(embedder.tokenize(SENTINEL.join(group).encode(), add_bos=False), dtype=np.intp)
            is_sentinel = np.isin(toks, sentinels)
            marks = np.flatnonzero(is_sentinel)
            gaps = np.diff(np.concatenate(([0], marks, [len(toks)])))
            assert len(gaps) == len(group), f"Sentinel `{SENTINEL}` appears in document"
            counts.extend(int(g) for g in gaps)
            group, chars = [], 0
    return np.asarray(counts, dtype=np.intp)


def plan_segments(num_tokens: np.ndarray, n_ctx: int, n_batch: int) -> list[tuple[int, int, int]]:
    """(segment_start, content_start, segment_end) sentence indices per segment (`_embed.py:38-58,99-110`).

    Each segment holds at most min(n_ctx, n_batch) - 16 tokens: up to 38.2 % preamble (context only)
    followed by content; preamble budget that is not used goes to the content."""
    budget = min(n_ctx, n_batch) - 16
    pre_budget = round(0.382 * budget)
    content_budget = budget - pre_budget
    prefix = np.concatenate(([0], np.cumsum(num_tokens)))  # prefix[i] = tokens before sentence i
    n = len(num_tokens)
    plan = []
    start = 0
    while start < n:
        # longest run of sentences ending just before `start` whose total is <= pre_budget
        seg_start = int(np.searchsorted(prefix[: start + 1], prefix[start] - pre_budget, side="left"))
        used_pre = int(prefix[start] - prefix[seg_start])
        room = content_budget + (pre_budget - used_pre)
        # longest run of sentences from `start` whose total is <= room
        end = int(np.searchsorted(prefix, prefix[start] + room, side="right")) - 1
        end = min(max(end, start), n)
        if end == start:
            # A single sentence larger than the whole budget: the reference's loop would never advance
            # (`_embed.py:103-110`); take the sentence alone and let the embedder truncate it.
            end = start + 1
        plan.append((seg_start, start, end))
        start = end
    return plan


def split_rows(n_rows: int, sentence_tokens: np.ndarray) -> np.ndarray:
    """Largest-remainder apportioning of a segment's `n_rows` token rows over its sentences
    (`_embed.py:122-129`; the embedder adds special tokens, so n_rows != sum(sentence_tokens)).
    Tie order among equal remainders is that of `np.argsort`, as in the reference."""
    share = n_rows * (sentence_tokens / np.sum(sentence_tokens))
    sizes = np.floor(share).astype(np.intp)
    missing = int(n_rows - sizes.sum())
    if missing > 0:
        sizes[np.argsort(share - sizes)[-missing:]] += 1
    return sizes


# ---- the three embed entry points ---------------------------------------------------------------------
def _is_device_tensor(x: Any) -> bool:
    return type(x).__module__.split(".")[0] == "torch" and bool(getattr(x, "is_cuda", False))


def _token_matrix(x: Any) -> Any:
    """llama.cpp returns fp32 values as Python floats (`_embed.py:119`); a GPU embedder (`_torch_embedder.py`)
    returns CUDA tensors, which stay where they are."""
    return x.float() if _is_device_tensor(x) else np.asarray(x, dtype=np.float32)


def _stack(blocks: list) -> Any:
    if len(blocks) == 1:
        return blocks[0]
    if _is_device_tensor(blocks[0]):
        import torch

        return torch.cat(blocks)
    return np.vstack(blocks)


def _pool(tokens: Any, begins: np.ndarray, ends: np.ndarray, *, normalize: bool, eps: float) -> np.ndarray:
    """`rl_pool_norm` on whichever side the token matrix lives; always returns the fp16 NumPy matrix of the contract."""
    if _is_device_tensor(tokens):
        import torch

        b = torch.as_tensor(begins, device=tokens.device)
        e = torch.as_tensor(ends, device=tokens.device)
        _, out = _ops.pool_norm(tokens, b, e, normalize=normalize, eps=eps)
        return out.cpu().numpy()
    _, out = _ops.pool_norm(tokens, begins, ends, normalize=normalize, eps=eps)
    return out


def plan_document(sentences: list[str], embedder: Any) -> tuple[Any, np.ndarray, np.ndarray]:
    """Everything the pooling kernel needs for one document: the concatenated token matrix of all
    segments (T, dim) float32 (NumPy, or a CUDA tensor when the embedder runs on the GPU) and, per content
    sentence, its row span [begin, end) in that matrix."""
    num_tokens = count_sentence_tokens(sentences, embedder)
    plan = plan_segments(num_tokens, embedder.n_ctx(), embedder.n_batch)
    token_blocks, begins, ends = [], [], []
    base = 0
    for seg_start, content_start, seg_end in plan:
        tokens = _token_matrix(embedder.embed("".join(sentences[seg_start:seg_end])))
        sizes = split_rows(len(tokens), num_tokens[seg_start:seg_end])
        bounds = base + np.concatenate(([0], np.cumsum(sizes)))
        first = content_start - seg_start
        begins.append(bounds[first:-1])
        ends.append(bounds[first + 1 :])
        token_blocks.append(tokens)
        base += len(tokens)
    return _stack(token_blocks), np.concatenate(begins).astype(np.int64), np.concatenate(ends).astype(np.int64)


def embed_strings_with_late_chunking(sentences: list[str], *, config: Any | None = None,
                                     embedder: Any | None = None) -> np.ndarray:
    """Embed a document's sentences with late chunking (GPU pooling)."""
    config = config or HotPathConfig()
    assert config.embedder.startswith("llama-cpp-python")
    embedder = embedder or embedder_for(config)
    if len(sentences) == 0:
        raise ValueError("need at least one sentence")
    tokens, begins, ends = plan_document(sentences, embedder)
    return _pool(tokens, begins, ends, normalize=bool(config.embedder_normalize), eps=0.0)


def _embed_string_batch(strings: list[str], *, config: Any, embedder: Any | None = None) -> np.ndarray:
    """`_embed.py:144-165`: one pooled vector per string; eps-guarded normalisation."""
    if config.embedder.startswith("llama-cpp-python"):
        embedder = embedder or embedder_for(config)
        mats = [_token_matrix(m) for m in embedder.embed(strings)]
        lengths = np.asarray([len(m) for m in mats], dtype=np.int64)
        tokens = _stack(mats)
    else:
        # API embedders return one vector per string (`_embed.py:156-158`): spans of a single row.
        embedder = embedder or embedder_for(config)
        tokens = np.asarray(embedder(strings), dtype=np.float32)
        lengths = np.ones(len(strings), dtype=np.int64)
    ends = np.cumsum(lengths)
    return _pool(tokens, ends - lengths, ends, normalize=bool(config.embedder_normalize),
                 eps=float(np.finfo(np.float64).eps))


def embed_strings_without_late_chunking(strings: list[str], *, config: Any | None = None,
                                        embedder: Any | None = None) -> np.ndarray:
    config = config or HotPathConfig()
    parts = [_embed_string_batch(strings[i : i + _BATCH], config=config, embedder=embedder)
             for i in range(0, len(strings), _BATCH)]
    return np.vstack(parts)


def embed_strings(strings: list[str], *, config: Any | None = None, embedder: Any | None = None) -> np.ndarray:
    """Embed the chunklets of a document as a float16 matrix with one row per chunklet."""
    config = config or HotPathConfig()
    if embedding_type(config=config) == "late_chunking":
        return embed_strings_with_late_chunking(strings, config=config, embedder=embedder)
    return embed_strings_without_late_chunking(strings, config=config, embedder=embedder)


def embed_strings_batch(documents: Sequence[list[str]], *, config: Any | None = None, embedder: Any | None = None) -> list[np.ndarray]:
    """`embed_strings` for MANY documents: one float16 matrix per document, each with `embed_strings(document)`'s contract.

    Late chunking: token counts and the segment plan per document, as `plan_document` makes them; then consecutive segments ACROSS
    documents go to `embedder.embed(list_of_segment_texts)` in groups of at most `embedder.pack_tokens` tokens (`embedder.n_batch` for
    an embedder without that attribute; a segment over the bound goes alone), so a short document no longer costs an encoder forward of
    its own; the token rows are apportioned per segment, ONE `rl_pool_norm` pools every document's spans, and the result is sliced per
    document.  Any llama-like embedder whose `embed(list)` returns a list works; a `TorchTokenEmbedder(batching="packed")` runs each
    group as one unpadded forward.  The token rows of all documents are resident at once (they are on the device with a GPU embedder):
    callers bound the documents per call.  Standard embedders: the strings of all documents through
    `embed_strings_without_late_chunking`, sliced.  An empty document raises ValueError, as `embed_strings` does; no documents: []."""
    config = config or HotPathConfig()
    docs = [d if isinstance(d, list) else list(d) for d in documents]
    if not docs:
        return []
    if any(len(d) == 0 for d in docs):
        raise ValueError("need at least one sentence")
    bounds = np.concatenate(([0], np.cumsum([len(d) for d in docs])))
    if embedding_type(config=config) != "late_chunking":
        flat = embed_strings_without_late_chunking([s for d in docs for s in d], config=config, embedder=embedder)
        return [flat[bounds[i] : bounds[i + 1]] for i in range(len(docs))]
    embedder = embedder or embedder_for(config)
    segments = []  # (text, token counts of its sentences, index of its first content sentence)
    for sentences in docs:
        num_tokens = count_sentence_tokens(sentences, embedder)
        for seg_start, content_start, seg_end in plan_segments(num_tokens, embedder.n_ctx(), embedder.n_batch):
            segments.append(("".join(sentences[seg_start:seg_end]), num_tokens[seg_start:seg_end], content_start - seg_start))
    token_blocks, begins, ends = [], [], []
    base = 0
    for lo, hi in pack_runs([int(s[1].sum()) for s in segments], int(getattr(embedder, "pack_tokens", embedder.n_batch))):
        mats = embedder.embed([s[0] for s in segments[lo:hi]])
        for (_, seg_tokens, first), mat in zip(segments[lo:hi], mats):
            tokens = _token_matrix(mat)
            edges = base + np.concatenate(([0], np.cumsum(split_rows(len(tokens), seg_tokens))))
            begins.append(edges[first:-1])
            ends.append(edges[first + 1 :])
            token_blocks.append(tokens)
            base += len(tokens)
    pooled = _pool(_stack(token_blocks), np.concatenate(begins).astype(np.int64), np.concatenate(ends).astype(np.int64),
                   normalize=bool(config.embedder_normalize), eps=0.0)
    return [pooled[bounds[i] : bounds[i + 1]] for i in range(len(docs))]
