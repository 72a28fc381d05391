"""Cross-encoder reranker in PyTorch-ROCm ("GPU cross-encoder rerank as an alternative
`BaseRanker`").

The reference's default rerankers are FlashRank cross-encoders -- `FlashRankRanker("ms-marco-MiniLM-L-12-v2")` for
English, `ms-marco-MultiBERT-L-12` otherwise (`src/raglite/_config.py:72-78`) -- called through
`reranker.rank(query=, docs=)` at `src/raglite/_search.py:394-396`.  FlashRank (a third-party dependency, absent from
the reference tree and from this image) runs the ONNX export of a BERT sequence classifier on the CPU, one
`[CLS] query [SEP] passage [SEP]` pair per candidate, and maps the single logit through a sigmoid.  This module is that
forward pass on the GPU behind the same plugin surface: a BERT encoder in the ms-marco-MiniLM-L-12 shape (12 layers,
d = 384, 12 heads, FFN 1536, vocabulary 30 522, 512 positions, two segment types), the pooler (dense + tanh on the
first token) and a one-logit head; all candidates of a query go through the encoder in length-sorted padded batches.

    config.reranker = TorchCrossEncoderRanker.minilm_l12_shaped(device="cuda")     # or {"en": ..., "other": ...}

PyTorch is plumbing here (GEMMs through hipBLASLt, attention through SDPA), as for `_torch_embedder.py`; the module
shares that encoder.  Its arithmetic is pinned against Hugging Face's `BertForSequenceClassification` with the same
weights (`tests/test_host_logic.py`, `tests/test_gpu_parity.py`).  No checkpoint can be fetched in this environment:
weights are random-initialised in the architecture's shape unless `load_hf_state_dict` is given the published ones,
and the default tokenizer is the hashing stand-in; pass `tokenizer=` (anything with `encode(str) -> list[int]`, e.g. the
model's WordPiece `tokenizers.Tokenizer` wrapped to return ids without special tokens) for real text.

`forward="native"` sends the pairs through the native encoder and its head kernel instead (`rl_encoder_classify_pack`:
one C call per pack of at most 8192 tokens), and `rank_batch` then reranks ALL queries of a batch in one forward per pack, every
`RankedResults` equal to `rank`'s for that query: a pair's logit bits do not depend on the pack it sits in.

With `tokenizer=DeviceWordPiece(tables)` on that route, the text itself goes to the device: the distinct strings of a
call are tokenized once by the WordPiece kernels, the `[CLS] q [SEP] d [SEP]` rows are assembled there, and only the pairs' offsets
come back before the forwards -- the same `doc_id`s, order and score bits as with the mirrored tokenizer wrapped as `encode`.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Sequence

from raglite_amd._torch_embedder import (BATCHING_MODES, EncoderShape, HashTokenizer, _build_encoder, native_state_from_hf, pack_runs,
                                         packed_inputs)


@dataclass(frozen=True)
class CrossEncoderShape(EncoderShape):
    """ms-marco-MiniLM-L-12-v2 (BERT, uncased WordPiece vocabulary)."""

    vocab_size: int = 30_522
    hidden: int = 384
    layers: int = 12
    heads: int = 12
    ffn: int = 1536
    max_positions: int = 512
    n_ctx: int = 512
    layer_norm_eps: float = 1e-12
    pad_id: int = 0
    bos_id: int = 101  # [CLS]
    eos_id: int = 102  # [SEP]
    type_vocab: int = 2
    position_offset: int = 0
    classifier: bool = True


FORWARD_MODES = ("torch", "native")


def _lengths(offsets: Any) -> list[int]:
    """The lengths behind host offsets, as Python integers."""
    return [int(b) - int(a) for a, b in zip(offsets[:-1], offsets[1:])]


def truncate_pair(n_query: int, n_doc: int, budget: int) -> tuple[int, int]:
    """Token counts kept of (query, passage) when the pair exceeds `budget`: the `longest_first` strategy of the
    `tokenizers` library FlashRank truncates with -- drop one token at a time from the longer sequence, from the
    passage on a tie -- in closed form."""
    over = n_query + n_doc - budget
    if over <= 0:
        return n_query, n_doc
    if n_query > n_doc:
        cut = min(over, n_query - n_doc)
        n_query, over = n_query - cut, over - cut
    elif n_doc > n_query:
        cut = min(over, n_doc - n_query)
        n_doc, over = n_doc - cut, over - cut
    n_doc -= (over + 1) // 2
    n_query -= over // 2
    return max(n_query, 0), max(n_doc, 0)


class TorchCrossEncoderRanker:
    """`rank(query=, docs=)` of the `rerankers.BaseRanker` surface the reference calls, on the GPU."""

    def __init__(self, shape: CrossEncoderShape | None = None, *, tokenizer: Any | None = None, device: str = "cuda",
                 dtype: Any | None = None, seed: int = 0, max_length: int | None = None, pairs_per_batch: int = 128,
                 batching: str = "padded", pack_tokens: int = 16384, forward: str = "torch") -> None:
        """batching "padded" (default): length-sorted padded batches of `pairs_per_batch` pairs; "packed": the pairs in input order in
        unpadded packs of at most `pack_tokens` tokens (`Encoder.forward_packed`; `pairs_per_batch` is ignored).
        forward "torch" (default): the module's own forward; "native": on a GPU in bf16 / fp16 with a shape the native encoder takes,
        the pairs in input order in packs of at most min(`pack_tokens`, 8192) tokens through `NativeEncoder.classify_rows`, whatever
        `batching` says; where that does not apply (CPU, fp32, an unsupported width) the `batching` route, silently."""
        import torch

        if batching not in BATCHING_MODES:
            raise ValueError('batching must be "padded" or "packed"')
        if forward not in FORWARD_MODES:
            raise ValueError('forward must be "torch" or "native"')
        self.forward = forward
        self._native: Any | None = None  # the NativeEncoder, made on the first native forward
        if pack_tokens < 1:
            raise ValueError("pack_tokens must be >= 1")
        self.batching, self.pack_tokens = batching, int(pack_tokens)
        self.shape = shape or CrossEncoderShape()
        if not self.shape.classifier:
            raise ValueError("a cross-encoder needs shape.classifier = True")
        self.tokenizer = tokenizer or HashTokenizer(self.shape.vocab_size, reserved=max(self.shape.eos_id, self.shape.bos_id) + 1)
        self.device = torch.device(device)
        self.dtype = dtype or (torch.bfloat16 if self.device.type == "cuda" else torch.float32)
        self.max_length = min(max_length or self.shape.n_ctx, self.shape.n_ctx, self.shape.max_positions - self.shape.position_offset)
        self.pairs_per_batch = pairs_per_batch
        gen_state = torch.random.get_rng_state()
        torch.manual_seed(seed)
        self.encoder = _build_encoder(self.shape).to(device=self.device, dtype=self.dtype).eval()
        torch.random.set_rng_state(gen_state)

    @classmethod
    def minilm_l12_shaped(cls, **kw: Any) -> "TorchCrossEncoderRanker":
        return cls(CrossEncoderShape(), **kw)

    def load_hf_state_dict(self, state: dict) -> None:
        """Weights in the layout the ms-marco cross-encoders are published in (`BertForSequenceClassification`)."""
        self.encoder.load_state_dict({k: v.to(self.dtype) for k, v in native_state_from_hf(state, self.shape).items()})

    # ------------------------------------------------------------------------------------------------------
    def encode_pairs(self, query: str, docs: Sequence[str]) -> list[tuple[list[int], int]]:
        """Per doc: the ids of `[CLS] q [SEP] d [SEP]` and the length of the first segment (type 0) inside them."""
        q_ids = list(self.tokenizer.encode(query))
        out = []
        for d in docs:
            d_ids = list(self.tokenizer.encode(d))
            nq, nd = truncate_pair(len(q_ids), len(d_ids), self.max_length - 3)
            out.append(([self.shape.bos_id, *q_ids[:nq], self.shape.eos_id, *d_ids[:nd], self.shape.eos_id], nq + 2))
        return out

    # ---- the native route -----------------------------------------------------------------
    def _native_applies(self) -> bool:
        """Does `forward="native"` hold for this ranker as it stands (its module's device and dtype are looked at on every call: a
        `.to(...)` of the module changes the answer)?"""
        if self.forward != "native":
            return False
        from raglite_amd._encoder import NativeEncoder

        w = self.encoder.tok.weight
        return NativeEncoder.supports_pack(self.shape, w.dtype, 1, w.device, classify=True)

    def _native_encoder(self) -> Any:
        if self._native is None:
            from raglite_amd._encoder import NativeEncoder

            self._native = NativeEncoder(self.encoder, self.shape)
        return self._native

    @property
    def native(self) -> Any | None:
        """The `NativeEncoder` behind `forward="native"` (its `pack_forwards` counts the forwards made), or None before the first one."""
        return self._native

    def _native_logits(self, pairs: Sequence[tuple[list[int], int]]):  # noqa: ANN202
        """The logits of encoded pairs, in order: packs of consecutive pairs of at most min(pack_tokens, 8192) tokens, one
        `classify_rows` each.  Where the cuts fall changes no bit: a pair's logit is a function of the pair alone."""
        import torch

        from raglite_amd._encoder import MAX_PACK_TOKENS

        native = self._native_encoder()
        parts = []
        for lo, hi in pack_runs([len(p[0]) for p in pairs], min(self.pack_tokens, MAX_PACK_TOKENS)):
            rows = [p[0] for p in pairs[lo:hi]]
            types = [[0] * first + [1] * (len(r) - first) for r, (_, first) in zip(rows, pairs[lo:hi])]
            parts.append(native.classify_rows(rows, types))
        if not parts:
            return torch.empty(0, dtype=torch.float32, device=self.device)
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def _device_pairs_apply(self) -> bool:
        """Does text go to logits on the device?  Only with a tokenizer that assembles the pairs there
        (`DeviceWordPiece.encode_pairs_device`) AND the native route; every other combination runs the code it ran before."""
        return hasattr(self.tokenizer, "encode_pairs_device") and self._native_applies()

    def _device_logits(self, queries: Sequence[str], docs_per_query: Sequence[Sequence[str]]):  # noqa: ANN202
        """The logits of the pairs (query b, each of its docs), in query and then doc order: the distinct strings tokenized once and the
        rows assembled on the device, the n_pairs + 1 offsets read back, the packs cut by `_native_logits`' rule and every pack a slice of
        the four arrays with its offsets rebased."""
        import torch

        from raglite_amd._encoder import MAX_PACK_TOKENS

        ids, positions, type_ids, seq, seq_host = self.tokenizer.encode_pairs_device(queries, docs_per_query, self.max_length, self.shape)
        lens = _lengths(seq_host)
        native = self._native_encoder()
        parts = []
        for lo, hi in pack_runs(lens, min(self.pack_tokens, MAX_PACK_TOKENS)):
            t0, t1 = int(seq_host[lo]), int(seq_host[hi])
            parts.append(native.classify_pack_i32(ids[t0:t1], positions[t0:t1], seq[lo: hi + 1] - t0, type_ids[t0:t1], hi - lo, t1 - t0, max(lens[lo:hi])))
        if not parts:
            return torch.empty(0, dtype=torch.float32, device=self.device)
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def logits(self, query: str, docs: Sequence[str]):  # noqa: ANN201
        """(len(docs),) float32 tensor of relevance logits on `self.device`."""
        import torch

        if self._device_pairs_apply():
            return self._device_logits([query], [list(docs)])
        pairs = self.encode_pairs(query, docs)
        if self._native_applies():
            return self._native_logits(pairs)
        out = torch.empty(len(pairs), dtype=torch.float32, device=self.device)
        if self.batching == "packed":
            for lo, hi in pack_runs([len(p[0]) for p in pairs], self.pack_tokens):
                rows = [p[0] for p in pairs[lo:hi]]
                types = [[0] * first + [1] * (len(r) - first) for r, (_, first) in zip(rows, pairs[lo:hi])]
                ids, off, lens, type_ids = packed_inputs(rows, self.device, types)
                with torch.inference_mode():
                    out[lo:hi] = self.encoder.forward_packed(ids, off, lens, type_ids).float()
            return out
        order = sorted(range(len(pairs)), key=lambda i: len(pairs[i][0]))  # length-sorted batches: little padding
        for lo in range(0, len(order), self.pairs_per_batch):
            sel = order[lo : lo + self.pairs_per_batch]
            lengths = torch.tensor([len(pairs[i][0]) for i in sel])
            T = int(lengths.max())  # noqa: N806
            ids = torch.full((len(sel), T), self.shape.pad_id, dtype=torch.long)
            for r, i in enumerate(sel):
                ids[r, : len(pairs[i][0])] = torch.tensor(pairs[i][0], dtype=torch.long)
            first = torch.tensor([pairs[i][1] for i in sel])
            ar = torch.arange(T)
            type_ids = ((ar[None, :] >= first[:, None]) & (ar[None, :] < lengths[:, None])).long()
            with torch.inference_mode():
                z = self.encoder(ids.to(self.device), lengths.to(self.device), type_ids.to(self.device))
            out[torch.tensor(sel, device=self.device)] = z.float()
        return out

    def score(self, query: str, docs: Sequence[str]):  # noqa: ANN201
        """FlashRank's score: sigmoid of the logit, as a NumPy float32 vector in input order."""
        import torch

        return torch.sigmoid(self.logits(query, docs)).cpu().numpy()

    def rank(self, query: str, docs: Sequence[Any], doc_ids: Sequence[int] | None = None, **_: Any):  # noqa: ANN201
        import numpy as np

        from raglite_amd._search import RankedResults, Result

        docs = [d if isinstance(d, str) else str(d) for d in docs]
        if not docs:
            return RankedResults([], query)
        scores = self.score(query, docs)
        key = np.where(np.isnan(scores), -np.inf, scores)
        order = np.lexsort((np.arange(len(docs)), -key))  # best first; equal scores keep input order
        ids = list(doc_ids) if doc_ids is not None else list(range(len(docs)))
        return RankedResults(
            [Result(doc_id=ids[i], score=float(scores[i]), rank=r + 1, text=docs[i]) for r, i in enumerate(order)], query)

    # ---- a batch of queries ----------------------------------------------------------------------------------
    def logits_batch(self, queries: Sequence[str], docs_per_query: Sequence[Sequence[str]]) -> list:
        """`logits(queries[b], docs_per_query[b])` for every b, with the same bits.  Native route: the pairs of ALL queries, in query
        order and then doc order, cut into packs by `logits`' rule -- one forward per pack, not per query.  Otherwise the loop."""
        queries, docs_per_query = list(queries), [list(d) for d in docs_per_query]
        if len(queries) != len(docs_per_query):
            raise ValueError("one list of docs per query is required")
        if not self._native_applies():
            return [self.logits(q, docs) for q, docs in zip(queries, docs_per_query)]
        if self._device_pairs_apply():
            bounds = [0]
            for docs in docs_per_query:
                bounds.append(bounds[-1] + len(docs))
            flat = self._device_logits(queries, docs_per_query)
            return [flat[lo:hi] for lo, hi in zip(bounds, bounds[1:])]
        pairs, bounds = [], [0]
        for q, docs in zip(queries, docs_per_query):
            pairs += self.encode_pairs(q, docs)
            bounds.append(len(pairs))
        flat = self._native_logits(pairs)
        return [flat[lo:hi] for lo, hi in zip(bounds, bounds[1:])]

    def score_batch(self, queries: Sequence[str], docs_per_query: Sequence[Sequence[str]]) -> list:
        """`score(queries[b], docs_per_query[b])` for every b: NumPy float32 vectors, the sigmoid taken by torch as in `score`."""
        import torch

        return [torch.sigmoid(z).cpu().numpy() for z in self.logits_batch(queries, docs_per_query)]

    def rank_batch(self, queries: Sequence[str], docs_per_query: Sequence[Sequence[Any]],
                   doc_ids_per_query: Sequence[Sequence[int] | None] | None = None) -> list:
        """`rank(queries[b], docs_per_query[b], doc_ids_per_query[b])` for every b -- the same `doc_id`s in the same order with the same
        score bits.  Native route: one forward per pack for the whole batch and one `rl_rerank_order` (ragged lists padded with candidate
        -1), whose order is `rank`'s lexsort: score descending, NaN as -inf, equal scores in input order.  Otherwise the loop of `rank`."""
        import numpy as np

        from raglite_amd import _ops
        from raglite_amd._search import RankedResults, Result

        queries = list(queries)
        docs_per_query = [[d if isinstance(d, str) else str(d) for d in docs] for docs in docs_per_query]
        ids_per_query = [None] * len(queries) if doc_ids_per_query is None else [None if i is None else list(i) for i in doc_ids_per_query]
        if len(queries) != len(docs_per_query) or len(queries) != len(ids_per_query):
            raise ValueError("one list of docs (and of doc ids, where given) per query is required")
        if not self._native_applies():
            return [self.rank(q, docs, ids) for q, docs, ids in zip(queries, docs_per_query, ids_per_query)]
        out = [RankedResults([], q) for q in queries]
        n_cand = max((len(docs) for docs in docs_per_query), default=0)
        if n_cand == 0:
            return out
        if n_cand > _ops.RERANK_MAX_ENTRIES:
            raise ValueError(f"TorchCrossEncoderRanker: at most {_ops.RERANK_MAX_ENTRIES} docs per query can be ordered on the device")
        scores = self.score_batch(queries, docs_per_query)
        padded = np.zeros((len(queries), n_cand), dtype=np.float32)
        cand = np.full((len(queries), n_cand), -1, dtype=np.int32)
        for b, sc in enumerate(scores):
            padded[b, : len(sc)] = sc
            cand[b, : len(sc)] = np.arange(len(sc), dtype=np.int32)
        _, _, pos, counts = _ops.rerank_order(padded, cand, n_cand)
        pos, counts = np.asarray(pos), np.asarray(counts)
        for b, (docs, ids, sc) in enumerate(zip(docs_per_query, ids_per_query, scores)):
            ids = ids if ids is not None else list(range(len(docs)))
            order = pos[b, : int(counts[b])].tolist()
            out[b] = RankedResults([Result(doc_id=ids[i], score=float(sc[i]), rank=r + 1, text=docs[i]) for r, i in enumerate(order)], queries[b])
        return out
