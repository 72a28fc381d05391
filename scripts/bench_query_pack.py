"""The text queries of a batched search: the loop of single native embeds against ONE packed native forward with its tail.

    python scripts/bench_query_pack.py [--rounds 5] [--batches 1,4,16,64,256] [--big-rows 1000000] [--out profiles/query_pack_bench.json]

The method is scripts/bench_query_encode.py's: bge-m3's shape (24 layers, hidden 1024, 16 heads, ffn 4096), random weights, bf16, ONE
encoder module behind every route, the routes alternating inside every round, the median over rounds with the smallest and the largest
round next to it, and two clocks per figure:
  device_ms  the span between two device events around `iters` back-to-back calls, per call
  wall_ms    the host clock around one call and the synchronise that ends it, per call
Per batch of B queries of 8 .. 16 tokens, to the (B, 1024) float32 query matrix the searches take:
  loop          `_search._embed_one_by_one` over a `short_forward="native"` embedder: one native forward, one `rl_pool_norm` (and one
                `rl_adapter_apply`) per query -- what the batched searches did before the pack route, the function unchanged: the yardstick
  pack          `_search._embed_queries`: one `rl_encoder_forward_pack`, one `rl_pool_norm`, (one `rl_adapter_apply_rows`,) one read-back
  torch_packed  `embed(list)` with `batching="packed"`: torch's forward of the same pack, token matrices only (no tail), for the record --
                its rows are NOT the single call's bits
and `hybrid_search_batch` of 256 query strings over a `--big-rows` x 1024 index with a Zipf keyword side (scripts/bench_hybrid.py's),
with the pack route and with `_embed_queries` put back to the loop.  Needs a GPU: there is no fallback."""

from __future__ import annotations

import argparse
import copy
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

WORDS = ["gpu", "wave", "tile", "rows", "fuse", "rank", "scan", "norm", "head", "span", "mask", "pool"]


def text_of(n_tokens: int, salt: int) -> str:
    """A string of exactly n_tokens tokens under HashTokenizer with <s> and </s> (words of up to four letters and single blanks are one
    token each); `salt` picks the words."""
    inner = n_tokens - 2
    words = [WORDS[(salt + 5 * i) % len(WORDS)] for i in range((inner + 1) // 2)]
    return " ".join(words) + (" " if words and inner % 2 == 0 else "")


def queries_of(B: int) -> list[str]:  # noqa: N803
    return [text_of(8 + (3 * b) % 9, b) for b in range(B)]  # 8 .. 16 tokens, 12 on average


def main() -> None:  # noqa: PLR0915
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=lambda s: [int(x) for x in s.split(",")], default=[1, 4, 16, 64, 256])
    ap.add_argument("--big-rows", type=int, default=1_000_000)
    ap.add_argument("--terms", type=int, default=200_000)
    ap.add_argument("--mean-len", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "query_pack_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import raglite_amd
    from raglite_amd import _keyword, _ops, _search
    from raglite_amd._encoder import MAX_PACK_TOKENS, MAX_TOKENS
    from raglite_amd._torch_embedder import EncoderShape, TorchTokenEmbedder

    if not torch.cuda.is_available():
        raise SystemExit("bench_query_pack.py measures on a GPU; none is visible")
    raglite_amd.set_device(0)
    shape = EncoderShape()
    base = TorchTokenEmbedder(shape, device="cuda", dtype=torch.bfloat16)
    native, packed = copy.copy(base), copy.copy(base)  # the same module and tokenizer behind two switches
    native.short_forward, native._native = "native", None  # noqa: SLF001
    packed.batching = "packed"
    raglite_amd.set_embedder_factory(lambda config: native)

    def clocks(call, iters: int) -> tuple[float, float]:
        call()
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            call()
        end.record()
        torch.cuda.synchronize()
        device_ms = start.elapsed_time(end) / iters
        t0 = time.perf_counter()
        for _ in range(iters):
            call()
            torch.cuda.synchronize()
        return device_ms, (time.perf_counter() - t0) * 1e3 / iters

    def measure(cases: dict, iters_of: dict) -> dict:
        """cases: label -> {route: callable}.  Every round runs every route of every case once, the routes alternating."""
        samples = {label: {r: ([], []) for r in calls} for label, calls in cases.items()}
        for calls in cases.values():  # warm-up: code objects, hipBLASLt's choices, the native handle, the workspace
            for call in calls.values():
                for _ in range(2):
                    call()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for label, calls in cases.items():
                for r, call in calls.items():
                    d, w = clocks(call, iters_of[label])
                    samples[label][r][0].append(d)
                    samples[label][r][1].append(w)
        stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}  # noqa: E731
        return {label: {r: {"device_ms": stat(d), "wall_ms": stat(w)} for r, (d, w) in rs.items()} for label, rs in samples.items()}

    result = {"shape": "bge-m3 (24 x 1024, 16 heads, ffn 4096), random weights, bf16", "rounds": args.rounds, "max_tokens": MAX_TOKENS,
              "max_pack_tokens": MAX_PACK_TOKENS, "device": torch.cuda.get_device_name(0), "queries": "8 .. 16 tokens each, 12 on average"}

    class Adapter:  # what `_embed_queries` reads of an index
        query_adapter = None

    with_adapter = Adapter()
    with_adapter.query_adapter = (np.eye(shape.hidden) + 0.01 * np.random.default_rng(1).standard_normal((shape.hidden, shape.hidden))).astype(np.float32)
    cases, iters_of, same = {}, {}, {}
    for B in args.batches:  # noqa: N806
        qs = queries_of(B)
        tokens = sum(len(base.tokenizer.encode(q)) + 2 for q in qs)
        for tag, gi, cfg in (("", Adapter(), raglite_amd.HotPathConfig(vector_search_query_adapter=False)),
                             ("_adapter", with_adapter, raglite_amd.HotPathConfig(vector_search_query_adapter=True))):
            if tag and B not in (1, 16, 256):
                continue
            label = f"embed_{B}_queries{tag}"
            cases[label] = {"loop": (lambda qs=qs, gi=gi, cfg=cfg: _search._embed_one_by_one(qs, None, cfg, gi)),  # noqa: SLF001
                            "pack": (lambda qs=qs, gi=gi, cfg=cfg: _search._embed_queries(qs, None, cfg, gi))}  # noqa: SLF001
            if not tag:
                cases[label]["torch_packed"] = lambda qs=qs: packed.embed(qs)
            iters_of[label] = max(1, 16 // B)
            same[label] = {"tokens": tokens, "pack_equals_loop_bits": bool(np.array_equal(cases[label]["loop"](), cases[label]["pack"]()))}
    result["embed"] = measure(cases, iters_of)
    for label, s in same.items():
        result["embed"][label].update(s)

    # hybrid_search_batch of 256 strings over a big index: the pack route against the loop put back in its place
    from tests import keyword_ref as ref

    rng = np.random.default_rng(0)
    t0 = time.perf_counter()
    flat, off = ref.zipf_corpus(rng, args.big_rows, args.terms, args.mean_len)
    postings = _keyword.build_from_term_ids(flat, off, args.terms)
    del flat
    E = torch.empty((args.big_rows, shape.hidden), dtype=torch.float32, device="cuda")  # noqa: N806
    raglite_amd.synth_fill(E, seed=7, kind="uniform")
    gi = raglite_amd.GpuIndex([f"c{i}" for i in range(args.big_rows)], E, chunk_offsets=np.arange(args.big_rows + 1, dtype=np.int64))
    gi.keyword, gi._kw_stems = _ops.KeywordIndex(postings), [[]]  # noqa: SLF001 - the Zipf postings directly: queries look their term ids up by text
    qs = queries_of(256)
    terms = {q: sorted({int(x) for x in t}) for q, t in zip(qs, ref.zipf_queries(rng, len(qs), args.terms, lo=4, hi=12))}
    gi.keyword_query_ids = lambda q: terms[q]
    cfg = raglite_amd.HotPathConfig(vector_search_query_adapter=False)
    setup_s = time.perf_counter() - t0
    pack_route = _search._embed_queries  # noqa: SLF001

    def loop_route(queries, query_vectors, cfg, gi, pack=None):  # noqa: ARG001 - the parent's body of the batched searches
        return _search._embed_one_by_one(queries, query_vectors, cfg, gi)  # noqa: SLF001

    def search(route):
        _search._embed_queries = route  # noqa: SLF001
        try:
            return raglite_amd.hybrid_search_batch(qs, num_results=8, oversample=4, config=cfg, index=gi)
        finally:
            _search._embed_queries = pack_route  # noqa: SLF001

    Q = pack_route(qs, None, cfg, gi)  # noqa: N806
    label = f"hybrid_search_batch_256_strings_{args.big_rows}_rows"
    got = {"loop": search(loop_route), "pack": search(pack_route)}
    m = measure({label: {"loop": lambda: search(loop_route), "pack": lambda: search(pack_route),
                         "given_vectors": lambda: raglite_amd.hybrid_search_batch(qs, num_results=8, oversample=4, config=cfg, index=gi, query_vectors=Q)}},
                {label: 1})
    m[label].update({"same_ids_and_scores_both_routes": got["loop"] == got["pack"], "setup_s": round(setup_s, 1), "postings": int(postings.post_chunk.size)})
    result["hybrid_search_batch"] = m
    raglite_amd.set_embedder_factory(None)
    gi.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    for label, rs in {**result["embed"], **result["hybrid_search_batch"]}.items():
        print(label, {r: (round(v["device_ms"]["median"], 3), round(v["wall_ms"]["median"], 3)) for r, v in rs.items() if isinstance(v, dict)},
              {k: v for k, v in rs.items() if not isinstance(v, dict)})


if __name__ == "__main__":
    main()
