"""Cross-encoder rerank of a batch of queries: torch's routes against the native forward and its `rank_batch`.

    python scripts/bench_cross_encoder_batch.py [--rounds 5] [--out profiles/cross_encoder_bench.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_cross_encoder_batch.py --trace     (a run of its own)

(scripts/bench_cross_encoder.py is the older single-query throughput figure of the torch route against the CPU.)

The real ms-marco-MiniLM-L-12 shape (12 layers, hidden 384, 12 heads, ffn 1536), random weights, bf16, ONE encoder module behind four
routes -- "torch_padded" and "torch_packed" (`batching`, a loop of `rank`), "native_per_query" (`forward="native"`, a loop of `rank`) and
"native_rank_batch" (one `rank_batch`) -- in one process, the routes alternating inside every round, the median over rounds reported
with the smallest and the largest round next to it.  Workloads: 1, 16 and 64 queries x 32 candidates of 100 .. 300 tokens (the
reference reranks oversample * num_results = 32 candidates per query).  Two clocks per figure, tokenisation included in both (it is
part of `rank`):
  device_ms  the span between two device events around `iters` back-to-back calls, per call
  wall_ms    the host clock around one call (every route ends in a copy of the scores to the host), per call
Needs a GPU: there is no fallback."""

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

ROUTES = ("torch_padded", "torch_packed", "native_per_query", "native_rank_batch")
WORKLOADS = {1: 10, 16: 2, 64: 1}  # queries -> calls between two device events
CANDIDATES = 32
WORDS = ["gpu", "wave", "tile", "rows", "fuse", "rank", "scan", "norm", "head", "span", "mask", "pool"]


def text_of(n_tokens: int, salt: int) -> str:
    """About n_tokens tokens under HashTokenizer: words of up to four letters and single blanks are one token each."""
    return " ".join(WORDS[(salt + 5 * i) % len(WORDS)] for i in range(max(1, n_tokens // 2)))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cross_encoder_bench.json"))
    ap.add_argument("--trace", action="store_true", help="only three rank_batch calls of 16 queries: the run a kernel trace is taken of")
    args = ap.parse_args()

    import numpy as np
    import torch

    import raglite_amd
    from raglite_amd._cross_encoder import TorchCrossEncoderRanker

    if not torch.cuda.is_available():
        raise SystemExit("bench_cross_encoder_batch.py measures on a GPU; none is visible")
    raglite_amd.set_device(0)
    base = TorchCrossEncoderRanker.minilm_l12_shaped(device="cuda", dtype=torch.bfloat16)
    rankers = {}
    for route in ROUTES:  # the same module and tokenizer behind the switches
        r = copy.copy(base)
        r.batching = "packed" if route == "torch_packed" else "padded"
        r.forward, r._native = ("native" if route.startswith("native") else "torch"), None  # noqa: SLF001
        rankers[route] = r
    rankers["native_rank_batch"]._native = rankers["native_per_query"]._native_encoder()  # noqa: SLF001  (one handle for both)

    rng = np.random.default_rng(0)

    def workload(n_queries: int):
        queries = [text_of(int(rng.integers(8, 24)), b) for b in range(n_queries)]
        docs = [[text_of(int(rng.integers(100, 301)), 7 * b + c) for c in range(CANDIDATES)] for b in range(n_queries)]
        return queries, docs

    def call_of(route: str, queries, docs):
        r = rankers[route]
        if route == "native_rank_batch":
            return lambda: r.rank_batch(queries, docs)
        return lambda: [r.rank(q, d) for q, d in zip(queries, docs)]

    if args.trace:
        queries, docs = workload(16)
        for _ in range(3):
            rankers["native_rank_batch"].rank_batch(queries, docs)
        torch.cuda.synchronize()
        print(json.dumps({"trace": "3 rank_batch calls of 16 queries x 32 candidates", "pack_forwards": rankers["native_rank_batch"].native.pack_forwards}))
        return

    def clocks(call, iters: int) -> tuple[float, float]:
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(iters):
            call()
        end.record()
        torch.cuda.synchronize()
        device_ms = start.elapsed_time(end) / iters
        t0 = time.perf_counter()
        for _ in range(iters):
            call()
        return device_ms, (time.perf_counter() - t0) * 1e3 / iters

    result = {"shape": "ms-marco-MiniLM-L-12 (12 x 384, 12 heads, ffn 1536), random weights, bf16", "rounds": args.rounds,
              "candidates": CANDIDATES, "doc_tokens": "100 .. 300", "device": torch.cuda.get_device_name(0), "workloads": {}}
    stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}  # noqa: E731
    for n_queries, iters in WORKLOADS.items():
        queries, docs = workload(n_queries)
        calls = {route: call_of(route, queries, docs) for route in ROUTES}
        tokens = sum(len(p[0]) for q, d in zip(queries, docs) for p in base.encode_pairs(q, d))
        native = rankers["native_rank_batch"].native
        same = True
        for route, call in calls.items():  # warm-up: code objects, hipBLASLt's choices, the workspace -- and the contract, while we are here
            got = call()
            if route == "native_per_query":
                loop = got
            if route == "native_rank_batch":
                same = all([(x.doc_id, x.score) for x in g.results] == [(x.doc_id, x.score) for x in w.results] for g, w in zip(got, loop))
        n0 = native.pack_forwards
        calls["native_rank_batch"]()
        forwards = native.pack_forwards - n0
        samples = {route: ([], []) for route in ROUTES}
        for _ in range(args.rounds):
            for route, call in calls.items():
                d, w = clocks(call, iters)
                samples[route][0].append(d)
                samples[route][1].append(w)
        entry = {route: {"device_ms": stat(d), "wall_ms": stat(w)} for route, (d, w) in samples.items()}
        entry.update({"queries": n_queries, "pairs": n_queries * CANDIDATES, "tokens": tokens, "iters": iters,
                      "rank_batch_forwards": forwards, "rank_batch_equals_the_loop": same})
        result["workloads"][f"{n_queries}_queries"] = entry
        print(n_queries, "queries,", tokens, "tokens,", forwards, "forwards:",
              {route: (round(entry[route]["device_ms"]["median"], 2), round(entry[route]["wall_ms"]["median"], 2)) for route in ROUTES}, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
