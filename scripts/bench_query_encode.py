"""A text query end to end: torch's encoder forward against the native forward for short packs.

    python scripts/bench_query_encode.py [--rounds 7] [--iters 20] [--big-rows 1000000] [--out profiles/encoder_native_bench.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_query_encode.py --trace     (a run of its own)

bge-m3's shape (24 layers, hidden 1024, 16 heads, ffn 4096), random weights, bf16, ONE encoder module shared by the three routes --
"torch_padded", "torch_packed" (`batching`) and "native" (`short_forward`) -- in one process, the routes alternating inside every
round, the median over rounds reported with the smallest and the largest round next to it.  Two clocks per figure:
  device_ms  the span between two device events around `iters` back-to-back calls, per call (what a stream of queries costs)
  wall_ms    the host clock around one call and the synchronise that ends it, per call (what one query waits)
Measured: embed(str) at 8 .. 256 tokens, embed(list) of 4 and 16 short queries, and vector_search(str) over a 10 k-row and a
`--big-rows` x 1024 index.  Needs a GPU: there is no fallback."""

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
TOKEN_COUNTS = (8, 16, 32, 64, 128, 256)
ROUTES = ("torch_padded", "torch_packed", "native")


def text_of(n_tokens: int) -> str:
    """A string of exactly n_tokens tokens under HashTokenizer with <s> and </s>: words of up to four letters and single blanks are one
    token each."""
    inner = n_tokens - 2
    words = [WORDS[i % len(WORDS)] for i in range((inner + 1) // 2)]
    return " ".join(words) + (" " if words and inner % 2 == 0 else "")


def linear_bounds(shape, hbm_bytes_per_s: float) -> dict:
    """The weight-streaming bound of each linear layer: bytes of W over the HBM rate (the least time a projection of a few rows can take)."""
    h, f = shape.hidden, shape.ffn
    return {name: {"weight_bytes": 2 * n * k, "bound_us": 2 * n * k / hbm_bytes_per_s * 1e6}
            for name, (n, k) in {"qkv": (3 * h, h), "out": (h, h), "up": (f, h), "down": (h, f)}.items()}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--big-rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "encoder_native_bench.json"))
    ap.add_argument("--trace", action="store_true", help="only a few native forwards of 16 tokens: the run a kernel trace is taken of")
    args = ap.parse_args()

    import numpy as np
    import torch

    import raglite_amd
    from raglite_amd._encoder import MAX_TOKENS
    from raglite_amd._torch_embedder import EncoderShape, TorchTokenEmbedder

    if not torch.cuda.is_available():
        raise SystemExit("bench_query_encode.py measures on a GPU; none is visible")
    raglite_amd.set_device(0)
    shape = EncoderShape()
    base = TorchTokenEmbedder(shape, device="cuda", dtype=torch.bfloat16)
    emb = {}
    for route in ROUTES:  # the same module and tokenizer behind three switches
        e = copy.copy(base)
        e.batching = "packed" if route == "torch_packed" else "padded"
        e.short_forward, e._native = ("native" if route == "native" else "torch"), None  # noqa: SLF001
        emb[route] = e

    if args.trace:
        q = text_of(16)
        for _ in range(5):
            emb["native"].embed(q)
        torch.cuda.synchronize()
        print(json.dumps({"trace": "5 native forwards of 16 tokens", "launches_per_forward": emb["native"]._native.info()["launches"]}))  # noqa: SLF001
        return

    def clocks(call) -> tuple[float, float]:
        call()
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.iters):
            call()
        end.record()
        torch.cuda.synchronize()
        device_ms = start.elapsed_time(end) / args.iters
        t0 = time.perf_counter()
        for _ in range(args.iters):
            call()
            torch.cuda.synchronize()
        return device_ms, (time.perf_counter() - t0) * 1e3 / args.iters

    def measure(cases: dict) -> dict:
        """cases: label -> {route: callable}.  Every round runs every route of every case once, the routes alternating."""
        samples = {label: {r: ([], []) for r in calls} for label, calls in cases.items()}
        for label, calls in cases.items():  # warm-up: code objects, hipBLASLt's choices, the native handle
            for call in calls.values():
                for _ in range(3):
                    call()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for label, calls in cases.items():
                for r, call in calls.items():
                    d, w = clocks(call)
                    samples[label][r][0].append(d)
                    samples[label][r][1].append(w)
        stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}  # noqa: E731
        return {label: {r: {"device_ms": stat(d), "wall_ms": stat(w)} for r, (d, w) in rs.items()} for label, rs in samples.items()}

    result = {"shape": "bge-m3 (24 x 1024, 16 heads, ffn 4096), random weights, bf16", "rounds": args.rounds, "iters": args.iters,
              "max_tokens": MAX_TOKENS, "device": torch.cuda.get_device_name(0)}
    cases = {}
    for n in TOKEN_COUNTS:
        q = text_of(n)
        assert len(base.tokenizer.encode(q)) + 2 == n, (n, len(base.tokenizer.encode(q)))
        cases[f"embed_str_{n}_tokens"] = {r: (lambda e=emb[r], q=q: e.embed(q)) for r in ROUTES}
    for count in (4, 16):
        qs = [text_of(8 + (3 * i) % 7) for i in range(count)]  # 8 .. 14 tokens each: 16 of them stay under the cap
        assert sum(len(base.tokenizer.encode(q)) + 2 for q in qs) <= MAX_TOKENS
        cases[f"embed_list_{count}_queries"] = {r: (lambda e=emb[r], qs=qs: e.embed(qs)) for r in ROUTES}
    result["embed"] = measure(cases)

    cfg = raglite_amd.HotPathConfig(vector_search_query_adapter=False)
    query = text_of(16)
    result["vector_search"] = {}
    for rows in (10_000, args.big_rows):
        E = torch.empty((rows, shape.hidden), dtype=torch.float32, device="cuda")  # noqa: N806
        raglite_amd.synth_fill(E, seed=7, kind="uniform")
        gi = raglite_amd.GpuIndex([f"c{i}" for i in range(rows)], E, chunk_offsets=np.arange(rows + 1, dtype=np.int64))

        def search(route, gi=gi):
            raglite_amd.set_embedder_factory(lambda config: emb[route])
            return raglite_amd.vector_search(query, num_results=10, config=cfg, index=gi)

        got = {r: search(r) for r in ("torch_padded", "native")}
        same = got["torch_padded"][0] == got["native"][0]
        m = measure({f"vector_search_{rows}_rows": {r: (lambda r=r: search(r)) for r in ("torch_padded", "native")}})
        m[f"vector_search_{rows}_rows"]["same_ids_both_routes"] = same
        result["vector_search"].update(m)
        gi.close()
        del E
    raglite_amd.set_embedder_factory(None)
    result["linear_bounds_at_8_TB_s"] = linear_bounds(shape, 8e12)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    for label, rs in {**result["embed"], **result["vector_search"]}.items():
        print(label, {r: (round(v["device_ms"]["median"], 3), round(v["wall_ms"]["median"], 3)) for r, v in rs.items() if isinstance(v, dict)})


if __name__ == "__main__":
    main()
