"""Batched search, rerank and chunk spans at corpus scale (search_and_rerank_chunk_spans_batch, rl_search_rerank_spans_per_query,
rl_chunk_spans).

    python scripts/bench_spans_batch.py [--chunks 1000000] [--dim 1024] [--batches 1,16,256] --out R.json
        the corpus of scripts/bench_hybrid.py (one row per chunk, synthetic, on the device; the Zipf keyword side) laid out in
        documents of 1 to 40 chunks, num_results 8, oversample 4, nq 32 token vectors per query, neighbours (-1, 1).  Per batch,
        after warm-up, with device events around each variant, every variant reading its results back:
          spans        search_and_rerank_chunk_spans_batch (one rl_search_rerank_spans_per_query call, one read-back)
          chunks_host  search_and_rerank_chunks_batch, then the Python restatement of retrieve_chunk_spans (tests/spans_ref.py) per
                       query: what a caller without the span kernel does once the positions are on the host
          chunks       search_and_rerank_chunks_batch alone: what `spans` adds to it is one launch, a larger read-back and the
                       ChunkSpan objects
          call_spans   DeviceIndex.search_rerank_spans with the batch's arguments prepared: the C call alone
          call_chunks  DeviceIndex.search_rerank likewise: what call_spans adds to it is the span kernel and its read-back
        and checks that spans and chunks_host return the same spans with the same scores.  Writes one JSON record.
    python scripts/bench_spans_batch.py --trace-summary kernel_trace.csv --out R.json
        adds chunk_spans_kernel's, rerank_order_kernel's and rrf_fuse_kernel's time per batch size (grid x = batch size) from a
        `rocprofv3 --kernel-trace` run of the first form.
"""

from __future__ import annotations

import argparse
import csv
import gc
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from scripts.bench_hybrid import build_index, timed

KERNELS = (("chunk_spans_kernel", "spans_kernel"), ("rerank_order_kernel", "order_kernel"), ("rrf_fuse_kernel", "fuse_kernel"))


def layout(rng, n_chunks: int, max_doc: int = 40) -> list[tuple[str, int]]:
    """Chunk c's (document_id, index): consecutive chunks fill documents of 1 to max_doc chunks."""
    positions: list[tuple[str, int]] = []
    d = 0
    while len(positions) < n_chunks:
        size = min(int(rng.integers(1, max_doc + 1)), n_chunks - len(positions))
        positions.extend((f"doc{d}", i) for i in range(size))
        d += 1
    return positions


def run(args) -> dict:
    import torch

    import raglite_amd
    from raglite_amd import _search
    from tests import keyword_ref
    from tests import spans_ref

    assert torch.cuda.is_available(), "bench_spans_batch needs a GPU"
    raglite_amd.set_device(0)
    t0 = time.perf_counter()
    gi, p, terms, rng = build_index(args)
    gi._rebuild_spans(layout(rng, args.chunks))  # noqa: SLF001
    table = spans_ref.Table(dict(zip(gi.chunk_ids, gi.positions)))
    tokens: dict[str, np.ndarray] = {}
    ranker = raglite_amd.MaxSimRanker(gi, lambda q: tokens[q])
    cfg = raglite_amd.HotPathConfig(vector_search_query_adapter=False, reranker=ranker)
    rec = {"chunks": args.chunks, "dim": args.dim, "terms": args.terms, "postings": int(p.post_chunk.size), "num_results": args.num_results,
           "oversample": args.oversample, "nq": args.nq, "neighbors": list(args.neighbors), "span_table_bytes": gi.spans.info()[2],
           "setup_s": round(time.perf_counter() - t0, 1), "batches": []}

    # (the corpus' host tables are millions of objects: kept out of the collector's way, or a collection during a timed call costs
    # more than the call)
    gc.collect()
    gc.freeze()
    for B in args.batches:
        queries = [f"q{B}_{b}" for b in range(B)]
        for q, t in zip(queries, keyword_ref.zipf_queries(rng, B, args.terms, lo=4, hi=12)):
            terms[q] = sorted(set(int(x) for x in t))
        Q = (rng.random((B, args.dim), dtype=np.float32) - 0.5).astype(np.float32)
        V = (rng.random((B, args.nq, args.dim), dtype=np.float32) - 0.5).astype(np.float32)
        V /= np.linalg.norm(V, axis=2, keepdims=True)
        common = {"num_results": args.num_results, "oversample": args.oversample, "config": cfg, "index": gi, "query_vectors": Q,
                  "query_token_vectors": V}

        def spans():
            return raglite_amd.search_and_rerank_chunk_spans_batch(queries, neighbors=args.neighbors, **common)

        def chunks():
            return raglite_amd.search_and_rerank_chunks_batch(queries, **common)

        def chunks_host():
            return [[_search.ChunkSpan(*s) for s in spans_ref.spans_of_chunks(table, ids, args.neighbors)] for ids in chunks()]

        hp = _search._plan_hybrid_batch(gi, cfg, queries, args.oversample * args.num_results, 2, None, Q)  # noqa: SLF001
        call = {"keyword": gi.keyword if hp.keyword else None, "query_term_ids": hp.term_ids, "weights": (0.75, 0.25), "rrf_k": 60}
        k = min(args.num_results, hp.k)

        def call_spans():
            return gi.index.search_rerank_spans(hp.Q, hp.num_hits, hp.n_each, hp.k, V, k, gi.spans, args.neighbors, **call)

        def call_chunks():
            return gi.index.search_rerank(hp.Q, hp.num_hits, hp.n_each, hp.k, V, k, **call)

        row = {"B": B}
        outs = {}
        for name, fn in (("spans", spans), ("chunks_host", chunks_host), ("chunks", chunks), ("call_spans", call_spans),
                         ("call_chunks", call_chunks)):
            outs[name], ms, wall = timed(fn, args.warmup, args.iters)
            row[f"{name}_ms"] = round(ms, 3)
            row[f"{name}_wall_ms"] = round(wall, 3)
            row[f"{name}_queries_per_s"] = round(B / ms * 1e3, 1)
        row["equal"] = outs["spans"] == outs["chunks_host"] and np.array_equal(outs["call_spans"][0], outs["call_chunks"][1])
        row["spans_per_query"] = round(sum(len(s) for s in outs["spans"]) / B, 2)
        row["chunks_per_query"] = round(sum(len(x.chunk_ids) for s in outs["spans"] for x in s) / B, 2)
        rec["batches"].append(row)
        print(json.dumps(row), flush=True)
        assert row["equal"], f"the device spans and the host restatement differ at B = {B}"
    gi.close()
    return rec


def trace_summary(path: str, rec: dict) -> dict:
    """Median time of the three one-workgroup-per-query kernels per batch size (Grid_Size_X = B workgroups x block size) from a
    rocprofv3 kernel_trace.csv."""
    times: dict[tuple[str, int], list[float]] = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for kernel, _ in KERNELS:
                if kernel in row["Kernel_Name"]:
                    B = int(row["Grid_Size_X"]) // int(row["Workgroup_Size_X"])
                    times.setdefault((kernel, B), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
    for b in rec["batches"]:
        for kernel, key in KERNELS:
            t = times.get((kernel, b["B"]))
            if t:
                b[f"{key}_us"] = round(float(np.median(t)), 2)
                b[f"{key}_dispatches"] = len(t)
    return rec


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--terms", type=int, default=200_000)
    ap.add_argument("--mean-len", type=int, default=150)
    ap.add_argument("--batches", type=lambda s: [int(x) for x in s.split(",")], default=[1, 16, 256])
    ap.add_argument("--num-results", type=int, default=8)
    ap.add_argument("--oversample", type=int, default=4)
    ap.add_argument("--nq", type=int, default=32)
    ap.add_argument("--neighbors", type=lambda s: tuple(int(x) for x in s.split(",") if x), default=(-1, 1))
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--trace-summary", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.trace_summary:
        with open(args.out) as f:
            rec = json.load(f)
        rec = trace_summary(args.trace_summary, rec)
    else:
        rec = run(args)
    text = json.dumps(rec, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
