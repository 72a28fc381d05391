"""Batched search-and-rerank at corpus scale (search_and_rerank_chunks_batch, rl_search_rerank_per_query, rl_rerank_order;
DESIGN.md §4.10).

    python scripts/bench_rerank_batch.py [--chunks 1000000] [--dim 1024] [--batches 1,16,256] --out R.json
        the corpus of scripts/bench_hybrid.py (one row per chunk, synthetic, on the device; the Zipf keyword side), num_results 8,
        oversample 4, nq 32 token vectors per query.  Per batch, after warm-up, with device events around each variant, every variant
        reading its results back:
          batch        search_and_rerank_chunks_batch (one rl_search_rerank_per_query call, one read-back)
          batch_rank   hybrid_search_batch for the 32 candidates, then MaxSimRanker.rank query by query
          loop         search_and_rerank_chunks query by query (hybrid_search's own steps for a query whose vector is at hand)
          search_only  hybrid_search_batch alone: what `batch` adds to it is one rerank launch and one ordering launch
        and checks that batch, batch_rank and loop return the same chunks in the same order.  Writes one JSON record.
    python scripts/bench_rerank_batch.py --trace-summary kernel_trace.csv --out R.json
        adds rerank_order_kernel's and rrf_fuse_kernel's time per batch size (grid x = batch size) from a `rocprofv3 --kernel-trace`
        run of the first form.
"""

from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from scripts.bench_hybrid import build_index, timed


def run(args) -> dict:
    import torch

    import raglite_amd
    from tests import keyword_ref as ref

    assert torch.cuda.is_available(), "bench_rerank_batch needs a GPU"
    raglite_amd.set_device(0)
    t0 = time.perf_counter()
    gi, p, terms, rng = build_index(args)
    gi.docs = gi.chunk_ids  # a chunk's text is its id: what MaxSimRanker.rank maps back to ordinals
    gi._doc_to_ordinal = gi._id_to_ordinal  # noqa: SLF001
    vectors: dict[str, np.ndarray] = {}
    tokens: dict[str, np.ndarray] = {}
    ranker = raglite_amd.MaxSimRanker(gi, lambda q: tokens[q])
    cfg = raglite_amd.HotPathConfig(vector_search_query_adapter=False, reranker=ranker)
    plain = raglite_amd.HotPathConfig(vector_search_query_adapter=False)
    n_cand = args.oversample * args.num_results
    rec = {"chunks": args.chunks, "dim": args.dim, "terms": args.terms, "postings": int(p.post_chunk.size), "num_results": args.num_results,
           "oversample": args.oversample, "n_cand": n_cand, "nq": args.nq, "setup_s": round(time.perf_counter() - t0, 1), "batches": []}

    def search(query, *, num_results, metadata_filter=None, config=None):  # hybrid_search's body for a query whose vector is at hand
        vs, _ = raglite_amd.vector_search(vectors[query], num_results=2 * num_results, config=config, index=gi)
        ks, _ = raglite_amd.keyword_search(query, num_results=2 * num_results, config=config, index=gi)
        ids, sc = raglite_amd.reciprocal_rank_fusion([vs, ks], weights=[0.75, 0.25])
        return ids[:num_results], sc[:num_results]

    for B in args.batches:
        queries = [f"q{B}_{b}" for b in range(B)]
        for q, t in zip(queries, ref.zipf_queries(rng, B, args.terms, lo=4, hi=12)):
            terms[q] = sorted(set(int(x) for x in t))
        Q = (rng.random((B, args.dim), dtype=np.float32) - 0.5).astype(np.float32)
        V = (rng.random((B, args.nq, args.dim), dtype=np.float32) - 0.5).astype(np.float32)
        V /= np.linalg.norm(V, axis=2, keepdims=True)
        for b, q in enumerate(queries):
            vectors[q], tokens[q] = Q[b], V[b]

        def batch():
            return raglite_amd.search_and_rerank_chunks_batch(queries, num_results=args.num_results, oversample=args.oversample, config=cfg,
                                                              index=gi, query_vectors=Q, query_token_vectors=V)

        def search_only():
            return raglite_amd.hybrid_search_batch(queries, num_results=n_cand, config=plain, index=gi, query_vectors=Q)

        def batch_rank():
            out = []
            for q, (ids, _) in zip(queries, search_only()):
                ranked = ranker.rank(query=q, docs=ids)
                out.append([ids[r.doc_id] for r in ranked.results][: args.num_results])
            return out

        def loop():
            return [raglite_amd.search_and_rerank_chunks(q, num_results=args.num_results, oversample=args.oversample, search=search, config=cfg,
                                                         chunk_lookup=list) for q in queries]

        row = {"B": B}
        outs = {}
        for name, fn, iters in (("batch", batch, args.iters), ("batch_rank", batch_rank, max(1, args.iters // 2)),
                                ("loop", loop, max(1, args.iters // 4)), ("search_only", search_only, args.iters)):
            outs[name], ms, wall = timed(fn, args.warmup, iters)
            row[f"{name}_ms"] = round(ms, 3)
            row[f"{name}_wall_ms"] = round(wall, 3)
            row[f"{name}_queries_per_s"] = round(B / ms * 1e3, 1)
        row["equal"] = outs["batch"] == outs["batch_rank"] == outs["loop"]
        row["reordered"] = sum(a != ids[: args.num_results] for a, (ids, _) in zip(outs["batch"], outs["search_only"]))
        rec["batches"].append(row)
        print(json.dumps(row), flush=True)
        assert row["equal"], f"the three variants differ at B = {B}"
    gi.close()
    return rec


def trace_summary(path: str, rec: dict) -> dict:
    """Median rerank_order_kernel and rrf_fuse_kernel time per batch size (Grid_Size_X = B workgroups x block size) from a rocprofv3
    kernel_trace.csv."""
    times: dict[tuple[str, int], list[float]] = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for kernel in ("rerank_order_kernel", "rrf_fuse_kernel"):
                if kernel in row["Kernel_Name"]:
                    B = int(row["Grid_Size_X"]) // int(row["Workgroup_Size_X"])
                    times.setdefault((kernel, B), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
    for b in rec["batches"]:
        for kernel, key in (("rerank_order_kernel", "order_kernel"), ("rrf_fuse_kernel", "fuse_kernel")):
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
