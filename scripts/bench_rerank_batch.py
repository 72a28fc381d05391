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
    python scripts/bench_rerank_batch.py --mixed [--mixed-queries 256] [--mixed-iters 20] --out R.json
        the same corpus; 256 queries whose number of token vectors is uniform in 4..32 (what text queries give: nothing pads them).
        search_and_rerank_chunks_batch with `ranker.ragged = True` (one rl_search_rerank_ragged call) against False (one
        rl_search_rerank_per_query call per distinct length), in one process, alternating, each call timed on its own by a host clock
        around the call and a device synchronise; the medians of --mixed-iters calls after warm-up (the staging blocks and the index's
        scratch are grown by then: nothing is allocated on the device in a timed call).  Asserts that both return the same ids.  Then
        one fp16-stored point: the same rows as halves, every query 40 token vectors (a shape the grouped route cannot score there).
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


def _alternating(fns: dict, warmup: int, iters: int) -> tuple[dict, dict]:
    """Each variant's results and per-call times in ms (host clock around the call, the device synchronised before and after), the
    variants taking turns so that whatever else the host does meets them alike."""
    import torch

    outs, times = {}, {name: [] for name in fns}
    for _ in range(warmup):
        for name, fn in fns.items():
            outs[name] = fn()
    for _ in range(iters):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs[name] = fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return outs, times


def _stats(ms: list) -> dict:
    a = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(a)), 3), "min_ms": round(float(a[0]), 3), "max_ms": round(float(a[-1]), 3), "calls": int(a.size)}


def run_mixed(args) -> dict:
    import torch

    import raglite_amd
    from tests import keyword_ref as ref

    assert torch.cuda.is_available(), "bench_rerank_batch needs a GPU"
    raglite_amd.set_device(0)
    t0 = time.perf_counter()
    gi, p, terms, rng = build_index(args)
    B = args.mixed_queries
    queries = [f"m{b}" for b in range(B)]
    for q, t in zip(queries, ref.zipf_queries(rng, B, args.terms, lo=4, hi=12)):
        terms[q] = sorted(set(int(x) for x in t))
    Q = (rng.random((B, args.dim), dtype=np.float32) - 0.5).astype(np.float32)
    lengths = rng.integers(4, 33, size=B)

    def token_vectors(n):
        V = (rng.random((n, args.dim), dtype=np.float32) - 0.5).astype(np.float32)
        return V / np.linalg.norm(V, axis=1, keepdims=True)

    vecs = [token_vectors(int(n)) for n in lengths]
    rec = {"chunks": args.chunks, "dim": args.dim, "terms": args.terms, "num_results": args.num_results, "oversample": args.oversample,
           "n_cand": args.oversample * args.num_results, "queries": B, "distinct_lengths": int(np.unique(lengths).size),
           "lengths": "uniform in 4..32", "warmup": args.warmup, "setup_s": round(time.perf_counter() - t0, 1)}

    def variant(index, ranker, ragged, V):
        cfg = raglite_amd.HotPathConfig(vector_search_query_adapter=False, reranker=ranker)

        def call():
            ranker.ragged = ragged
            return raglite_amd.search_and_rerank_chunks_batch(queries, num_results=args.num_results, oversample=args.oversample, config=cfg,
                                                              index=index, query_vectors=Q, query_token_vectors=V)
        return call

    ranker = raglite_amd.MaxSimRanker(gi, lambda q: None)
    outs, times = _alternating({"ragged": variant(gi, ranker, True, vecs), "grouped": variant(gi, ranker, False, vecs)}, args.warmup,
                               args.mixed_iters)
    rec["mixed_f32"] = {name: _stats(ms) for name, ms in times.items()}
    rec["mixed_f32"]["grouped_over_ragged"] = round(rec["mixed_f32"]["grouped"]["median_ms"] / rec["mixed_f32"]["ragged"]["median_ms"], 2)
    rec["mixed_f32"]["equal"] = outs["ragged"] == outs["grouped"]
    print(json.dumps(rec["mixed_f32"]), flush=True)
    assert rec["mixed_f32"]["equal"], "the ragged and the grouped batch return different ids"

    # fp16-stored rows (the same values as halves), 40 token vectors per query: only the ragged route scores them there
    t0 = time.perf_counter()
    half = raglite_amd.GpuIndex(gi.chunk_ids, gi._E.half(), chunk_offsets=np.arange(args.chunks + 1, dtype=np.int64), storage="f16")  # noqa: SLF001
    half.keyword, half._kw_stems, half.keyword_query_ids = gi.keyword, gi._kw_stems, gi.keyword_query_ids  # noqa: SLF001
    long = [token_vectors(40) for _ in range(B)]
    long_ranker = raglite_amd.MaxSimRanker(half, lambda q: None)
    outs, times = _alternating({"ragged": variant(half, long_ranker, True, long)}, args.warmup, args.mixed_iters)
    rec["long_f16"] = {"nq": 40, "setup_s": round(time.perf_counter() - t0, 1), "ragged": _stats(times["ragged"]),
                       "results_per_query": sorted({len(x) for x in outs["ragged"]})}
    print(json.dumps(rec["long_f16"]), flush=True)
    half.keyword = None  # (the keyword index belongs to `gi`)
    half.close()
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
    ap.add_argument("--mixed", action="store_true")
    ap.add_argument("--mixed-queries", type=int, default=256)
    ap.add_argument("--mixed-iters", type=int, default=20)
    ap.add_argument("--trace-summary", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.trace_summary:
        with open(args.out) as f:
            rec = json.load(f)
        rec = trace_summary(args.trace_summary, rec)
    elif args.mixed:
        rec = run_mixed(args)
    else:
        rec = run(args)
    text = json.dumps(rec, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
