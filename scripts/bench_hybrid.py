"""Batched hybrid search at corpus scale (hybrid_search_batch, rl_hybrid_search, rl_rrf_fuse; DESIGN.md "Batched hybrid search").

    python scripts/bench_hybrid.py [--chunks 1000000] [--dim 1024] [--batches 1,16,256] --out R.json
        one row per chunk (synthetic, on the device), the Zipf keyword side of scripts/bench_keyword.py, num_results 8, oversample 4
        (the search_and_rerank_chunks shape).  Per batch, after warm-up, with device events around each variant:
          batch      hybrid_search_batch (one rl_hybrid_search call, one read-back)
          loop       the same queries one by one through hybrid_search's own steps (vector_search, keyword_search, RRF on the host)
          two_plus_host  the two batched searches (search_chunks, KeywordIndex.search) and reciprocal_rank_fusion on the host
        and checks that the three give the same ids and scores.  Writes one JSON record.
    python scripts/bench_hybrid.py --trace-summary kernel_trace.csv --out R.json
        adds rrf_fuse_kernel's time per batch size (grid x = batch size) from a `rocprofv3 --kernel-trace` run of the first form.
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


def build_index(args):
    import torch

    import raglite_amd
    from raglite_amd import _keyword, _ops
    from tests import keyword_ref as ref

    rng = np.random.default_rng(args.seed)
    flat, off = ref.zipf_corpus(rng, args.chunks, args.terms, args.mean_len)
    p = _keyword.build_from_term_ids(flat, off, args.terms)
    del flat
    E = torch.empty((args.chunks, args.dim), dtype=torch.float32, device="cuda")
    raglite_amd.synth_fill(E, seed=args.seed + 1)
    E = torch.nn.functional.normalize(E - 0.5, dim=1)
    gi = raglite_amd.GpuIndex([f"c{i}" for i in range(args.chunks)], E, chunk_offsets=np.arange(args.chunks + 1, dtype=np.int64))
    gi._E = E  # noqa: SLF001 (the index borrows the device rows)
    # the keyword side from the Zipf postings directly (no text): queries are named, their term ids looked up by name
    gi.keyword, gi._kw_stems = _ops.KeywordIndex(p), [[]]  # noqa: SLF001
    terms = {}
    gi.keyword_query_ids = lambda q: terms[q]
    return gi, p, terms, rng


def timed(fn, warmup, iters):
    import torch

    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / iters
    return out, e0.elapsed_time(e1) / iters, wall


def run(args) -> dict:
    import torch

    import raglite_amd
    from raglite_amd import _search
    from tests import keyword_ref as ref

    assert torch.cuda.is_available(), "bench_hybrid needs a GPU"
    raglite_amd.set_device(0)
    t0 = time.perf_counter()
    gi, p, terms, rng = build_index(args)
    cfg = raglite_amd.HotPathConfig(vector_search_query_adapter=False)
    n_each = args.oversample * args.num_results
    num_hits = round(_search.VECTOR_SEARCH_OVERSAMPLE * cfg.chunk_max_size / _search.DEFAULT_CHUNK_MAX_SIZE) * max(n_each, 10)
    rec = {"chunks": args.chunks, "dim": args.dim, "terms": args.terms, "postings": int(p.post_chunk.size), "num_results": args.num_results,
           "oversample": args.oversample, "n_each": n_each, "num_hits": num_hits, "setup_s": round(time.perf_counter() - t0, 1), "batches": []}
    for B in args.batches:
        queries = [f"q{B}_{b}" for b in range(B)]
        for q, t in zip(queries, ref.zipf_queries(rng, B, args.terms, lo=4, hi=12)):
            terms[q] = sorted(set(int(x) for x in t))
        Q = (rng.random((B, args.dim), dtype=np.float32) - 0.5).astype(np.float32)
        kw = dict(num_results=args.num_results, oversample=args.oversample, config=cfg, index=gi)

        def batch():
            return raglite_amd.hybrid_search_batch(queries, query_vectors=Q, **kw)

        def loop():  # hybrid_search's body for a query whose vector is at hand
            out = []
            for b, q in enumerate(queries):
                vs, _ = raglite_amd.vector_search(Q[b], num_results=n_each, config=cfg, index=gi)
                ks, _ = raglite_amd.keyword_search(q, num_results=n_each, config=cfg, index=gi)
                ids, sc = raglite_amd.reciprocal_rank_fusion([vs, ks], weights=[0.75, 0.25])
                out.append((ids[: args.num_results], sc[: args.num_results]))
            return out

        def two_plus_host():
            _, vc, vn = gi.index.search_chunks(Q, num_hits, n_each)
            _, kc, kn = gi.keyword.search([terms[q] for q in queries], n_each)
            out = []
            for b in range(B):
                vs = [gi.chunk_ids[c] for c in vc[b, : int(vn[b])].tolist()]
                ks = [gi.chunk_ids[c] for c in kc[b, : int(kn[b])].tolist()]
                ids, sc = raglite_amd.reciprocal_rank_fusion([vs, ks], weights=[0.75, 0.25])
                out.append((ids[: args.num_results], sc[: args.num_results]))
            return out

        row = {"B": B}
        outs = {}
        for name, fn, iters in (("batch", batch, args.iters), ("loop", loop, max(1, args.iters // 4)), ("two_plus_host", two_plus_host, args.iters)):
            outs[name], ms, wall = timed(fn, args.warmup, iters)
            row[f"{name}_ms"] = round(ms, 3)
            row[f"{name}_wall_ms"] = round(wall, 3)
            row[f"{name}_queries_per_s"] = round(B / ms * 1e3, 1)
        row["equal"] = outs["batch"] == outs["loop"] == outs["two_plus_host"]
        rec["batches"].append(row)
        print(json.dumps(row), flush=True)
        assert row["equal"], f"the three variants differ at B = {B}"
    gi.close()
    return rec


def trace_summary(path: str, rec: dict) -> dict:
    """Median rrf_fuse_kernel time per batch size (Grid_Size_X = B workgroups x block size) from a rocprofv3 kernel_trace.csv."""
    times: dict[int, list[float]] = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if "rrf_fuse_kernel" not in row["Kernel_Name"]:
                continue
            B = int(row["Grid_Size_X"]) // int(row["Workgroup_Size_X"])
            times.setdefault(B, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
    for b in rec["batches"]:
        t = times.get(b["B"])
        if t:
            b["fuse_kernel_us"] = round(float(np.median(t)), 2)
            b["fuse_kernel_dispatches"] = len(t)
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
