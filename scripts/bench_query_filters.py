"""Per-query metadata filters in one hybrid batch: B queries with F distinct tenant filters.

    python scripts/bench_query_filters.py [--chunks 1000000] [--dim 1024] [--batches 16,256] [--filters 1,16,B] --out R.json
        one row per chunk (synthetic, on the device) and the Zipf keyword side of scripts/bench_hybrid.py (its build_index), one tenant per
        chunk (256 Zipf-sized tenants), num_results 8, oversample 4 (n_each 32, num_hits 128).  Query b's filter is tenant b mod F.  Per
        (B, F), after warm-up, with device events around each variant (host arrays in and out, as hybrid_search_batch hands them over):
          per_query   (a) one rl_hybrid_search_per_query call with one tenant mask per query
          per_filter  (b) one rl_hybrid_search call per distinct filter (what a caller had to do before)
          loop        (c) one rl_hybrid_search call per query (the loop of hybrid_search)
          unfiltered  (d) the same batch without filters (the yardstick)
        and checks that (a), (b) and (c) return the same bits.  The masks are evaluated and packed once, outside the timed window: the
        host's JSON containment over the chunks' metadata (`_search.plan_filters`) costs the same per distinct filter in (a) and (b), once
        per query in (c); its time for one filter over this corpus is recorded as `eval_one_filter_ms`.  Writes one JSON record.
    python scripts/bench_query_filters.py --trace-calls N --batches 256 --filters 1 ...
        warm-up + N calls of (a) only, for a `rocprofv3 --kernel-trace --stats` run; then --count-kernels <its kernel_stats.csv> --calls N+1
        prints the launches per call and the mean time of each kernel (the index build's kernels show up with fewer than one per call).
"""

from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np


def tenants(rng, n_chunks: int, n_tenants: int = 256) -> np.ndarray:
    p = 1.0 / np.arange(1, n_tenants + 1) ** 1.1
    return rng.choice(n_tenants, size=n_chunks, p=p / p.sum()).astype(np.int32)


def run(args) -> dict:
    import torch

    import raglite_amd
    from raglite_amd import _ops, _search
    from bench_hybrid import build_index, timed
    from tests import keyword_ref as ref

    assert torch.cuda.is_available(), "bench_query_filters needs a GPU"
    raglite_amd.set_device(0)
    t0 = time.perf_counter()
    gi, p, _, rng = build_index(args)
    tenant = tenants(rng, args.chunks)
    masks = [_ops.pack_bits(tenant == t) for t in range(256)]  # packed once: the calls below take them as they are
    rows = np.bincount(tenant, minlength=256)  # (one row per chunk)
    limits = [_search.ORDER_FIRST_LIMIT if int(rows[t]) > _search.FILTER_FIRST_MAX_ROWS else 0 for t in range(256)]
    cfg = raglite_amd.HotPathConfig(vector_search_query_adapter=False)
    n_each = args.oversample * args.num_results
    num_hits = round(_search.VECTOR_SEARCH_OVERSAMPLE * cfg.chunk_max_size / _search.DEFAULT_CHUNK_MAX_SIZE) * max(n_each, 10)
    k = args.num_results
    meta = [{"tenant": f"t{t}"} for t in tenant[: args.eval_chunks]]
    te = time.perf_counter()
    _search.plan_filters([{"tenant": ["t0"]}], meta, np.ones(len(meta), np.int64))
    eval_ms = (time.perf_counter() - te) * 1e3 * args.chunks / len(meta)
    rec = {"chunks": args.chunks, "dim": args.dim, "postings": int(p.post_chunk.size), "num_results": args.num_results, "n_each": n_each,
           "num_hits": num_hits, "tenant_rows_max": int(rows.max()), "tenant_rows_min": int(rows.min()),
           "eval_one_filter_ms": round(eval_ms, 1), "setup_s": round(time.perf_counter() - t0, 1), "runs": []}
    kw = dict(keyword=gi.keyword, weights=(0.75, 0.25), rrf_k=60)
    for B in args.batches:
        Q = (rng.random((B, args.dim), dtype=np.float32) - 0.5).astype(np.float32)
        terms = [sorted(set(int(x) for x in t)) for t in ref.zipf_queries(rng, B, args.terms, lo=4, hi=12)]
        for F in sorted({B if f == "B" else int(f) for f in args.filters}):
            tq = [b % F for b in range(B)]
            qf = [masks[t] for t in tq]
            ql = [limits[t] for t in tq]

            def per_query():
                return gi.index.hybrid_search(Q, num_hits, n_each, k, query_term_ids=terms, query_filters=qf, rank_limit=ql, **kw)

            if args.trace_calls:
                for _ in range(args.trace_calls + 1):
                    per_query()
                torch.cuda.synchronize()
                continue

            def per_filter():
                s, c, n = np.empty((B, k)), np.empty((B, k), np.int32), np.empty(B, np.int32)
                for t in range(F):
                    sel = [b for b in range(B) if tq[b] == t]
                    s[sel], c[sel], n[sel] = gi.index.hybrid_search(Q[sel], num_hits, n_each, k, query_term_ids=[terms[b] for b in sel],
                                                                    chunk_filter=masks[t], rank_limit=limits[t], **kw)
                return s, c, n

            def loop():
                s, c, n = np.empty((B, k)), np.empty((B, k), np.int32), np.empty(B, np.int32)
                for b in range(B):
                    s[b], c[b], n[b] = gi.index.hybrid_search(Q[b], num_hits, n_each, k, query_term_ids=[terms[b]], chunk_filter=qf[b],
                                                              rank_limit=ql[b], **kw)
                return s, c, n

            def unfiltered():
                return gi.index.hybrid_search(Q, num_hits, n_each, k, query_term_ids=terms, **kw)

            row = {"B": B, "F": F}
            outs = {}
            for name, fn, iters in (("per_query", per_query, args.iters), ("per_filter", per_filter, max(1, args.iters // 2)),
                                    ("loop", loop, max(1, args.iters // 4)), ("unfiltered", unfiltered, args.iters)):
                outs[name], ms, wall = timed(fn, args.warmup, iters)
                row[f"{name}_ms"] = round(ms, 3)
                row[f"{name}_wall_ms"] = round(wall, 3)
            a, b_, c_ = outs["per_query"], outs["per_filter"], outs["loop"]
            row["equal"] = all(np.array_equal(a[0].view(np.uint64), x[0].view(np.uint64)) and np.array_equal(a[1], x[1])
                               and np.array_equal(a[2], x[2]) for x in (b_, c_))
            rec["runs"].append(row)
            print(json.dumps(row), flush=True)
            assert row["equal"], f"the variants differ at B = {B}, F = {F}"
    for r in rec["runs"]:  # (a) at F against (a) at F = 1, same B
        one = next((x for x in rec["runs"] if x["B"] == r["B"] and x["F"] == 1), None)
        if one:
            r["per_query_vs_F1"] = round(r["per_query_ms"] / one["per_query_ms"], 3)
    gi.close()
    return rec


def count_kernels(path: str, calls: int) -> dict:
    """Launches per call and mean time of every kernel in the rocprofv3 kernel_stats.csv of a --trace-calls run."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Name"].replace("(anonymous namespace)::", "").split("(")[0][:90]
            out[name] = {"per_call": round(int(row["Calls"]) / calls, 2), "mean_us": round(float(row["AverageNs"]) * 1e-3, 2)}
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--terms", type=int, default=200_000)
    ap.add_argument("--mean-len", type=int, default=150)
    ap.add_argument("--batches", type=lambda s: [int(x) for x in s.split(",")], default=[16, 256])
    ap.add_argument("--filters", type=lambda s: s.split(","), default=["1", "16", "B"])
    ap.add_argument("--num-results", type=int, default=8)
    ap.add_argument("--oversample", type=int, default=4)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--eval-chunks", type=int, default=200_000)  # the metadata evaluation is timed on this many chunks and scaled
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--count-kernels", default=None)
    ap.add_argument("--calls", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rec = count_kernels(args.count_kernels, args.calls) if args.count_kernels else run(args)
    text = json.dumps(rec, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
