"""BM25 keyword search on the device at corpus scale (raglite_amd/csrc/keyword.hip; DESIGN.md "Keyword search"), seeded, no text.

    python scripts/bench_keyword.py [--chunks 1000000] [--terms 200000] [--mean-len 150] [--batches 1,16,256] --out R.json
        builds a Zipf corpus of pre-tokenised chunks (tests/keyword_ref.py), times rl_keyword_search per batch with device events
        after warm-up (device pointers, nothing synchronises inside the timed window), times the NumPy restatement on the same
        queries and checks the device results against it bitwise.  Writes one JSON record.
    python scripts/bench_keyword.py --trace-summary kernel_trace.csv --out R.json
        adds the score kernel's time per batch size from a `rocprofv3 --kernel-trace` run of the first form (grid y = batch size)
        and its share of the HBM bound: (postings read + tile writes) / 6.3 TB/s over kernel time.
"""

from __future__ import annotations

import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

HBM_BYTES_PER_S = 6.3e12  # achievable HBM3E rate of an MI355X (float4 copy)


def corpus(args):
    from raglite_amd import _keyword
    from tests import keyword_ref as ref

    rng = np.random.default_rng(args.seed)
    t0 = time.perf_counter()
    flat, off = ref.zipf_corpus(rng, args.chunks, args.terms, args.mean_len)
    p = _keyword.build_from_term_ids(flat, off, args.terms)
    del flat
    queries = {B: ref.zipf_queries(rng, B, args.terms, lo=4, hi=12) for B in args.batches}
    return p, queries, time.perf_counter() - t0


def score_bytes(p, queries) -> int:
    """What the score kernel must move for one batch: 8 B per posting of every distinct in-vocabulary query term (chunk ordinal +
    impact), and the [B x n_chunks] float scores it writes."""
    df = p.df
    total = 0
    for q in queries:
        t = np.unique(q)
        t = t[(t >= 0) & (t < p.n_terms)]
        total += 8 * int(df[t].sum()) + 4 * p.n_chunks
    return total


def run(args) -> dict:
    import torch

    import raglite_amd
    from raglite_amd import _abi, _ops
    from tests import keyword_ref as ref

    assert torch.cuda.is_available(), "bench_keyword needs a GPU"
    raglite_amd.set_device(0)
    p, queries, build_s = corpus(args)
    t0 = time.perf_counter()
    kw = _ops.KeywordIndex(p)
    upload_s = time.perf_counter() - t0
    lib = _abi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    imp = ref.impacts_f32(p)
    rec = {"chunks": p.n_chunks, "terms": p.n_terms, "postings": int(p.post_chunk.size), "mean_len": float(p.avgdl), "k": args.k,
           "build_host_s": round(build_s, 2), "index_create_s": round(upload_s, 3), "batches": []}
    for B in args.batches:
        qs = [np.unique(q) for q in queries[B]]
        q_off = torch.tensor(np.concatenate(([0], np.cumsum([q.size for q in qs]))), dtype=torch.int64, device="cuda")
        q_terms = torch.tensor(np.concatenate(qs), dtype=torch.int32, device="cuda")
        out_s = torch.empty((B, args.k), dtype=torch.float32, device="cuda")
        out_c = torch.empty((B, args.k), dtype=torch.int32, device="cuda")
        out_n = torch.empty(B, dtype=torch.int32, device="cuda")

        def step():
            _abi.check(lib.rl_keyword_search(kw._handle, q_off.data_ptr(), q_terms.data_ptr(), B, args.k, None, out_s.data_ptr(),  # noqa: SLF001
                                             out_c.data_ptr(), out_n.data_ptr(), _abi.MEM_DEVICE, C.c_void_p(stream)))

        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            step()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.iters
        # the NumPy restatement on the same queries (at most --numpy-queries of them, scaled to the batch), and the bitwise check
        n_np = min(B, args.numpy_queries)
        got_s, got_c, got_n = out_s.cpu().numpy(), out_c.cpu().numpy(), out_n.cpu().numpy()
        t0 = time.perf_counter()
        ok = True
        for b in range(n_np):
            ws, wc = ref.topk_f32(ref.scores_f32(p, imp, qs[b]), args.k)
            n = len(wc)
            ok &= int(got_n[b]) == n and np.array_equal(got_c[b, :n], wc) and np.array_equal(got_s[b, :n].view(np.uint32), ws.view(np.uint32))
        np_ms = (time.perf_counter() - t0) * 1e3 / n_np * B
        nbytes = score_bytes(p, queries[B])
        rec["batches"].append({"B": B, "ms_per_batch": round(ms, 4), "queries_per_s": round(B / ms * 1e3, 1),
                               "numpy_ms_per_batch": round(np_ms, 1), "numpy_queries_timed": n_np, "bitwise_equal_checked": bool(ok),
                               "score_bytes": nbytes, "score_bytes_per_query": nbytes // B,
                               "score_hbm_bound_ms": round(nbytes / HBM_BYTES_PER_S * 1e3, 4)})
        print(json.dumps(rec["batches"][-1]), flush=True)
        assert ok, f"device results differ from the restatement at B = {B}"
    kw.close()
    return rec


def trace_summary(path: str, rec: dict) -> dict:
    """Mean bm25_score_kernel time per batch size (Grid_Size_Y = B) from a rocprofv3 kernel_trace.csv."""
    times: dict[int, list[float]] = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if "bm25_score_kernel" not in row["Kernel_Name"]:
                continue
            B = int(row["Grid_Size_Y"])
            times.setdefault(B, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6)
    for b in rec["batches"]:
        t = times.get(b["B"])
        if not t:
            continue
        kms = float(np.median(t))
        b["score_kernel_ms"] = round(kms, 4)
        b["score_kernel_dispatches"] = len(t)
        b["score_kernel_TBps"] = round(b["score_bytes"] / (kms * 1e-3) / 1e12, 3)
        b["score_kernel_hbm_fraction"] = round(b["score_hbm_bound_ms"] / kms, 3)
    return rec


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=1_000_000)
    ap.add_argument("--terms", type=int, default=200_000)
    ap.add_argument("--mean-len", type=int, default=150)
    ap.add_argument("--batches", type=lambda s: [int(x) for x in s.split(",")], default=[1, 16, 256])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--numpy-queries", type=int, default=4)
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
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
