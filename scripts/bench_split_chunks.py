"""Semantic chunking of many documents: today's per-document `split_chunks` (host MILP) against `split_chunks_batch` (one
`rl_split_chunks` call).

    python scripts/bench_split_chunks.py [--docs 1000] [--dim 1024] [--small] --out R.json
        Seeded synthetic documents: --docs documents of U{20 .. 300} chunklets, a chunklet of U{40 .. 200} characters, one in
        twelve a Markdown heading, max_size 2048, embeddings standard normal float32 [chunklets x dim] as CUDA tensors (where the
        encoder leaves them).  --small: 40 documents of U{5 .. 60} chunklets at dim 64, a quick check of the script, not a measurement.
        One run reports, in milliseconds for all documents together:
          loop_ms            a loop of split_chunks(partition="milp") over the documents -- the baseline -- and of that
          loop_milp_ms       the time inside _solve_partition (scipy's HiGHS), timed around every call
          batch_ms           split_chunks_batch over the same documents, warm (median of --iters)
          call_ms            the rl_split_chunks call alone on prepared device arrays (device events; wall next to it)
          similarity_ms      the rl_partition_similarity call alone (device events)
          partition_ms       the rl_partition_chunks call alone on the costs of call_ms (device events): memset, prefix sums, window
                             ends, the DP kernel with its backtrack; partition_bytes is what those must move at least
          host_*_ms          the host remainder of split_chunks_batch: string lengths, quantiles, heading regex, joins
        and how many documents come out with other chunks than the loop's, with both objectives for each of them (a tie, or the
        MILP's relative gap).  Writes one JSON record.
    python scripts/bench_split_chunks.py --device-only --out T.json
        only the C calls on the same documents (no loop, no batch): the run to put under `rocprofv3 --kernel-trace --stats`.
    python scripts/bench_split_chunks.py --kernel-stats <kernel_stats.csv> --out R.json
        adds to the record R.json each kernel's mean time per launch from that run (every launch of it is at the full size):
        partition_dp_kernel alone -- the DP with its backtrack, set against partition_dp_bytes, the bytes that one kernel must move
        -- and the prefix, ends, headings and similarity kernels.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np


def make_documents(rng, n_docs: int, lo: int, hi: int) -> list[list[str]]:
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz      ", dtype="S1")
    docs = []
    for _ in range(n_docs):
        doc = []
        for _ in range(int(rng.integers(lo, hi + 1))):
            body = b"".join(rng.choice(letters, size=int(rng.integers(38, 199)))).decode()
            doc.append("# " + body if rng.integers(0, 12) == 0 else body + ". ")
        docs.append(doc)
    return docs


def events_ms(torch, fn, warmup: int, iters: int) -> tuple[float, float]:
    """(median device-event ms, median wall ms) of fn, every call ending in a synchronise."""
    ev, wall = [], []
    for i in range(warmup + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(a.elapsed_time(b))
    return float(np.median(ev)), float(np.median(wall))


def run(args) -> dict:
    import torch

    import raglite_amd
    from raglite_amd import _chunking, _ops
    from raglite_amd._abi import check, lib

    assert torch.cuda.is_available(), "bench_split_chunks needs a GPU"
    raglite_amd.set_device(0)
    rng = np.random.default_rng(args.seed)
    lo, hi = (5, 60) if args.small else (20, 300)
    docs = make_documents(rng, args.docs, lo, hi)
    counts = np.asarray([len(d) for d in docs], np.int64)
    off = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    n = int(off[-1])
    x = torch.randn((n, args.dim), dtype=torch.float32, device="cuda", generator=torch.Generator("cuda").manual_seed(args.seed))
    embs = [x[off[d]:off[d + 1]] for d in range(len(docs))]
    rec = {"docs": args.docs, "dim": args.dim, "chunklets": n, "chunklets_per_doc": f"U{{{lo}..{hi}}}", "chunklet_chars": "U{40..200}",
           "max_size": args.max_size, "small": bool(args.small), "iters": args.iters}

    # -- the baseline: today's loop, the MILP's share timed around every call
    milp = {"s": 0.0}
    solve = _chunking._solve_partition  # noqa: SLF001

    def timed_solve(*a, **k):
        t0 = time.perf_counter()
        try:
            return solve(*a, **k)
        finally:
            milp["s"] += time.perf_counter() - t0

    out, loop = {"batch": []}, []
    if not args.device_only:
        raglite_amd.split_chunks(docs[0], embs[0], max_size=args.max_size)  # warm: library, scipy import
        _chunking._solve_partition = timed_solve  # noqa: SLF001
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop = [raglite_amd.split_chunks(d, e, max_size=args.max_size) for d, e in zip(docs, embs)]
            torch.cuda.synchronize()
            rec["loop_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        finally:
            _chunking._solve_partition = solve  # noqa: SLF001
        rec["loop_milp_ms"] = round(milp["s"] * 1e3, 2)

        # -- the batched call, warm
        def batch():
            out["batch"] = raglite_amd.split_chunks_batch(docs, x, max_size=args.max_size)

        _, rec["batch_ms"] = (round(v, 3) for v in events_ms(torch, batch, 1, args.iters))
        rec["docs_with_other_chunks_than_the_loop"] = sum(a[0] != b[0] for a, b in zip(out["batch"], loop))
        rec["chunks"] = sum(len(a[0]) for a in out["batch"])

    # -- the host remainder, step by step
    t0 = time.perf_counter()
    sizes = np.fromiter((len(c) for d in docs for c in d), dtype=np.int64, count=n)
    t1 = time.perf_counter()
    sel = np.concatenate([_chunking._nonoutlying(sizes[off[d]:off[d + 1]]) for d in range(len(docs))])  # noqa: SLF001
    t2 = time.perf_counter()
    head = np.concatenate([_chunking._heading_flags(d) for d in docs])  # noqa: SLF001
    t3 = time.perf_counter()
    joined = [["".join(d[i:i + 8]) for i in range(0, len(d), 8)] for d in docs]  # joins of the size the partition produces
    del joined
    t4 = time.perf_counter()
    rec.update(host_lengths_ms=round((t1 - t0) * 1e3, 3), host_quantiles_ms=round((t2 - t1) * 1e3, 3),
               host_heading_regex_ms=round((t3 - t2) * 1e3, 3), host_joins_ms=round((t4 - t3) * 1e3, 3))

    # -- the C calls alone, on prepared device arrays
    d_off, d_sel, d_head, d_sizes = (torch.from_numpy(a).cuda() for a in (off, sel, head, sizes))

    def call():
        out["call"] = _ops.split_chunks_call(x, d_off, d_sel, d_head, d_sizes, args.max_size, want_cost=True)

    rec["call_ms"], rec["call_wall_ms"] = (round(v, 3) for v in events_ms(torch, call, 1, args.iters))
    cost = out["call"][1]
    # where the batch cut elsewhere than the loop: both objectives on the call's costs (a tie, or the MILP's relative gap, shows here)
    cost_host, gaps = cost.cpu().numpy().astype(np.float64), []
    for d, (a, b) in enumerate(zip(out["batch"], loop)):
        if a[0] != b[0]:
            objective = [float(cost_host[off[d] + np.cumsum([len(p) for p in r[1]])[:-1] - 1].sum()) for r in (a, b)]
            gaps.append({"doc": d, "batch_objective": objective[0], "loop_objective": objective[1]})
    rec["other_chunks"] = gaps
    sim = torch.empty(n, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def similarity():
        check(lib().rl_partition_similarity(x.data_ptr(), n, args.dim, d_off.data_ptr(), len(docs), d_sel.data_ptr(), sim.data_ptr(),
                                            _ops.MEM_DEVICE, stream))

    rec["similarity_ms"], _ = (round(v, 3) for v in events_ms(torch, similarity, 1, args.iters))

    def partition():
        out["partition"] = raglite_amd.partition_chunks(cost, d_sizes, d_off, args.max_size)

    rec["partition_ms"], rec["partition_wall_ms"] = (round(v, 3) for v in events_ms(torch, partition, 1, args.iters))
    assert torch.equal(out["partition"][0], out["call"][0]), "rl_partition_chunks and rl_split_chunks disagree on the cuts"
    # cost 4 + sizes 8 + cut 1 (memset) + 1 (cuts) bytes per chunklet in and out; csum, end, prev, g written once and read at least once
    rec["partition_bytes"] = n * (4 + 8 + 2) + n * 32 * 2
    # the DP kernel alone: cost 4 and end 8 read, g and prev 8 each written and read once, cut 1 written, per chunklet
    rec["partition_dp_bytes"] = n * (4 + 8 + 16 * 2 + 1)
    rec["similarity_bytes"] = n * args.dim * 4 * 3  # the rows are read by the norm and pair kernels, the selected ones by the discourse kernel
    return rec


KERNELS = ("partition_dp_kernel", "pd_prefix_kernel", "pd_ends_kernel", "ps_headings_kernel", "ps_norms_kernel", "ps_discourse_kernel",
           "ps_pairs_kernel", "ps_choose_kernel")


def kernel_stats(path: str, rec: dict) -> dict:
    """Mean time per launch of the call's kernels from the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of
    --device-only, where every launch of a kernel is at the full size."""
    import csv

    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for kernel in KERNELS:
                if kernel in row["Name"]:
                    rec[f"{kernel}_us"] = round(float(row["AverageNs"]) * 1e-3, 2)
                    rec[f"{kernel}_launches"] = int(row["Calls"])
    return rec


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--max-size", type=int, default=2048)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.small:
        args.docs, args.dim = 40, 64
    if args.kernel_stats:
        with open(args.out) as f:
            rec = kernel_stats(args.kernel_stats, json.loads(f.read()))
    else:
        rec = run(args)
    text = json.dumps(rec)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
