"""The query-adapter fit with the targets solved on the device (`update_query_adapter(targets="device")`, one `rl_query_targets` call;
DESIGN.md §4.15) against the per-eval host NNLS (`targets="nnls"`, the reference's `lsq_linear` call).

    python scripts/bench_query_adapter.py [--chunks 100000] [--dim 1024] [--evals 1024] [--top-k 40] [--small] --out R.json
        Seeded synthetic index: --chunks one-row chunks in clusters of --top-k around unit centres (fp16-rounded unit rows, f16
        storage), --evals evals whose question is a noisy cluster member and whose relevant chunks are five members of that cluster,
        so every eval retrieves positives and negatives and qualifies.  --small: 4 000 chunks at dim 128, 64 evals, top-k 10 -- a quick
        check of the script, not a measurement.  One run reports, in milliseconds:
          device_wall_ms       update_query_adapter(targets="device") for all evals, warm, and of that
          targets_call_wall_ms   the optimize_query_targets call inside it (host arrays in and out: staging, three kernels, read-back)
          adapter_ms             _adapter_from_targets (normalisation, T^T Q, rank, pseudo-inverse, SVD) and  svd_ms  the SVD alone
          host_remainder_ms      the rest: embedding casts, the two searches' calls, relevance masks from string ids
          query_targets_ms     the rl_query_targets call alone on device arrays (device events; wall next to it)
          nnls_*               the baseline, update_query_adapter(targets="nnls") on the FIRST --nnls-evals evals only (the full loop
                               takes minutes): its wall clock, the share inside _optimize_query_target, and that share scaled to all
                               evals (nnls_loop_scaled_ms = share x evals / nnls-evals)
          norm_ratio           per baseline eval |t_nnls|^2 / |t_device|^2 (float64, before the cast): min, median, max; nothing below
                               1 - 1e-12 is possible for a converged solve, and how far above 1 shows how far lsq_linear stopped short
          adapter_rel_diff     |A_nnls - A_device|_F / |A_device|_F of the two adapters fitted on those evals
    python scripts/bench_query_adapter.py --device-only --out T.json
        only the rl_query_targets calls: the run to put under `rocprofv3 --kernel-trace --stats`.
    python scripts/bench_query_adapter.py --kernel-stats <kernel_stats.csv> --out R.json
        adds to the record R.json each kernel's mean time per launch from that run.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np


def make_index(rng, n_chunks: int, dim: int, per_cluster: int):
    """(rows float16 (n_chunks, dim), cluster of every chunk): unit rows 0.5 away from their cluster's unit centre."""
    n_clusters = -(-n_chunks // per_cluster)
    cluster = np.repeat(np.arange(n_clusters), per_cluster)[:n_chunks]
    rows = np.empty((n_chunks, dim), np.float16)
    for lo in range(0, n_clusters, 256):  # in slabs: the float64 normals of 100 000 x 1024 at once would be 800 MB
        hi = min(lo + 256, n_clusters)
        centres = rng.standard_normal((hi - lo, dim), dtype=np.float32)
        centres /= np.linalg.norm(centres, axis=1, keepdims=True)
        sel = slice(lo * per_cluster, min(hi * per_cluster, n_chunks))
        x = centres[cluster[sel] - lo] + 0.5 * rng.standard_normal((sel.stop - sel.start, dim), dtype=np.float32) / np.sqrt(dim)
        rows[sel] = x / np.linalg.norm(x, axis=1, keepdims=True)
    return rows, cluster


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


class Timed:
    """Wraps an attribute of a module with a wall-clock accumulator for the time of a `with` block."""

    def __init__(self, owner, name):
        self.owner, self.name, self.real, self.ms, self.calls, self.last = owner, name, getattr(owner, name), 0.0, 0, None

    def __enter__(self):
        def timed(*a, **k):
            t0 = time.perf_counter()
            try:
                self.last = (a, k)
                return self.real(*a, **k)
            finally:
                self.ms += (time.perf_counter() - t0) * 1e3
                self.calls += 1

        setattr(self.owner, self.name, timed)
        return self

    def __exit__(self, *exc):
        setattr(self.owner, self.name, self.real)


def run(args) -> dict:
    import torch

    import raglite_amd
    from raglite_amd import _query_adapter as qa

    assert torch.cuda.is_available(), "bench_query_adapter needs a GPU"
    raglite_amd.set_device(0)
    rng = np.random.default_rng(args.seed)
    rows, cluster = make_index(rng, args.chunks, args.dim, args.top_k)
    ids = [f"{i:08x}" for i in range(args.chunks)]
    gi = raglite_amd.GpuIndex(ids, rows, chunk_offsets=np.arange(args.chunks + 1, dtype=np.int64), storage="f16")
    evals = []
    for _ in range(args.evals):
        t = int(rng.integers(0, args.chunks))
        members = np.flatnonzero(cluster == cluster[t])
        q = rows[t].astype(np.float32) + 0.3 * rng.standard_normal(args.dim, dtype=np.float32) / np.sqrt(args.dim)
        evals.append((q.astype(np.float16), [ids[m] for m in rng.choice(members, size=min(5, len(members)), replace=False)]))
    cfg = raglite_amd.HotPathConfig()
    rec = {"chunks": args.chunks, "dim": args.dim, "evals": args.evals, "optimize_top_k": args.top_k, "storage": "f16",
           "small": bool(args.small), "iters": args.iters}

    # -- the call alone, on device arrays: the inputs update_query_adapter hands it
    with Timed(qa, "optimize_query_targets") as call:
        raglite_amd.update_query_adapter(evals, optimize_top_k=args.top_k, config=cfg, index=gi, targets="device")  # also the warm-up
    (Q, ex_rows, ex_rel), kw = call.last  # noqa: N806
    rec["qualifying_evals"] = len(Q)
    rec["positives_per_eval_mean"] = round(float(np.mean(np.sum((ex_rel != 0) & (ex_rows >= 0), axis=1))), 2)
    d_q, d_rows, d_rel = (torch.as_tensor(a, device="cuda") for a in (Q, ex_rows, ex_rel))
    out = {}

    def targets():
        out["t"] = raglite_amd.optimize_query_targets(d_q, d_rows, d_rel, gap=kw["gap"], index=gi)

    rec["query_targets_ms"], rec["query_targets_wall_ms"] = (round(v, 3) for v in events_ms(torch, targets, 1, args.iters))
    status, iters = out["t"][3].cpu().numpy(), out["t"][4].cpu().numpy()
    rec["status_counts"] = np.bincount(status, minlength=5).tolist()
    rec["entering_steps"] = {"mean": round(float(iters.mean()), 2), "max": int(iters.max())}
    rec["row_read_bytes"] = int(np.sum(ex_rows >= 0)) * args.dim * 2 * 2  # the example rows, fp16, by the Gram and by the target kernel
    rec["gram_flop"] = int(len(Q)) * args.top_k * args.top_k * args.dim * 2
    if args.device_only:
        return rec

    # -- the whole fit with device targets, warm, and where its wall clock goes
    walls = []
    for _ in range(args.iters):
        with Timed(qa, "optimize_query_targets") as call, Timed(qa, "_adapter_from_targets") as fit:
            t0 = time.perf_counter()
            a_dev = raglite_amd.update_query_adapter(evals, optimize_top_k=args.top_k, config=cfg, index=gi, targets="device")
            walls.append(((time.perf_counter() - t0) * 1e3, call.ms, fit.ms))
    wall, call_ms, fit_ms = sorted(walls)[len(walls) // 2]
    rec.update(device_wall_ms=round(wall, 2), targets_call_wall_ms=round(call_ms, 2), adapter_ms=round(fit_ms, 2),
               host_remainder_ms=round(wall - call_ms - fit_ms, 2))
    m = rng.standard_normal((args.dim, args.dim))
    t0 = time.perf_counter()
    np.linalg.svd(m, full_matrices=False)
    rec["svd_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    del a_dev

    # -- the baseline on the first evals, and how far its solver stops from the optimum
    first = evals[: args.nnls_evals]
    with Timed(qa, "_optimize_query_target") as nnls, Timed(qa, "_adapter_from_targets") as fit:
        t0 = time.perf_counter()
        a_nnls = raglite_amd.update_query_adapter(first, optimize_top_k=args.top_k, config=cfg, index=gi, targets="nnls")
        rec["nnls_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    rec.update(nnls_evals=len(first), nnls_qualifying_evals=nnls.calls, nnls_loop_ms=round(nnls.ms, 2),
               nnls_loop_scaled_ms=round(nnls.ms * len(Q) / max(nnls.calls, 1), 1),
               nnls_note="timed on the first evals only and scaled by the count of qualifying evals: the full loop takes minutes")
    a_dev = raglite_amd.update_query_adapter(first, optimize_top_k=args.top_k, config=cfg, index=gi, targets="device")
    rec["adapter_rel_diff"] = float(np.linalg.norm(a_nnls - a_dev) / np.linalg.norm(a_dev))
    # per eval: the reference's call in float64 (before the cast) against the device's target
    n_first = nnls.calls
    t_dev = out["t"][0][:n_first].cpu().numpy()
    ratios = []
    for b in range(n_first):
        have = ex_rows[b] >= 0
        P = rows[ex_rows[b][have & (ex_rel[b] != 0)]].astype(np.float64)  # noqa: N806
        N = rows[ex_rows[b][have & (ex_rel[b] == 0)]].astype(np.float64)  # noqa: N806
        t_ref = qa._optimize_query_target(Q[b].astype(np.float64), P, N, alpha=kw["gap"])  # noqa: SLF001
        ratios.append(float(t_ref @ t_ref) / float(t_dev[b] @ t_dev[b]))
    rec["norm_ratio"] = {"min": min(ratios), "median": float(np.median(ratios)), "max": max(ratios), "per_eval": [round(r, 9) for r in ratios]}
    gi.close()
    return rec


KERNELS = ("qt_gram_kernel", "qt_solve_kernel", "qt_target_kernel")


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
    ap.add_argument("--chunks", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--evals", type=int, default=1024)
    ap.add_argument("--top-k", type=int, default=40)
    ap.add_argument("--nnls-evals", type=int, default=32)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.small:
        args.chunks, args.dim, args.evals, args.top_k, args.nnls_evals = 4000, 128, 64, 10, 8
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
