"""The fusion step of a sharded hybrid batch on ONE GPU (rl_shard_hybrid_fuse; DESIGN.md "Sharded keyword and hybrid search").

    python scripts/bench_shard_fuse.py [--world 8] [--batches 16,256] [--num-hits 128] [--n-each 32] [--iters 200] --out R.json
        the records every rank of a `world`-rank batch hands into the one all-gather (tests/shard_fuse_ref.py's random records:
        integer scores, several rows per chunk, padding), already on the device.  Per batch, with device events around each variant:
          kernel   rl_shard_hybrid_fuse on device pointers (one launch)
          compose  the composition the Python layer falls back to past the kernel's limits: the row merge, group_chunk_max_host,
                   the keyword merge on the host, then rl_rrf_fuse (device -> host -> device)
          rrf      rl_rrf_fuse alone over two lists of n_each per query (the fusion the kernel ends with), for scale
        and checks that kernel and compose agree bit for bit.  Writes one JSON record.  One GPU: this times the step after the
        exchange, not the exchange, and says nothing about multi-GPU scaling.
"""

from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np


def timed(fn, iters: int) -> float:
    """Median microseconds per call over `iters` calls, each between two device events."""
    import torch

    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1000.0)
    return float(np.median(times))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--batches", default="16,256")
    ap.add_argument("--num-hits", type=int, default=128)
    ap.add_argument("--n-each", type=int, default=32)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import raglite_amd
    from raglite_amd import _ops
    from raglite_amd._sharded import compose_hybrid_fuse
    from tests import shard_fuse_ref as ref

    raglite_amd.set_device(0)
    rng = np.random.default_rng(0)
    rows = []
    for B in (int(x) for x in args.batches.split(",")):
        g = torch.from_numpy(ref.random_records(rng, args.world, B, args.num_hits, args.n_each, True)).cuda()
        kw = dict(num_hits=args.num_hits, n_each=args.n_each, keywords=True, weights=(0.75, 0.25), rrf_k=60, k=2 * args.n_each)
        lists = torch.from_numpy(rng.integers(-1, 4 * args.n_each, size=(2, B, args.n_each)).astype(np.int32)).cuda()
        got, want = _ops.shard_hybrid_fuse(g, **kw), compose_hybrid_fuse(g, **kw)
        same = all(torch.equal(x.view(torch.uint8) if x.dtype == torch.float64 else x, y.view(torch.uint8) if y.dtype == torch.float64 else y)
                   for x, y in zip(got, want))
        rec = {"world": args.world, "batch": B, "num_hits": args.num_hits, "n_each": args.n_each, "equal": bool(same),
               "kernel_us": round(timed(lambda: _ops.shard_hybrid_fuse(g, **kw), args.iters), 2),
               "compose_us": round(timed(lambda: compose_hybrid_fuse(g, **kw), max(10, args.iters // 10)), 2),
               "rrf_us": round(timed(lambda: _ops.rrf_fuse(lists, (0.75, 0.25), rrf_k=60, k=2 * args.n_each), args.iters), 2)}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
    out = {"bench": "shard_hybrid_fuse", "device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    if not all(r["equal"] for r in rows):
        raise SystemExit("kernel and composition disagree")


if __name__ == "__main__":
    main()
