"""Chunklet splitting of many documents: a loop of the host `split_chunklets` against `split_chunklets_batch` (one
`rl_partition_chunklets` call).

    python scripts/bench_split_chunklets.py [--docs 1000] [--small] --out R.json
        Seeded synthetic Markdown documents (the text generator of tests/chunklets_ref.py: headings, paragraphs, lists, quotes):
        --docs documents of U{20 .. 2000} sentences, max_size 2048.  --small: 30 documents of U{5 .. 80} sentences, a quick check of
        the script, not a measurement.  One run reports, in milliseconds for all documents together:
          loop_ms              a loop of split_chunklets(partition="host") over the documents -- the baseline -- and of that
          loop_parse_ms        the time inside markdown_chunklet_boundaries (markdown-it), timed around every call
          loop_recurrence_ms   the time inside chunklet_dp, the host statement of the recurrence, timed around every call
          batch_ms             split_chunklets_batch over the same documents, warm, Markdown parse included (one run: the parse
                               dominates it and does not change between runs)
          call_ms              the rl_partition_chunklets call alone on prepared device arrays (device events; wall next to it,
                               median of --iters): memset, prefixes, window ends, the recurrence with its backtrack.  This is what
                               replaces loop_recurrence_ms; recurrence_over_call is their ratio
          call_host_ms         the same call on host pointers (staging and the read-back included), wall
          host_*_ms            the host remainder of split_chunklets_batch: Markdown parse, counts and quantiles (word counts,
                               compute_num_statements, string lengths), joins
        and how many documents come out with other chunklets than the loop's (0 is expected: both are exact and share their tie
        rule).  Writes one JSON record.
    python scripts/bench_split_chunklets.py --device-only --out T.json
        only the C call on the same documents (boundary probabilities drawn, not parsed): the run to put under a kernel trace.
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
    from tests.chunklets_ref import make_sentences

    return [make_sentences(int(rng.integers(1, 1 << 30)), int(rng.integers(lo, hi + 1)), "mixed") for _ in range(n_docs)]


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


class Stopwatch:
    """Wraps a module-level function and adds up the time spent inside it."""

    def __init__(self, module, name: str) -> None:
        self.module, self.name, self.fn, self.seconds = module, name, getattr(module, name), 0.0

    def __enter__(self):
        def timed(*a, **k):
            t0 = time.perf_counter()
            try:
                return self.fn(*a, **k)
            finally:
                self.seconds += time.perf_counter() - t0

        setattr(self.module, self.name, timed)
        return self

    def __exit__(self, *exc) -> None:
        setattr(self.module, self.name, self.fn)


def run(args) -> dict:
    import torch

    import raglite_amd
    from raglite_amd import _chunklets

    assert torch.cuda.is_available(), "bench_split_chunklets needs a GPU"
    raglite_amd.set_device(0)
    rng = np.random.default_rng(args.seed)
    lo, hi = (5, 80) if args.small else (20, 2000)
    docs = make_documents(rng, args.docs, lo, hi)
    counts = np.asarray([len(d) for d in docs], np.int64)
    off = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    n = int(off[-1])
    rec = {"docs": args.docs, "sentences": n, "sentences_per_doc": f"U{{{lo}..{hi}}}", "characters": int(sum(len(s) for d in docs for s in d)),
           "max_size": args.max_size, "small": bool(args.small), "iters": args.iters}
    print(f"{args.docs} documents, {n} sentences", file=sys.stderr, flush=True)

    out = {}
    if not args.device_only:
        # -- the baseline: a loop of the host function, the parse's and the recurrence's shares timed around every call
        raglite_amd.split_chunklets(docs[0], max_size=args.max_size)  # warm: markdown-it import
        with Stopwatch(_chunklets, "markdown_chunklet_boundaries") as parse, Stopwatch(_chunklets, "chunklet_dp") as recurrence:
            t0 = time.perf_counter()
            loop = [raglite_amd.split_chunklets(d, max_size=args.max_size) for d in docs]
            rec["loop_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        rec["loop_parse_ms"], rec["loop_recurrence_ms"] = round(parse.seconds * 1e3, 2), round(recurrence.seconds * 1e3, 2)
        print("loop done", file=sys.stderr, flush=True)

        # -- the batched call, warm, and the host remainder step by step
        raglite_amd.split_chunklets_batch(docs[:2], args.max_size)  # warm: library, device
        t0 = time.perf_counter()
        batch = raglite_amd.split_chunklets_batch(docs, args.max_size)
        rec["batch_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        rec["docs_with_other_chunklets_than_the_loop"] = sum(a != b for a, b in zip(batch, loop))
        rec["chunklets"] = sum(len(c) for c in batch)
        print("batch done", file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        boundary = np.concatenate([_chunklets.markdown_chunklet_boundaries(d) for d in docs])
        t1 = time.perf_counter()
        statements = np.concatenate([_chunklets.compute_num_statements(d) for d in docs])
        lengths = np.fromiter((len(s) for d in docs for s in d), dtype=np.int64, count=n)
        t2 = time.perf_counter()
        joined = [["".join(d[i:i + 3]) for i in range(0, len(d), 3)] for d in docs]  # joins of the size the partition produces
        del joined
        t3 = time.perf_counter()
        rec.update(host_parse_ms=round((t1 - t0) * 1e3, 2), host_counts_quantiles_ms=round((t2 - t1) * 1e3, 2),
                   host_joins_ms=round((t3 - t2) * 1e3, 2))
    else:
        boundary = rng.choice(np.asarray([0.0, 0.0, 0.0, 0.25, 0.5, 1.0]), size=n)
        statements = np.concatenate([_chunklets.compute_num_statements(d) for d in docs])
        lengths = np.fromiter((len(s) for d in docs for s in d), dtype=np.int64, count=n)

    # -- the C call alone
    d_b, d_s, d_len, d_off = (torch.from_numpy(a).cuda() for a in (boundary, statements, lengths, off))

    def call():
        out["call"] = raglite_amd.partition_chunklets(d_b, d_s, d_len, d_off, args.max_size)

    rec["call_ms"], rec["call_wall_ms"] = (round(v, 3) for v in events_ms(torch, call, 1, args.iters))
    wall = []
    for _ in range(args.iters):
        t0 = time.perf_counter()
        out["host"] = raglite_amd.partition_chunklets(boundary, statements, lengths, off, args.max_size)
        wall.append((time.perf_counter() - t0) * 1e3)
    rec["call_host_ms"] = round(float(np.median(wall)), 3)
    assert np.array_equal(out["call"][0].cpu().numpy(), out["host"][0]), "host and device pointers disagree on the cuts"
    rec["cuts"] = int(out["host"][0].sum())
    rec["status_counts"] = np.bincount(out["host"][2], minlength=3).tolist()
    if "loop_recurrence_ms" in rec:
        rec["recurrence_over_call"] = round(rec["loop_recurrence_ms"] / rec["call_ms"], 1)
    # boundary 8 + statements 8 + lengths 8 read, cut 1 (memset) + 1 (cuts) per sentence; the six scratch arrays written once and read
    # at least once (dp, pb, ps and boundary once per window position on top of that, from L2)
    rec["call_bytes_min"] = n * (24 + 2) + (n + args.docs) * 48 * 2
    return rec


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000)
    ap.add_argument("--max-size", type=int, default=2048)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.small:
        args.docs = 30
    rec = run(args)
    text = json.dumps(rec)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
