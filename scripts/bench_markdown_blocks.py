"""The Markdown parse of the two batched splitters: markdown-it on the host against `rl_markdown_blocks`.

    python scripts/bench_markdown_blocks.py [--docs 1000] [--small] --out R.json
        The corpora of scripts/bench_split_sentences.py and scripts/bench_split_chunklets.py (the same seeded synthetic Markdown:
        documents of U{20 .. 2000} sentences; for the sentence splitter joined, for the chunklet splitter as sentence lists).  --small:
        30 documents of U{5 .. 80} sentences, a quick check of the script, not a measurement.  One run reports, per splitter and in
        milliseconds for all documents together:
          host_batch_ms        split_*_batch(markdown="host"), warm: what the parent commit does (one run: the parse alone takes seconds),
                               and of that host_parse_ms, the time inside markdown_*_boundaries (markdown-it), timed around every call
          device_batch_ms      split_*_batch(markdown="device"), warm, median of --iters; of that device_fallback_parse_ms, the time
                               inside markdown-it for the documents the device parser gave up
          blocks_call_ms       rl_markdown_blocks alone on device arrays (device events; wall next to it), median of --iters
          derived_call_ms      rl_markdown_sentence_known / rl_markdown_chunklet_boundary alone, the same way
          undecided_docs       how many documents the device parser gave up, and undecided_share
          docs_that_differ     documents whose device-route result differs from the host route's (0 is the contract)
        Writes one JSON record.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from scripts.bench_split_chunklets import Stopwatch, events_ms, make_documents
from scripts.bench_split_sentences import make_predictions


def _median_wall(fn, iters: int) -> tuple[float, object]:
    wall, out = [], None
    for _ in range(iters):
        t0 = time.perf_counter()
        out = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(wall)), out


def run(args) -> dict:
    import torch

    import raglite_amd
    from raglite_amd import _chunklets, _markdown, _sentences

    assert torch.cuda.is_available(), "bench_markdown_blocks needs a GPU"
    raglite_amd.set_device(0)
    rng = np.random.default_rng(args.seed)
    lo, hi = (5, 80) if args.small else (20, 2000)
    lists = make_documents(rng, args.docs, lo, hi)
    docs = ["".join(d) for d in lists]
    predicted = [make_predictions(rng, d) for d in docs]
    n = sum(len(d) for d in docs)
    n_sent = sum(len(d) for d in lists)
    rec = {"docs": args.docs, "characters": n, "sentences": n_sent, "small": bool(args.small), "iters": args.iters,
           "min_len": args.min_len, "max_len": args.max_len, "max_size": args.max_size}
    print(f"{args.docs} documents, {n} characters, {n_sent} sentences", file=sys.stderr, flush=True)

    # -- the parser alone, on device arrays
    cp = torch.from_numpy(_sentences.codepoints_of("".join(docs)).view(np.int32).copy()).cuda()
    off = np.concatenate(([0], np.cumsum([len(d) for d in docs]))).astype(np.int64)
    d_off = torch.from_numpy(off).cuda()
    out = {}

    def blocks():
        out["blocks"] = _markdown.markdown_blocks(cp, d_off)

    rec["blocks_call_ms"], rec["blocks_call_wall_ms"] = (round(v, 3) for v in events_ms(torch, blocks, 1, args.iters))
    first_open, heading_end, line_start, line_offsets, status = out["blocks"]
    undecided = int((status != 0).sum().item())
    rec.update(lines=int(line_offsets[-1].item()), undecided_docs=undecided, undecided_share=round(undecided / max(args.docs, 1), 4))
    again = _markdown.markdown_blocks(cp, d_off)
    n_lines = rec["lines"]
    rec["same_bytes_run_to_run"] = bool(all(torch.equal(a[:n_lines], b[:n_lines]) for a, b in zip(out["blocks"][:3], again[:3]))
                                        and torch.equal(line_offsets, again[3]) and torch.equal(status, again[4]))
    rec["sentence_known_call_ms"] = round(events_ms(torch, lambda: _markdown.markdown_sentence_known(heading_end, line_start, line_offsets, status, d_off, n), 1, args.iters)[0], 3)
    sent_off = np.concatenate(([0], np.cumsum([len(s) for d in lists for s in d]))).astype(np.int64)
    sent_doc_off = np.concatenate(([0], np.cumsum([len(d) for d in lists]))).astype(np.int64)
    d_soff, d_sdoff = torch.from_numpy(sent_off).cuda(), torch.from_numpy(sent_doc_off).cuda()
    rec["chunklet_boundary_call_ms"] = round(events_ms(
        torch, lambda: _markdown.markdown_chunklet_boundary(first_open, line_start, line_offsets, status, d_soff, d_sdoff), 1, args.iters)[0], 3)
    print("calls done", file=sys.stderr, flush=True)

    # -- split_sentences_batch, both routes
    small = docs[:2]
    for route in ("host", "device"):
        raglite_amd.split_sentences_batch(small, args.min_len, args.max_len, predicted_probas=predicted[:2], markdown=route)  # warm
    sentences = {}
    with Stopwatch(_sentences, "markdown_sentence_boundaries") as parse:
        t0 = time.perf_counter()
        sentences["host"] = raglite_amd.split_sentences_batch(docs, args.min_len, args.max_len, predicted_probas=predicted)
        host_ms = (time.perf_counter() - t0) * 1e3
    rec["sentences_route"] = {"host_batch_ms": round(host_ms, 2), "host_parse_ms": round(parse.seconds * 1e3, 2)}
    with Stopwatch(_sentences, "markdown_sentence_boundaries") as parse:
        device_ms, sentences["device"] = _median_wall(
            lambda: raglite_amd.split_sentences_batch(docs, args.min_len, args.max_len, predicted_probas=predicted, markdown="device"), args.iters)
    rec["sentences_route"].update(device_batch_ms=round(device_ms, 2), device_fallback_parse_ms=round(parse.seconds * 1e3 / args.iters, 2),
                                  docs_that_differ=sum(a != b for a, b in zip(sentences["host"], sentences["device"])),
                                  host_over_device=round(host_ms / device_ms, 2))
    print("sentences done", file=sys.stderr, flush=True)

    # -- split_chunklets_batch, both routes
    for route in ("host", "device"):
        raglite_amd.split_chunklets_batch(lists[:2], args.max_size, markdown=route)  # warm
    chunklets = {}
    with Stopwatch(_chunklets, "markdown_chunklet_boundaries") as parse:
        t0 = time.perf_counter()
        chunklets["host"] = raglite_amd.split_chunklets_batch(lists, args.max_size)
        host_ms = (time.perf_counter() - t0) * 1e3
    rec["chunklets_route"] = {"host_batch_ms": round(host_ms, 2), "host_parse_ms": round(parse.seconds * 1e3, 2)}
    with Stopwatch(_chunklets, "markdown_chunklet_boundaries") as parse:
        device_ms, chunklets["device"] = _median_wall(lambda: raglite_amd.split_chunklets_batch(lists, args.max_size, markdown="device"), args.iters)
    rec["chunklets_route"].update(device_batch_ms=round(device_ms, 2), device_fallback_parse_ms=round(parse.seconds * 1e3 / args.iters, 2),
                                  docs_that_differ=sum(a != b for a, b in zip(chunklets["host"], chunklets["device"])),
                                  host_over_device=round(host_ms / device_ms, 2))
    assert _markdown.MARKDOWN_OK == 0
    return rec


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000)
    ap.add_argument("--min-len", type=int, default=4)
    ap.add_argument("--max-len", type=int, default=2048)
    ap.add_argument("--max-size", type=int, default=2048)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
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
