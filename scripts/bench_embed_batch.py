"""Measure the variable-length attention kernel and the packed embedding route on one MI355X.

    python scripts/bench_embed_batch.py                      # both parts -> profiles/attention_varlen_bench.json
    python scripts/bench_embed_batch.py --only attention     # the attention alone
    python scripts/bench_embed_batch.py --only embedder --docs 1000
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_embed_batch.py --only trace   # kernel time, a run of its own

Part 1, the attention alone at 16 heads x 64, bf16, on the SAME fused-QKV tensor for every variant: `attention_varlen`, torch's SDPA
called once per sequence on views of that tensor, and the padded batch with an additive key mask (what the padded encoder forward
runs); for one 7 778-token sequence and for a mixed pack of 64 sequences of 30..500 tokens.  Times are device events around `--iters`
calls, the variants alternating inside every round, the median of `--rounds` rounds reported next to the extremes.  FLOP counts are
4 * heads * head_dim * sum(len^2) (QK^T and PV, no mask savings: the attention is non-causal).

Part 2, the embedder end to end at the bge-m3 shape (random weights): token rows per second of `embed_strings_batch` over `--docs` short
documents with a "packed" embedder, of the same call with a "padded" embedder, and of the per-document loop of `embed_strings`; host
clock around calls that end synchronised (they return NumPy matrices).

Needs a GPU: there is no fallback, and nothing here is a CPU number."""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import raglite_amd  # noqa: E402
from raglite_amd._torch_embedder import EncoderShape, TorchTokenEmbedder  # noqa: E402

HEADS, HEAD_DIM = 16, 64


def _packs() -> dict[str, list[int]]:
    rng = np.random.default_rng(64)
    return {"one_7778": [7778], "mixed_64x30to500": [int(x) for x in rng.integers(30, 501, size=64)]}


def _variants(lengths: list[int]):
    """name -> zero-argument callable, all reading one qkv tensor."""
    from torch.nn import functional as F  # noqa: N812

    n, d = sum(lengths), HEADS * HEAD_DIM
    g = torch.Generator(device="cuda").manual_seed(1)
    qkv = torch.randn((n, 3 * d), generator=g, device="cuda", dtype=torch.float32).to(torch.bfloat16)
    off_host = [0, *np.cumsum(lengths).tolist()]
    off = torch.tensor(off_host, dtype=torch.int32, device="cuda")
    max_len = max(lengths)
    q, k, v = qkv.view(n, 3, HEADS, HEAD_DIM).permute(1, 2, 0, 3)  # each (heads, n, head_dim): views, as the encoder takes them

    def kernel():
        return raglite_amd.attention_varlen(qkv, off, max_len, HEADS)

    def sdpa_per_sequence():
        return [F.scaled_dot_product_attention(q[None, :, lo:hi], k[None, :, lo:hi], v[None, :, lo:hi])
                for lo, hi in zip(off_host[:-1], off_host[1:])]

    # the padded batch: built once (the padded forward never builds it from a packed tensor), (B, heads, T, head_dim) views of (B, T, 3d)
    B, T = len(lengths), max_len  # noqa: N806
    padded = torch.zeros((B, T, 3 * d), device="cuda", dtype=torch.bfloat16)
    for i, (lo, hi) in enumerate(zip(off_host[:-1], off_host[1:])):
        padded[i, : hi - lo] = qkv[lo:hi]
    pq, pk, pv = padded.view(B, T, 3, HEADS, HEAD_DIM).permute(2, 0, 3, 1, 4)
    valid = torch.arange(T, device="cuda")[None, :] < torch.tensor(lengths, device="cuda")[:, None]
    mask = torch.zeros((B, 1, 1, T), dtype=torch.bfloat16, device="cuda").masked_fill(~valid[:, None, None, :], float("-inf"))

    def padded_key_mask():
        return F.scaled_dot_product_attention(pq, pk, pv, attn_mask=mask)

    got = kernel().view(n, HEADS, HEAD_DIM).float()
    want = torch.cat([o[0].transpose(0, 1) for o in sdpa_per_sequence()]).float()
    diff = float((got - want).abs().max())
    return {"attention_varlen": kernel, "sdpa_per_sequence": sdpa_per_sequence, "sdpa_padded_key_mask": padded_key_mask}, diff


def _time_ms(fn, iters: int) -> float:
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def bench_attention(iters: int, rounds: int) -> dict:
    out = {}
    for name, lengths in _packs().items():
        variants, diff = _variants(lengths)
        for fn in variants.values():  # warm every shape the timed window uses
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {v: [] for v in variants}
        for _ in range(rounds):
            for v, fn in variants.items():
                times[v].append(_time_ms(fn, iters))
        flops = 4.0 * HEADS * HEAD_DIM * float(sum(n * n for n in lengths))
        out[name] = {"sequences": len(lengths), "tokens": sum(lengths), "max_len": max(lengths), "flop": flops,
                     "max_abs_diff_kernel_vs_sdpa": diff,
                     "ms": {v: {"median": statistics.median(t), "min": min(t), "max": max(t)} for v, t in times.items()},
                     "kernel_tflops": flops / (statistics.median(times["attention_varlen"]) * 1e-3) / 1e12}
        print(name, json.dumps(out[name]["ms"]), file=sys.stderr)
    return out


def _short_documents(n_docs: int) -> list[list[str]]:
    """Seeded pseudo-prose: 1..6 sentences of 4..20 words per document (a few dozen to a few hundred tokens)."""
    rng = np.random.default_rng(7)
    docs = []
    for _ in range(n_docs):
        sentences = []
        for _ in range(int(rng.integers(1, 7))):
            words = ["".join(chr(97 + int(c)) for c in rng.integers(0, 26, size=int(rng.integers(2, 10)))) for _ in range(int(rng.integers(4, 21)))]
            sentences.append(" ".join(words).capitalize() + ". ")
        docs.append(sentences)
    return docs


def bench_embedder(n_docs: int) -> dict:
    config = raglite_amd.HotPathConfig(embedder="llama-cpp-python/bench/bge-m3-shaped")
    emb = TorchTokenEmbedder(EncoderShape(), device="cuda")
    docs = _short_documents(n_docs)

    def loop(d):
        return [raglite_amd.embed_strings(x, config=config, embedder=emb) for x in d]

    def batch(d):
        return raglite_amd.embed_strings_batch(d, config=config, embedder=emb)

    routes = {"embed_strings_batch_packed": ("packed", batch), "embed_strings_batch_padded": ("padded", batch),
              "embed_strings_loop_padded": ("padded", loop)}
    out = {"documents": n_docs, "sentences": sum(len(d) for d in docs), "pack_tokens": emb.pack_tokens, "routes": {}}
    results = {}
    for name, (batching, fn) in routes.items():
        emb.batching = batching
        fn(docs[: min(64, n_docs)])  # warm-up: code objects, GEMM algorithm choice
        torch.cuda.synchronize()
        calls = emb.embed_calls
        rows = _TokenRows(emb)
        t0 = time.perf_counter()
        results[name] = fn(docs)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out["routes"][name] = {"seconds": dt, "token_rows": rows.stop(), "token_rows_per_s": rows.total / dt, "embed_calls": emb.embed_calls - calls}
        print(name, json.dumps(out["routes"][name]), file=sys.stderr)
    base = results["embed_strings_loop_padded"]
    out["max_abs_diff_vs_loop"] = {name: max(float(np.abs(a.astype(np.float32) - b.astype(np.float32)).max()) for a, b in zip(r, base))
                                   for name, r in results.items() if name != "embed_strings_loop_padded"}
    return out


class _TokenRows:
    """Counts the token rows `embedder.embed` returns while it is active (host-side shapes only)."""

    def __init__(self, emb) -> None:
        self.emb, self.total, self._embed = emb, 0, emb.embed
        emb.embed = self._counting

    def _counting(self, text):
        got = self._embed(text)
        self.total += int(got.shape[0]) if isinstance(text, str) else sum(int(m.shape[0]) for m in got)
        return got

    def stop(self) -> int:
        del self.emb.embed  # back to the class's method
        return self.total


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", choices=["attention", "embedder", "trace"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--docs", type=int, default=1000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "attention_varlen_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_embed_batch.py needs a GPU")
    raglite_amd.set_device(0)
    if args.only == "trace":  # for the profiler: the kernel alone, a few dozen launches per pack
        for lengths in _packs().values():
            kernel = _variants(lengths)[0]["attention_varlen"]
            for _ in range(30):
                kernel()
        torch.cuda.synchronize()
        return
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "heads": HEADS, "head_dim": HEAD_DIM, "dtype": "bfloat16",
              "iters": args.iters, "rounds": args.rounds}
    if args.only != "embedder":
        result["attention"] = bench_attention(args.iters, args.rounds)
    if args.only != "attention":
        result["embedder"] = bench_embedder(args.docs)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
