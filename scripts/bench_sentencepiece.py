"""The device SentencePiece Unigram tokenizer against the `sentencepiece` library on the same host, alone and inside the embedder
(DESIGN.md 4.25).

    python scripts/bench_sentencepiece.py [--rounds 7] [--out profiles/sentencepiece_bench.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_sentencepiece.py --trace     (a run of its own, no counters)

The model is the committed 2 000-piece Unigram fixture (tests/golden/unigram_2k.model, trained on this repository's Markdown): the
published 250 k-piece vocabulary is not in this tree, and every number below is about the synthetic fixture.  Texts are made of the
words of this repository's Markdown.  The routes alternate inside every round; the median over rounds is reported with the smallest
and the largest round next to it.  No factor is fixed in advance.
  encode   `DeviceSentencePiece.encode_batch` (the UTF-32 encode, the upload, the kernels and the copy of the results into torch tensors
           included; host clock around a call that ends synchronised) against `SentencePieceProcessor.encode(list_of_texts)` of the
           same library in the same run, at three shapes: 256 queries of 8 .. 16 tokens, 1 000 documents of about 120 tokens, one
           document of about 8 000 tokens (one wave walks it alone: expected to lose)
  embedder `TorchTokenEmbedder(short_forward="native").embed_pack` of the 256 queries and `embed(list)` of the 1 000 documents in groups
           of 100 (batching="packed": the call `embed_strings_batch` makes per group) with the device tokenizer against the same calls
           with `SentencePieceTokenizer`; outputs compared first
Needs a GPU: there is no fallback."""

from __future__ import annotations

import argparse
import json
import re
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
MODEL = ROOT / "tests" / "golden" / "unigram_2k.model"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sentencepiece_bench.json"))
    ap.add_argument("--trace", action="store_true", help="three encode_batch calls per shape: the run a kernel trace is taken of")
    args = ap.parse_args()

    import numpy as np
    import torch

    import raglite_amd
    from raglite_amd._sentencepiece import DeviceSentencePiece, UnigramTables
    from raglite_amd._torch_embedder import EncoderShape, SentencePieceTokenizer, TorchTokenEmbedder

    if not torch.cuda.is_available():
        raise SystemExit("bench_sentencepiece.py measures on a GPU; none is visible")
    raglite_amd.set_device(0)
    rng = np.random.default_rng(0)
    t0 = time.perf_counter()
    tables = UnigramTables.from_model(MODEL)
    build_s = time.perf_counter() - t0
    device_tok = DeviceSentencePiece(tables)
    sp = tables.processor()
    words = sorted({w for p in sorted(ROOT.glob("*.md")) for w in re.findall(r"[A-Za-z][A-Za-z0-9_\-']{0,15}", p.read_text(errors="replace"))})
    per_word = sum(map(len, sp.encode(words))) / len(words)  # (each word alone: a dummy prefix per word, as inside a text)

    def text_of(n_tokens: float) -> str:
        return " ".join(rng.choice(words, size=max(int(round(n_tokens / per_word)), 1)).tolist())

    shapes = {
        "queries_256x8-16": [text_of(float(rng.uniform(8, 16))) for _ in range(256)],
        "documents_1000x120": [text_of(float(rng.normal(120, 20))) for _ in range(1000)],
        "one_document_8000": [text_of(8000)],
    }
    if args.trace:
        for texts in shapes.values():
            for _ in range(3):
                device_tok.encode_batch(texts)
        torch.cuda.synchronize()
        print(json.dumps({"trace": "3 encode_batch calls per shape: " + ", ".join(shapes)}))
        return

    stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}  # noqa: E731

    def wall(call) -> float:
        torch.cuda.synchronize()
        t = time.perf_counter()
        call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    result = {"model": f"tests/golden/unigram_2k.model: synthetic, {tables.vocab_size} pieces, longest {tables.longest_piece}; tables built in {build_s:.1f} s",
              "note": "the published 250 k-piece vocabulary is not in this tree: every number is about the synthetic fixture",
              "table": device_tok.info(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "host_library": "sentencepiece, sp.encode(list)",
              "encode": {}, "embedder": {}}
    for name, texts in shapes.items():
        ids, offsets, counts = device_tok.encode_batch(texts, xlmr=False)
        off, flat = offsets.cpu().tolist(), ids.cpu().tolist()
        same = [flat[off[i]: off[i + 1]] for i in range(len(texts))] == sp.encode(texts)
        dev, host = [], []
        for _ in range(args.rounds):
            dev.append(wall(lambda t=texts: device_tok.encode_batch(t)))
            host.append(wall(lambda t=texts: sp.encode(t)))
        n = counts["tokens"]
        result["encode"][name] = {"texts": len(texts), "tokens": n, "symbols": counts["symbols"], "flagged": counts["flagged"], "ids_equal_the_library": same,
                                  "device_ms": stat(dev), "host_ms": stat(host), "device_tokens_per_s": n / statistics.median(dev) * 1e3,
                                  "host_tokens_per_s": n / statistics.median(host) * 1e3, "host_over_device": statistics.median(host) / statistics.median(dev)}
        print(name, json.dumps(result["encode"][name]), flush=True)

    shape = EncoderShape(vocab_size=tables.vocab_size + 8, hidden=384, layers=12, heads=12, ffn=1536, max_positions=520, n_ctx=512)
    host_tok = SentencePieceTokenizer(model_proto=tables.model_proto)
    make = lambda tok, **kw: TorchTokenEmbedder(shape, tokenizer=tok, device="cuda", seed=1, **kw)  # noqa: E731
    pairs = {"embed_pack_256_queries": (make(device_tok, short_forward="native"), make(host_tok, short_forward="native"), shapes["queries_256x8-16"]),
             "embed_packed_1000_documents": (make(device_tok, batching="packed"), make(host_tok, batching="packed"), shapes["documents_1000x120"])}
    for name, (on_device, on_host, texts) in pairs.items():
        if name == "embed_pack_256_queries":
            call = lambda e, t=texts: e.embed_pack(t)  # noqa: E731
            same = all(torch.equal(a, b) for a, b in zip(call(on_device), call(on_host)))
        else:
            # (`embed_strings_batch` itself needs the sentinel of `_embed.py` in the vocabulary, which the 2 000-piece fixture does not
            # hold: what is timed is the call it makes per group, `embed(list)` on the packed route, in groups of `pack_tokens` tokens)
            groups = [texts[i: i + 100] for i in range(0, len(texts), 100)]
            call = lambda e, g=groups: [m for part in g for m in e.embed(part)]  # noqa: E731
            same = all(torch.equal(a, b) for a, b in zip(call(on_device), call(on_host)))
        dev, host = [], []
        for _ in range(args.rounds):
            dev.append(wall(lambda: call(on_device)))
            host.append(wall(lambda: call(on_host)))
        result["embedder"][name] = {"shape": "12 x 384, 12 heads, ffn 1536, bf16, random weights", "texts": len(texts), "outputs_equal": same,
                                    "device_tokenizer_ms": stat(dev), "host_tokenizer_ms": stat(host),
                                    "host_over_device": statistics.median(host) / statistics.median(dev)}
        print(name, json.dumps(result["embedder"][name]), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
