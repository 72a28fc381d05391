"""The device WordPiece tokenizer against the `tokenizers` library on the same host, alone and inside `rank_batch`.

    python scripts/bench_wordpiece.py [--rounds 5] [--out profiles/wordpiece_bench.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_wordpiece.py --trace     (a run of its own, no counters)

A synthetic BERT vocabulary of 30 522 pieces (the size of bert-base-uncased's; no file is fetched) and texts made of its pieces: 64
queries x 32 candidates of 100 .. 300 tokens, the shape of profiles/cross_encoder_bench.json.  Two comparisons, the routes alternating
inside every round, the median over rounds reported with the smallest and the largest round next to it:
  encode      tokens/s of `DeviceWordPiece.encode_batch` over the call's distinct strings (the UTF-32 encode, the upload, the kernels
              and the copy of the results into torch tensors included; host clock around a call that ends synchronised) against
              `tokenizers.Tokenizer.encode_batch` of the same strings on the host's threads (RAYON_NUM_THREADS, 16 unless set)
  rank_batch  `TorchCrossEncoderRanker(forward="native").rank_batch` (12 x 384, bf16, random weights) with the device tokenizer
              against the same ranker given that tokenizer wrapped as `encode(str) -> list[int]`; the results are compared first
Needs a GPU: there is no fallback."""

from __future__ import annotations

import argparse
import copy
import json
import os
import statistics
import sys
import time
from pathlib import Path

os.environ.setdefault("RAYON_NUM_THREADS", "16")  # the CPUs a job gets; read by the `tokenizers` library's thread pool
os.environ.setdefault("TOKENIZERS_PARALLELISM", "true")

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

LETTERS = "abcdefghijklmnopqrstuvwxyz"
N_VOCAB = 30_522
QUERIES, CANDIDATES = 64, 32


def vocabulary(rng) -> dict:
    vocab: dict = {}
    for t in ["[PAD]", *[f"[unused{i}]" for i in range(99)], "[UNK]", "[CLS]", "[SEP]", "[MASK]"]:
        vocab[t] = len(vocab)
    for ch in LETTERS + "0123456789" + "!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~":
        vocab.setdefault(ch, len(vocab))
        vocab.setdefault("##" + ch, len(vocab))
    while len(vocab) < N_VOCAB:  # pieces of 2 .. 10 letters, a fifth of them continuations (as in bert-base-uncased)
        w = "".join(rng.choice(list(LETTERS), size=int(rng.integers(2, 11))))
        vocab.setdefault("##" + w if rng.integers(0, 5) == 0 else w, len(vocab))
    return vocab


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "wordpiece_bench.json"))
    ap.add_argument("--trace", action="store_true", help="three encode_batch calls and one rank_batch of 16 queries: the run a kernel trace is taken of")
    args = ap.parse_args()

    import numpy as np
    import torch

    import raglite_amd
    from raglite_amd._cross_encoder import CrossEncoderShape, TorchCrossEncoderRanker
    from raglite_amd._wordpiece import DeviceWordPiece, WordPieceTables, bert_tokenizer

    if not torch.cuda.is_available():
        raise SystemExit("bench_wordpiece.py measures on a GPU; none is visible")
    raglite_amd.set_device(0)
    rng = np.random.default_rng(0)
    vocab = vocabulary(rng)
    tok = bert_tokenizer(vocab)
    t0 = time.perf_counter()
    tables = WordPieceTables.from_tokenizer(tok)
    probe_s = time.perf_counter() - t0
    device_tok = DeviceWordPiece(tables)
    heads = [t for t in vocab if t[0] in LETTERS and len(t) > 1]
    conts = [t[2:] for t in vocab if t.startswith("##") and len(t) > 3]

    def text_of(n_tokens: int) -> str:
        """About n_tokens tokens: words of one head piece and 0 .. 2 continuations, some capitalised, a comma or a full stop now and then."""
        out, n = [], 0
        while n < n_tokens:
            k = int(rng.integers(0, 3))
            w = str(rng.choice(heads)) + "".join(str(rng.choice(conts)) for _ in range(k))
            n += 1 + k
            if rng.integers(0, 8) == 0:
                w = w.capitalize()
            if rng.integers(0, 10) == 0:
                w += ",."[int(rng.integers(0, 2))]
                n += 1
            out.append(w)
        return " ".join(out)

    def workload(n_queries: int):
        queries = [text_of(int(rng.integers(8, 24))) for _ in range(n_queries)]
        docs = [[text_of(int(rng.integers(100, 301))) for _ in range(CANDIDATES)] for _ in range(n_queries)]
        return queries, docs

    class Wrapped:
        def encode(self, text: str) -> list[int]:
            return tok.encode(text, add_special_tokens=False).ids

    shape = CrossEncoderShape(vocab_size=N_VOCAB, bos_id=vocab["[CLS]"], eos_id=vocab["[SEP]"])
    on_device = TorchCrossEncoderRanker(shape, tokenizer=device_tok, device="cuda", dtype=torch.bfloat16, forward="native")
    on_host = copy.copy(on_device)  # the same module and native handle behind the other tokenizer
    on_host.tokenizer = Wrapped()
    on_host._native = on_device._native_encoder()  # noqa: SLF001

    if args.trace:
        queries, docs = workload(16)
        strings = list(dict.fromkeys([*queries, *[d for ds in docs for d in ds]]))
        for _ in range(3):
            device_tok.encode_batch(strings)
        on_device.rank_batch(queries, docs)
        torch.cuda.synchronize()
        print(json.dumps({"trace": "3 encode_batch calls of 528 strings, 1 rank_batch of 16 queries x 32 candidates"}))
        return

    queries, docs = workload(QUERIES)
    strings = list(dict.fromkeys([*queries, *[d for ds in docs for d in ds]]))
    stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}  # noqa: E731

    # ---- the contract first: the same ids, the same results -----------------------------------------------------------------
    ids, offsets, counts = device_tok.encode_batch(strings)
    want = [e.ids for e in tok.encode_batch(strings, add_special_tokens=False)]
    off = offsets.cpu().tolist()
    flat = ids.cpu().tolist()
    same_ids = all(flat[off[i]: off[i + 1]] == w for i, w in enumerate(want))
    got, ref = on_device.rank_batch(queries, docs), on_host.rank_batch(queries, docs)
    same_rank = all([(x.doc_id, np.float32(x.score).tobytes()) for x in g.results] == [(x.doc_id, np.float32(x.score).tobytes()) for x in w.results]
                    for g, w in zip(got, ref))

    def device_encode():
        device_tok.encode_batch(strings)
        torch.cuda.synchronize()

    def host_encode():
        tok.encode_batch(strings, add_special_tokens=False)

    def wall(call) -> float:
        torch.cuda.synchronize()
        t = time.perf_counter()
        call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    for call in (device_encode, host_encode):
        call()
    enc = {"device": [], "host": []}
    rank = {"device_tokenizer": [], "host_tokenizer": []}
    for _ in range(args.rounds):
        enc["device"].append(wall(device_encode))
        enc["host"].append(wall(host_encode))
        rank["device_tokenizer"].append(wall(lambda: on_device.rank_batch(queries, docs)))
        rank["host_tokenizer"].append(wall(lambda: on_host.rank_batch(queries, docs)))
    n_tokens = counts["tokens"]
    result = {
        "vocabulary": f"synthetic, {len(vocab)} pieces; tables probed in {probe_s:.1f} s", "table": device_tok.info(),
        "host_threads": os.environ["RAYON_NUM_THREADS"], "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
        "strings": len(strings), "codepoints": sum(map(len, strings)), "tokens": n_tokens, "counts": counts,
        "ids_equal_the_library": same_ids, "rank_batch_equal_bits": same_rank,
        "encode": {"device_ms": stat(enc["device"]), "host_ms": stat(enc["host"]),
                   "device_tokens_per_s": n_tokens / statistics.median(enc["device"]) * 1e3,
                   "host_tokens_per_s": n_tokens / statistics.median(enc["host"]) * 1e3,
                   "device_over_host": statistics.median(enc["host"]) / statistics.median(enc["device"])},
        "rank_batch": {"shape": "12 x 384, 12 heads, ffn 1536, bf16, random weights; 64 queries x 32 candidates of 100 .. 300 tokens",
                       "pairs": QUERIES * CANDIDATES, "device_tokenizer_ms": stat(rank["device_tokenizer"]),
                       "host_tokenizer_ms": stat(rank["host_tokenizer"]),
                       "host_over_device": statistics.median(rank["host_tokenizer"]) / statistics.median(rank["device_tokenizer"])},
    }
    print(json.dumps(result["encode"]), json.dumps(result["rank_batch"]), same_ids, same_rank, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
