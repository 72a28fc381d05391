"""Analyzing chunk bodies for BM25: the host analyzer against the device analyzer (raglite_amd/csrc/keyword_analyze.hip; DESIGN.md
4.18), seeded.

    python scripts/bench_keyword_analyze.py [--chunks 100000] [--mean-len 150] --out R.json
        a corpus of `--chunks` bodies of about `--mean-len` index stems each: words drawn by a Zipf law from ~51 k (head + real
        suffix) words and the stopword list, about 1 % of the code points outside ASCII.  In one run on one GPU:
          host         `_keyword.index_stems` + `stems_to_store_ids` on the first `--host-chunks` bodies, cold (an empty stem cache)
                       and warm (every stem cached), SCALED to the corpus by the chunk count and labelled so
          device       `analyze_texts_batch` over the whole corpus after a warm-up call, split into the host's UTF-32 encode, the two
                       device steps, the host's vocabulary step and the read-back; its ids are compared with the host's on the
                       bodies the host analyzed
          incremental  `--increment` more bodies analyzed and appended device to device onto the loaded `KeywordStore`, then the
                       rebuild of the postings
    python scripts/bench_keyword_analyze.py --device-only ...
        skips the host analyzer (and the comparison): the form to run under `rocprofv3 --kernel-trace --stats`.
    python scripts/bench_keyword_analyze.py --trace-summary kernel_trace.csv --out R.json
        adds, per kernel, the median time of its largest dispatches and their share of the HBM bound: the bytes such a dispatch reads
        and writes (from the sizes of the largest call, below) / 6.3 TB/s over its time.
"""

from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

HBM_BYTES_PER_S = 6.3e12  # achievable HBM3E rate of an MI355X (float4 copy)
SUFFIXES = ["", "s", "es", "ed", "ing", "er", "ers", "ly", "ness", "ful", "ment", "ments", "ation", "ations", "ational", "ize", "izes",
            "ized", "izing", "ization", "ity", "ities", "ive", "iveness", "able", "ible", "al", "ally", "ism", "ist", "ous", "ously", "ance",
            "ence", "ant", "ent", "ate", "ated", "ating", "ator", "ical"]
NON_ASCII = ["café", "naïve", "über", "Ⅷ", "ﬁnal", "résumé", "Ångström", "ßtraße", "mañana", "–", "“quoted”", "Ελληνικά", "日本語", "смысл"]


def make_corpus(rng, n_chunks: int, mean_len: int) -> list[str]:
    from raglite_amd import _keyword

    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype="S1")
    heads = ["".join(rng.choice(letters, size=int(rng.integers(3, 8))).astype(str)) for _ in range(1250)]
    words = [h + s for h in heads for s in SUFFIXES]  # 51 250
    order = rng.permutation(len(words))
    words = [words[i] for i in order]
    stop = sorted(_keyword.STOPWORDS)
    p = 1.0 / np.arange(1, len(words) + 1)
    p /= p.sum()
    # per token: 60 % a Zipf word, 36 % a stopword (they are dropped: 1.6 tokens per index stem), 4 % a word outside ASCII
    n_tokens = int(n_chunks * mean_len * 1.6)
    kind = rng.random(n_tokens)
    picks = rng.choice(len(words), size=n_tokens, p=p)
    stops = rng.integers(0, len(stop), size=n_tokens)
    other = rng.integers(0, len(NON_ASCII), size=n_tokens)
    tokens = [words[w] if k < 0.6 else (stop[s] if k < 0.96 else NON_ASCII[o]) for k, w, s, o in zip(kind.tolist(), picks.tolist(), stops.tolist(), other.tolist())]
    sizes = rng.poisson(mean_len * 1.6, size=n_chunks)
    bounds = np.minimum(np.concatenate(([0], np.cumsum(sizes))), n_tokens).tolist()
    return [" ".join(tokens[bounds[i] : bounds[i + 1]]) for i in range(n_chunks)]


def run(args) -> dict:
    import torch

    import raglite_amd
    from raglite_amd import _keyword, _ops

    assert torch.cuda.is_available(), "bench_keyword_analyze needs a GPU"
    raglite_amd.set_device(0)
    rng = np.random.default_rng(args.seed)
    t0 = time.perf_counter()
    texts = make_corpus(rng, args.chunks + args.increment, args.mean_len)
    texts, more = texts[: args.chunks], texts[args.chunks :]
    n_chars = sum(map(len, texts))
    rec = {"chunks": args.chunks, "increment_chunks": args.increment, "code_points": n_chars,
           "non_ascii_fraction": round(sum(sum(ord(c) > 127 for c in t) for t in texts[:2000]) / max(1, sum(map(len, texts[:2000]))), 4),
           "corpus_s": round(time.perf_counter() - t0, 1), "max_chars_per_call": args.max_chars}

    host = None
    if not args.device_only:
        part = texts[: args.host_chunks]
        timings = []
        for label in ("cold", "warm"):
            if label == "cold":
                _keyword.stem.cache_clear()
            vocab = _keyword.Vocabulary()
            t0 = time.perf_counter()
            host = _keyword.stems_to_store_ids([_keyword.index_stems(t) for t in part], vocab)
            timings.append(time.perf_counter() - t0)
        host = (*host, vocab.stems)
        scale = args.chunks / len(part)
        rec.update(host_chunks=len(part), host_tokens=int(host[0].size), host_cold_s=round(timings[0], 3), host_warm_s=round(timings[1], 3),
                   host_cold_us_per_token=round(timings[0] / host[0].size * 1e6, 2), host_warm_us_per_token=round(timings[1] / host[0].size * 1e6, 2),
                   host_cold_scaled_to_corpus_s=round(timings[0] * scale, 1), host_warm_scaled_to_corpus_s=round(timings[1] * scale, 1))

    t0 = time.perf_counter()
    table = _keyword.fold_table()
    rec["fold_table_s"] = round(time.perf_counter() - t0, 2)
    t0 = time.perf_counter()
    analyzer = _ops.KeywordAnalyzer(table, sorted(_keyword.STOPWORDS))
    rec["analyzer_create_s"] = round(time.perf_counter() - t0, 3)
    raglite_amd.analyze_texts_batch(texts[:1000], _keyword.Vocabulary(), analyzer=analyzer)  # warm-up: code objects, first allocations

    rounds = []
    for _ in range(args.iters):
        vocab, timings = _keyword.Vocabulary(), {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        flat, off = raglite_amd.analyze_texts_batch(texts, vocab, analyzer=analyzer, max_chars_per_call=args.max_chars, timings=timings)
        timings["total"] = time.perf_counter() - t0  # (every device step returns synchronised)
        rounds.append(timings)
    best = min(rounds, key=lambda r: r["total"])
    rec["calls"] = best.pop("calls")
    rec["device"] = {k + "_s": round(v, 4) for k, v in best.items()}
    rec["device_rounds_total_s"] = [round(r["total"], 4) for r in rounds]
    rec.update(tokens=int(flat.size), vocabulary=len(vocab))
    rec["device_us_per_token"] = round(best["total"] / flat.size * 1e6, 4)
    if host is not None:
        n_host = int(host[1][-1])
        same = (np.array_equal(flat[:n_host], host[0]) and np.array_equal(off[: len(host[1])], host[1]) and vocab.stems[: len(host[3])] == host[3])
        rec["equal_to_host_on_host_chunks"] = bool(same)
        assert same, "the device analyzer differs from the host analyzer"
        rec["host_cold_scaled_over_device"] = round(rec["host_cold_scaled_to_corpus_s"] / best["total"], 1)
        rec["host_warm_scaled_over_device"] = round(rec["host_warm_scaled_to_corpus_s"] / best["total"], 1)

    # the incremental case: `increment` bodies onto the loaded store
    store = _ops.KeywordStore()
    store.append(flat, off)
    ranks = vocab.ranks()
    df, length, n_live, total_length, _ = store.count(len(vocab), ranks)
    store.build(*_keyword.bm25_weights(df, length, n_live, total_length)[:2]).close()
    timings = {}
    t0 = time.perf_counter()
    for result in _keyword.analyze_texts_device(more, vocab, analyzer=analyzer, timings=timings):
        store.append(result)
    t1 = time.perf_counter()
    ranks = vocab.ranks()
    df, length, n_live, total_length, _ = store.count(len(vocab), ranks)
    kw = store.build(*_keyword.bm25_weights(df, length, n_live, total_length)[:2])
    t2 = time.perf_counter()
    rec["increment"] = {"analyze_and_append_ms": round((t1 - t0) * 1e3, 2), "rebuild_ms": round((t2 - t1) * 1e3, 2),
                        **{k + "_ms": round(v * 1e3, 2) for k, v in timings.items() if k != "calls"}, "sizes": analyzer.last_sizes}
    if not args.device_only:
        t0 = time.perf_counter()
        _keyword.stems_to_store_ids([_keyword.index_stems(t) for t in more], _keyword.Vocabulary())
        rec["increment"]["host_warm_analyze_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    kw.close()
    store.close()
    analyzer.close()
    return rec


def trace_summary(path: str, rec: dict) -> dict:
    """Per kernel: the median time of its LARGEST dispatches from a rocprofv3 kernel_trace.csv, the bytes such a dispatch reads and
    writes -- counted from the sizes of the largest call: n code points, m folded symbols, T tokens, K kept ones -- and bytes / 6.3 TB/s
    over that time.  The table gathers (4 B per code point, mostly from cache) and the byte compares of the distinct pass are not counted."""
    big = max(rec["calls"], key=lambda c: c["code_points"])
    n, m, T, K = big["code_points"], big["symbols"], big["all_tokens"], big["tokens"]
    cap = 1 << int(np.ceil(np.log2(max(2 * T, 64))))
    must_move = {
        "ka_fold_count_kernel": 4 * n + 8 * n,
        "kb_scan_tile_kernel": 16 * max(n, m),
        "kb_add_base_kernel": 16 * max(n, m),
        "ka_fold_write_kernel": 4 * n + 8 * n + m,
        "ka_letters_kernel": 3 * m,
        "ka_heads_kernel": 2 * m + 8 * m,
        "ka_token_pos_kernel": 2 * m + 16 * T,
        "ka_stem_kernel": 4 * m + 24 * T,
        "ka_distinct_kernel": 32 * T + 8 * cap,
        "ka_flags_kernel": 32 * T + 8 * K,
        "ka_distinct_out_kernel": 16 * T,
        "ka_emit_kernel": 16 * T + 20 * K,
    }
    times: dict[str, list[tuple[int, float]]] = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for name in must_move:
                if name in row["Kernel_Name"]:
                    times.setdefault(name, []).append((int(row["Grid_Size_X"]) if "Grid_Size_X" in row else int(row["Grid_Size"]),
                                                       (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6))
    out = {}
    for name, rows in times.items():
        top = max(g for g, _ in rows)
        t = [ms for g, ms in rows if g >= 0.9 * top]
        kms = float(np.median(t))
        out[name] = {"dispatches_at_full_size": len(t), "dispatches": len(rows), "median_ms": round(kms, 4), "total_ms": round(sum(ms for _, ms in rows), 3),
                     "must_move_bytes": must_move[name], "hbm_bound_ms": round(must_move[name] / HBM_BYTES_PER_S * 1e3, 4),
                     "hbm_fraction": round(must_move[name] / HBM_BYTES_PER_S * 1e3 / kms, 3)}
    rec["kernels"] = out
    rec["kernels_sized_for"] = {**big, "slots": cap}
    return rec


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=100_000)
    ap.add_argument("--mean-len", type=int, default=150)
    ap.add_argument("--host-chunks", type=int, default=5000)
    ap.add_argument("--increment", type=int, default=1000)
    ap.add_argument("--max-chars", type=int, default=1 << 24)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device-only", action="store_true")
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
