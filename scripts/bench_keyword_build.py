"""Building the BM25 postings: the host build against the device build (raglite_amd/csrc/keyword_build.hip), seeded.

    python scripts/bench_keyword_build.py [--chunks 1000000] [--terms 200000] [--mean-len 150] --out R.json
        the Zipf corpus of scripts/bench_keyword.py (tests/keyword_ref.zipf_corpus), in one run on one GPU:
          host         `_keyword.build_from_term_ids` + `KeywordIndex` (the upload and the impacts)
          device       everything appended to a `KeywordStore`, then `count` + `bm25_weights` + `build`: device events and wall clock,
                       after a first (cold) round; the arrays are compared with the host build's, impacts bit for bit
          incremental  1 000 more chunks appended to the store, then `count` + `build`, against the host rebuild it replaces
        The bar: the warm device rebuild takes at most a tenth of the host build's time.
    python scripts/bench_keyword_build.py --device-only ...
        skips the host builds (and the comparison): the form to run under `rocprofv3 --kernel-trace --stats`.
    python scripts/bench_keyword_build.py --trace-summary kernel_trace.csv --out R.json
        adds, per build kernel, the median time of a dispatch at full size and its share of the HBM bound: the bytes the kernel must
        move (8 B per token read and written per scatter, 4 B per token per histogram, ...) / 6.3 TB/s over its time.
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


def _timed(fn):
    """(result, device ms, wall ms) of fn() on the default stream."""
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def _rebuild(store, n_terms, rank):
    from raglite_amd import _keyword

    df, length, n_live, total_length, n_postings = store.count(n_terms, rank)
    idf, nrm, _ = _keyword.bm25_weights(df, length, n_live, total_length)
    return store.build(idf, nrm), n_postings


def run(args) -> dict:
    import torch

    import raglite_amd
    from raglite_amd import _keyword, _ops
    from tests import keyword_ref as ref

    assert torch.cuda.is_available(), "bench_keyword_build needs a GPU"
    raglite_amd.set_device(0)
    rng = np.random.default_rng(args.seed)
    flat, off = ref.zipf_corpus(rng, args.chunks, args.terms, args.mean_len)
    flat2, off2 = ref.zipf_corpus(rng, args.increment, args.terms, args.mean_len)
    rank = rng.permutation(args.terms).astype(np.int32)  # (ids are not ranks: the device applies the permutation)
    ids, ids2 = flat.astype(np.int32), flat2.astype(np.int32)
    rec = {"chunks": args.chunks, "terms": args.terms, "tokens": int(flat.size), "increment_chunks": args.increment}

    def host_build(f, o):
        t0 = time.perf_counter()
        p = _keyword.build_from_term_ids(rank[f], o, args.terms)
        t1 = time.perf_counter()
        kw = _ops.KeywordIndex(p)
        return p, kw, t1 - t0, time.perf_counter() - t1

    host = None
    if not args.device_only:
        p, host, build_s, create_s = host_build(flat, off)
        rec.update(postings=int(p.post_chunk.size), host_build_s=round(build_s, 3), host_index_create_s=round(create_s, 3),
                   host_total_s=round(build_s + create_s, 3))
        del p
    store = _ops.KeywordStore()
    _, _, wall = _timed(lambda: store.append(ids, off))
    rec["device_append_all_ms"] = round(wall, 1)
    (kw, n_postings), dev_ms, wall = _timed(lambda: _rebuild(store, args.terms, rank))
    rec.update(postings=n_postings, device_cold_ms=round(dev_ms, 2), device_cold_wall_ms=round(wall, 2))
    if host is not None:
        same = all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(kw.read(), host.read()))
        rec["equal_to_host_build_bitwise"] = bool(same)
        assert same, "the device build differs from the host build"
        host.close()
    warm = []
    for _ in range(args.iters):
        kw.close()
        (kw, _), dev_ms, wall = _timed(lambda: _rebuild(store, args.terms, rank))
        warm.append((dev_ms, wall))
    rec["device_rebuild_ms"] = round(float(np.median([w[0] for w in warm])), 2)
    rec["device_rebuild_wall_ms"] = round(float(np.median([w[1] for w in warm])), 2)
    rec["store_info"] = store.info()
    # the incremental case: 1 000 chunks more
    _, _, wall = _timed(lambda: store.append(ids2, off2))
    rec["increment_append_ms"] = round(wall, 2)
    kw.close()
    (kw, n_postings), dev_ms, wall = _timed(lambda: _rebuild(store, args.terms, rank))
    rec.update(increment_postings=n_postings, increment_rebuild_ms=round(dev_ms, 2), increment_rebuild_wall_ms=round(wall, 2))
    if not args.device_only:
        p, host, build_s, create_s = host_build(np.concatenate((flat, flat2)), np.concatenate((off, off[-1] + off2[1:])))
        same = all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(kw.read(), host.read()))
        rec.update(increment_host_total_s=round(build_s + create_s, 3), increment_equal_to_host_build_bitwise=bool(same))
        host.close()
        rec["host_over_device"] = round(rec["host_total_s"] * 1e3 / rec["device_rebuild_wall_ms"], 1)
        rec["increment_host_over_device"] = round(rec["increment_host_total_s"] * 1e3 / (rec["increment_append_ms"] + rec["increment_rebuild_wall_ms"]), 1)
        rec["speed_bar_met"] = bool(rec["device_rebuild_wall_ms"] * 10 <= rec["host_total_s"] * 1e3)
        assert same, "the incremental device build differs from the host build"
    kw.close()
    store.close()
    return rec


def trace_summary(path: str, rec: dict) -> dict:
    """Per build kernel: the median time of its LARGEST dispatches (the full-size ones: the scan kernels also run on small tables) from a
    rocprofv3 kernel_trace.csv, the bytes such a dispatch must move, and bytes / 6.3 TB/s over that time."""
    m, n_post, terms = rec["tokens"], rec["postings"], rec["terms"]
    table = 256 * ((m + 4095) // 4096) * 8
    must_move = {
        "kb_emit_kernel": 4 * m + 8 * m,                 # the ids read, (key, value) written
        "kb_hist_kernel": 4 * m + table,                 # the keys read, the (digit, block) table written
        "kb_scan_tile_kernel": 2 * table,                # the table read and written
        "kb_add_base_kernel": 2 * table,
        "kb_scatter_kernel": 8 * m + 8 * m + table,      # 8 B per token read and written
        "kb_rle_count_kernel": 8 * m,
        "kb_rle_write_kernel": 8 * m + 16 * n_post,      # post_term, post_chunk and the 8-byte head position written
        "kb_tf_kernel": 12 * n_post,
        "kb_term_off_kernel": 8 * (terms + 1),           # (plus its binary-search reads)
        "bm25_impact_kernel": 16 * n_post,
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
        t = [ms for g, ms in rows if g == top]
        kms = float(np.median(t))
        out[name] = {"dispatches_at_full_size": len(t), "dispatches": len(rows), "median_ms": round(kms, 4), "total_ms": round(sum(ms for _, ms in rows), 3),
                     "must_move_bytes": must_move[name], "hbm_bound_ms": round(must_move[name] / HBM_BYTES_PER_S * 1e3, 4),
                     "hbm_fraction": round(must_move[name] / HBM_BYTES_PER_S * 1e3 / kms, 3)}
    rec["kernels"] = out
    return rec


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=1_000_000)
    ap.add_argument("--terms", type=int, default=200_000)
    ap.add_argument("--mean-len", type=int, default=150)
    ap.add_argument("--increment", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=3)
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
