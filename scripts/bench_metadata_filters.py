"""Metadata filters evaluated on the device: the workload of scripts/bench_query_filters.py (§4.9) -- one row per
chunk, 256 Zipf-sized tenants, B queries with F distinct tenant filters, query b's filter tenant b mod F -- with the evaluation inside
the timed window.

    python scripts/bench_metadata_filters.py [--chunks 1000000] [--dim 1024] [--batch 256] [--filters 1,16,256] --out R.json
        Per F, after warm-up:
          kernel_ms          rl_metadata_filters alone, device events around `MetadataStore.filters` (F filters in, 16 F bytes out), and
                             its fraction of the HBM bound: the tag CSR read once plus F x chunks / 8 bytes written
          per_query_*_ms     rl_hybrid_search_per_query alone with the F bitsets as a host table (checked, packed and staged by the
                             call, as §4.9 measured it) against the device table under RL_MEM_FILTERS_DEVICE; wall clock, same bits
          public_*_ms        the public hybrid_search_batch, planning included, wall clock, over two indexes of the same data:
                             metadata_filters="host" (a Python loop over one dict per chunk per distinct filter; --host-iters runs, 0
                             skips it) and "device"; same results
        Writes one JSON record.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np


def wall_ms(fn, warmup: int, iters: int):
    import torch

    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3 / iters


def run(args) -> dict:
    import torch

    import raglite_amd
    from raglite_amd import _metadata, _ops, _search
    from bench_hybrid import build_index, timed
    from bench_query_filters import tenants
    from tests import keyword_ref as ref

    assert torch.cuda.is_available(), "bench_metadata_filters needs a GPU"
    raglite_amd.set_device(0)
    t0 = time.perf_counter()
    gi, p, terms_of, rng = build_index(args)  # (no metadata: the "host" index of this run; the "device" one shares its device arrays)
    tenant = tenants(rng, args.chunks)
    gi.metadata = [{"tenant": f"t{t}"} for t in tenant]
    te = time.perf_counter()
    vocab = _metadata.TagVocabulary()
    tag_off, tags = vocab.encode_chunks(gi.metadata)
    encode_s = time.perf_counter() - te
    te = time.perf_counter()
    store = _ops.MetadataStore(tag_off, tags)
    upload_s = time.perf_counter() - te
    dev = raglite_amd.GpuIndex.__new__(raglite_amd.GpuIndex)  # the same index with its metadata on the device
    dev.__dict__.update(gi.__dict__)
    dev.metadata_filters, dev._meta_vocab, dev._meta_store = "device", vocab, store  # noqa: SLF001
    gi.metadata_filters = "host"
    cfg = raglite_amd.HotPathConfig(vector_search_query_adapter=False)
    n_each = args.oversample * args.num_results
    num_hits = round(_search.VECTOR_SEARCH_OVERSAMPLE * cfg.chunk_max_size / _search.DEFAULT_CHUNK_MAX_SIZE) * max(n_each, 10)
    k = args.num_results
    B = args.batch
    rec = {"chunks": args.chunks, "dim": args.dim, "B": B, "tags": int(tags.size), "distinct_tags": len(vocab),
           "encode_chunks_s": round(encode_s, 2), "store_upload_s": round(upload_s, 3), "store_bytes": store.memory()[0],
           "setup_s": round(time.perf_counter() - t0, 1), "runs": []}
    queries = [f"q{b}" for b in range(B)]
    for q, t in zip(queries, ref.zipf_queries(rng, B, args.terms, lo=4, hi=12)):
        terms_of[q] = sorted(set(int(x) for x in t))
    terms = [terms_of[q] for q in queries]
    Q = (rng.random((B, args.dim), dtype=np.float32) - 0.5).astype(np.float32)
    kw = dict(keyword=gi.keyword, weights=(0.75, 0.25), rrf_k=60)
    fs = None
    for F in args.filters:
        tq = [b % F for b in range(B)]
        filters = [{"tenant": [f"t{t}"]} for t in range(F)]
        f_off, f_tags = vocab.encode_filters(filters)

        def kernel():
            nonlocal fs
            fs, n, r = store.filters(gi.index, f_off, f_tags, filter_set=fs)
            return n, r

        (n_chunks, n_rows), kernel_ms, kernel_wall = timed(kernel, args.warmup, args.iters)
        assert n_chunks.tolist() == np.bincount(tenant, minlength=256)[:F].tolist() and np.array_equal(n_chunks, n_rows)
        hbm_bytes = 8 * (args.chunks + 1) + 4 * int(tags.size) + F * ((args.chunks + 31) // 32) * 4
        row = {"F": F, "kernel_ms": round(kernel_ms, 4), "kernel_wall_ms": round(kernel_wall, 4),
               "hbm_bound_fraction": round(hbm_bytes / args.hbm_gbs / 1e6 / kernel_ms, 4)}
        limits = [_search.ORDER_FIRST_LIMIT if int(n_rows[t]) > _search.FILTER_FIRST_MAX_ROWS else 0 for t in tq]
        table = fs.read()
        host_filters = [table[t] for t in tq]
        device_filters = fs.select(tq)
        outs = {}
        for name, qf in (("host_table", host_filters), ("device_table", device_filters)):
            outs[name], row[f"per_query_{name}_ms"] = wall_ms(
                lambda: gi.index.hybrid_search(Q, num_hits, n_each, k, query_term_ids=terms, query_filters=qf, rank_limit=limits, **kw),
                args.warmup, args.iters)
            row[f"per_query_{name}_ms"] = round(row[f"per_query_{name}_ms"], 3)
        row["per_query_equal"] = all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(outs["host_table"], outs["device_table"]))
        public = dict(num_results=args.num_results, oversample=args.oversample, config=cfg, query_vectors=Q,
                      metadata_filter=[{"tenant": f"t{t}"} for t in tq])
        got, row["public_device_ms"] = wall_ms(lambda: raglite_amd.hybrid_search_batch(queries, index=dev, **public), args.warmup, args.iters)
        row["public_device_ms"] = round(row["public_device_ms"], 3)
        if args.host_iters:
            want, row["public_host_ms"] = wall_ms(lambda: raglite_amd.hybrid_search_batch(queries, index=gi, **public), 0, args.host_iters)
            row["public_host_ms"] = round(row["public_host_ms"], 1)
            row["public_equal"] = got == want
        rec["runs"].append(row)
        print(json.dumps(row), flush=True)
        assert row["per_query_equal"] and row.get("public_equal", True), f"the paths differ at F = {F}"
    store.close()
    gi.close()
    return rec


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--terms", type=int, default=200_000)
    ap.add_argument("--mean-len", type=int, default=150)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--filters", type=lambda s: [int(x) for x in s.split(",")], default=[1, 16, 256])
    ap.add_argument("--num-results", type=int, default=8)
    ap.add_argument("--oversample", type=int, default=4)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-iters", type=int, default=1)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)  # the MI355X's peak HBM bandwidth, for the bound
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rec = run(args)
    text = json.dumps(rec, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
