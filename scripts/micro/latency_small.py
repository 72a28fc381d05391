"""Latency of a single-query search on small indexes (the reference's typical database sizes); at 10 k rows also of the two calls that
drive the index and a keyword index from api_retrieval.hip: hybrid_search with host arguments, search_rerank with device arguments."""
import sys, time, json
import numpy as np, torch
sys.path.insert(0, ".")
import raglite_amd
from raglite_amd import _keyword
raglite_amd.set_device(0)
out = {}
def timed(name, fn):
    for _ in range(5): fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(200): fn()
    torch.cuda.synchronize(); out[name] = round((time.perf_counter() - t0) / 200 * 1e6, 1)
for n in (10_000, 100_000, 1_000_000):
    d = 1024
    E = torch.empty((n, d), dtype=torch.float32, device="cuda"); raglite_amd.synth_fill(E, seed=1)
    off = np.arange(0, n + 1, 5, dtype=np.int64)
    idx = raglite_amd.DeviceIndex(E, off, metric="cosine")
    q = torch.empty((d,), dtype=torch.float32, device="cuda"); raglite_amd.synth_fill(q, seed=2)
    qh = q.cpu().numpy()
    for name, fn in (("search_rows_dev", lambda: idx.search_rows(q, 10)), ("search_chunks_dev", lambda: idx.search_chunks(q, 40, 10)),
                     ("search_chunks_host_args", lambda: idx.search_chunks(qh, 40, 10))):
        timed(f"{name}_n{n}_us", fn)
    if n == 10_000:
        n_chunks, n_terms, per_chunk = off.size - 1, 5000, 40
        rng = np.random.default_rng(3)
        kw = raglite_amd.KeywordIndex(_keyword.build_from_term_ids(rng.integers(0, n_terms, n_chunks * per_chunk),
                                                                   np.arange(0, n_chunks * per_chunk + 1, per_chunk), n_terms))
        terms = [rng.integers(0, n_terms, 5).tolist()]
        qv = torch.empty((1, 8, d), dtype=torch.float32, device="cuda"); raglite_amd.synth_fill(qv, seed=4)  # nq = 8 vectors per query
        timed(f"hybrid_search_host_args_n{n}_us", lambda: idx.hybrid_search(qh[None], 40, 10, 10, keyword=kw, query_term_ids=terms))
        timed(f"search_rerank_dev_n{n}_us", lambda: idx.search_rerank(q[None], 40, 32, 32, qv, 10, keyword=kw, query_term_ids=terms))
        kw.close()
    idx.close(); del E
print(json.dumps(out))
