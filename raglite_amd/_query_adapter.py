"""Host mirror of `src/raglite/_query_adapter.py` with the searches batched on the GPU.

    update_query_adapter(evals, *, max_evals=4096, optimize_top_k=40, optimize_gap=0.05, config=None, index=None)
        -> (d, d) float64 adapter, also installed as `index.query_adapter`              (`_query_adapter.py:41-219`)

The reference loops over the evals: embed the question, run one vector search WITHOUT the adapter, pick the best row
of every retrieved chunk as positive / negative example, solve a small NNLS for the target vector, and finally fit
the adapter in closed form.  Here every eval's search goes through ONE `rl_search_chunks` call (the B = hundreds-to-
thousands batched shape of BASELINE cfg 5, i.e. the fp32 MFMA GEMM path), the best rows through ONE
`rl_chunk_best_rows`, the example rows come back through ONE `rl_gather_rows`; the NNLS (`scipy.optimize.lsq_linear`)
and the Procrustes / pseudo-inverse algebra stay on the host in fp64 exactly as written in the reference.  Evals come
from the store in the reference (`select(Eval)`, `:150`); here they are passed in.

`targets="device"` replaces the per-eval host NNLS by ONE `rl_query_targets` call: the exact target of every eval from
the Gram matrix of its example rows, read in place from the index (no `rl_gather_rows`); DESIGN.md section 4.15.
`optimize_query_target_active_set` is the host statement of that solver, `optimize_query_targets` the batched call.
"""

from __future__ import annotations

from dataclasses import replace
from typing import Any, Sequence

import numpy as np

from raglite_amd import _ops
from raglite_amd._config import DEFAULT_CHUNK_MAX_SIZE, HotPathConfig
from raglite_amd._embed import embed_strings, embedding_type
from raglite_amd._search import GpuIndex, _index_for


def _optimize_query_target(q: np.ndarray, P: np.ndarray, N: np.ndarray, *, alpha: float = 0.05) -> np.ndarray:  # noqa: N803
    """`_query_adapter.py:20-38`: t* = q + Dᵀ μ*, μ* = argmin ½‖q + Dᵀ μ‖² s.t. μ ≥ 0, D = P_i − (1 + α) N_j."""
    from scipy.optimize import lsq_linear

    q_dtype = q.dtype
    q, P, N = q.astype(np.float64), P.astype(np.float64), N.astype(np.float64)  # noqa: N806
    D = np.reshape(P[:, np.newaxis, :] - (1.0 + alpha) * N[np.newaxis, :, :], (-1, P.shape[1]))  # noqa: N806
    mu = lsq_linear(D.T, -q, bounds=(0.0, np.inf), tol=np.finfo(np.float64).eps).x
    return (q + D.T @ mu).astype(q_dtype)


QT_MAX_EXAMPLES = 64  # RL_QT_MAX_EXAMPLES
QT_STATUS = {1: "no positive or no negative example", 2: "a non-finite example row or query (or a row ordinal outside the index)",
             3: "zero target: the constraints cannot be met", 4: "the entering-step cap was reached"}


def _active_set_from_gram(K: np.ndarray, e: np.ndarray, p: int, n: int, c: float) -> tuple[np.ndarray, int, int]:  # noqa: N803
    """Lawson-Hanson on min ½ μᵀGμ + hᵀμ, μ ≥ 0, with G and h read off the Gram matrix K = E Eᵀ and e = E q of the examples
    (positives first): pair (i, j) -> i·n + j, G[(i,j),(i',j')] = K[i,i'] − c (K[i,j'] + K[j,i']) + c² K[j,j'], h[(i,j)] = e[i] − c e[j].
    Returns (μ by pair, status 0 / 4, entering steps).  `query_targets.hip: qt_solve_kernel` runs the same iteration."""
    k, m = p + n, p * n
    pi, nj = np.repeat(np.arange(p), n), p + np.tile(np.arange(n), p)  # the two examples of every pair
    h = e[pi] - c * e[nj]
    g_diag = K[pi, pi] - c * (K[pi, nj] + K[nj, pi]) + c * c * K[nj, nj]
    tol = 64.0 * np.finfo(np.float64).eps * max(float(np.max(np.abs(h))), float(np.max(np.abs(K))))

    def g_col(a: int, idx: list[int]) -> np.ndarray:
        return K[pi[idx], pi[a]] - c * (K[pi[idx], nj[a]] + K[nj[idx], pi[a]]) + c * c * K[nj[idx], nj[a]]

    L = np.zeros((k, k))  # noqa: N806  Cholesky factor of G over the passive list, in list order
    passive: list[int] = []
    mu = np.zeros(0)  # by passive slot
    state = np.zeros(m, np.int8)  # 0 free, 1 passive, 2 banned

    def append_row(a: int) -> bool:
        """Factor row of pair a behind the passive list; False (nothing changed) when its squared pivot is too small."""
        s = len(passive)
        if s >= k:
            return False
        col, y = g_col(a, passive), np.zeros(s)
        for r in range(s):
            y[r] = (col[r] - L[r, :r] @ y[:r]) / L[r, r]
        d = g_diag[a] - y @ y
        if not d > 1e-12 * g_diag[a]:
            return False
        L[s, :s], L[s, s] = y, np.sqrt(d)
        passive.append(a)
        return True

    def solve() -> np.ndarray:
        s = len(passive)
        z = -h[passive]
        for r in range(s):
            z[r] = (z[r] - L[r, :r] @ z[:r]) / L[r, r]
        for r in range(s - 1, -1, -1):
            z[r] = (z[r] - L[r + 1 : s, r] @ z[r + 1 : s]) / L[r, r]
        return z

    status, iterations = 0, 0
    while True:
        w = np.zeros(k)  # the marginals: w_i = Σ_j μ_ij, w_j = −c Σ_i μ_ij
        for slot, a in enumerate(passive):
            w[pi[a]] += mu[slot]
            w[nj[a]] -= c * mu[slot]
        u = e + K @ w
        score = np.where(state == 0, -(u[pi] - c * u[nj]), -np.inf)
        cand = int(np.argmax(score))  # the first maximum
        if not score[cand] > tol:
            break
        if iterations >= 4 * k:
            status = 4
            break
        iterations += 1
        if not append_row(cand):
            state[cand] = 2
            continue
        z = solve()
        if not z[-1] > 0.0:  # a dependent column met from the other side
            passive.pop()
            state[cand] = 2
            continue
        state[state == 2] = 0
        state[cand] = 1
        mu = np.append(mu, 0.0)
        while np.any(z <= 0.0):
            neg = z <= 0.0
            ratio = np.where(neg, mu / np.where(neg, mu - z, 1.0), np.inf)
            step = float(np.min(ratio))
            mu = mu + step * (z - mu)
            drop = (neg & (ratio == step)) | (mu <= 0.0)
            kept = [a for a, d in zip(passive, drop) if not d]
            state[[a for a, d in zip(passive, drop) if d]] = 0
            mu = mu[~drop]
            passive.clear()
            for a in kept:  # a subset of a passive list keeps its pivots (they only grow)
                col, s = g_col(a, passive), len(passive)
                for r in range(s):
                    L[s, r] = (col[r] - L[r, :r] @ L[s, :r]) / L[r, r]
                L[s, s] = np.sqrt(max(g_diag[a] - L[s, :s] @ L[s, :s], 1e-12 * g_diag[a]))
                passive.append(a)
            z = solve()
        mu = z
    out = np.zeros(m)
    out[passive] = mu
    return out, status, iterations


def optimize_query_target_active_set(q: np.ndarray, P: np.ndarray, N: np.ndarray, *,  # noqa: N803
                                     alpha: float = 0.05) -> tuple[np.ndarray, np.ndarray, float, int, int]:
    """The exact target of `_query_adapter.py:20-38`: t* = argmin ‖q + Dᵀμ‖² over μ ≥ 0 is the projection of the origin onto
    q + cone(D), D = P_i − (1 + α) N_j, solved by an active-set iteration on the Gram matrix of the examples;
    D is never formed.  Returns (t float64[dim], weights float64[p + n] -- the non-negative marginals a_i = Σ_j μ_ij, b_j = Σ_i μ_ij,
    t = q + Σ a_i P_i − (1 + α) Σ b_j N_j --, objective ‖t‖², status, entering steps).  Status: 0 ok, 1 no positive or no negative,
    2 a non-finite input, 3 zero target (‖t‖ ≤ 1e-9 ‖q‖: the constraints cannot be met), 4 entering-step cap (4 (p + n)) reached."""
    q = np.ravel(np.asarray(q)).astype(np.float64)
    P = np.asarray(P).astype(np.float64).reshape(-1, q.size)  # noqa: N806
    N = np.asarray(N).astype(np.float64).reshape(-1, q.size)  # noqa: N806
    p, n = len(P), len(N)
    if p == 0 or n == 0:
        return np.full(q.size, np.nan), np.zeros(p + n), float("nan"), 1, 0
    if not (np.all(np.isfinite(q)) and np.all(np.isfinite(P)) and np.all(np.isfinite(N))):
        return np.full(q.size, np.nan), np.zeros(p + n), float("nan"), 2, 0
    c = 1.0 + float(alpha)
    E = np.vstack([P, N])  # noqa: N806
    mu, status, iterations = _active_set_from_gram(E @ E.T, E @ q, p, n, c)
    mu = mu.reshape(p, n)
    weights = np.concatenate([mu.sum(axis=1), mu.sum(axis=0)])
    t = q + weights[:p] @ P - c * (weights[p:] @ N)
    objective = float(t @ t)
    if objective <= 1e-18 * float(q @ q):
        status = 3
    return t, weights, objective, status, iterations


def optimize_query_targets(Q: Any, rows: Any, relevant: Any, *, gap: float = 0.05, index: Any) -> tuple[Any, Any, Any, Any, Any]:  # noqa: N803
    """The exact targets of many evals in one `rl_query_targets` call.  Q (B, dim) queries, rows (B, n_examples) int32 row ordinals
    of the index (-1 = no example in this slot), relevant (B, n_examples) true = positive example; `index` a `GpuIndex` or a
    `DeviceIndex` -> (T float64 (B, dim), weights float64 (B, n_examples), objective (B,), status int32 (B,), iterations int32 (B,)),
    NumPy for NumPy inputs and CUDA tensors for CUDA inputs.  Status as `optimize_query_target_active_set`; a failed eval (NaN target
    for 1 and 2) leaves its neighbours alone."""
    return getattr(index, "index", index).query_targets(Q, rows, relevant, gap)


def _adapter_from_targets(Q: np.ndarray, T: np.ndarray, metric: str) -> np.ndarray:  # noqa: N803
    """`_query_adapter.py:182-208`."""
    Q = Q / np.linalg.norm(Q, axis=1, keepdims=True)  # noqa: N806
    if metric == "cosine":
        T = T / np.linalg.norm(T, axis=1, keepdims=True)  # noqa: N806
    n, d = Q.shape
    M = (1 / n) * T.T @ Q  # noqa: N806
    if n < d or np.linalg.matrix_rank(Q) < d:
        M += np.eye(d) - Q.T @ np.linalg.pinv(Q @ Q.T) @ Q  # noqa: N806
    if metric == "dot":
        return M / np.linalg.norm(M, ord="fro") * np.sqrt(d)
    if metric == "cosine":
        U, _, VT = np.linalg.svd(M, full_matrices=False)  # noqa: N806
        return U @ VT
    raise ValueError(f"Unsupported metric: {metric}")


def _eval_fields(ev: Any) -> tuple[Any, Sequence[str]]:
    if isinstance(ev, (tuple, list)):
        return ev[0], ev[1]
    return ev.question, ev.chunk_ids  # the reference's `Eval` row (`_database.py`, fields question / chunk_ids)


def update_query_adapter(evals: Sequence[Any], *, max_evals: int = 4096, optimize_top_k: int = 40,
                         optimize_gap: float = 0.05, oversample: int = 4, config: Any | None = None,
                         index: GpuIndex | None = None, targets: str = "nnls") -> np.ndarray:
    """Compute the optimal query adapter from evals and install it on the index.

    evals: `Eval`-like objects (`.question`, `.chunk_ids`) or `(question, chunk_ids)` pairs; a question may be a
    string (embedded with `embed_strings`) or an already embedded vector.
    targets: "nnls" solves every eval's target on the host with the reference's `lsq_linear` call; "device" solves them
    all exactly in one `rl_query_targets` call (at most 64 examples per eval)."""
    if targets not in ("nnls", "device"):
        raise ValueError(f"Unsupported targets: {targets!r} (expected 'nnls' or 'device')")
    if targets == "device" and optimize_top_k > QT_MAX_EXAMPLES:
        raise ValueError(f"targets='device' takes at most {QT_MAX_EXAMPLES} examples per eval: optimize_top_k = {optimize_top_k}")
    config = config or HotPathConfig()
    gi = index or _index_for(config)
    if gi.index.n_rows == 0:
        raise ValueError("First run `insert_documents()` to insert documents.")  # `_query_adapter.py:146-148`
    evals = list(evals)[:max_evals]
    if len(evals) == 0:
        raise ValueError("First run `insert_evals()` to generate evals.")  # `:150-152`
    metric = config.vector_search_distance_metric
    if metric not in ("cosine", "dot"):
        raise ValueError(f"Unsupported metric: {metric}")  # `:206-208` (checked up front: nothing is computed for l2)
    no_adapter = replace(config, vector_search_query_adapter=False) if hasattr(config, "__dataclass_fields__") else config
    # ---- embed the questions (`:160`) -----------------------------------------------------------------------
    fields = [_eval_fields(ev) for ev in evals]
    texts = [q for q, _ in fields if isinstance(q, str)]
    # A late-chunking embedder treats a LIST of strings as the sentences of one document (they are joined and pooled
    # with each other's context); the reference embeds each question alone (`embed_strings([eval_.question])[0]`,
    # `_query_adapter.py:160`) and so does `vector_search` at query time.  Only the standard embedder is batched.
    if texts and embedding_type(config=no_adapter) == "late_chunking":
        embedded = iter([embed_strings([t], config=no_adapter)[0] for t in texts])
    else:
        embedded = iter(embed_strings(texts, config=no_adapter)) if texts else iter(())
    qs = [next(embedded) if isinstance(q, str) else np.ravel(np.asarray(q)) for q, _ in fields]
    Q_all = np.vstack([np.asarray(q, dtype=np.float32) for q in qs])  # noqa: N806
    # ---- ONE batched search without the adapter (`:162-165`, num_hits as in `_search.py:66-67`) --------------
    chunk_max_size = getattr(config, "chunk_max_size", DEFAULT_CHUNK_MAX_SIZE)
    num_hits = round(oversample * chunk_max_size / 2048) * max(optimize_top_k, 10)
    k = min(optimize_top_k, _ops.K_MAX)
    _, chunks, counts = gi.index.search_chunks(Q_all, min(num_hits, _ops.K_MAX), k)
    chunks = np.asarray(chunks).reshape(len(qs), k)
    counts = np.asarray(counts).reshape(len(qs))
    # ---- best row of every retrieved chunk (`:174,180`), ONE launch ------------------------------------------
    best = np.asarray(gi.index.chunk_best_rows(Q_all, chunks.astype(np.int32))).reshape(len(qs), k)
    # ---- which evals qualify (`:168-173`) --------------------------------------------------------------------------
    keep, rel_masks = [], []
    for i, (_, relevant) in enumerate(fields):
        n = int(counts[i])
        relevant = set(relevant)
        rel = np.fromiter((gi.chunk_ids[c] in relevant for c in chunks[i, :n]), dtype=bool, count=n)
        if rel.any() and not rel.all():
            keep.append(i)
            rel_masks.append(rel)
    if not keep:
        raise ValueError("No eval retrieved both relevant and irrelevant chunks; cannot fit a query adapter.")
    if targets == "device":
        # ---- every qualifying eval's exact target in one call; the example rows stay on the device (`:183`) ------
        ex_rows = np.full((len(keep), k), -1, np.int32)
        ex_rel = np.zeros((len(keep), k), np.uint8)
        for j, (i, rel) in enumerate(zip(keep, rel_masks)):
            ex_rows[j, : len(rel)] = best[i, : len(rel)]
            ex_rel[j, : len(rel)] = rel
        T_dev, _, _, status, _ = optimize_query_targets(Q_all[keep], ex_rows, ex_rel, gap=optimize_gap, index=gi)  # noqa: N806
        for j in np.flatnonzero(np.asarray(status) != 0):
            raise ValueError(f"eval {keep[j]}: no query target ({QT_STATUS[int(status[j])]})")
        T_rows = [np.asarray(T_dev[j]).astype(qs[i].dtype) for j, i in enumerate(keep)]  # noqa: N806  the cast of `:37`
        Q_rows = [qs[i] for i in keep]  # noqa: N806
        A_star = _adapter_from_targets(np.vstack(Q_rows).astype(np.float64), np.vstack(T_rows).astype(np.float64), metric)  # noqa: N806
        gi.query_adapter = np.asarray(A_star, dtype=np.float32)
        return A_star
    # ---- fetch the example rows in one go, solve the per-eval NNLS on the host (`:183`) ------------------------
    wanted = np.concatenate([best[i, : len(rel)] for i, rel in zip(keep, rel_masks)]).astype(np.int32)
    rows = np.asarray(gi.index.gather_rows(wanted))
    Q_rows, T_rows, base = [], [], 0  # noqa: N806
    for i, rel in zip(keep, rel_masks):
        ex = rows[base : base + len(rel)].astype(qs[i].dtype)  # `Chunk.embedding_matrix` has the stored dtype
        base += len(rel)
        q = qs[i]
        T_rows.append(_optimize_query_target(q, ex[rel], ex[~rel], alpha=optimize_gap))
        Q_rows.append(q)
    A_star = _adapter_from_targets(np.vstack(Q_rows).astype(np.float64), np.vstack(T_rows).astype(np.float64), metric)  # noqa: N806
    gi.query_adapter = np.asarray(A_star, dtype=np.float32)  # `IndexMetadata["query_adapter"]` (`:210-214`)
    return A_star
