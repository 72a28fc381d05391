"""Shared by tests/test_query_targets_host.py and tests/test_gpu_query_targets.py: seeded cases of the query-target problem
(`_query_adapter.py:20-38`) and the certificate that characterises its solution without any other solver.

t* is the projection of the origin onto q + cone(D), D_ij = P_i - (1 + alpha) N_j.  t = q + D^T mu with mu >= 0 is that projection
exactly when  D_ij . t >= 0 for every pair  and  <t, t - q> = 0  (Moreau: t in the dual cone, t - q in the cone, orthogonal)."""

import numpy as np

# The worst certificate residual of the host statement over `host_cases()` / over the evals of tests/test_gpu_query_targets.py,
# measured on the CPU; the tests assert 32 x these.  The solver reads G off the Gram matrix K, so the
# residual is cancellation in K - c (K + K) + c^2 K (relative 1e-14 of entries near 1), not dim-dependent summation error.
HOST_RESIDUAL = 4.7e-13
GPU_CASES_HOST_RESIDUAL = 2.2e-13


def make_case(rng, dim, p, n, spread, *, dup=None, q_noise=0.3):
    """fp16-rounded unit rows around a common centre (spread = how far apart), a query near the centre; dup: None, "pp" (the last
    negative equals the first positive) or "nn" (two equal negatives, or two equal positives when n == 1)."""
    k = p + n
    centre = rng.standard_normal(dim)
    E = centre + spread * rng.standard_normal((k, dim))  # noqa: N806
    E = (E / np.linalg.norm(E, axis=1, keepdims=True)).astype(np.float16)  # noqa: N806
    q = (centre / np.linalg.norm(centre) + q_noise * rng.standard_normal(dim) / np.sqrt(dim)).astype(np.float16)
    if dup == "pp" and k > 2:
        E[-1] = E[0]
    elif dup == "nn" and k > 2:
        if n > 1:
            E[-1] = E[p]
        else:
            E[p - 1] = E[0]
    return q, E[:p], E[p:]


def host_cases():
    """(q, P, N, alpha): dims 8 / 32 / 1024, k 2 .. 40, p = 1 / n = 1 / p = n, alpha 0 / 0.05 / 0.5, spreads 0.1 / 0.7 / 3, every
    fifth case with a duplicated row (alternately a negative equal to a positive, and two equal rows of one kind)."""
    rng = np.random.default_rng(0)
    out, count = [], 0
    for dim in (8, 32, 1024):
        for k in (2, 3, 5, 9, 17, 31, 40):
            for shape in ("p1", "n1", "pn"):
                for alpha in (0.0, 0.05, 0.5):
                    for spread in (0.1, 0.7, 3.0):
                        p = 1 if shape == "p1" else (k - 1 if shape == "n1" else k // 2)
                        dup = None if count % 5 else ("pp" if count % 10 == 0 else "nn")
                        count += 1
                        out.append((*make_case(rng, dim, p, k - p, spread, dup=dup), alpha))
    return out


def certificate(q, P, N, alpha, t, weights):  # noqa: N803
    """(sum_a, sum_b, relative error of t against its recomputation from the weights, the certificate residual r):
    min_ij D_ij . t >= -r s  and  |<t, t - q>| <= r s  with  s = max |D_ij| |q|.  Everything in float64 on the host."""
    c = 1.0 + alpha
    q, P, N = q.astype(np.float64), P.astype(np.float64), N.astype(np.float64)  # noqa: N806
    p = len(P)
    a, b = weights[:p], weights[p:]
    again = q + a @ P - c * (b @ N)
    rel = float(np.linalg.norm(again - t) / max(np.linalg.norm(t), np.finfo(np.float64).tiny))
    D = (P[:, None, :] - c * N[None, :, :]).reshape(-1, q.size)  # noqa: N806
    s = float(np.max(np.linalg.norm(D, axis=1)) * np.linalg.norm(q))
    r = max(max(0.0, -float(np.min(D @ t))), abs(float(t @ (t - q)))) / s
    return float(np.sum(a)), float(np.sum(b)), rel, r


# ---- batches for the device (tests/test_gpu_query_targets.py) ----------------------------------------------------------------------
def _eval(rows, rel, q, status=None):
    return {"rows": list(rows), "rel": list(rel), "q": np.asarray(q, np.float32), "status": status}


def gpu_batch(dim, n_examples, gap, seed, *, repeat=1):
    """One `rl_query_targets` call's worth of evals over one index: (E float32 (n_rows, dim) with fp16-representable values, Q (B, dim)
    float32, rows (B, n_examples) int32, relevant (B, n_examples) uint8, forced status per eval or -1).  Evals with different p, padding
    (-1) at the end of and inside the list, duplicated rows and a repeated ordinal, and failed evals (status 1, 2, 3) between healthy
    ones.  A forced status marks what the host statement cannot see (an ordinal outside the index)."""
    rng = np.random.default_rng(seed)
    K = n_examples  # noqa: N806
    pool, evals = [], []

    def add(q, P, N, order=None, pad_inside=False, pad_end=0):  # noqa: N803
        base = sum(len(b) for b in pool)
        pool.append(np.vstack([P, N]))
        rows = [base + i for i in range(len(P) + len(N))]
        rel = [1] * len(P) + [0] * len(N)
        if order is not None:  # interleave positives and negatives
            rows, rel = [rows[i] for i in order], [rel[i] for i in order]
        if pad_inside:
            for at in (1, len(rows) // 2 + 1):
                rows.insert(at, -1)
                rel.insert(at, int(rng.integers(0, 2)))  # the flag of an empty slot means nothing
        rows += [-1] * pad_end
        rel += [0] * pad_end
        assert len(rows) == K, (len(rows), K)
        evals.append(_eval(rows, rel, q))

    for _ in range(repeat):
        ps = sorted({1, K - 1, max(K // 2, 1), int(rng.integers(1, K))})
        for i, p in enumerate(ps):  # the full list, different p, every spread
            spread = (0.1, 0.7, 3.0)[i % 3]
            q, P, N = make_case(rng, dim, p, K - p, spread)  # noqa: N806
            add(q, P, N, order=rng.permutation(K) if i % 2 else None)
        if K >= 4:
            m = K - 2  # two empty slots: at the end, then inside
            q, P, N = make_case(rng, dim, m // 2, m - m // 2, 0.7)  # noqa: N806
            add(q, P, N, pad_end=2)
            q, P, N = make_case(rng, dim, 1, m - 1, 0.7)  # noqa: N806
            add(q, P, N, pad_inside=True)
            q, P, N = make_case(rng, dim, 2, K - 2, 0.7, dup="pp")  # noqa: N806  a negative that equals a positive
            add(q, P, N)
            q, P, N = make_case(rng, dim, K // 2, K - K // 2, 3.0, dup="nn")  # noqa: N806  two equal negatives
            add(q, P, N)
            q, P, N = make_case(rng, dim, 2, K - 2, 0.7)  # noqa: N806  one ordinal twice in the list
            add(q, P, N)
            evals[-1]["rows"][-1] = evals[-1]["rows"][-2]
        if K == 3:
            q, P, N = make_case(rng, dim, 1, 1, 0.7)  # noqa: N806
            add(q, P, N, pad_end=1)
        # failed evals, each followed by a healthy one
        q, P, N = make_case(rng, dim, 1, K - 1, 0.7)  # noqa: N806
        add(q, P, N)
        evals[-1]["rel"] = [0] * K  # status 1: no positive
        q, P, N = make_case(rng, dim, 1, K - 1, 0.7)  # noqa: N806
        add(q, P, N)
        q, P, N = make_case(rng, dim, 1, K - 1, 0.7)  # noqa: N806
        add(q, P, N)
        evals[-1]["rows"] = [-1] * K  # status 1: no example at all
        q, P, N = make_case(rng, dim, K - 1, 1, 0.7)  # noqa: N806
        add(q, P, N)
        evals[-1]["rows"][0] = -7  # status 2: ordinals outside the index, below and (set once the index is complete) above
        evals[-1]["status"] = 2
        q, P, N = make_case(rng, dim, 1, K - 1, 3.0)  # noqa: N806
        add(q, P, N)
        q, P, N = make_case(rng, dim, 1, K - 1, 0.7)  # noqa: N806
        add(q, P, N)
        evals[-1]["rows"][K - 1] = 1 << 30
        evals[-1]["status"] = 2
        q, P, N = make_case(rng, dim, 1, K - 1, 0.7)  # noqa: N806
        q = q.astype(np.float32)
        q[dim // 2] = np.nan  # status 2: a non-finite query
        add(q, P, N)
        q, P, N = make_case(rng, dim, 1, K - 1, 0.1)  # noqa: N806
        add(q, P, N)
        if gap > 0:  # status 3: a positive that equals a negative, seen from that very row
            q, P, N = make_case(rng, dim, 1, 1, 0.7)  # noqa: N806
            add(P[0], P, P, pad_end=K - 2)
            q, P, N = make_case(rng, dim, 1, K - 1, 0.7)  # noqa: N806
            add(q, P, N)
    E = np.vstack(pool).astype(np.float32)  # noqa: N806
    for ev in evals:
        ev["rows"] = [len(E) + 3 if r == 1 << 30 else r for r in ev["rows"]]
    return (E, np.vstack([ev["q"] for ev in evals]), np.asarray([ev["rows"] for ev in evals], np.int32),
            np.asarray([ev["rel"] for ev in evals], np.uint8), np.asarray([-1 if ev["status"] is None else ev["status"] for ev in evals]))


def host_solution(E, Q, rows, relevant, forced, gap):  # noqa: N803
    """The host statement on every eval of a batch, in the layout of `rl_query_targets`: (T, weights by slot, objective, status,
    iterations, certificate residual per eval or NaN)."""
    from raglite_amd import optimize_query_target_active_set

    B, K = rows.shape  # noqa: N806
    T, W = np.full((B, E.shape[1]), np.nan), np.zeros((B, K))  # noqa: N806
    obj, status, iters, resid = np.full(B, np.nan), np.zeros(B, np.int32), np.zeros(B, np.int32), np.full(B, np.nan)
    for b in range(B):
        if forced[b] >= 0:
            status[b] = forced[b]
            continue
        have = rows[b] >= 0
        ps, ns = np.flatnonzero(have & (relevant[b] != 0)), np.flatnonzero(have & (relevant[b] == 0))
        P, N = E[rows[b, ps]], E[rows[b, ns]]  # noqa: N806
        t, w, obj[b], status[b], iters[b] = optimize_query_target_active_set(Q[b], P, N, alpha=gap)
        T[b] = t
        W[b, ps], W[b, ns] = w[: len(ps)], w[len(ps) :]
        if status[b] == 0:
            resid[b] = certificate(Q[b], P, N, gap, t, w)[3]
    return T, W, obj, status, iters, resid


def batch_certificate(E, Q, rows, relevant, gap, T, W, b):  # noqa: N803
    """`certificate` for eval b of a batch from targets and weights in the call's layout."""
    have = rows[b] >= 0
    ps, ns = np.flatnonzero(have & (relevant[b] != 0)), np.flatnonzero(have & (relevant[b] == 0))
    return certificate(Q[b], E[rows[b, ps]], E[rows[b, ns]], gap, T[b], np.concatenate([W[b, ps], W[b, ns]]))


GPU_BATCHES = [(dim, K, 0.05, 100 * dim + K) for dim in (8, 96, 1024) for K in (2, 3, 40, 64)] + [(96, 40, 0.0, 1), (96, 40, 0.5, 2)]
