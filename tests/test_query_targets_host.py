"""`raglite_amd.optimize_query_target_active_set`: the exact query target of `_query_adapter.py:20-38` as an active-set iteration on
the Gram matrix of the examples.  It is the single host statement of what `query_targets.hip` runs and the
reference of tests/test_gpu_query_targets.py, so here it is held against the reference's own outputs, a certificate that needs no
other solver, the reference's solver, and the degenerate shapes.  Also: the argument checks of `rl_query_targets` that return before
any HIP call, and the `ValueError`s of `update_query_adapter(targets=...)`."""

from pathlib import Path

import numpy as np
import pytest

import raglite_amd
from raglite_amd import _abi, _search
from raglite_amd._query_adapter import _optimize_query_target
from raglite_amd import optimize_query_target_active_set as active_set
from tests.query_targets_ref import HOST_RESIDUAL, certificate, host_cases, make_case

GOLDEN = Path(__file__).parent / "golden" / "query_adapter.npz"


def test_reference_targets_of_the_golden_cases_bit_for_bit():
    g = np.load(GOLDEN)
    assert int(g["n_target_cases"]) == 5
    for i in range(5):
        q, want = g[f"target{i}_q"], g[f"target{i}_t"]
        t, _, _, status, _ = active_set(q, g[f"target{i}_P"], g[f"target{i}_N"], alpha=float(g[f"target{i}_alpha"]))
        assert status == 0 and t.dtype == np.float64
        differing = int(np.sum(t.astype(q.dtype).view(np.uint16) != want.view(np.uint16)))
        print(f"golden target {i}: {differing} differing elements of {want.size}")
        assert differing == 0


def test_certificate_on_seeded_cases():
    """weights >= 0, sum a = sum b, t is what the weights say, and t is the projection: no other solver involved."""
    worst, worst_iters, solved, zero = 0.0, 0.0, 0, 0
    for q, P, N, alpha in host_cases():  # noqa: N806
        t, w, obj, status, iters = active_set(q, P, N, alpha=alpha)
        k = len(P) + len(N)
        assert status in (0, 3), (q.size, k, alpha, status)
        assert np.all(w >= 0.0) and w.shape == (k,) and iters <= 4 * k
        sum_a, sum_b, rel, r = certificate(q, P, N, alpha, t, w)
        assert abs(sum_a - sum_b) <= 1e-12 * max(sum_a, sum_b)
        if status == 3:  # the constraints cannot be met (few dimensions, many pairs): t is numerically zero
            zero += 1
            assert np.linalg.norm(t) <= 1e-9 * np.linalg.norm(q.astype(np.float64)) and q.size == 8
            continue
        solved += 1
        assert rel <= 1e-13 and obj == float(t @ t)
        worst, worst_iters = max(worst, r), max(worst_iters, iters / k)
        assert r <= 32 * HOST_RESIDUAL, (q.size, k, len(P), alpha, r)
    print(f"certificate residual: worst {worst:.3g} over {solved} solved cases ({zero} zero targets); entering steps / k <= {worst_iters:.2f}")
    assert solved >= 500


def test_never_worse_than_the_reference_solver():
    """`lsq_linear(tol=eps)` stops unconverged from three positives on (status -1); the optimum cannot exceed any feasible point."""
    rng = np.random.default_rng(1)
    shapes = ((1, 5, 16), (2, 3, 8), (1, 11, 32), (3, 5, 32), (4, 8, 64), (6, 6, 32), (2, 9, 1024), (3, 3, 16))
    assert sum(p >= 3 for p, _, _ in shapes) >= 3
    for p, n, dim in shapes:
        q, P, N = make_case(rng, dim, p, n, 0.7)  # noqa: N806
        t, _, obj, status, _ = active_set(q, P, N)
        t_ref = _optimize_query_target(q.astype(np.float64), P, N)  # float64 in, float64 out: before the cast of `:37`
        assert status == 0 and t_ref.dtype == np.float64
        ref = float(t_ref @ t_ref)
        print(f"p x n = {p} x {n}, dim {dim}: |t|^2 = {obj:.17g}, the reference's {ref:.17g} (ratio - 1 = {ref / obj - 1:.3g})")
        assert obj <= ref * (1 + 1e-12)


def test_degenerate_shapes():
    rng = np.random.default_rng(2)
    x = np.zeros(8, np.float16)
    x[0] = 1.0
    # every constraint already holds: nothing enters, t is q itself
    q = (x + np.float16(0.25)).astype(np.float16)
    t, w, obj, status, iters = active_set(q, x[None], -x[None])
    assert status == 0 and iters == 0 and np.array_equal(t, q.astype(np.float64)) and np.all(w == 0.0)
    assert obj == float(q.astype(np.float64) @ q.astype(np.float64))
    # p = n = 1: one pair, mu = max(0, -h / G)
    for alpha in (0.0, 0.05, 0.5):
        for _ in range(6):
            q, P, N = make_case(rng, 32, 1, 1, 3.0)  # noqa: N806
            d = P[0].astype(np.float64) - (1 + alpha) * N[0].astype(np.float64)
            mu = max(0.0, -float(d @ q.astype(np.float64)) / float(d @ d))
            t, w, _, status, iters = active_set(q, P, N, alpha=alpha)
            assert status == 0 and iters == (1 if mu > 0 else 0)
            np.testing.assert_allclose(w, [mu, mu], rtol=1e-13, atol=0)
            np.testing.assert_allclose(t, q.astype(np.float64) + mu * d, rtol=1e-13, atol=1e-15)
    # more pairs than eight dimensions can separate: the cone reaches -q, the target is zero
    q, P, N = make_case(np.random.default_rng(3), 8, 15, 16, 3.0)  # noqa: N806
    t, w, obj, status, iters = active_set(q, P, N)
    assert status == 3 and np.linalg.norm(t) <= 1e-9 * np.linalg.norm(q.astype(np.float64)) and iters <= 4 * 31
    # a positive that equals a negative, seen from that very row: t = (1 - alpha mu) q reaches zero
    t, _, _, status, _ = active_set(x, x[None], x[None], alpha=0.05)
    assert status == 3
    # no positives / no negatives: the eval does not qualify
    for P, N in ((np.zeros((0, 8), np.float16), x[None]), (x[None], np.zeros((0, 8), np.float16))):  # noqa: N806
        t, w, obj, status, iters = active_set(q, P, N)
        assert status == 1 and iters == 0 and np.all(np.isnan(t)) and np.isnan(obj) and np.all(w == 0.0) and w.shape == (1,)
    # a non-finite value anywhere
    bad = x.copy()
    bad[3] = np.nan
    for args in ((q, bad[None], -x[None]), (q, x[None], np.vstack([-x, bad])), (bad, x[None], -x[None])):
        t, w, obj, status, iters = active_set(*args)
        assert status == 2 and iters == 0 and np.all(np.isnan(t)) and np.isnan(obj) and np.all(w == 0.0)
    inf = x.copy()
    inf[1] = np.inf
    assert active_set(q, inf[None], -x[None])[3] == 2


def test_c_entry_rejects_bad_arguments_before_any_hip_call():
    lib = _abi.lib()
    B, k, dim = 2, 3, 8  # noqa: N806
    Q = np.ones((B, dim), np.float32)  # noqa: N806
    rows = np.zeros((B, k), np.int32)
    rel = np.ones((B, k), np.uint8)
    T, w = np.zeros((B, dim)), np.zeros((B, k))  # noqa: N806
    obj, status, iters = np.zeros(B), np.zeros(B, np.int32), np.zeros(B, np.int32)
    handle = np.zeros(64, np.uint8)  # stands in for an index: every check here returns before the handle is looked at
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def call(handle=handle, Q=Q, B=B, rows=rows, rel=rel, k=k, gap=0.05, T=T, w=w, obj=obj, status=status, iters=iters,  # noqa: N803
             mem=_abi.MEM_HOST):
        return lib.rl_query_targets(p(handle), p(Q), B, p(rows), p(rel), k, gap, p(T), p(w), p(obj), p(status), p(iters), mem, None)

    for kwargs, word in (({"handle": None}, "index"), ({"Q": None}, "queries"), ({"rows": None}, "rows"), ({"rel": None}, "relevant"),
                         ({"T": None}, "targets"), ({"w": None}, "weights"), ({"obj": None}, "objective"), ({"status": None}, "status"),
                         ({"iters": None}, "iterations"), ({"B": 0}, "n_queries"), ({"B": -3}, "n_queries"), ({"k": 1}, "n_examples"),
                         ({"k": 65}, "n_examples"), ({"gap": -0.01}, "gap"), ({"gap": float("nan")}, "gap"),
                         ({"gap": float("inf")}, "gap"), ({"mem": 7}, "mem")):
        assert call(**kwargs) == _abi.RL_ERR_INVALID, kwargs
        err = _abi.last_error()
        assert "rl_query_targets" in err and word in err, (kwargs, err)
    assert np.all(T == 0) and np.all(status == 0)
    assert lib.rl_version() == 100


class _FakeDeviceIndex:
    """The fake of tests/test_host_logic.py, as far as `update_query_adapter` reaches before it checks `targets`."""

    def __init__(self, E, off):  # noqa: N803
        self.E, self.off = E, off
        self.n_rows, self.n_chunks = len(E), len(off) - 1


def _gpu_index(n_chunks=12, dim=16):
    rng = np.random.default_rng(0)
    off = np.arange(n_chunks + 1, dtype=np.int64)
    gi = _search.GpuIndex.__new__(_search.GpuIndex)
    gi.chunk_ids = [f"chunk{i:04d}" for i in range(n_chunks)]
    gi.index = _FakeDeviceIndex(rng.standard_normal((n_chunks, dim)).astype(np.float32), off)
    gi.metric = "cosine"
    gi.query_adapter = None
    return gi


def test_update_query_adapter_rejects_bad_targets_arguments():
    gi = _gpu_index()
    evals = [(np.ones(16, np.float16), [gi.chunk_ids[0]])]
    with pytest.raises(ValueError, match="bogus"):
        raglite_amd.update_query_adapter(evals, index=gi, targets="bogus")
    with pytest.raises(ValueError, match="optimize_top_k"):
        raglite_amd.update_query_adapter(evals, index=gi, targets="device", optimize_top_k=65)
    assert gi.query_adapter is None
