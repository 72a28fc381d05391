"""`rl_query_targets` / `optimize_query_targets` / `update_query_adapter(targets="device")` on the device against the host statement
`optimize_query_target_active_set` (tests/test_query_targets_host.py holds that one against the reference); DESIGN.md section 4.15.

The two need not agree bit for bit (the device sums in another order), so each eval is judged by what characterises the solution:
equal status, the certificate of tests/query_targets_ref.py evaluated on the host in float64 from the device's targets and weights,
and the distance of the two targets, which a certificate residual delta bounds by O(sqrt(delta))."""

import functools
from pathlib import Path

import numpy as np
import pytest

import raglite_amd
from raglite_amd import _query_adapter
from oracle import oracle
from tests.query_targets_ref import GPU_BATCHES, GPU_CASES_HOST_RESIDUAL, batch_certificate, gpu_batch, host_solution

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float64).eps)


@functools.lru_cache(maxsize=None)
def _batch(dim, n_examples, gap, seed, repeat=1):
    """A batch and the host statement's answer to it: computed once, shared by the storages, never written to."""
    E, Q, rows, rel, forced = gpu_batch(dim, n_examples, gap, seed, repeat=repeat)  # noqa: N806
    host = host_solution(E, Q, rows, rel, forced, gap)
    for a in (E, Q, rows, rel, *host):
        a.setflags(write=False)
    return E, Q, rows, rel, host


def _check(E, Q, rows, rel, gap, host, got, what):  # noqa: N803
    """Every eval of a call against the host statement; returns (worst certificate residual, worst distance / |q|)."""
    T_h, W_h, obj_h, st_h, it_h, res_h = host  # noqa: N806
    T, W, obj, st, it = (np.asarray(x) for x in got)  # noqa: N806
    assert T.dtype == np.float64 and W.dtype == np.float64 and obj.dtype == np.float64 and st.dtype == np.int32 and it.dtype == np.int32
    assert np.array_equal(st, st_h), (what, st.tolist(), st_h.tolist())
    worst_r, worst_d = 0.0, 0.0
    for b in range(len(Q)):
        K = rows.shape[1]  # noqa: N806
        assert np.all(W[b] >= 0.0) and np.all(W[b][rows[b] < 0] == 0.0) and 0 <= it[b] <= 4 * K
        if st[b] in (1, 2):
            assert np.all(np.isnan(T[b])) and np.isnan(obj[b]) and np.all(W[b] == 0.0) and it[b] == 0, (what, b)
            continue
        qn = float(np.linalg.norm(Q[b].astype(np.float64)))
        assert abs(obj[b] - float(T[b] @ T[b])) <= 1e-12 * max(float(T[b] @ T[b]), 1e-300)
        if st[b] == 3:
            assert np.linalg.norm(T[b]) <= 1e-9 * qn and np.linalg.norm(T_h[b]) <= 1e-9 * qn, (what, b)
            continue
        sum_a, sum_b, rel_t, r = batch_certificate(E, Q, rows, rel, gap, T, W, b)
        dist = float(np.linalg.norm(T[b] - T_h[b])) / qn
        worst_r, worst_d = max(worst_r, r), max(worst_d, dist)
        assert abs(sum_a - sum_b) <= 1e-12 * max(sum_a, sum_b), (what, b)
        assert rel_t <= 1e-13, (what, b, rel_t)
        assert r <= 32 * GPU_CASES_HOST_RESIDUAL, (what, b, r)
        assert dist <= 32 * np.sqrt(max(r, res_h[b], EPS)), (what, b, dist, r, res_h[b])
    print(f"{what}: B = {len(Q)}, status counts {np.bincount(st, minlength=5).tolist()}, device certificate residual <= {worst_r:.3g} "
          f"(host {np.nanmax(res_h):.3g}), |t_dev - t_host| / |q| <= {worst_d:.3g}, entering steps <= {int(it.max())} (host {int(it_h.max())})")
    return worst_r, worst_d


# an fp16-stored index exists only at dims that are a multiple of 128 (rl_index_create_f16): of the dims here, 1024
@pytest.mark.parametrize("dim,n_examples,gap,seed,storage",
                         [(*b, s) for b in GPU_BATCHES for s in ("f32", "f16") if s == "f32" or b[0] % 128 == 0])
def test_device_against_the_host_statement(dim, n_examples, gap, seed, storage):
    E, Q, rows, rel, host = _batch(dim, n_examples, gap, seed)  # noqa: N806
    idx = raglite_amd.DeviceIndex(E, metric="cosine", storage=storage)  # (the rows are fp16 values: both storages hold the same numbers)
    got = raglite_amd.optimize_query_targets(Q, rows, rel, gap=gap, index=idx)
    _check(E, Q, rows, rel, gap, host, got, f"dim {dim}, {n_examples} examples, gap {gap}, {storage}")
    again = raglite_amd.optimize_query_targets(Q, rows, rel, gap=gap, index=idx)
    for a, b in zip(got, again):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()  # the same bits run to run
    # one eval alone (a healthy one between two failed ones): what its neighbours are does not reach it
    b = int(np.flatnonzero(host[3] == 0)[-1])
    one = raglite_amd.optimize_query_targets(Q[b : b + 1], rows[b : b + 1], rel[b : b + 1], gap=gap, index=idx)
    for a, full in zip(one, got):
        assert np.asarray(a)[0].tobytes() == np.asarray(full)[b].tobytes()
    idx.close()


def test_more_evals_than_the_grid_and_device_pointers(torch_cuda):
    """1 300 evals: every kernel's grid-stride loop (1 024 workgroups) takes a second round; CUDA tensors in, CUDA tensors out, the
    same bits as through host pointers."""
    torch = torch_cuda
    E, Q, rows, rel, host = _batch(8, 3, 0.05, 7, 100)  # noqa: N806
    assert len(Q) > 1024

    def cuda(a):
        return torch.as_tensor(np.array(a), device="cuda")  # (a copy: the shared batch is read-only)

    idx = raglite_amd.DeviceIndex(E, metric="cosine")
    got = raglite_amd.optimize_query_targets(Q, rows, rel, gap=0.05, index=idx)
    _check(E, Q, rows, rel, 0.05, host, got, "dim 8, 3 examples, two rounds")
    dev = raglite_amd.optimize_query_targets(cuda(Q), cuda(rows), cuda(rel), gap=0.05, index=idx)
    assert all(x.is_cuda for x in dev)
    for a, b in zip(got, dev):
        assert a.tobytes() == b.cpu().numpy().tobytes()
    idx.close()
    # ... and at the widest shape
    E, Q, rows, rel, host = _batch(1024, 64, 0.05, 100 * 1024 + 64)  # noqa: N806
    idx = raglite_amd.DeviceIndex(cuda(E), metric="cosine", storage="f16")
    got = raglite_amd.optimize_query_targets(Q, rows, rel, gap=0.05, index=idx)
    dev = raglite_amd.optimize_query_targets(cuda(Q), cuda(rows), cuda(rel.astype(bool)), gap=0.05, index=idx)
    for a, b in zip(got, dev):
        assert a.tobytes() == b.cpu().numpy().tobytes()
    idx.close()


def test_golden_cases_through_the_device():
    """The reference's own `_optimize_query_target` outputs (tests/golden/query_adapter.npz): within 1 fp16 ulp after the cast."""
    g = np.load(Path(__file__).parent / "golden" / "query_adapter.npz")
    total = 0
    for i in range(int(g["n_target_cases"])):
        q, P, N, want = g[f"target{i}_q"], g[f"target{i}_P"], g[f"target{i}_N"], g[f"target{i}_t"]  # noqa: N806
        E = np.vstack([P, N]).astype(np.float32)  # noqa: N806
        rows = np.arange(len(E), dtype=np.int32)[None]
        rel = (rows < len(P)).astype(np.uint8)
        for storage in ("f32", "f16"):
            if storage == "f16":  # fp16 storage needs a multiple of 128 columns: zero columns change neither K, e nor the target's
                E = np.pad(E, ((0, 0), (0, 128 - E.shape[1])))  # noqa: N806
                q = np.pad(q, (0, 128 - q.size))
                want = np.pad(want, (0, 128 - want.size))
            idx = raglite_amd.DeviceIndex(E, metric="cosine", storage=storage)
            T, _, _, status, _ = raglite_amd.optimize_query_targets(q.astype(np.float32)[None], rows, rel, gap=float(g[f"target{i}_alpha"]),  # noqa: N806
                                                                    index=idx)
            idx.close()
            got = T[0].astype(np.float16)
            differing = int(np.sum(got.view(np.uint16) != want.view(np.uint16)))
            total += differing
            print(f"golden target {i} ({storage}): {differing} differing elements of {want.size}")
            assert status[0] == 0
            ulp = np.spacing(np.abs(want).astype(np.float16)).astype(np.float64)
            assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp)
    print(f"golden targets through the device: {total} differing elements in all (0 expected)")


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_update_query_adapter_with_device_targets(metric, monkeypatch):
    """64 chunks, dim 64, optimize_top_k 10: the adapter from the device's targets equals `_adapter_from_targets` fed with the host
    statement's targets for the same evals; targets="nnls" is what it was."""
    rng = np.random.default_rng(21)
    dim, n_chunks = 64, 64
    mats = [oracle.synth_matrix(900 + i, int(rng.integers(1, 5)), dim) for i in range(n_chunks)]
    mats = [(m / np.linalg.norm(m, axis=1, keepdims=True)).astype(np.float16) for m in mats]
    ids = [f"{i:016x}" for i in range(n_chunks)]
    gi = raglite_amd.GpuIndex(ids, mats, metric=metric)
    E = np.vstack(mats).astype(np.float32)  # noqa: N806
    off = np.concatenate(([0], np.cumsum([len(m) for m in mats]))).astype(np.int64)
    evals = []
    for _ in range(40):
        t = int(rng.integers(0, n_chunks))
        q = (mats[t][0].astype(np.float32) + 0.08 * rng.standard_normal(dim)).astype(np.float16)
        evals.append((q, [ids[t], ids[(t + 11) % n_chunks]]))
    cfg = raglite_amd.HotPathConfig(vector_search_distance_metric=metric)
    calls = []
    real = _query_adapter.optimize_query_targets

    def recording(Q, rows, relevant, *, gap, index):  # noqa: N803
        out = real(Q, rows, relevant, gap=gap, index=index)
        calls.append((np.array(Q), np.array(rows), np.array(relevant), gap, [np.array(x) for x in out]))
        return out

    monkeypatch.setattr(_query_adapter, "optimize_query_targets", recording)
    monkeypatch.setattr(gi.index, "gather_rows", None)  # the device path fetches no rows
    A = raglite_amd.update_query_adapter(evals, optimize_top_k=10, config=cfg, index=gi, targets="device")  # noqa: N806
    monkeypatch.undo()
    assert len(calls) == 1 and gi.query_adapter is not None and gi.query_adapter.shape == (dim, dim)
    np.testing.assert_array_equal(gi.query_adapter, A.astype(np.float32))
    Q, rows, rel, gap, (T_dev, _, _, status, _) = calls[0]  # noqa: N806
    assert gap == 0.05 and rows.shape[1] == 10 and len(Q) > 20 and np.all(status == 0)
    T_host = host_solution(E, Q, rows, rel, np.full(len(Q), -1), gap)[0]  # noqa: N806
    dist = float(np.max(np.linalg.norm(T_dev - T_host, axis=1) / np.linalg.norm(Q, axis=1)))

    def adapter(T):  # noqa: N803
        return _query_adapter._adapter_from_targets(Q.astype(np.float64), T.astype(np.float16).astype(np.float64), metric)  # noqa: SLF001

    want = adapter(T_host)
    # what the adapter moves by when the host statement's targets move by 32 x the distance seen in test_device_against_the_host_statement
    # (2.7e-13 |q|) in a seeded direction: mostly nothing, the targets pass through a cast to fp16
    noise = np.random.default_rng(5).standard_normal(T_host.shape)
    noise *= 32 * DISTANCE_MEASURED * np.linalg.norm(Q, axis=1, keepdims=True) / np.linalg.norm(noise, axis=1, keepdims=True)
    moved = float(np.max(np.abs(adapter(T_host + noise) - want)))
    diff = float(np.max(np.abs(A - want)))
    print(f"{metric}: {len(Q)} evals, |t_dev - t_host| / |q| <= {dist:.3g}; adapter: device vs host statement {diff:.3g}, "
          f"host statement perturbed {moved:.3g}")
    assert diff <= 32 * moved
    # the default path is untouched
    A_nnls = raglite_amd.update_query_adapter(evals, optimize_top_k=10, config=cfg, index=gi)  # noqa: N806
    ref, Qs, _ = oracle.update_query_adapter(evals, E, off, ids, optimize_top_k=10, metric=metric, dtype=np.float32)  # noqa: N806
    assert len(Qs) == len(Q)
    np.testing.assert_allclose(A_nnls, ref, rtol=0, atol=1e-6)
    np.testing.assert_array_equal(A_nnls, raglite_amd.update_query_adapter(evals, optimize_top_k=10, config=cfg, index=gi, targets="nnls"))
    # a failed eval is named
    def poisoned(Q, rows, relevant, *, gap, index):  # noqa: N803
        Q = np.array(Q, np.float32)  # noqa: N806
        Q[0, 3] = np.nan
        return real(Q, rows, relevant, gap=gap, index=index)

    monkeypatch.setattr(_query_adapter, "optimize_query_targets", poisoned)
    with pytest.raises(ValueError, match=r"eval \d+: no query target \(a non-finite"):
        raglite_amd.update_query_adapter(evals, optimize_top_k=10, config=cfg, index=gi, targets="device")
    gi.close()


# |t_dev - t_host| / |q|, the worst over test_device_against_the_host_statement's evals as measured on an MI355X
DISTANCE_MEASURED = 2.7e-13
