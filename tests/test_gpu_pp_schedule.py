"""The workgroup order of the sixteen-query MaxSim pass (RL_OPT_PP_SCHEDULE, raglite_amd/csrc/pp_schedule.h) changes where and when its
workgroups run, never what they compute: every score of the pass, and every result of the pipelines built on it, is bit-identical
under the co-scheduled order (1, the default) and the pass-major order (0).

Covered: one to nine passes per launch (1, 15, 17, 100, 128, 130 queries), row-range counts that are and are not multiples of eight
(small wide-dim corpora put fewer row ranges than CUs in the launch), tombstoned chunks in the bound-filtered pipeline, and an
fp16-stored index with fp16 queries, whose result is the pass's own top-k."""

import numpy as np
import pytest

import raglite_amd
from oracle import oracle
from tests.util import ragged_offsets

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    raglite_amd.set_device(0)
    return torch


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _bits(t):
    return np.ascontiguousarray(_np(t)).view(np.uint32)


def _both(idx, fn):
    with idx.options(pp_schedule=0):
        a = fn()
    with idx.options(pp_schedule=1):
        b = fn()
    return a, b


def test_default_is_coscheduled():
    assert raglite_amd.get_default_option("pp_schedule") == 1


@pytest.mark.parametrize("n,dim,nq,n_queries", [
    (70_003, 1024, 32, 1),      # one pass: both orders are the same grid
    (70_003, 1024, 32, 15),
    (70_003, 1024, 17, 17),     # two passes, the second with one query
    (70_003, 1024, 32, 100),    # seven passes, the last partial
    (70_003, 1024, 32, 128),    # the headline batch: eight passes
    (70_003, 1024, 32, 130),    # nine passes
    (22_000, 3072, 32, 130),    # 172 row ranges (172 % 8 = 4): the last four keep the pass-major order
    (30_000, 3072, 9, 100),     # 235 row ranges (235 % 8 = 3)
])
def test_approximate_scores_are_bit_identical(n, dim, nq, n_queries):
    torch = _torch()
    rng = np.random.default_rng(n + n_queries)
    off = ragged_offsets(rng, n, 1, 15)
    E = torch.empty((n, dim), dtype=torch.float32, device="cuda")
    raglite_amd.synth_fill(E, seed=1100 + nq)
    Q = torch.empty((n_queries, nq, dim), dtype=torch.float32, device="cuda")
    raglite_amd.synth_fill(Q, seed=1200 + n_queries)
    idx = raglite_amd.DeviceIndex(E, off, metric="dot")
    (a, ma), (b, mb) = _both(idx, lambda: idx.maxsim_approx_scores(Q, kernel=0))
    assert np.array_equal(_bits(a), _bits(b)), f"{int((a != b).sum())} of {a.numel()} scores differ"
    assert np.array_equal(_bits(ma), _bits(mb))
    idx.close()


def test_pipeline_with_tombstones_is_bit_identical():
    torch = _torch()
    n, dim, nq, n_queries, k = 70_000, 1024, 32, 130, 100
    rng = np.random.default_rng(5)
    off = ragged_offsets(rng, n, 1, 15)
    E = torch.empty((n, dim), dtype=torch.float32, device="cuda")
    raglite_amd.synth_fill(E, seed=1300)
    Q = torch.empty((n_queries, nq, dim), dtype=torch.float32, device="cuda")
    raglite_amd.synth_fill(Q, seed=1301)
    idx = raglite_amd.DeviceIndex(E, off, metric="dot")
    n_chunks = len(off) - 1
    _, full_c = idx.maxsim_topk_batch(Q, k)
    dead = np.unique(np.concatenate((_np(full_c)[:, :5].reshape(-1), rng.choice(n_chunks, 500, replace=False)))).astype(np.int64)
    dead = dead[dead >= 0]
    idx.delete_chunks(dead)
    (sa, ca), (sb, cb) = _both(idx, lambda: idx.maxsim_topk_batch(Q, k))
    assert idx.filter_stats()["kind"] == "maxsim_batch_hi"
    assert np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(_np(ca), _np(cb))
    assert not np.isin(_np(cb), dead).any()
    idx.close()


def test_fp16_stored_index_with_fp16_queries_is_bit_identical():
    n, dim, nq, n_queries, k = 70_000, 1024, 32, 130, 100
    rng = np.random.default_rng(6)
    off = ragged_offsets(rng, n, 1, 15)
    E16 = oracle.synth_matrix(1400, n, dim).astype(np.float16)
    Q16 = np.stack([oracle.synth_matrix(1500 + i, nq, dim) for i in range(n_queries)]).astype(np.float16)
    idx = raglite_amd.DeviceIndex(E16, off, metric="dot", storage="f16")
    (sa, ca), (sb, cb) = _both(idx, lambda: idx.maxsim_topk_batch(Q16, k))
    assert idx.filter_stats()["kind"] == "maxsim_batch_f16_exact"
    assert np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(_np(ca), _np(cb))
    idx.close()
