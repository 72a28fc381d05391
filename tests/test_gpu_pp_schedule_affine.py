"""The XCD-affine workgroup orders of the sixteen-query MaxSim pass (RL_OPT_PP_XCD_PASSES = 4, 2, 1 under RL_OPT_PP_SCHEDULE = 1;
raglite_amd/csrc/pp_schedule.h: pp_schedule_affine) change where and when the pass's workgroups run, and with which cache hint they
fetch the corpus, never what they compute: every score of the pass, and every result of the pipelines built on it, is bit-identical
under every width, to the co-scheduled order (8) and to the pass-major order (RL_OPT_PP_SCHEDULE = 0).

Covered: the cases of tests/test_gpu_pp_schedule.py -- one to nine passes per launch (1, 15, 17, 100, 128, 130 queries), row-range counts
that are and are not multiples of eight or of the width (172 and 235 ranges), tombstoned chunks in the bound-filtered pipeline, an
fp16-stored index with fp16 queries -- and a 17-pass batch (two affine blocks of eight passes and one trailing pass)."""

import numpy as np
import pytest

import raglite_amd
from oracle import oracle
from tests.util import ragged_offsets

pytestmark = pytest.mark.gpu

WIDTHS = (8, 4, 2, 1)


def _torch():
    import torch

    raglite_amd.set_device(0)
    return torch


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _bits(t):
    return np.ascontiguousarray(_np(t)).view(np.uint32)


def _every_order(idx, fn):
    """fn() under the pass-major order, then under every width of the 1-D grid: [(label, result)], the pass-major result first."""
    with idx.options(pp_schedule=0):
        out = [("pass-major", fn())]
    for w in WIDTHS:
        with idx.options(pp_schedule=1, pp_xcd_passes=w):
            assert idx.get_option("pp_xcd_passes") == w
            out.append((f"w={w}", fn()))
    return out


def test_default_and_values():
    _torch()
    assert raglite_amd.get_default_option("pp_schedule") == 1
    assert raglite_amd.get_default_option("pp_xcd_passes") in WIDTHS
    E = np.zeros((64, 256), dtype=np.float32)
    E[:, 0] = 1.0
    idx = raglite_amd.DeviceIndex(E, np.arange(0, 65, 8), metric="dot")
    before = idx.get_option("pp_xcd_passes")
    for bad in (3, 0, 16, -1):
        with pytest.raises(Exception):
            idx.set_option("pp_xcd_passes", bad)
        assert idx.get_option("pp_xcd_passes") == before
    for w in WIDTHS:
        idx.set_option("pp_xcd_passes", w)
        assert idx.get_option("pp_xcd_passes") == w
    idx.close()


@pytest.mark.parametrize("n,dim,nq,n_queries", [
    (70_003, 1024, 32, 1),      # one pass: every order is the same grid
    (70_003, 1024, 32, 15),
    (70_003, 1024, 17, 17),     # two passes, the second with one query
    (70_003, 1024, 32, 100),    # seven passes: fewer than a block of eight, every width falls back to the co-scheduled order
    (70_003, 1024, 32, 128),    # the headline batch: eight passes, one affine block
    (70_003, 1024, 32, 130),    # nine passes: one affine block and one trailing pass
    (22_000, 3072, 32, 130),    # 172 row ranges (172 % 8 = 4, 172 % 4 = 0)
    (30_000, 3072, 9, 100),     # 235 row ranges (235 % 8 = 3; odd: widths 4 and 2 fall back), seven passes
    (30_000, 3072, 9, 130),     # 235 row ranges, nine passes: width 1 is affine, 4 and 2 fall back
    (70_003, 1024, 32, 272),    # seventeen passes: two affine blocks and one trailing pass
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
    runs = _every_order(idx, lambda: tuple(_np(t).copy() for t in idx.maxsim_approx_scores(Q, kernel=0)))
    _, (a, ma) = runs[0]
    for label, (b, mb) in runs[1:]:
        assert np.array_equal(_bits(a), _bits(b)), f"{label}: {int((a != b).sum())} of {a.size} scores differ"
        assert np.array_equal(_bits(ma), _bits(mb)), label
    idx.close()


def test_option_is_ignored_under_the_pass_major_order():
    """Same bits under every width with RL_OPT_PP_SCHEDULE = 0 (the width is not read there; that is all a test can say)."""
    torch = _torch()
    n, dim, nq, n_queries = 70_003, 1024, 32, 130
    rng = np.random.default_rng(11)
    off = ragged_offsets(rng, n, 1, 15)
    E = torch.empty((n, dim), dtype=torch.float32, device="cuda")
    raglite_amd.synth_fill(E, seed=1600)
    Q = torch.empty((n_queries, nq, dim), dtype=torch.float32, device="cuda")
    raglite_amd.synth_fill(Q, seed=1601)
    idx = raglite_amd.DeviceIndex(E, off, metric="dot")
    outs = []
    for w in WIDTHS:
        with idx.options(pp_schedule=0, pp_xcd_passes=w):
            outs.append(tuple(_np(t).copy() for t in idx.maxsim_approx_scores(Q, kernel=0)))
    for b, mb in outs[1:]:
        assert np.array_equal(_bits(outs[0][0]), _bits(b)) and np.array_equal(_bits(outs[0][1]), _bits(mb))
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

    def run():
        s, c = idx.maxsim_topk_batch(Q, k)
        assert idx.filter_stats()["kind"] == "maxsim_batch_hi"
        return _np(s).copy(), _np(c).copy()

    runs = _every_order(idx, run)
    _, (sa, ca) = runs[0]
    for label, (sb, cb) in runs[1:]:
        assert np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(ca, cb), label
        assert not np.isin(cb, dead).any()
    idx.close()


def test_fp16_stored_index_with_fp16_queries_is_bit_identical():
    n, dim, nq, n_queries, k = 70_000, 1024, 32, 130, 100
    rng = np.random.default_rng(6)
    off = ragged_offsets(rng, n, 1, 15)
    E16 = oracle.synth_matrix(1400, n, dim).astype(np.float16)
    Q16 = np.stack([oracle.synth_matrix(1500 + i, nq, dim) for i in range(n_queries)]).astype(np.float16)
    idx = raglite_amd.DeviceIndex(E16, off, metric="dot", storage="f16")

    def run():
        s, c = idx.maxsim_topk_batch(Q16, k)
        assert idx.filter_stats()["kind"] == "maxsim_batch_f16_exact"
        return _np(s).copy(), _np(c).copy()

    runs = _every_order(idx, run)
    _, (sa, ca) = runs[0]
    for label, (sb, cb) in runs[1:]:
        assert np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(ca, cb), label
    idx.close()
