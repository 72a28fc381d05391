"""GPU parity of the pass kernel's alternating loop (raglite_amd/csrc/maxsim_pp.hip, MODE 4; RL_OPT_PP_LOOP = 1) through
`rl_maxsim_approx_scores`:

score[c] ~ sum_i max_{j in chunk c} Q[i].D[j] -- the multi-vector generalisation of `src/raglite/_search.py:143-149` of the reference.

The alternating loop multiplies the same products in the same order per accumulator as the tile loop (RL_OPT_PP_LOOP = 0) and runs the
same epilogue; what it changes is when a wave loads: a K slab is a compute segment and a load segment, each ended by the workgroup
barrier, and waves 4-7 run one segment behind waves 0-3.  So float data must come out BIT FOR BIT as under the tile loop, and the shapes
are those of tests/test_gpu_pp_tile_loop.py, the smallest indexes that reach the kernel (256 row ranges of 1 024 / 832 / 256 rows at the
widths 256 / 320 / 1024): one-tile workgroups (prologue -> skew -> one tile -> tail; layout "one_tile"), many-tile workgroups, chunks
open across tiles and ranges, partial passes, an index that ends inside a 16-row block.  Width 288 (nine K slabs: odd) runs the
slab-counting loop under either value.

Bars: float data -- `torch.equal` between the two loops and between two calls; integer-valued data -- the NumPy oracle bit for bit
(every partial sum is an integer below 2^24)."""

import numpy as np
import pytest

import raglite_amd
from oracle import oracle
from tests.util import ragged_offsets

pytestmark = pytest.mark.gpu

RANGE_ROWS = {256: 1024, 320: 832, 1024: 256, 288: 912}  # rows per row range at 256 ranges: the smallest index of 64 Mi elements
WIDTHS = (256, 320, 1024)  # even numbers of K slabs: 8, 10, 32
LAYOUTS = ("ragged", "ones", "uniform8", "rows300", "one_tile")
QUERY_SHAPES = ((1, 1), (16, 9), (17, 32))  # (queries, vectors): one query in a one-query pass; a full pass; a full pass and a one-query pass


def _torch():
    import torch

    raglite_amd.set_device(0)
    return torch


def _offsets(layout, n, dim):
    if layout == "ragged":
        return ragged_offsets(np.random.default_rng(n), n, 1, 15)
    if layout == "ones":
        return np.arange(n + 1, dtype=np.int64)
    if layout == "one_tile":  # every other row range is 112 rows from its first 16-row block: one tile (tests/test_gpu_pp_tile_loop.py)
        R = RANGE_ROWS[dim]
        assert n % (2 * R) == 0
        k = np.arange(n // (2 * R), dtype=np.int64) * (2 * R)
        return np.concatenate(([0], np.sort(np.concatenate((k + R - 106, k + R))), [n])).astype(np.int64)
    step = {"uniform8": 8, "rows300": 300}[layout]  # rows300: the open chunk's maximum is carried across two tile boundaries
    return np.concatenate((np.arange(0, n, step), [n])).astype(np.int64)


_CORPUS = {}


def _corpus(torch, n, dim, kind):
    """Corpus, generated once per shape on the device and shared (unchanged) by the cases that use it."""
    if (n, dim, kind) not in _CORPUS:
        _CORPUS.clear()  # (one shape at a time: 256 MiB each)
        E = torch.empty((n, dim), dtype=torch.float32, device="cuda")
        raglite_amd.synth_fill(E, seed=40_000 + dim, kind=kind)
        _CORPUS[(n, dim, kind)] = E
    return _CORPUS[(n, dim, kind)]


def _both_loops_agree(n, dim, layout, n_queries, nq):
    torch = _torch()
    E = _corpus(torch, n, dim, "uniform")
    Q = torch.empty((n_queries, nq, dim), dtype=torch.float32, device="cuda")
    raglite_amd.synth_fill(Q, seed=41_000 + dim + nq, kind="uniform")
    idx = raglite_amd.DeviceIndex(E, _offsets(layout, n, dim), metric="dot")
    with idx.options(pp_loop=0):
        a, ma = idx.maxsim_approx_scores(Q, kernel=0)
    with idx.options(pp_loop=1):
        assert idx.get_option("pp_loop") == 1
        b, mb = idx.maxsim_approx_scores(Q, kernel=0)
        b2, mb2 = idx.maxsim_approx_scores(Q, kernel=0)
    differ = int((a != b).sum())
    print(f"dim {dim} {layout} {n_queries} x {nq}: {differ} of {a.numel()} scores differ between the loops")
    assert torch.equal(a, b), differ  # same products, same order
    assert torch.equal(ma, mb)
    assert torch.equal(b, b2) and torch.equal(mb, mb2)  # deterministic
    idx.close()


# every width meets every layout, every layout every query shape (a Latin square, not the full product)
@pytest.mark.parametrize("dim,layout,shape", [(d, lay, QUERY_SHAPES[(i + j) % 3]) for i, d in enumerate(WIDTHS) for j, lay in enumerate(LAYOUTS)])
def test_float_data_is_the_tile_loop_bit_for_bit(dim, layout, shape):
    _both_loops_agree(256 * RANGE_ROWS[dim], dim, layout, *shape)


@pytest.mark.parametrize("dim,layout,shape", [(256, "ones", (16, 9)), (320, "ragged", (17, 32)), (1024, "ones", (1, 1)), (1024, "ragged", (16, 9))])
def test_index_that_ends_inside_a_block(dim, layout, shape):
    """Thirteen rows more: the index ends in the middle of a 16-row block (the last tile's corpus pieces and bitmap load)."""
    _both_loops_agree(256 * RANGE_ROWS[dim] + 13, dim, layout, *shape)


def test_odd_slab_count_takes_the_slab_counting_loop_under_either_value():
    _both_loops_agree(256 * RANGE_ROWS[288] + 13, 288, "ragged", 17, 32)


@pytest.mark.parametrize("dim,layout,shape", [(256, "one_tile", (17, 32)), (320, "rows300", (16, 9)), (1024, "ragged", (17, 32))])
def test_integer_data_is_the_oracle_bit_for_bit(dim, layout, shape):
    torch = _torch()
    n, (n_queries, nq) = 256 * RANGE_ROWS[dim], shape
    off = _offsets(layout, n, dim)
    E = _corpus(torch, n, dim, "small_int")
    E_host = E.cpu().numpy()
    Qb = np.stack([oracle.synth_matrix(42_000 + 37 * i + nq, nq, dim, "small_int") for i in range(n_queries)])
    idx = raglite_amd.DeviceIndex(E, off, metric="dot")
    with idx.options(pp_loop=1):
        got, _ = idx.maxsim_approx_scores(torch.from_numpy(Qb).cuda(), kernel=0)
    got = got.cpu().numpy()
    idx.close()
    for i in sorted({0, n_queries - 1}):
        want = oracle.maxsim_scores(E_host, off, Qb[i], np.float32)
        bad = np.flatnonzero(got[i] != want)
        assert bad.size == 0, (i, bad.size, bad[:8].tolist(), got[i][bad[:4]].tolist(), want[bad[:4]].tolist())


def test_default_and_values():
    _torch()
    assert raglite_amd.get_default_option("pp_loop") in (0, 1)
    E = np.zeros((64, 256), dtype=np.float32)
    E[:, 0] = 1.0
    idx = raglite_amd.DeviceIndex(E, np.arange(0, 65, 8), metric="dot")
    before = idx.get_option("pp_loop")
    assert before == raglite_amd.get_default_option("pp_loop")
    for bad in (2, -1, 3, 66):
        with pytest.raises(Exception):
            idx.set_option("pp_loop", bad)
        assert idx.get_option("pp_loop") == before
    for v in (1, 0, 1):
        idx.set_option("pp_loop", v)
        assert idx.get_option("pp_loop") == v
    with idx.options(pp_loop=0):
        assert idx.get_option("pp_loop") == 0
    assert idx.get_option("pp_loop") == 1
    idx.close()
