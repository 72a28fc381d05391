"""GPU parity of the pass kernel's explicit tile loop (raglite_amd/csrc/maxsim_pp.hip, MODE 3: an even number of K slabs, dim % 64 == 0)
through `rl_maxsim_approx_scores`:

score[c] ~ sum_i max_{j in chunk c} Q[i].D[j] -- the multi-vector generalisation of `src/raglite/_search.py:143-149` of the reference.

What the loop changes is where a tile begins and ends: its first K slab multiplies into a zero C operand instead of accumulators the
epilogue zeroed, the eight block epilogues stand behind the slab loop, and the tile's 128 chunk-end bits come by one scalar load of
eight words.  So the shapes here are about tile boundaries: workgroups with ONE tile (prologue -> first slab -> epilogue -> flush),
with three and more (every later tile starts from C = 0 behind an epilogue), chunks that stay open across tiles, the widths 256
(8 slabs, the smallest), 320 (10), 1024 (32) and 288 (9 slabs: odd, the slab-counting loop), partial passes, and an index that ends
in the middle of a 16-row block (the bitmap load of the last tile).

The library runs this pass only over an index of at least 64 Mi elements (api.hip: big_corpus), so the row counts are the smallest
that reach the kernel at each width -- 256 row ranges (one per CU) of 1 024 / 832 / 912 / 256 rows: at width 256 every workgroup
walks eight tiles, at 1024 two or three.  A one-tile workgroup needs a row range of at most 128 rows, which ranges of 256 rows and
more only have where the chunks make them: layout "one_tile" alternates chunks of 106 and 2 R - 106 rows (R = rows per range), so
that every other range is [R b + R - 106, R b + R) -- 112 rows from its first 16-row block: one tile -- and the ranges between have
2 R - 106 rows of one chunk whose maximum stays open across all their tiles.

Bars: integer-valued data bit for bit against the NumPy oracle (every partial sum is an integer below 2^24); float data against the
eight-queries-per-pass kernel of maxsim_gemm.hip within 4 float32 ulps of the score scale -- the bar of tests/test_gpu_pp_pass.py (same
products and sums over K; the 32 per-vector maxima are added in another order)."""

import numpy as np
import pytest

import raglite_amd
from oracle import oracle
from tests.util import ragged_offsets

pytestmark = pytest.mark.gpu

RANGE_ROWS = {256: 1024, 320: 832, 288: 912, 1024: 256}  # rows per row range at 256 ranges: the smallest index of 64 Mi elements
WIDTHS = tuple(RANGE_ROWS)
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
    if layout == "one_tile":
        R = RANGE_ROWS[dim]
        assert n % (2 * R) == 0
        k = np.arange(n // (2 * R), dtype=np.int64) * (2 * R)
        return np.concatenate(([0], np.sort(np.concatenate((k + R - 106, k + R))), [n])).astype(np.int64)
    step = {"uniform8": 8, "rows300": 300}[layout]  # rows300: the open chunk's maximum is carried across two tile boundaries
    return np.concatenate((np.arange(0, n, step), [n])).astype(np.int64)


_CORPUS = {}


def _int_corpus(torch, n, dim):
    """Integer corpus, generated once per shape on the device and shared (unchanged) by the cases that use it: (device, host)."""
    if (n, dim) not in _CORPUS:
        _CORPUS.clear()  # (one shape at a time: 256 MiB each)
        E = torch.empty((n, dim), dtype=torch.float32, device="cuda")
        raglite_amd.synth_fill(E, seed=30_000 + dim, kind="small_int")
        _CORPUS[(n, dim)] = (E, E.cpu().numpy())
    return _CORPUS[(n, dim)]


def _check_int(n, dim, layout, n_queries, nq):
    torch = _torch()
    off = _offsets(layout, n, dim)
    E, E_host = _int_corpus(torch, n, dim)
    Qb = np.stack([oracle.synth_matrix(31_000 + 37 * i + nq, nq, dim, "small_int") for i in range(n_queries)])
    idx = raglite_amd.DeviceIndex(E, off, metric="dot")
    got, _ = idx.maxsim_approx_scores(torch.from_numpy(Qb).cuda(), kernel=0)
    got = got.cpu().numpy()
    idx.close()
    for i in sorted({0, n_queries - 1}):
        want = oracle.maxsim_scores(E_host, off, Qb[i], np.float32)
        bad = np.flatnonzero(got[i] != want)
        assert bad.size == 0, (i, bad.size, bad[:8].tolist(), got[i][bad[:4]].tolist(), want[bad[:4]].tolist())


# every width meets every layout, every layout every query shape (a Latin square, not the full product)
@pytest.mark.parametrize("dim,layout,shape", [(d, lay, QUERY_SHAPES[(i + j) % 3])
                                              for i, d in enumerate(WIDTHS) for j, lay in enumerate(("ragged", "uniform8", "rows300", "one_tile"))])
def test_integer_data_is_the_oracle_bit_for_bit(dim, layout, shape):
    _check_int(256 * RANGE_ROWS[dim], dim, layout, *shape)


@pytest.mark.parametrize("dim,layout", [(256, "ones"), (256, "ragged"), (1024, "ones"), (1024, "ragged")])
def test_index_that_ends_inside_a_block(dim, layout):
    """Thirteen rows more: the index ends in the middle of a 16-row block, and the last tile's eight-word bitmap load reaches past the
    corpus' last word.  One-row chunks: every bit of the bitmap is a score."""
    _check_int(256 * RANGE_ROWS[dim] + 13, dim, layout, 16, 9)


@pytest.mark.parametrize("dim", WIDTHS)
def test_float_data_against_the_eight_query_kernel(dim):
    torch = _torch()
    n, n_queries, nq = 256 * RANGE_ROWS[dim] + 13, 17, 32
    off = _offsets("ragged", n, dim)
    E = torch.empty((n, dim), dtype=torch.float32, device="cuda")
    raglite_amd.synth_fill(E, seed=32_000 + dim, kind="uniform")
    Q = torch.empty((n_queries, nq, dim), dtype=torch.float32, device="cuda")
    raglite_amd.synth_fill(Q, seed=32_001 + dim, kind="uniform")
    idx = raglite_amd.DeviceIndex(E, off, metric="dot")
    a, ma = idx.maxsim_approx_scores(Q, kernel=0)
    b, mb = idx.maxsim_approx_scores(Q, kernel=1)
    ulp = float(b.abs().max()) * 2.0 ** -23
    worst = float((a - b).abs().max())
    print(f"dim {dim}: worst |sixteen - eight| = {worst:.3g} = {worst / ulp:.2f} ulp of the score scale")
    assert worst <= 4 * ulp, (worst, ulp)
    assert torch.equal(ma, mb)
    a2, _ = idx.maxsim_approx_scores(Q, kernel=0)
    assert torch.equal(a, a2)  # deterministic
    idx.close()
