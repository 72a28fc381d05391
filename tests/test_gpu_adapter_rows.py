"""`chunk_best_rows_kernel` and `gather_rows_kernel` (adapter_fit.hip; `rl_chunk_best_rows`, `rl_gather_rows`) on float data, at widths
off a multiple of 64 and of 4, past 16 384 items (the grid-stride loops) and at the special candidates, in both storage precisions.
The argmax is compared with float64 wherever float64 is decisive: where its gap between the best and the second-best row exceeds the
float32 error of the two dots, (ceil(dim / 64) + 8) * 2^-24 * ||row|| ||q|| (a chain of ceil(dim / 64) fmas, 6 butterfly adds, the
products' roundings; ||row|| the largest of the chunk).  At most 2 % of the items may fall under that gap.

An fp16-stored index exists only at widths that are a multiple of 128 (`rl_index_create_f16` refuses the others), so fp16 storage runs at
128, 384, 1024 and 4096, and its special-candidate and stride cases at 128; every width runs on fp32 storage."""

import numpy as np
import pytest

import raglite_amd
from raglite_amd._abi import UnsupportedError
from tests.util import ragged_offsets

pytestmark = pytest.mark.gpu

INT32_MAX = np.iinfo(np.int32).max


def cases(dims):
    """(dim, storage) for every width, fp16 storage where an fp16 index of that width exists."""
    return [(d, "f32") for d in dims] + [(d, "f16") for d in dims if d % 128 == 0]


def stored(E, storage):
    """What the index keeps, as float32: the rows themselves, or their fp16 rounding widened."""
    return E if storage == "f32" else E.astype(np.float16).astype(np.float32)


def best_rows_ref(E, off, Q, cand):
    """float64 argmax of every (query, candidate) -> (rows int32 (B, n_cand), decisive bool (B, n_cand))."""
    E64, Q64 = E.astype(np.float64), Q.astype(np.float64)
    dim, n_chunks = E.shape[1], len(off) - 1
    S = E64 @ Q64.T
    e_norm, q_norm = np.linalg.norm(E64, axis=1), np.linalg.norm(Q64, axis=1)
    bound = (-(-dim // 64) + 8) * 2.0 ** -24
    want = np.full(cand.shape, -1, np.int32)
    decisive = np.ones(cand.shape, bool)
    for b in range(cand.shape[0]):
        for j, c in enumerate(cand[b]):
            if c < 0 or c >= n_chunks or off[c + 1] == off[c]:
                continue
            lo, hi = int(off[c]), int(off[c + 1])
            s = S[lo:hi, b]
            r = int(np.argmax(s))
            want[b, j] = lo + r
            if hi - lo > 1:
                gap = s[r] - np.max(np.delete(s, r))
                decisive[b, j] = gap > bound * e_norm[lo:hi].max() * q_norm[b]
    return want, decisive


def assert_best_rows(got, want, decisive):
    assert got.dtype == np.int32 and got.shape == want.shape
    share = 1.0 - decisive.mean()
    assert share <= 0.02, share
    assert np.array_equal(got[decisive], want[decisive]), np.argwhere(decisive & (got != want))[:5]


@pytest.mark.parametrize("dim,storage", cases([1, 63, 64, 65, 100, 128, 384, 1000, 1024, 4096]))
def test_chunk_best_rows_on_float_data(torch_cuda, dim, storage):
    rng = np.random.default_rng(100 + dim)
    n = 300
    off = ragged_offsets(rng, n, 0, 9)
    n_chunks = len(off) - 1
    assert np.any(np.diff(off) == 0) and np.any(np.diff(off) == 9)
    E = rng.standard_normal((n, dim)).astype(np.float32)
    Q = rng.standard_normal((4, dim)).astype(np.float32)
    cand = rng.integers(0, n_chunks, size=(4, 40)).astype(np.int32)
    want, decisive = best_rows_ref(stored(E, storage), off, Q, cand)
    assert np.sum(want >= 0) > 120
    idx = raglite_amd.DeviceIndex(E, off, metric="dot", storage=storage)
    try:
        got = idx.chunk_best_rows(Q, cand)
        assert_best_rows(got, want, decisive)
        t = idx.chunk_best_rows(torch_cuda.as_tensor(Q, device="cuda"), torch_cuda.as_tensor(cand, device="cuda"))
        assert np.array_equal(t.cpu().numpy(), got)
    finally:
        idx.close()


@pytest.mark.parametrize("dim,storage", [(100, "f32"), (128, "f16")])
def test_chunk_best_rows_special_candidates(torch_cuda, dim, storage):
    """Exact ties give the first row; candidates -1, n_chunks and huge ordinals give -1, and so does an empty chunk."""
    rng = np.random.default_rng(7)
    sizes = [4, 0, 6, 5, 0, 0, 7, 3, 1]
    off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    n_chunks = len(sizes)
    E = stored(rng.standard_normal((int(off[-1]), dim)).astype(np.float32), "f16")  # (exact in both storages)
    Q = rng.standard_normal((2, dim)).astype(np.float32)
    E[off[0]:off[1]] = E[off[0]]                       # chunk 0: four equal rows -> the first
    S = E.astype(np.float64) @ Q.astype(np.float64).T
    r2 = int(off[2] + np.argmax(S[off[2]:off[3], 0]))  # chunk 2: query 0's best row copied to the chunk's last row, if it is not that row
    E[off[3] - 1] = E[r2]
    r3 = int(off[3] + 1 + np.argmax(S[off[3] + 1:off[4], 1]))  # chunk 3: query 1's best row (not the first) copied to the first row
    E[off[3]] = E[r3]
    S = E.astype(np.float64) @ Q.astype(np.float64).T
    assert np.argmax(S[off[2]:off[3], 0]) == r2 - off[2] and np.argmax(S[off[3]:off[4], 1]) == 0 and r3 > off[3]
    cand = np.asarray([[0, 2, 1, -1, n_chunks, INT32_MAX, 4, 8, -INT32_MAX - 1, n_chunks + 1, 6],
                       [0, 3, 5, -1, n_chunks, INT32_MAX, 1, 8, -2, 7, 2]], np.int32)
    want, decisive = best_rows_ref(E, off, Q, cand)
    assert want[0, :2].tolist() == [0, r2] and want[1, :2].tolist() == [0, off[3]] and not decisive[:, 0].any() and not decisive[1, 1]
    assert want[0, 2:9].tolist() == [-1, -1, -1, -1, -1, off[8], -1] and want[1, 2:9].tolist() == [-1, -1, -1, -1, -1, off[8], -1]
    assert decisive[:, 2:].all()  # everything but the planted ties (a zero gap: the first-row rule decides) is clear in float64
    idx = raglite_amd.DeviceIndex(E, off, metric="dot", storage=storage)
    try:
        assert np.array_equal(idx.chunk_best_rows(Q, cand), want)
        assert np.array_equal(idx.chunk_best_rows(Q[0], cand[0]), want[0])
    finally:
        idx.close()


@pytest.mark.parametrize("dim,storage", [(64, "f32"), (128, "f16")])
def test_chunk_best_rows_more_items_than_waves_in_the_grid(torch_cuda, dim, storage):
    """40 x 420 = 16 800 items: past 16 384 a wave takes item `i + 16 384` next."""
    rng = np.random.default_rng(16384)
    n = 2500
    off = ragged_offsets(rng, n, 0, 9)
    n_chunks = len(off) - 1
    E = rng.standard_normal((n, dim)).astype(np.float32)
    Q = rng.standard_normal((40, dim)).astype(np.float32)
    cand = rng.integers(-1, n_chunks + 1, size=(40, 420)).astype(np.int32)
    want, decisive = best_rows_ref(stored(E, storage), off, Q, cand)
    late = want.reshape(-1)[16384:]
    assert np.sum(late >= 0) > 300 and np.sum(late == -1) > 10
    idx = raglite_amd.DeviceIndex(E, off, metric="dot", storage=storage)
    try:
        assert_best_rows(idx.chunk_best_rows(Q, cand), want, decisive)
    finally:
        idx.close()


def assert_gathered(got, E32, rows):
    ok = (rows >= 0) & (rows < len(E32))
    assert got.dtype == np.float32 and got.shape == (len(rows), E32.shape[1])
    assert np.isnan(got[~ok]).all()
    assert got[ok].tobytes() == E32[rows[ok]].tobytes()


@pytest.mark.parametrize("dim,storage", cases([3, 4, 100, 128, 257, 1024]))
def test_gather_rows(torch_cuda, dim, storage):
    """dim % 4 != 0: the scalar path; 4 and 1024: the 16-byte path (f32 storage).  Ordinals below 0 and from n_rows on give NaN rows, the
    rows next to them are intact; values are the stored bits (fp16 storage: widened)."""
    rng = np.random.default_rng(200 + dim)
    n = 90
    E = rng.standard_normal((n, dim)).astype(np.float32)
    E[5, :] = [-0.0, 65504.0, 1e-7][: min(dim, 3)] + [0.0] * max(dim - 3, 0)  # signed zero, the fp16 maximum, an fp16 subnormal
    rows = np.asarray([0, -1, n - 1, n, 5, 5, INT32_MAX, 17, -INT32_MAX - 1, n + 1, 88, 1, -7, 44], np.int32)
    idx = raglite_amd.DeviceIndex(E, metric="dot", storage=storage)
    try:
        got = idx.gather_rows(rows)
        assert_gathered(got, stored(E, storage), rows)
        t = idx.gather_rows(torch_cuda.as_tensor(rows, device="cuda"))
        assert t.cpu().numpy().tobytes() == got.tobytes()
        assert_gathered(idx.gather_rows(rows[:1]), stored(E, storage), rows[:1])
    finally:
        idx.close()


@pytest.mark.parametrize("dim,storage", [(8, "f32"), (128, "f16")])
def test_gather_rows_more_rows_than_waves_in_the_grid(torch_cuda, dim, storage):
    rng = np.random.default_rng(8)
    n = 500
    E = rng.standard_normal((n, dim)).astype(np.float32)
    rows = rng.integers(-3, n + 3, size=16384 + 100).astype(np.int32)
    rows[[16383, 16389, 16483]] = [-1, n, -2]  # NaN rows at the end of the first round, in the second, and last of all
    idx = raglite_amd.DeviceIndex(E, metric="dot", storage=storage)
    try:
        assert_gathered(idx.gather_rows(rows), stored(E, storage), rows)
    finally:
        idx.close()


def test_an_fp16_index_refuses_widths_off_a_multiple_of_128(torch_cuda):
    """Why the fp16 cases above stop at multiples of 128: should this ever pass, give them the other widths too."""
    for dim in (1, 8, 64, 100):
        with pytest.raises(UnsupportedError, match="multiple of 128"):
            raglite_amd.DeviceIndex(np.ones((4, dim), np.float32), metric="dot", storage="f16")
