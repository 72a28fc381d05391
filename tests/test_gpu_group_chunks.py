"""`DeviceIndex.search_chunks` past 256 hits: the `max(sim) GROUP BY chunk` kernel (csrc/select.hip `group_chunk_max_kernel`) walks the hits
256 at a time and carries the number of kept hits from round to round; every two-stage, hybrid and rerank search goes through it.  The hit
lists are PLANTED (tests/long_lists_ref.py: similarity 1 + v_b[r], exact in float32), so each case puts first hits, ties, the k-th kept
hit and repeated chunks where it wants them -- tests/test_long_lists_host.py checks that on the CPU.  Everything is compared bit for
bit with `oracle.topk_desc` + `oracle.group_chunk_max` over the exact similarities: the `search_rows` hits first (so a failure names the
stage), then the grouped scores, chunk ordinals, counts and the (-inf, -1) tail."""

import numpy as np
import pytest
import torch

import raglite_amd
from tests import long_lists_ref as ref

pytestmark = pytest.mark.gpu

NUM_HITS = [1, 255, 256, 257, 511, 512, 513, 1024, 2047, 2048]  # one round, the round edges, all eight rounds
N_NAMED = 6    # the named plants of ref.mixed_plants
N_PLANTS = 17  # ... and random hit orders up to the largest batch


class Case:
    """An index over a planted corpus, with the expected hits of (query, num_hits, filter, limit) computed once."""

    def __init__(self, E, Q, offsets, *, storage="f32", dead=()):
        self.E, self.Q = E, Q
        self.r2c = np.arange(len(E)) if offsets is None else ref.row_to_chunk(offsets)
        self.n_chunks = len(E) if offsets is None else len(offsets) - 1
        self.idx = raglite_amd.DeviceIndex(E, offsets, metric="dot", storage=storage)
        self.live = None
        if len(dead):
            self.idx.delete_chunks(dead)
            self.live = np.ones(self.n_chunks, dtype=bool)
            self.live[list(dead)] = False
        self._hits = {}

    def hits(self, b, num_hits, chunk_ok=None, rank_limit=None):
        key = (b, num_hits, None if chunk_ok is None else chunk_ok.tobytes(), rank_limit or 0)
        if key not in self._hits:
            self._hits[key] = ref.expected_hits(self.E, self.r2c, self.Q[b], num_hits, chunk_ok, rank_limit, self.live)
        return self._hits[key]

    def ks(self, queries, num_hits, filters=None, limits=None):
        """k in {1, one fewer than the distinct chunks among the hits, that number, num_hits, 2048}, for every query of the batch."""
        out = {1, num_hits, ref.K_MAX}
        for j, b in enumerate(queries):
            d = ref.distinct_chunks(self.hits(b, num_hits, filters[j] if filters else None, limits[j] if limits else None)[1], self.r2c)
            out.update((d - 1, d))
        return sorted(k for k in out if 1 <= k <= ref.K_MAX)

    def check(self, queries, num_hits, ks=None, *, chunk_filter=None, query_filters=None, rank_limit=None, device=False):
        """search_rows and search_chunks of the batch Q[queries] against the expected answer, every bit of every slot."""
        idx, Qb, B = self.idx, self.Q[queries], len(queries)
        filters = query_filters if query_filters is not None else [chunk_filter] * B
        limits = list(rank_limit) if np.ndim(rank_limit) else [rank_limit] * B
        ks = self.ks(queries, num_hits, filters, limits) if ks is None else ks
        want = [self.hits(b, num_hits, filters[j], limits[j]) for j, b in enumerate(queries)]
        Qd = torch.as_tensor(Qb, device="cuda") if device else Qb
        if query_filters is None and not np.ndim(rank_limit):
            hs, hr = idx.search_rows(Qd, num_hits, chunk_filter, rank_limit)
            rows = [(_np(hs)[j], _np(hr)[j]) for j in range(B)]
        else:  # (search_rows takes one filter and one limit)
            rows = [idx.search_rows(Qb[j], num_hits, filters[j], limits[j]) for j in range(B)]
        for j, ((ws, wr), (hs, hr)) in enumerate(zip(want, rows)):
            assert np.array_equal(hr, wr), f"search_rows: query {queries[j]} num_hits {num_hits}: rows differ first at {_first(hr, wr)}"
            assert np.array_equal(ref.bits(hs), ref.bits(ws)), f"search_rows: query {queries[j]} num_hits {num_hits}: scores"
        counts = {}
        for k in ks:
            s, c, n = idx.search_chunks(Qd, num_hits, k, chunk_filter, rank_limit, query_filters=query_filters)
            if device:
                assert s.is_cuda and c.is_cuda and n.is_cuda
            s, c, n = _np(s), _np(c), _np(n)
            assert s.shape == c.shape == (B, k) and n.shape == (B,) and s.dtype == np.float32 and c.dtype == n.dtype == np.int32
            for j, (ws, wr) in enumerate(want):
                es, ec, cnt = ref.expected_chunks(ws, wr, self.r2c, k)
                where = f"query {queries[j]} num_hits {num_hits} k {k}"
                assert int(n[j]) == cnt, f"{where}: count {int(n[j])}, expected {cnt}"
                assert np.array_equal(c[j], ec), f"{where}: chunks differ first at slot {_first(c[j], ec)}"
                assert np.array_equal(ref.bits(s[j]), ref.bits(es)), f"{where}: scores differ first at slot {_first(s[j], es)}"
                counts[(queries[j], k)] = cnt
        return counts


def _np(x):
    return x.cpu().numpy() if hasattr(x, "is_cuda") else x


def _first(a, b):
    d = np.nonzero(np.asarray(a) != np.asarray(b))[0]
    return int(d[0]) if len(d) else None


def _plants(rng, n_rows=ref.N_ROWS, top=ref.TOP, floor=-(1 << 19), n=N_PLANTS):
    groups = list(ref.mixed_plants(rng).values())
    while len(groups) < n:  # random hit orders over all chunks: many first hits in every round
        groups.append(rng.permutation(n_rows)[:2048].tolist())
    return [ref.plant(n_rows, g[:top], rng, top, floor) for g in groups[:n]]  # (at most `top` planted values: the last one is 1)


@pytest.fixture(scope="module")
def mixed(torch_cuda):
    """The named plants (queries 0..5) and random hit orders (6..16) over the layout of ref.MIXED_OFFSETS: 402 chunks of 2100, 300, 1 and 3 rows."""
    rng = np.random.default_rng(31)
    E, Q = ref.corpus(_plants(rng), rng)
    case = Case(E, Q, ref.MIXED_OFFSETS)
    yield case
    case.idx.close()


@pytest.fixture(scope="module")
def own_rows(torch_cuda):
    """Every row its own chunk: every hit is kept, `running` carries through all eight rounds."""
    rng = np.random.default_rng(32)
    E, Q = ref.corpus([ref.plant(ref.N_ROWS, rng.permutation(ref.N_ROWS)[:2048].tolist(), rng) for _ in range(5)], rng)
    case = Case(E, Q, None)
    yield case
    case.idx.close()


@pytest.mark.parametrize("num_hits", NUM_HITS)
def test_planted_hit_lists_at_every_round_edge(mixed, num_hits):
    named = list(range(N_NAMED))
    counts = mixed.check(named, num_hits)  # one batch of six queries, each with its own plant
    assert counts[(0, ref.K_MAX)] == 1  # all hits in one chunk
    if num_hits == 2048:  # A, B and 299 one-row chunks; the five round edges; 250 one-row chunks; 60 triples; every chunk
        assert [counts[(b, ref.K_MAX)] for b in named] == [1, 301, 6, 251, 62, 402]
    mixed.check([3], num_hits, [1, 150, 151, ref.K_MAX])  # a single query (another scoring route); k = 150 is reached in the middle of round 2
    mixed.check([5], num_hits, [200, 201, 270, 271, 402])  # the tie runs, cut inside and at their ends


@pytest.mark.parametrize("num_hits", NUM_HITS)
def test_every_row_its_own_chunk(own_rows, num_hits):
    counts = own_rows.check([0, 1, 2, 3, 4], num_hits)
    for (b, k), cnt in counts.items():
        assert cnt == min(k, num_hits)
    own_rows.check([1], num_hits, sorted({1, max(num_hits - 1, 1), num_hits, ref.K_MAX}))


@pytest.mark.parametrize("B", [1, 5, 17])
def test_batches_where_each_query_carries_its_own_plant(mixed, B):
    queries = list(range(N_PLANTS - B, N_PLANTS)) if B < N_PLANTS else list(range(N_PLANTS))
    for num_hits in (257, 2048):
        counts = mixed.check(queries, num_hits, [1, 150, num_hits, ref.K_MAX])
        assert all(cnt > 20 for (b, k), cnt in counts.items() if k == ref.K_MAX and b >= N_NAMED)  # random orders: first hits in every round
    named = list(range(min(B, N_NAMED)))
    mixed.check(named, 1024, [1, 7, 300, 1024])


def test_device_tensors_in_and_out(mixed):
    for num_hits in (257, 2048):
        mixed.check(list(range(N_NAMED)), num_hits, [1, 150, 402, ref.K_MAX], device=True)
    mixed.check([4], 513, [61, 62, 513], device=True)


def test_short_lists_filters_and_limits(mixed, torch_cuda):
    named = list(range(N_NAMED))
    n_chunks = mixed.n_chunks
    ok270 = np.zeros(n_chunks, dtype=bool)
    ok270[2:272] = True  # 270 one-row chunks: 270 matching rows, fewer than num_hits
    for num_hits in (257, 2048):
        counts = mixed.check(named, num_hits, chunk_filter=ok270)
        assert all(cnt == min(k, 257 if num_hits == 257 else 270) for (b, k), cnt in counts.items())
    # per query: no filter, the 270 rows, a filter that leaves nothing, every third chunk, chunks A and B alone, no filter
    third = np.arange(n_chunks) % 3 == 0
    only_ab = np.zeros(n_chunks, dtype=bool)
    only_ab[:2] = True
    qf = [None, ok270, np.zeros(n_chunks, dtype=bool), third, only_ab, None]
    for num_hits in (300, 2048):
        counts = mixed.check(named, num_hits, query_filters=qf)
        assert all(cnt == 0 for (b, k), cnt in counts.items() if b == 2)
        assert counts[(4, ref.K_MAX)] == (2 if num_hits == 2048 else 1)  # (its first 300 matching hits are all rows of chunk B)
    mixed.check(named, 1024, [1, 270, 2048], query_filters=qf, device=True)
    # a rank limit below num_hits: only the 300 (700, 10, ...) nearest rows are eligible, the rest of the list is padding
    mixed.check(named, 1024, rank_limit=300)
    mixed.check(named, 2048, rank_limit=[0, 300, 10, 700, 257, 2047])
    mixed.check(named, 2048, [1, 100, 2048], query_filters=[third, None, only_ab, None, third, ok270], rank_limit=[900, 0, 2300, 512, 0, 2500])
    # fewer rows than num_hits: 300 rows in chunks of 1..3, num_hits = 2048
    rng = np.random.default_rng(33)
    sizes = []
    while sum(sizes) < 300:
        sizes.append(min(int(rng.integers(1, 4)), 300 - sum(sizes)))
    E, Q = ref.corpus([ref.plant(300, rng.permutation(300).tolist(), rng) for _ in range(5)], rng)
    small = Case(E, Q, ref.offsets_from_sizes(sizes))
    try:
        for queries in ([0, 1, 2, 3, 4], [2]):
            counts = small.check(queries, 2048)
            assert all(cnt == min(k, len(sizes)) for (b, k), cnt in counts.items())
            small.check(queries, 299)
    finally:
        small.idx.close()


def test_tombstoned_chunks(torch_cuda):
    """Chunk A (2100 rows), every fifth one-row chunk and the first ten triples deleted: the hits skip their rows; 900 - 60 - 30 rows stay."""
    rng = np.random.default_rng(31)
    E, Q = ref.corpus(_plants(rng, n=N_NAMED), rng)
    dead = [0] + list(range(2, 302, 5)) + list(range(302, 312))
    case = Case(E, Q, ref.MIXED_OFFSETS, dead=dead)
    try:
        named = list(range(N_NAMED))
        for num_hits in (257, 513, 2048):
            counts = case.check(named, num_hits)
            assert counts[(0, ref.K_MAX)] > 100  # (query 0 planted chunk A alone: whatever ranks next)
        hs, hr = case.idx.search_rows(Q[:N_NAMED], 2048)
        assert ((hr >= 0).sum(axis=1) == 900 - 60 - 30).all() and not np.isin(case.r2c[hr[hr >= 0]], dead).any()
        case.check(named, 2048, [1, 50, 2048], rank_limit=400)
        third = np.arange(case.n_chunks) % 3 == 0
        case.check(named, 1024, [1, 50, 1024], chunk_filter=third)
    finally:
        case.idx.close()


def test_fp16_stored_index_of_dim_128(torch_cuda):
    """Planted values up to 2048, which fp16 holds exactly: the same answers from an fp16-stored index."""
    rng = np.random.default_rng(34)
    E, Q = ref.corpus(_plants(rng, top=2048, floor=-2048, n=N_NAMED), rng, dim=128)
    assert np.array_equal(E.astype(np.float16).astype(np.float32), E)
    case = Case(E, Q, ref.MIXED_OFFSETS, storage="f16")
    try:
        named = list(range(N_NAMED))
        for num_hits in (256, 257, 2048):
            case.check(named, num_hits)
        case.check([2], 2048)
        case.check(named, 2048, [1, 150, 2048], device=True)
    finally:
        case.idx.close()
