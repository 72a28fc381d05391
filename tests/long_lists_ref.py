"""Result lists past 256 hits: planted corpora, the expected two-stage answer and a merge restatement (test infrastructure, NumPy only).

A planted-score corpus lets a test DICTATE the hit list of a query.  Metric "dot", query b is the one-hot e_b, column b of E holds
integers v_b[r] with |v| < 2^20 and the other columns small random integers, so the similarity of row r to query b is exactly
1 + v_b[r] in float32 (`tests/util.sim_fp32_exact`) whatever kernel computes it.  `plant` turns a wanted hit sequence into v_b;
`mixed_plants` names the sequences the grouping kernel (`group_chunk_max_kernel`, csrc/select.hip) is held against on the `MIXED_OFFSETS`
layout, and tests/test_long_lists_host.py checks on the CPU that each one puts its hits where its name says.

The expected answer is the oracle's: `oracle.topk_desc` over the exact similarities, then `oracle.group_chunk_max`.

`merge_ref` restates `rl_merge_topk` by an explicit Python sort on (key, id), `score_key` being the device's order on score bits
(csrc/common.h): NaN last, +0.0 before -0.0."""

import functools

import numpy as np

from oracle import oracle

DIM = 64
N_ROWS = 3000
TOP = 1 << 19  # the first planted hit's value; unplanted rows lie below zero
K_MAX = 2048

# ---- the chunk layouts --------------------------------------------------------------------------------------------------------------


def offsets_from_sizes(sizes) -> np.ndarray:
    """Contiguous chunk offsets (n_chunks + 1,) int64 from rows per chunk."""
    return np.concatenate(([0], np.cumsum(np.asarray(sizes, dtype=np.int64)))).astype(np.int64)


# chunk A = rows [0, 2100), chunk B = rows [2100, 2400), 300 one-row chunks (rows 2400..2699), 100 three-row chunks (rows 2700..2999)
MIXED_SIZES = [2100, 300] + [1] * 300 + [3] * 100
MIXED_OFFSETS = offsets_from_sizes(MIXED_SIZES)
A_ROWS = np.arange(0, 2100)
B_ROWS = np.arange(2100, 2400)
SINGLE_ROWS = np.arange(2400, 2700)          # row r is chunk r - 2398
TRIPLE_ROWS = np.arange(2700, 3000).reshape(100, 3)  # triple t is chunk 302 + t


def row_to_chunk(offsets) -> np.ndarray:
    off = np.asarray(offsets, dtype=np.int64)
    return np.repeat(np.arange(len(off) - 1), np.diff(off))


# ---- planting -------------------------------------------------------------------------------------------------------------------------


def plant(n_rows: int, groups, rng, top: int = TOP, floor: int = -(1 << 19)) -> np.ndarray:
    """v (n_rows,) int64 such that the hits of the query are the rows of groups[0], then those of groups[1], ...: group g gets the one
    value top - g, so a group of several rows is a run of TIED hits (which the search returns in ascending row order); rows in no
    group get random values in [floor, 0), below every planted one.  A group is a row or a sequence of rows."""
    v = rng.integers(floor, 0, size=n_rows).astype(np.int64)
    seen = np.zeros(n_rows, dtype=bool)
    assert len(groups) <= top  # the last planted value is still positive
    for g, rows in enumerate(groups):
        rows = np.atleast_1d(np.asarray(rows, dtype=np.int64))
        assert not seen[rows].any(), "a row is planted once"
        seen[rows] = True
        v[rows] = top - g
    assert np.abs(v).max() < (1 << 20)
    return v


def corpus(plants, rng, dim: int = DIM, lo: int = -3, hi: int = 3) -> tuple[np.ndarray, np.ndarray]:
    """(E (n_rows, dim) float32, Q (B, dim) float32): column b of E is plants[b], the rest random integers in [lo, hi]; Q[b] = e_b."""
    n_rows, B = len(plants[0]), len(plants)
    assert B <= dim
    E = rng.integers(lo, hi + 1, size=(n_rows, dim)).astype(np.float32)
    for b, v in enumerate(plants):
        E[:, b] = np.asarray(v, dtype=np.float32)
    return E, np.eye(B, dim, dtype=np.float32)


def _filler(rows, used):
    """Iterator over `rows` minus the set `used`."""
    return iter([r for r in rows.tolist() if r not in used])


def _sequence(length, fixed, filler_rows):
    """A hit sequence of `length` rows: position p holds fixed[p] where given, the next unused filler row elsewhere."""
    used = set(fixed.values())
    fill = _filler(filler_rows, used)
    return [fixed[p] if p in fixed else next(fill) for p in range(length)]


def mixed_plants(rng) -> dict[str, list]:
    """name -> groups (for `plant`) over the MIXED_OFFSETS layout; tests/test_long_lists_host.py states what each name promises."""
    S, T = SINGLE_ROWS.tolist(), TRIPLE_ROWS
    out = {}
    # every one of the 2048 best hits lies in chunk A
    out["one_chunk"] = A_ROWS[rng.permutation(2100)[:2048]].tolist()
    # chunk A owns hits 0..299, chunk B's first hit is hit 300; after that A, B and one-row chunks alternate
    tail = [x for trio in zip(A_ROWS[300:800].tolist(), B_ROWS.tolist()[1:], S) for x in trio]
    out["a_then_b_at_300"] = A_ROWS[:300].tolist() + [int(B_ROWS[0])] + tail + A_ROWS[800:2100].tolist()
    # first hits of new chunks exactly at 255, 256, 511, 512 and 2047 (hit 0 opens chunk A, which fills the rest)
    out["first_hits_at_round_edges"] = _sequence(2048, {255: S[10], 256: S[3], 511: S[200], 512: S[100], 2047: S[7]}, A_ROWS)
    # k = 150 is reached in the middle of round 2 (hits 512..767): 50 new chunks in round 0, 50 in round 1, 100 at hits 640..739, 50 more at 1000..
    fixed = {p: S[p] for p in range(50)}
    fixed.update({256 + p: S[50 + p] for p in range(50)})
    fixed.update({640 + p: S[100 + p] for p in range(100)})
    fixed.update({1000 + p: S[200 + p] for p in range(50)})
    out["k_reached_mid_round_2"] = _sequence(2048, fixed, A_ROWS)
    # look-back across round boundaries: the three rows of triple t lie at hits 10 + t, 300 + t and 1900 + t; B rows fill
    fixed = {}
    for t in range(60):
        fixed[10 + t], fixed[300 + t], fixed[1900 + t] = (int(x) for x in T[t])
    out["look_back_across_rounds"] = _sequence(2048, fixed, np.concatenate((B_ROWS, A_ROWS)))
    # equal scores across chunks: hits 200..329 are ONE tie over triples and one-row chunks (a run across the first round boundary, several
    # rows of one chunk inside it), hits 330..999 a second tie over every other chunk (100 rows of A, all of B, the remaining one-row and
    # three-row chunks); hits 0..199 are distinct one-row chunks
    run = sorted(T[40:70].ravel().tolist() + S[250:290])
    rest = sorted(set(range(N_ROWS)) - set(run) - set(S[:200]) - set(A_ROWS[100:].tolist()))
    out["ties_across_chunks"] = [[r] for r in S[:200]] + [run, rest]
    return out


def group_sequence(groups) -> list[int]:
    """The hit order a list of groups promises: groups in order, the rows of a tied group ascending."""
    seq = []
    for g in groups:
        seq.extend(sorted(np.atleast_1d(np.asarray(g)).tolist()))
    return seq


# ---- the expected answer ----------------------------------------------------------------------------------------------------------------


def pad_list(scores, ids, k):
    """(scores (k,) float32, ids (k,) int32) with the (-inf, -1) tail."""
    s = np.full(k, -np.inf, dtype=np.float32)
    i = np.full(k, -1, dtype=np.int32)
    n = min(len(ids), k)
    s[:n], i[:n] = np.asarray(scores, dtype=np.float32)[:n], np.asarray(ids)[:n]
    return s, i


def expected_hits(E, r2c, q, num_hits, chunk_ok=None, rank_limit=None, live=None):
    """What `search_rows(q, num_hits, ...)` must return: (scores (num_hits,) float32, rows (num_hits,) int32), padding (-inf, -1).
    chunk_ok: the filter; live: the chunks not tombstoned; rank_limit: the order-first cut (`oracle.search_rows_ranked`)."""
    n_chunks = int(r2c.max()) + 1 if len(r2c) else 0
    ok = np.ones(n_chunks, dtype=bool) if chunk_ok is None else np.asarray(chunk_ok, dtype=bool)
    alive = np.ones(n_chunks, dtype=bool) if live is None else np.asarray(live, dtype=bool)
    if rank_limit:
        s, rows = oracle.search_rows_ranked(E, r2c, q, num_hits, ok, rank_limit, alive, "dot")
    else:
        s, rows = oracle.search_rows_filtered(E, r2c, q, num_hits, ok & alive, "dot")
    assert np.array_equal(s.astype(np.float32).astype(np.float64), s)  # exact in float32
    keep = rows >= 0
    return pad_list(s[keep], rows[keep], num_hits)


def expected_chunks(hit_scores, hit_rows, r2c, k):
    """`oracle.group_chunk_max` over expected hits -> (scores (k,) float32, chunk ordinals (k,) int32, count) with the (-inf, -1) tail."""
    keep = hit_rows >= 0
    s, c = oracle.group_chunk_max(hit_scores[keep], r2c[hit_rows[keep]], k)
    return (*pad_list(s, c, k), len(c))


def distinct_chunks(hit_rows, r2c) -> int:
    keep = hit_rows >= 0
    return len(set(r2c[hit_rows[keep]].tolist()))


def first_hit_positions(hit_rows, r2c) -> dict[int, int]:
    """chunk ordinal -> position of its first hit."""
    first = {}
    for p, r in enumerate(hit_rows.tolist()):
        if r >= 0:
            first.setdefault(int(r2c[r]), p)
    return first


# ---- rl_merge_topk restated -----------------------------------------------------------------------------------------------------------


def score_key(x) -> np.ndarray:
    """The device's monotone map float32 -> uint32 (csrc/common.h `score_key`): larger score <=> larger key, every NaN -> 0."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return np.where((u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), np.uint32(0), key).astype(np.uint32)


NAN_BITS = 0x7FC00000  # the one NaN the selection kernels write (every NaN has key 0: its payload is not kept)


def merge_ref(scores, ids, k):
    """`rl_merge_topk`: scores / ids (n_lists, B, k_in), id < 0 = padding -> (scores (B, k) float32, ids (B, k) int32): per query the
    entries with id >= 0 sorted by (key desc, id asc), the first k of them, then (-inf, -1).  Plain Python sorting of tuples."""
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    ids = np.asarray(ids)
    n_lists, B, k_in = scores.shape
    keys, bits = score_key(scores), scores.view(np.uint32)
    out_s = np.full((B, k), -np.inf, dtype=np.float32)
    out_i = np.full((B, k), -1, dtype=np.int32)
    for b in range(B):
        entries = [(-key, i, u) for key, i, u in zip(keys[:, b].ravel().tolist(), ids[:, b].ravel().tolist(), bits[:, b].ravel().tolist())
                   if i >= 0]
        entries.sort(key=lambda e: (e[0], e[1]))
        for p, (nk, i, u) in enumerate(entries[:k]):
            out_s.view(np.uint32)[b, p] = NAN_BITS if nk == 0 else u
            out_i[b, p] = i
    return out_s, out_i


def _before(a, b) -> int:
    """Comparator of two (score, id) entries by the stated rule, no key involved: a real score before NaN; the larger score first;
    +0.0 before -0.0; then the lower id."""
    (sa, ia), (sb, ib) = a, b
    na, nb = bool(np.isnan(sa)), bool(np.isnan(sb))
    if na != nb:
        return -1 if nb else 1
    if not na:
        if sa > sb:
            return -1
        if sa < sb:
            return 1
        za, zb = bool(np.signbit(sa)), bool(np.signbit(sb))
        if sa == 0 and za != zb:
            return -1 if zb else 1
    return -1 if ia < ib else (1 if ia > ib else 0)


def merge_brute(scores, ids, k):
    """`merge_ref`'s answer by a comparison sort under `_before` (the rule in words); small inputs only."""
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    ids = np.asarray(ids)
    n_lists, B, k_in = scores.shape
    out_s = np.full((B, k), -np.inf, dtype=np.float32)
    out_i = np.full((B, k), -1, dtype=np.int32)
    for b in range(B):
        entries = [(scores[l, b, j], int(ids[l, b, j])) for l in range(n_lists) for j in range(k_in) if ids[l, b, j] >= 0]
        entries.sort(key=functools.cmp_to_key(_before))
        for p, (s, i) in enumerate(entries[:k]):
            out_s[b, p] = np.float32(np.nan) if np.isnan(s) else s
            out_i[b, p] = i
    out_s.view(np.uint32)[np.isnan(out_s)] = NAN_BITS
    return out_s, out_i


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


SPECIALS = np.array([np.nan, -np.nan, np.inf, -np.inf, np.finfo(np.float32).max, -np.finfo(np.float32).max, np.finfo(np.float32).tiny,
                     -np.finfo(np.float32).tiny, 1e-45, -1e-45, 3e-39, -3e-39, 0.0, -0.0, 1.0, -1.0], dtype=np.float32)


def merge_contents(rng, n_lists, B, k_in) -> dict[str, tuple[np.ndarray, np.ndarray]]:
    """name -> (scores, ids) of shape (n_lists, B, k_in): the contents `rl_merge_topk` is held against."""
    shape, total = (n_lists, B, k_in), n_lists * k_in

    def distinct_ids(spread=4):
        """ids distinct within a query, scattered over the lists (per query a random sample of [0, spread * total))."""
        ids = np.stack([rng.permutation(spread * total)[:total] for _ in range(B)])  # (B, total)
        return np.ascontiguousarray(ids.reshape(B, n_lists, k_in).transpose(1, 0, 2)).astype(np.int32)

    out = {}
    normal = rng.standard_normal(shape).astype(np.float32)
    out["normal"] = (normal, distinct_ids())
    out["three_values"] = (rng.integers(0, 3, size=shape).astype(np.float32), distinct_ids())
    ids = distinct_ids()
    ids[rng.random(shape) < 0.3] = -1
    out["padding_scattered"] = (normal, ids)
    ids = distinct_ids()
    ids[n_lists // 2] = -1
    out["one_list_padding"] = (normal, ids)
    out["all_padding"] = (normal, np.full(shape, -1, dtype=np.int32))
    out["specials"] = (rng.choice(SPECIALS, size=shape), distinct_ids())
    # a block of +-0.0 with interleaved ids: odd ids hold -0.0, even ids +0.0 (the lowest id is a -0.0 wherever id 1 is present)
    ids = distinct_ids(spread=1)
    zeros = np.where(ids % 2 == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    mixed = np.where(rng.random(shape) < 0.8, zeros, rng.integers(-1, 2, size=shape).astype(np.float32)).astype(np.float32)
    out["signed_zeros"] = (mixed, ids)
    return out
