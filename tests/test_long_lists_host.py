"""tests/long_lists_ref.py on the CPU: every planted case puts its hits where its name promises (so no GPU case can silently
degenerate), the merge restatement equals a brute-force comparison sort, and the host merges follow the device's signed-zero rule
(include/raglite_hip.h, rl_topk / rl_merge_topk: +0.0 ranks before -0.0 whatever the ids)."""

import numpy as np
import pytest

from oracle import oracle
from raglite_amd import _sharded
from raglite_amd._sharded import merge_topk_host
from tests import long_lists_ref as ref
from tests.util import sim_fp32_exact


@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(31)
    groups = ref.mixed_plants(rng)
    plants = [ref.plant(ref.N_ROWS, g, rng) for g in groups.values()]
    E, Q = ref.corpus(plants, rng)
    r2c = ref.row_to_chunk(ref.MIXED_OFFSETS)
    hits = {name: ref.expected_hits(E, r2c, Q[b], 2048) for b, name in enumerate(groups)}
    return groups, E, Q, r2c, hits


def test_planted_similarities_are_exact_and_dictate_the_hit_list(mixed):
    groups, E, Q, r2c, hits = mixed
    assert len(r2c) == ref.N_ROWS and int(ref.MIXED_OFFSETS[-1]) == ref.N_ROWS
    for b, (name, g) in enumerate(groups.items()):
        sims = sim_fp32_exact(E, Q[b], "dot")
        assert np.array_equal(sims, (1 + E[:, b].astype(np.int64)).astype(np.float32)), name  # 1 + v_b[r], exactly
        s, rows = hits[name]
        want = ref.group_sequence(g)[:2048]
        assert len(want) >= 1000 and rows[: len(want)].tolist() == want, name
        assert np.array_equal(s, sims[rows]) and np.all(np.diff(s) <= 0), name
        es, er = oracle.topk_desc(sims, 2048)
        assert np.array_equal(er, rows) and np.array_equal(es, s), name


def test_each_plant_keeps_its_promise(mixed):
    groups, E, Q, r2c, hits = mixed
    first = {name: ref.first_hit_positions(hits[name][1], r2c) for name in groups}
    S = ref.SINGLE_ROWS
    # all 2048 hits in one chunk
    assert first["one_chunk"] == {0: 0}
    # A owns hits 0..299, B's first hit is hit 300, and more chunks follow
    f = first["a_then_b_at_300"]
    assert f[0] == 0 and f[1] == 300 and sorted(f.values())[:3] == [0, 300, 303] and len(f) > 300
    assert (r2c[hits["a_then_b_at_300"][1][:300]] == 0).all()
    # first hits exactly at the round edges
    f = first["first_hits_at_round_edges"]
    assert sorted(f.values()) == [0, 255, 256, 511, 512, 2047]
    assert [c for c, _ in sorted(f.items(), key=lambda kv: kv[1])] == [0] + [int(r2c[S[i]]) for i in (10, 3, 200, 100, 7)]
    # k = 150 lies in the middle of round 2, with kept hits before it in rounds 0 and 1 and first hits after it in rounds 2 and 3
    pos = sorted(first["k_reached_mid_round_2"].values())
    assert len(pos) == 251 and 512 < pos[149] < 767 and pos[149] == 640 + 48  # (chunk A opens at the first filler hit, hit 50)
    assert sum(p < 256 for p in pos) == 51 and sum(256 <= p < 512 for p in pos) == 50 and pos[150] == pos[149] + 1 and pos[-1] > 1000
    # every triple's chunk is opened in round 0 and met again in rounds 1 and 7
    rows = hits["look_back_across_rounds"][1]
    for t in range(60):
        c = 302 + t
        where = np.nonzero(r2c[rows] == c)[0].tolist()
        assert where == [10 + t, 300 + t, 1900 + t] and first["look_back_across_rounds"][c] == 10 + t
    # ties across chunks: one score over hits 200..329 (across the round boundary at 256), chunk ordinals ascending, repeated chunks inside
    s, rows = hits["ties_across_chunks"]
    assert len(set(s[200:330].tolist())) == 1 and s[199] > s[200] > s[330] and len(set(s[330:1000].tolist())) == 1 and s[999] > s[1000]
    run_chunks = r2c[rows[200:330]]
    assert np.all(np.diff(run_chunks) >= 0) and len(set(run_chunks.tolist())) == 70 and np.all(np.diff(rows[200:330]) > 0)
    ws, wc, n = ref.expected_chunks(s, rows, r2c, 2048)
    assert n == 402 and np.all(np.diff(wc[200:270]) > 0)
    assert wc[270:272].tolist() == [0, 1] and np.all(np.diff(wc[270:402]) > 0)  # the second tie: chunks A and B, then every remaining chunk


def test_expected_chunks_pads_and_counts(mixed):
    groups, E, Q, r2c, hits = mixed
    s, rows = hits["first_hits_at_round_edges"]
    for k, n in ((1, 1), (5, 5), (6, 6), (7, 6), (2048, 6)):
        ws, wc, cnt = ref.expected_chunks(s, rows, r2c, k)
        assert cnt == n and ws.shape == wc.shape == (k,) and ws.dtype == np.float32 and wc.dtype == np.int32
        assert (wc[cnt:] == -1).all() and np.isneginf(ws[cnt:]).all() and ws[0] == s[0] and wc[0] == 0
    assert ref.distinct_chunks(rows, r2c) == 6 and ref.distinct_chunks(rows[:256], r2c) == 2
    # the same grouping as the sharded path's host restatement, bit for bit
    hs, hc, hn = _sharded.group_chunk_max_host(s[None, :], r2c[rows][None, :], 7)
    ws, wc, cnt = ref.expected_chunks(s, rows, r2c, 7)
    assert hn[0] == cnt and np.array_equal(hc[0], wc) and np.array_equal(ref.bits(hs[0]), ref.bits(ws))
    # short lists: fewer matching rows than num_hits, a cut below num_hits, tombstones
    ok = np.zeros(402, dtype=bool)
    ok[2:272] = True  # 270 one-row chunks
    fs, fr = ref.expected_hits(E, r2c, Q[0], 2048, chunk_ok=ok)
    assert (fr[:270] >= 0).all() and (fr[270:] == -1).all() and np.isneginf(fs[270:]).all() and set(r2c[fr[:270]].tolist()) == set(range(2, 272))
    cs, cr = ref.expected_hits(E, r2c, Q[2], 2048, rank_limit=300)
    assert (cr[:300] >= 0).all() and (cr[300:] == -1).all() and np.array_equal(cr[:300], rows[:300])
    live = np.ones(402, dtype=bool)
    live[0] = False
    ts, tr = ref.expected_hits(E, r2c, Q[2], 2048, live=live)
    assert (r2c[tr[tr >= 0]] != 0).all() and (tr[:900] >= 0).all() and (tr[900:] == -1).all()


# ---- the merge restatement ------------------------------------------------------------------------------------------------------------
def test_score_key_is_the_total_order_on_bits():
    x = np.array([np.inf, 3.4e38, 1.0, 1e-45, 0.0, -0.0, -1e-45, -1.0, -3.4e38, -np.inf, np.nan, -np.nan], dtype=np.float32)
    k = ref.score_key(x).astype(np.int64)
    assert np.all(np.diff(k[:10]) < 0) and k[10] == 0 and k[11] == 0 and k[9] > 0


@pytest.mark.parametrize("n_lists,B,k_in", [(1, 1, 1), (1, 3, 65), (2, 5, 100), (3, 7, 33), (64, 2, 8)])
def test_merge_ref_equals_the_brute_force_sort(n_lists, B, k_in):
    rng = np.random.default_rng(n_lists * 1000 + k_in)
    total = n_lists * k_in
    for name, (s, i) in ref.merge_contents(rng, n_lists, B, k_in).items():
        for k in sorted({1, min(5, total), total, total + 3}):
            rs, ri = ref.merge_ref(s, i, k)
            bs, bi = ref.merge_brute(s, i, k)
            assert np.array_equal(ri, bi) and np.array_equal(ref.bits(rs), ref.bits(bs)), (name, k)
            n_valid = np.minimum((i >= 0).sum(axis=(0, 2)), k)
            assert all((ri[b, : n_valid[b]] >= 0).all() and (ri[b, n_valid[b]:] == -1).all() for b in range(B)), (name, k)
            # the host merge: the same ids, and the same scores (it hands a NaN's own payload through, the device writes one NaN)
            hs, hi = merge_topk_host(s, i, k)
            if name == "signed_zeros" and total > 1:
                assert (s == 0).any() and np.signbit(s[s == 0]).any() and not np.signbit(s[s == 0]).all()
            assert np.array_equal(hi, ri), (name, k)
            assert np.array_equal(np.isnan(hs), np.isnan(rs)) and np.array_equal(ref.bits(hs)[~np.isnan(hs)], ref.bits(rs)[~np.isnan(rs)]), (name, k)
            ts, ti = _torch_merge(s, i, k)
            assert np.array_equal(ti, ri), (name, k)


def _torch_merge(s, i, k):
    import torch

    n_lists, B, k_in = s.shape
    fs = torch.from_numpy(np.ascontiguousarray(np.transpose(s, (1, 0, 2))).reshape(B, -1))
    fi = torch.from_numpy(np.ascontiguousarray(np.transpose(i, (1, 0, 2))).reshape(B, -1).astype(np.int64))
    order, n_valid = _sharded.merge_order_torch(fs, fi, k)
    ids = fi.gather(1, order)
    ids[torch.arange(order.shape[1])[None, :] >= n_valid[:, None]] = -1
    out = np.full((B, k), -1, dtype=np.int64)
    out[:, : order.shape[1]] = ids.numpy()
    return None, out


def test_signed_zeros_rank_by_the_key_on_the_host():
    """The device's key puts +0.0 before -0.0 whatever the ids; the host restatements follow it."""
    s = np.array([-0.0, 0.0], dtype=np.float32).reshape(1, 1, 2)
    i = np.array([3, 7], dtype=np.int32).reshape(1, 1, 2)
    hs, hi = merge_topk_host(s, i, 2)
    assert hi.tolist() == [[7, 3]] and ref.bits(hs).tolist() == [[0x00000000, 0x80000000]]
    assert ref.merge_ref(s, i, 2)[1].tolist() == [[7, 3]] and ref.merge_brute(s, i, 2)[1].tolist() == [[7, 3]]
    es, ei = oracle.topk_desc(np.array([-0.0, 1.0, 0.0, -0.0, 0.0, -1.0], dtype=np.float32), 6)
    assert ei.tolist() == [1, 2, 4, 0, 3, 5] and ref.bits(es).tolist() == [0x3F800000, 0, 0, 0x80000000, 0x80000000, 0xBF800000]
    ms, mi = oracle.merge_topk([np.array([-0.0], np.float32), np.array([0.0], np.float32)], [np.array([3]), np.array([7])], 2)
    assert mi.tolist() == [7, 3]
    order, n_valid = _sharded._merge_order(s.reshape(1, 2), i.reshape(1, 2).astype(np.int64), 2)
    assert order.tolist() == [[1, 0]] and n_valid.tolist() == [2]
    # a padding slot's score is ignored, signed zero or not
    order, n_valid = _sharded._merge_order(np.array([[-0.0, 0.0, -0.0]], np.float32), np.array([[5, -1, 2]], np.int64), 3)
    assert order.tolist() == [[2, 0, 1]] and n_valid.tolist() == [2]
