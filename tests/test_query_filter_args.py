"""Per-query metadata filters, without a GPU: the arguments of rl_search_chunks_per_query, rl_keyword_search_per_query
and rl_hybrid_search_per_query that need no index are checked before the index is looked at, and the host plan of a batch's filters
(`_ops.filter_set`, `_search.plan_filters`) holds against a plain loop."""

import ctypes as C

import numpy as np
import pytest

from raglite_amd import _abi, _ops, _search

B = 3
ENTRIES = {"chunks": "rl_search_chunks_per_query", "keyword": "rl_keyword_search_per_query", "hybrid": "rl_hybrid_search_per_query"}


def _arr(ctype, values):
    return (ctype * len(values))(*values)


def _call(entry, filters, n_filters, query_filter, rank_limits):
    """The entry point with a null index and this set of per-query arguments; everything else valid-looking."""
    lib = _abi.lib()
    q = _arr(C.c_float, [0.0] * 8)
    out_f = _arr(C.c_float, [0.0] * 8)
    out_d = _arr(C.c_double, [0.0] * 8)
    out_i = _arr(C.c_int32, [0] * 8)
    out_n = _arr(C.c_int32, [0] * B)
    q_off = _arr(C.c_int64, [0, 1, 2, 3])
    q_terms = _arr(C.c_int32, [0, 1, 2])
    if entry == "chunks":
        return lib.rl_search_chunks_per_query(None, q, B, 4, 2, filters, n_filters, query_filter, rank_limits, out_f, out_i, out_n,
                                              _abi.MEM_HOST, None)
    if entry == "keyword":
        return lib.rl_keyword_search_per_query(None, q_off, q_terms, B, 2, filters, n_filters, query_filter, out_f, out_i, out_n,
                                               _abi.MEM_HOST, None)
    w = _arr(C.c_double, [0.75, 0.25])
    return lib.rl_hybrid_search_per_query(None, None, q, B, 4, 2, q_off, q_terms, filters, n_filters, query_filter, rank_limits, w, 60, 2,
                                          out_d, out_i, out_n, _abi.MEM_HOST, None)


BITS = _arr(C.c_uint32, [0xFFFFFFFF] * 4)
CASES = [  # (chunk_filters, n_filters, query_filter, rank_limits, what the message names)
    (BITS, -1, None, None, "n_filters"),
    (None, 2, _arr(C.c_int32, [0, 1, -1]), None, "chunk_filters"),
    (BITS, 2, _arr(C.c_int32, [0, 2, -1]), None, "query_filter[1]"),
    (BITS, 2, _arr(C.c_int32, [0, -2, 1]), None, "query_filter[1]"),
    (None, 0, _arr(C.c_int32, [-1, -1, 0]), None, "query_filter[2]"),
    (BITS, 1, _arr(C.c_int32, [0, 0, 0]), _arr(C.c_int64, [0, 5, -1]), "rank_limits[2]"),
]


@pytest.mark.parametrize(("entry", "case"), [(e, c) for e in sorted(ENTRIES) for c in range(len(CASES))
                                             if not (e == "keyword" and CASES[c][3] is not None)])  # (no rank limits in the keyword call)
def test_invalid_per_query_arguments_are_named_before_the_index(entry, case):
    filters, n_filters, query_filter, rank_limits, name = CASES[case]
    assert _call(entry, filters, n_filters, query_filter, rank_limits) == _abi.RL_ERR_INVALID
    msg = _abi.last_error()
    assert msg.startswith(ENTRIES[entry]) and name in msg, msg


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_valid_per_query_arguments_reach_the_index_check(entry):
    rank_limits = _arr(C.c_int64, [0, 5, 1 << 40])
    for filters, n_filters, query_filter in ((BITS, 2, _arr(C.c_int32, [0, 1, -1])), (None, 0, None), (BITS, 1, None)):
        assert _call(entry, filters, n_filters, query_filter, rank_limits) == _abi.RL_ERR_INVALID
        assert "null index" in _abi.last_error()


def test_filter_set_dedups_by_packed_bytes():
    rng = np.random.default_rng(0)
    n = 77
    pool = [rng.random(n) < p for p in (0.0, 0.01, 0.5, 1.0)] + [np.zeros(n, bool)]  # (all clear twice, as two objects)
    entries = [None if i % 5 == 4 else pool[int(rng.integers(len(pool)))] for i in range(40)]
    entries[3] = _ops.pack_bits(pool[2])  # a filter already packed
    entries[6] = list(pool[1])  # and one as a plain list
    table, qf = _ops.filter_set(entries, n, len(entries))
    assert table.dtype == np.uint32 and table.shape[1] == (n + 31) // 32
    assert len({row.tobytes() for row in table}) == len(table)  # each distinct filter once
    for b, e in enumerate(entries):  # a plain loop: every query reads its own bits
        if e is None:
            assert qf[b] == -1
        else:
            assert np.array_equal(table[qf[b]], _ops.pack_bits(e))
    assert _ops.filter_set([None] * 3, n, 3)[0].shape == (0, 3)
    with pytest.raises(ValueError, match="one entry per query"):
        _ops.filter_set(entries, n, len(entries) + 1)
    with pytest.raises(ValueError, match="one entry per chunk"):
        _ops.filter_set([np.ones(n + 40, bool)], n, 1)


def test_rank_limits_argument():
    assert _ops._rank_limits(None, 4) is None  # noqa: SLF001
    assert _ops._rank_limits(0, 4) is None  # noqa: SLF001
    assert _ops._rank_limits(7, 3).tolist() == [7, 7, 7]  # noqa: SLF001
    assert _ops._rank_limits([None, 5, 0], 3).tolist() == [0, 5, 0]  # noqa: SLF001
    with pytest.raises(ValueError, match="one entry per query"):
        _ops._rank_limits([1, 2], 3)  # noqa: SLF001


def test_plan_filters_equals_a_plain_loop(monkeypatch):
    rng = np.random.default_rng(1)
    n = 300
    metadata = [{"tenant": f"t{int(rng.integers(6))}", "lang": ["en", "de"][i % 2]} for i in range(n)]
    rows_per_chunk = rng.integers(1, 5, size=n)
    monkeypatch.setattr(_search, "FILTER_FIRST_MAX_ROWS", 150)
    monkeypatch.setattr(_search, "ORDER_FIRST_LIMIT", 1000)
    raw = [None, {"tenant": "t1"}, {}, {"lang": "en", "tenant": ["t1", "t2"]}, {"tenant": "t1"}, {"tenant": ["t1", "t2"], "lang": "en"},
           {"tenant": "zz"}, {"lang": ["en"]}, None, {"lang": "de"}]
    filters = _search._batch_filters(raw, len(raw))  # noqa: SLF001
    assert _search._batch_filters({"tenant": "t1"}, 3) == [{"tenant": ["t1"]}] * 3  # noqa: SLF001
    assert _search._batch_filters(None, 2) == [None, None]  # noqa: SLF001
    with pytest.raises(ValueError, match="one entry per query"):
        _search._batch_filters([None], 2)  # noqa: SLF001
    calls = []
    real = _search._matches  # noqa: SLF001
    monkeypatch.setattr(_search, "_matches", lambda m, f: calls.append(1) or real(m, f))
    plan = _search.plan_filters(filters, metadata, rows_per_chunk)
    # {"tenant": "t1"} twice and the two spellings of (lang en, tenant t1 / t2): five distinct filters, each evaluated once
    assert len(plan.allowed) == len(plan.rank_limit) == 5
    assert len(calls) == 5 * n
    for b, f in enumerate(filters):  # a plain loop, deciding as vector_search decides for one query
        if not f:
            assert plan.query_filter[b] == -1 and plan.of(b) == (None, 0)
            continue
        allowed, limit = plan.of(b)
        want = np.array([real(m, f) for m in metadata])
        assert np.array_equal(allowed, want)
        assert limit == (1000 if int(rows_per_chunk[want].sum()) > 150 else 0)
    assert set(plan.rank_limit) == {0, 1000}  # both branches at this scale
    # an index without metadata: nothing is evaluated (the searches raise where the loop raises)
    plan = _search.plan_filters(filters, None, rows_per_chunk)
    assert all(a is None for a in plan.allowed) and plan.query_filter[1] == plan.query_filter[4]
