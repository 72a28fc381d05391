"""Chunk spans, without a GPU: hand-built cases for the restatement of `retrieve_chunk_spans` (tests/spans_ref.py)
with the expected spans written out, the argument checks of rl_chunk_spans and rl_search_rerank_spans_per_query that run before any
HIP call, the Python errors around `positions`, and the store reader's positions."""

import ctypes as C

import numpy as np
import pytest

import raglite_amd
from raglite_amd import _abi, _ops, _search, _store
from tests import spans_ref as ref
from tests import store_fixture


# ---- the restatement, case by case ----------------------------------------------------------------------------------------------
def _table(**docs):
    """doc=[indices] -> chunks named '<doc>/<index>'."""
    return ref.Table({f"{d}/{i}": (d, i) for d, indices in docs.items() for i in indices})


def test_default_neighbours_merge_and_rank():
    t = _table(a=range(10), b=range(4))
    got = ref.spans_of_ids(t, ["a/5", "b/0", "a/7"])
    # a/5 -> a/4..a/6, a/7 -> a/6..a/8: one span a/4..a/8 scoring 1/1 + 1/3; b/0 -> b/0, b/1 scoring 1/2
    assert got == [(["a/4", "a/5", "a/6", "a/7", "a/8"], "a", 1 + 1 / 3), (["b/0", "b/1"], "b", 0.5)]


def test_no_neighbours():
    t = _table(a=range(10))
    for none in (None, ()):
        got = ref.spans_of_ids(t, ["a/5", "a/7", "a/6"], none)
        assert got == [(["a/5", "a/6", "a/7"], "a", ref.left_to_right([1.0, 1 / 3, 0.5]))]
        assert ref.spans_of_ids(t, ["a/5", "a/7"], none) == [(["a/5"], "a", 1.0), (["a/7"], "a", 0.5)]
    assert ref.spans_of_ids(t, []) == [] and ref.spans_of_ids(t, ["unknown"]) == []


def test_offset_zero_and_repeated_offsets():
    t = _table(a=range(10))
    assert ref.spans_of_ids(t, ["a/5"], (0,)) == [(["a/5"], "a", 1.0)]
    assert ref.spans_of_ids(t, ["a/5"], (1, 1, 0, 1)) == [(["a/5", "a/6"], "a", 1.0)]
    # an offset that is no neighbour of a span: a span of its own, scoring 0.0, after the scored ones
    assert ref.spans_of_ids(t, ["a/5"], (-3, 3)) == [(["a/5"], "a", 1.0), (["a/2"], "a", 0.0), (["a/8"], "a", 0.0)]
    assert ref.spans_of_ids(t, ["a/9"], (1, 2 ** 31 - 1, -2 ** 31)) == [(["a/9"], "a", 1.0)]


def test_one_chunk_document_and_gaps_in_index():
    t = _table(solo=[0], gap=[0, 1, 3, 4, 7])
    assert ref.spans_of_ids(t, ["solo/0"]) == [(["solo/0"], "solo", 1.0)]
    got = ref.spans_of_ids(t, ["gap/3", "gap/1"])
    # gap/3 -> gap/4 (there is no gap/2); gap/1 -> gap/0: two spans, not one
    assert got == [(["gap/3", "gap/4"], "gap", 1.0), (["gap/0", "gap/1"], "gap", 0.5)]
    assert ref.spans_of_ids(t, ["gap/7"]) == [(["gap/7"], "gap", 1.0)]


def test_document_ids_compare_as_strings():
    t = _table(doc9=[0, 5], doc10=[0, 5])
    got = ref.spans_of_ids(t, ["doc9/0", "doc10/0"], (5,))
    # the two neighbours tie at 0.0 and keep their (document_id, index) order: "doc10" < "doc9"
    assert got == [(["doc9/0"], "doc9", 1.0), (["doc10/0"], "doc10", 0.5), (["doc10/5"], "doc10", 0.0), (["doc9/5"], "doc9", 0.0)]
    got = ref.spans_of_chunks(t, ["doc9/0", "doc10/0", "doc9/0", "doc10/0"], None)  # the last scores stand: 1/3 and 1/4
    assert got == [(["doc9/0"], "doc9", 1 / 3), (["doc10/0"], "doc10", 0.25)]


def tie_case():
    """{rank 2} against {ranks 3 and 6, adjacent}: 1/3 + 1/6 is exactly 0.5 in doubles, so the two spans tie and keep their
    (document_id, index) order -- the pair comes first although the single chunk ranks higher."""
    t = _table(a=[0, 1], b=[0], c=[0, 2, 4])
    ids = ["c/0", "b/0", "a/0", "c/2", "c/4", "a/1"]
    want = [(["c/0"], "c", 1.0), (["a/0", "a/1"], "a", 0.5), (["b/0"], "b", 0.5), (["c/2"], "c", 0.25), (["c/4"], "c", 0.2)]
    return t, ids, want


def last_bit_case():
    """Ranks 1, 3 and 7 in ascending index: (1/1 + 1/3) + 1/7 = 0x1.79e79e79e79e7p+0, while 1/1 + (1/3 + 1/7) and the correctly
    rounded sum are 0x1.79e79e79e79e8p+0.  The span of ranks 2, 4, 5, 6 ... is there so that the list is long enough."""
    t = _table(a=[0, 1, 2], b=[0, 2, 4, 6])
    ids = ["a/0", "b/0", "a/1", "b/2", "b/4", "b/6", "a/2"]
    return t, ids, float.fromhex("0x1.79e79e79e79e7p+0")


def test_exact_tie_keeps_document_order():
    t, ids, want = tie_case()
    assert 1 / 3 + 1 / 6 == 0.5
    assert ref.spans_of_ids(t, ids, None) == want


def test_the_sum_runs_left_to_right():
    import math

    t, ids, want = last_bit_case()
    got = ref.spans_of_ids(t, ids, None)
    assert got[0][0] == ["a/0", "a/1", "a/2"] and got[0][2] == want
    assert 1.0 + (1 / 3 + 1 / 7) != want and math.fsum([1.0, 1 / 3, 1 / 7]) != want  # another order, and the exact sum, differ


def test_id_branch_keeps_first_places_and_object_branch_last_scores():
    t = _table(a=range(6))
    ids = ["a/4", "nope", "a/0", "a/4", "a/2", "a/0"]
    assert ref.resolve_ids(t, ids) == ["a/4", "a/0", "a/2"]
    assert ref.spans_of_ids(t, ids, None) == [(["a/4"], "a", 1.0), (["a/0"], "a", 0.5), (["a/2"], "a", 1 / 3)]
    # objects: a/4 scores 1/3 (its last place), a/0 1/5, a/2 1/4; the unknown entry of a device list takes no rank
    assert ref.spans_of_entries(t, ids, None) == [(["a/4"], "a", 1 / 3), (["a/2"], "a", 0.25), (["a/0"], "a", 0.2)]


# ---- the C argument checks that run before any HIP call -------------------------------------------------------------------------
def _spans(table, chunks, B, n_in, offsets, n_off, outs=True, mem=_abi.MEM_HOST):
    out = [np.zeros(max(1, B * n_in * (1 + max(n_off, 0))), np.int32) for _ in range(2)]
    out.append(np.zeros(out[0].size, np.float64))
    out += [np.zeros(max(1, B), np.int32) for _ in range(2)]
    ptrs = [o.ctypes.data if outs else None for o in out]
    return _abi.lib().rl_chunk_spans(table, None if chunks is None else chunks.ctypes.data, B, n_in,
                                     None if offsets is None else offsets.ctypes.data, n_off, *ptrs, mem, None)


def test_chunk_spans_argument_checks():
    fake = C.create_string_buffer(256)  # stands where a table goes in calls that return before they read it
    table = C.cast(fake, C.c_void_p)
    chunks, offs = np.zeros(4096, np.int32), np.zeros(64, np.int32)
    assert _spans(None, chunks, 1, 4, offs, 2) == _abi.RL_ERR_INVALID and "null span table" in _abi.last_error()
    for B, n_in, n_off in ((-1, 4, 2), (1, 0, 2), (1, 4, -1), (1, 4, 65), (1, 4097, 0), (1, 1366, 2), (1, 64, 64)):
        assert _spans(table, chunks, B, n_in, offs, n_off) == _abi.RL_ERR_INVALID, (B, n_in, n_off)
        assert "rl_chunk_spans" in _abi.last_error()
    assert _spans(table, chunks, 1, 4, None, 2) == _abi.RL_ERR_INVALID and "null offsets" in _abi.last_error()
    assert _spans(table, chunks, 1, 4, offs, 2, mem=7) == _abi.RL_ERR_INVALID and "bad mem" in _abi.last_error()
    assert _spans(table, None, 1, 4, offs, 2) == _abi.RL_ERR_INVALID and "null argument" in _abi.last_error()
    assert _spans(table, chunks, 1, 4, offs, 2, outs=False) == _abi.RL_ERR_INVALID and "null argument" in _abi.last_error()
    assert _spans(table, chunks, 0, 1365, offs, 2) == _abi.RL_OK  # the largest E, and nothing to do
    assert _spans(table, None, 0, 4096, None, 0, outs=False) == _abi.RL_OK


def test_span_table_argument_checks():
    lib = _abi.lib()
    h = C.c_void_p()
    doc, pos = np.array([0, 0, -1], np.int32), np.array([1, 1, 0], np.int32)
    assert lib.rl_span_table_create(None, doc.ctypes.data, pos.ctypes.data, 3) == _abi.RL_ERR_INVALID
    assert lib.rl_span_table_create(C.byref(h), None, None, 3) == _abi.RL_ERR_INVALID and not h.value
    assert lib.rl_span_table_create(C.byref(h), doc.ctypes.data, pos.ctypes.data, -1) == _abi.RL_ERR_INVALID
    assert lib.rl_span_table_create(C.byref(h), doc.ctypes.data, pos.ctypes.data, 3) == _abi.RL_ERR_INVALID and not h.value
    assert "share a (doc, pos)" in _abi.last_error()
    pos[1] = -2
    assert lib.rl_span_table_create(C.byref(h), doc.ctypes.data, pos.ctypes.data, 3) == _abi.RL_ERR_INVALID
    assert "pos must be >= 0" in _abi.last_error()
    assert lib.rl_span_table_info(None, None, None, None) == _abi.RL_ERR_INVALID
    assert lib.rl_span_table_destroy(None) == _abi.RL_OK


def _pipeline(table, n_cand, k, n_off, idx=None, outs=True, nq=4, offsets=True):
    q, v, w = np.zeros((2, 8), np.float32), np.zeros((2, 4, 8), np.float32), np.array([0.75, 0.25])
    offs = np.zeros(64, np.int32)
    n = 2 * max(1, k) * (1 + max(0, n_off))
    top_c, top_n = np.zeros(n, np.int32), np.zeros(2, np.int32)
    o_c, o_l, o_s, o_ns, o_nc = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float64), np.zeros(2, np.int32), np.zeros(2, np.int32)
    ptrs = [o.ctypes.data if outs else None for o in (top_c, top_n, o_c, o_l, o_s, o_ns, o_nc)]
    return _abi.lib().rl_search_rerank_spans_per_query(idx, None, q.ctypes.data, 2, 40, 16, None, None, None, 0, None, None, w.ctypes.data, 60,
                                                       n_cand, v.ctypes.data, nq, k, table, offs.ctypes.data if offsets else None, n_off,
                                                       *ptrs, _abi.MEM_HOST, None)


def test_search_rerank_spans_argument_checks():
    fake = C.create_string_buffer(256)
    table = C.cast(fake, C.c_void_p)
    assert _pipeline(None, 16, 8, 2) == _abi.RL_ERR_INVALID and "null span table" in _abi.last_error()
    for n_cand, k, n_off in ((16, 8, -1), (16, 8, 65), (4096, 1366, 2), (4096, 4096, 1), (16, 0, 2)):
        assert _pipeline(table, n_cand, k, n_off) == _abi.RL_ERR_INVALID, (n_cand, k, n_off)
        assert "rl_search_rerank_spans_per_query" in _abi.last_error()
    assert _pipeline(table, 16, 8, 2, offsets=False) == _abi.RL_ERR_INVALID and "null offsets" in _abi.last_error()
    # rl_search_rerank_per_query's own checks follow
    assert _pipeline(table, 16, 8, 2, nq=0) == _abi.RL_ERR_INVALID and "nq must be" in _abi.last_error()
    assert _pipeline(table, 4097, 8, 2) == _abi.RL_ERR_INVALID and "n_cand" in _abi.last_error()
    assert _pipeline(table, 8, 9, 2) == _abi.RL_ERR_INVALID and "k must be" in _abi.last_error()
    assert _pipeline(table, 16, 8, 2) == _abi.RL_ERR_INVALID and "null index" in _abi.last_error()
    # the factored pipeline keeps rl_search_rerank_per_query's answers
    lib = _abi.lib()
    assert lib.rl_search_rerank_per_query(None, None, None, 2, 40, 16, None, None, None, 0, None, None, None, 60, 16, None, 0, 8, None, None,
                                          None, _abi.MEM_HOST, None) == _abi.RL_ERR_INVALID and "nq must be" in _abi.last_error()
    assert lib.rl_search_rerank_per_query(None, None, None, 2, 40, 16, None, None, None, 0, None, None, None, 60, 16, None, 4, 8, None, None,
                                          None, _abi.MEM_HOST, None) == _abi.RL_ERR_INVALID and "null index" in _abi.last_error()


# ---- Python errors -----------------------------------------------------------------------------------------------------------------
class _StubDevice:
    """Stands where a DeviceIndex goes: counts what it is given."""

    def __init__(self, matrix, offsets, *, metric="cosine", storage="f32"):
        self.n_rows = int(offsets[-1])
        self.n_chunks = len(offsets) - 1

    def append(self, rows, sizes):
        self.n_rows += len(rows)
        self.n_chunks += len(sizes)

    def delete_chunks(self, ordinals):
        pass

    def close(self):
        pass


class _StubTable:
    """Stands where a SpanTable goes: keeps what it was built from."""

    built = []

    def __init__(self, doc, pos):
        self.doc, self.pos = np.array(doc), np.array(pos)
        _StubTable.built.append(self)

    def close(self):
        pass


@pytest.fixture
def stubs(monkeypatch):
    monkeypatch.setattr(_ops, "DeviceIndex", _StubDevice)
    monkeypatch.setattr(_ops, "SpanTable", _StubTable)
    _StubTable.built = []


def _mats(n):
    return [np.ones((1, 4), np.float32) for _ in range(n)]


def test_an_index_without_positions_says_so(stubs):
    gi = raglite_amd.GpuIndex(["c0", "c1"], _mats(2))
    assert not gi.has_positions
    for call in (lambda: raglite_amd.retrieve_chunk_spans(["c0"], index=gi),
                 lambda: raglite_amd.retrieve_chunk_spans_batch([["c0"], []], index=gi),
                 lambda: raglite_amd.search_and_rerank_chunk_spans("q", index=gi),
                 lambda: raglite_amd.search_and_rerank_chunk_spans_batch(["q"], index=gi)):
        with pytest.raises(ValueError, match="positions"):
            call()
    assert raglite_amd.retrieve_chunk_spans([], index=gi) == []  # (`_search.py:314-315`: before anything is looked at)
    assert raglite_amd.search_and_rerank_chunk_spans_batch([], index=gi) == []
    with pytest.raises(ValueError, match="positions must be given iff"):
        gi.insert_chunks(["c2"], _mats(1), positions=[("d", 0)])
    with pytest.raises(ValueError, match="search must be"):
        raglite_amd.search_and_rerank_chunk_spans_batch(["q"], index=gi, search="keyword")


def test_positions_are_checked_and_follow_the_index(stubs):
    with pytest.raises(ValueError, match="one .* position per chunk"):
        raglite_amd.GpuIndex(["c0", "c1"], _mats(2), positions=[("d", 0)])
    with pytest.raises(ValueError, match="two live chunks are at .*'d'.*index=3"):
        raglite_amd.GpuIndex(["c0", "c1"], _mats(2), positions=[("d", 3), ("d", 3)])
    with pytest.raises(ValueError, match="document_id must be a str"):
        raglite_amd.GpuIndex(["c0", "c1"], _mats(2), positions=[("d", 3), ("d", -1)])
    gi = raglite_amd.GpuIndex(["c0", "c1", "c2"], _mats(3), positions=[("doc9", 0), ("doc10", 4), None])
    assert gi.has_positions
    # documents are numbered in string order: "doc10" before "doc9"; a chunk without a position is -1
    assert gi.spans.doc.tolist() == [1, 0, -1] and gi.spans.pos.tolist()[:2] == [0, 4]
    with pytest.raises(ValueError, match="positions must be given iff"):
        gi.insert_chunks(["c3"], _mats(1))
    with pytest.raises(ValueError, match="one .* position per chunk id"):
        gi.insert_chunks(["c3"], _mats(1), positions=[("a", 0), ("a", 1)])
    with pytest.raises(ValueError, match="two live chunks"):
        gi.insert_chunks(["c3"], _mats(1), positions=[("doc10", 4)])
    assert gi.chunk_ids == ["c0", "c1", "c2"] and gi.index.n_chunks == 3 and len(gi.positions) == 3  # nothing changed
    gi.insert_chunks(["c3"], _mats(1), positions=[("a", 7)])
    assert gi.spans.doc.tolist() == [2, 1, -1, 0] and gi.positions[3] == ("a", 7)
    # a deleted chunk frees its position
    assert gi.delete_chunks(["c1"]) == 1
    assert gi.spans.doc.tolist() == [1, -1, -1, 0] and gi.positions[1] is None
    gi.insert_chunks(["c4"], _mats(1), positions=[("doc10", 4)])
    assert gi.spans.doc.tolist() == [2, -1, -1, 0, 1] and gi.spans is _StubTable.built[-1]


def test_neighbour_offsets_are_checked():
    for bad in ([0] * 65, [2 ** 31], [-2 ** 31 - 1]):
        with pytest.raises(ValueError, match="offsets"):
            _ops._span_offsets(bad)  # noqa: SLF001
    assert _ops._span_offsets(None).size == 0 and _ops._span_offsets(()).size == 0  # noqa: SLF001
    assert _ops._span_offsets((-1, 1, 1)).tolist() == [-1, 1, 1]  # noqa: SLF001


def test_retrieve_context_needs_a_search_method():
    with pytest.raises(ValueError, match="search_method"):
        raglite_amd.retrieve_context("q", config=raglite_amd.HotPathConfig())
    spans = [_search.ChunkSpan(["c0"], "d", 1.0)]
    cfg = raglite_amd.HotPathConfig(search_method=lambda query, **kw: spans)
    assert raglite_amd.retrieve_context("q", config=cfg) is not None and raglite_amd.retrieve_context("q", config=cfg) == spans
    assert raglite_amd.retrieve_context("q", config=raglite_amd.HotPathConfig(search_method=lambda query, **kw: ([], []))) == []
    assert raglite_amd.retrieve_context("q", config=raglite_amd.HotPathConfig(search_method=lambda query, **kw: [1.5])) == []


# ---- the store ---------------------------------------------------------------------------------------------------------------------
def test_read_chunks_returns_positions():
    rng = np.random.default_rng(0)
    engine = store_fixture.create_store()
    docs = store_fixture.synthetic_documents(rng, 3, 8)
    for doc_id, chunks in docs:
        store_fixture.insert_document(engine, doc_id, chunks)
    want = {cid: (doc_id, i) for doc_id, chunks in docs for i, (cid, *_rest) in enumerate(chunks)}
    with engine.connect() as conn:
        img = _store.read_chunks(conn)
        assert len(img.positions) == len(img.chunk_ids) == len(want)
        assert {cid: p for cid, p in zip(img.chunk_ids, img.positions)} == want
        some = sorted(want)[:2]
        part = _store.read_chunks(conn, some)
        assert part.chunk_ids == some and part.positions == [want[c] for c in some]
