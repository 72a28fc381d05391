"""Metadata filters as tag containment, without a GPU: the host encoding (`raglite_amd._metadata`) and its NumPy
restatement of the kernel against a plain `_search._matches` loop, the host-only / fallback decisions, stable ids across an append,
and the arguments of the new C calls that need no handle."""

import ctypes as C

import numpy as np
import pytest

from raglite_amd import _abi, _metadata, _search


def _random_metadata(rng, n):
    """List-valued keys, missing keys, and 1 / 1.0 / True under one key."""
    out = []
    for i in range(n):
        m = {}
        if rng.random() < 0.8:
            m["tenant"] = f"t{int(rng.integers(5))}"
        if rng.random() < 0.7:
            m["topics"] = [["a", "b", "c", "d"][int(k)] for k in rng.integers(0, 4, size=int(rng.integers(0, 4)))]  # (repeats, empty)
        if rng.random() < 0.6:
            m["flag"] = [1, 1.0, True, 0, 2, False, 2.5][int(rng.integers(7))]
        if rng.random() < 0.3:
            m["pair"] = ("x", int(rng.integers(3)))  # a tuple is a list of values
        if i % 17 == 0:
            m["labels"] = {"red", "blue"} if i % 2 else {"red"}
        out.append(m)
    return out


FILTERS = [
    {"tenant": "t1"},
    {"tenant": ["t1"], "topics": ["a", "b"]},
    {"topics": []},                          # an empty wanted list: matches every chunk
    {"topics": [], "tenant": []},
    {"tenant": "never-seen"},                # a value the corpus never had
    {"tenant": "t2", "topics": "zz"},
    {"topics": ["a", "a", "c", "a"]},        # a repeated wanted value
    {"flag": 1}, {"flag": 1.0}, {"flag": True}, {"flag": [True, 1]}, {"flag": 0}, {"flag": False}, {"flag": 2.5}, {"flag": 2.0},
    {"pair": ["x", 1]}, {"pair": 2},
    {"labels": ["red", "blue"]}, {"labels": "red"},
    {"missing-key": "v"},
    {"tenant": "t0", "flag": 1, "topics": "d"},
]


def _loop(metadata, flt):
    return np.array([_search._matches(m, flt) for m in metadata], dtype=bool)  # noqa: SLF001


def _unpack(bits, n):
    return np.unpackbits(np.ascontiguousarray(bits).view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)


@pytest.mark.parametrize("n", [1, 31, 33, 64, 65, 257, 1000])
def test_filter_bits_host_equals_the_matches_loop(n):
    rng = np.random.default_rng(n)
    metadata = _random_metadata(rng, n)
    vocab = _metadata.TagVocabulary()
    tag_off, tags = vocab.encode_chunks(metadata)
    assert not vocab.host_only
    assert tag_off.dtype == np.int64 and tags.dtype == np.int32 and tag_off[0] == 0 and tag_off[-1] == tags.size
    for c in range(n):  # ascending and free of duplicates
        row = tags[tag_off[c] : tag_off[c + 1]]
        assert np.all(np.diff(row) > 0)
    filters = [_search._adapt_metadata(f) for f in FILTERS]  # noqa: SLF001
    f_off, f_tags = vocab.encode_filters(filters)
    bits = _metadata.filter_bits_host(tag_off, tags, f_off, f_tags)
    assert bits.dtype == np.uint32 and bits.shape == (len(filters), (n + 31) // 32)
    got = _unpack(bits, n)
    rows = rng.integers(1, 6, size=n)
    chunks, row_sums = _metadata.filter_counts_host(bits, rows)
    for j, f in enumerate(filters):
        want = _loop(metadata, f)
        assert np.array_equal(got[j], want), FILTERS[j]
        assert chunks[j] == want.sum() and row_sums[j] == rows[want].sum()
    # the bits past n are zero
    full = np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")
    assert not full[:, n:].any()


def test_filter_encoding():
    vocab = _metadata.TagVocabulary()
    vocab.encode_chunks([{"k": [1, "a"], "j": 2.0}, {"k": True}])
    assert vocab.ids[("k", 1)] == vocab.ids[("k", True)] == vocab.ids[("k", 1.0)]  # one tag, as they match each other
    assert len(vocab) == 3
    assert vocab.encode_filter({"k": [1.0, True, 1]}) == [vocab.ids[("k", 1)]]  # distinct tag ids
    assert vocab.encode_filter({"k": ["b"]}) == [_metadata.NO_TAG]  # never seen: the sentinel no chunk carries
    assert vocab.encode_filter({"k": [], "j": []}) == []  # matches every chunk
    assert vocab.encode_filter({"j": [2], "k": ["a", "zz"]}) == sorted([vocab.ids[("j", 2.0)], vocab.ids[("k", "a")], _metadata.NO_TAG])
    f_off, f_tags = vocab.encode_filters([{"k": ["a"]}, {"k": []}, {"j": [2, 2.0], "k": [1]}])
    assert f_off.tolist() == [0, 1, 1, 3] and f_tags.dtype == np.int32


@pytest.mark.parametrize("bad", [None, float("nan"), {"a": 1}, [["nested"]], ["ok", None], b"bytes", np.float64(1.0)])
def test_a_value_that_cannot_be_a_tag_makes_its_key_host_only(bad):
    vocab = _metadata.TagVocabulary()
    metadata = [{"good": "x", "odd": "fine"}, {"good": ["x", "y"], "odd": bad}]
    tag_off, tags = vocab.encode_chunks(metadata)
    assert vocab.host_only == {"odd"}
    assert vocab.encode_filter({"odd": ["fine"]}) is None  # touches a host-only key: the call takes the host path
    assert vocab.encode_filters([{"good": ["x"]}, {"odd": ["fine"]}]) is None  # ... the whole call
    good = vocab.encode_filters([{"good": ["x"]}, {"good": ["y"]}])  # the other keys are still evaluated from the tags
    got = _unpack(_metadata.filter_bits_host(tag_off, tags, *good), 2)
    assert got.tolist() == [[True, True], [False, True]]


@pytest.mark.parametrize("wanted", [None, float("nan"), {"a": 1}, ["nested"], b"x"])
def test_a_wanted_value_outside_the_four_types_is_not_encodable(wanted):
    vocab = _metadata.TagVocabulary()
    vocab.encode_chunks([{"k": "v"}])
    assert vocab.encode_filter({"k": [wanted]}) is None
    assert vocab.encode_filter({"k": ["v"]}) == [0]


def test_append_keeps_earlier_ids():
    vocab = _metadata.TagVocabulary()
    first = [{"a": 1, "b": ["x", "y"]}, {"a": 2}]
    off1, tags1 = vocab.encode_chunks(first)
    before = dict(vocab.ids)
    more = [{"b": "y", "c": 3}, {"a": 1, "d": None}]
    off2, tags2 = vocab.encode_chunks(more)
    assert all(vocab.ids[k] == v for k, v in before.items()) and len(vocab) == len(before) + 1
    assert off2[0] == 0 and vocab.host_only == {"d"}
    # the store's CSR after the append, as rl_metadata_store_append builds it
    tag_off = np.concatenate([off1, off1[-1] + off2[1:]])
    tags = np.concatenate([tags1, tags2])
    metadata = first + more
    filters = [{"a": [1]}, {"b": ["y"]}, {"c": [3]}, {"a": [1], "b": ["x"]}]
    got = _unpack(_metadata.filter_bits_host(tag_off, tags, *vocab.encode_filters(filters)), len(metadata))
    for j, f in enumerate(filters):
        assert np.array_equal(got[j], _loop(metadata, f))


# ---- the C calls: what needs no handle is checked first ------------------------------------------------------------------
def _i64(values):
    return (C.c_int64 * len(values))(*values)


def test_metadata_calls_check_their_arguments_before_the_handles():
    lib = _abi.lib()
    off, tags = _i64([0, 1]), (C.c_int32 * 1)(0)
    out = C.c_void_p()
    cases = [  # (the call, the entry point its message names, what it names)
        (lambda: lib.rl_metadata_store_create(None, off, tags, 1, _abi.MEM_HOST, None), "rl_metadata_store_create", "null output handle"),
        (lambda: lib.rl_metadata_store_create(C.byref(out), off, tags, -1, _abi.MEM_HOST, None), "rl_metadata_store_create", "negative size"),
        (lambda: lib.rl_metadata_store_create(C.byref(out), off, tags, 1, 7, None), "rl_metadata_store_create", "bad mem"),
        (lambda: lib.rl_metadata_store_create(C.byref(out), None, tags, 1, _abi.MEM_HOST, None), "rl_metadata_store_create", "null tag_off"),
        (lambda: lib.rl_metadata_store_append(None, off, tags, -1, _abi.MEM_HOST, None), "rl_metadata_store_append", "negative size"),
        (lambda: lib.rl_metadata_store_append(None, off, tags, 1, 2, None), "rl_metadata_store_append", "bad mem"),
        (lambda: lib.rl_metadata_store_append(None, off, tags, 1, _abi.MEM_HOST, None), "rl_metadata_store_append", "null store"),
        (lambda: lib.rl_metadata_store_memory(None, _i64([0, 0])), "rl_metadata_store_memory", "null"),
        (lambda: lib.rl_filter_set_bits(None, None, None, None), "rl_filter_set_bits", "null filter set"),
    ]
    for call, who, what in cases:
        assert call() == _abi.RL_ERR_INVALID
        msg = _abi.last_error()
        assert msg.startswith(who) and what in msg, msg
    assert out.value is None
    assert lib.rl_metadata_store_destroy(None) == _abi.RL_OK and lib.rl_filter_set_destroy(None) == _abi.RL_OK


def test_metadata_filters_checks_its_arguments_before_the_handles():
    lib = _abi.lib()
    f_off, f_tags = _i64([0, 1, 1]), (C.c_int32 * 1)(0)
    counts, rows = _i64([0, 0]), _i64([0, 0])
    fs = C.c_void_p()

    def call(f_off=f_off, n=2, set_ref=C.byref(fs), out=counts, mem=_abi.MEM_HOST):
        status = lib.rl_metadata_filters(None, None, f_off, f_tags, n, set_ref, out, rows, mem, None)
        return status, _abi.last_error()

    for kwargs, what in (({"n": -1}, "n_filters"), ({"mem": 2}, "bad mem"), ({"mem": 5}, "bad mem"), ({"set_ref": None}, "inout_set"),
                         ({"f_off": None}, "null f_off"), ({"out": None}, "output"), ({}, "null store")):
        status, msg = call(**kwargs)
        assert status == _abi.RL_ERR_INVALID and msg.startswith("rl_metadata_filters") and what in msg, (kwargs, msg)
    assert fs.value is None  # nothing was created


# ---- RL_MEM_FILTERS_DEVICE: the values 0 and 1 mean what they meant, the flag is accepted beside them ----------------------
B = 3


def _per_query_call(entry, mem):
    lib = _abi.lib()
    q = (C.c_float * 8)()
    out_f, out_d, out_i, out_n = (C.c_float * 8)(), (C.c_double * 8)(), (C.c_int32 * 8)(), (C.c_int32 * B)()
    q_off, q_terms = _i64([0, 1, 2, 3]), (C.c_int32 * 3)(0, 1, 2)
    bits = (C.c_uint32 * 4)(*([0xFFFFFFFF] * 4))
    qf = (C.c_int32 * B)(0, 1, -1)
    if entry == "chunks":
        return lib.rl_search_chunks_per_query(None, q, B, 4, 2, bits, 2, qf, None, out_f, out_i, out_n, mem, None)
    if entry == "keyword":
        return lib.rl_keyword_search_per_query(None, q_off, q_terms, B, 2, bits, 2, qf, out_f, out_i, out_n, mem, None)
    w = (C.c_double * 2)(0.75, 0.25)
    return lib.rl_hybrid_search_per_query(None, None, q, B, 4, 2, q_off, q_terms, bits, 2, qf, None, w, 60, 2, out_d, out_i, out_n, mem, None)


@pytest.mark.parametrize("entry", ["chunks", "hybrid", "keyword"])
@pytest.mark.parametrize("mem", [_abi.MEM_HOST, _abi.MEM_DEVICE, _abi.MEM_HOST | _abi.MEM_FILTERS_DEVICE,
                                 _abi.MEM_DEVICE | _abi.MEM_FILTERS_DEVICE])
def test_mem_values_reach_the_index_check(entry, mem):
    assert _abi.MEM_FILTERS_DEVICE == 2
    assert _per_query_call(entry, mem) == _abi.RL_ERR_INVALID
    assert "null index" in _abi.last_error()
