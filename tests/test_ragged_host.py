"""The ragged MaxSim rerank without a GPU: the argument checks of rl_maxsim_rerank_ragged, rl_search_rerank_ragged and
rl_search_rerank_spans_ragged that run before any HIP call, the routes `MaxSimRanker` chooses for a batch, and `_ragged`'s packing of
a list of matrices.

rl_maxsim_rerank_ragged keeps rl_maxsim_rerank's size checks (n_cand < 0 is an error, n_cand == 0 scores nothing and returns RL_OK, no
upper limit: nothing is ordered); the two pipeline entries keep rl_search_rerank_per_query's (1 <= k <= n_cand <= 4096)."""

import ctypes as C

import numpy as np
import pytest

import raglite_amd
from raglite_amd import _abi, _ragged, _search

OFF = {"ok": [0, 3, 40], "first": [1, 3, 40], "empty": [0, 3, 3], "decreasing": [0, 5, 3]}
FAKE = C.create_string_buffer(256)  # stands where a span table goes: the calls below fail before they read it


def _rerank(off, idx=None, n_queries=2, n_cand=4, null=()):
    q = np.zeros((40, 8), np.float32)
    o = None if off is None else np.asarray(OFF[off], np.int64)
    c, s = np.zeros((2, max(n_cand, 1)), np.int32), np.zeros((2, max(n_cand, 1)), np.float32)
    ptr = {"query_vecs": q.ctypes.data, "candidates": c.ctypes.data, "out_scores": s.ctypes.data}
    ptr.update(dict.fromkeys(null))
    return _abi.lib().rl_maxsim_rerank_ragged(idx, ptr["query_vecs"], None if o is None else o.ctypes.data, n_queries, ptr["candidates"],
                                              n_cand, ptr["out_scores"], _abi.MEM_HOST, None)


def _pipeline(off, spans=False, n_queries=2, n_cand=4, k=2, outs=True):
    q, v, w = np.zeros((2, 8), np.float32), np.zeros((40, 8), np.float32), np.array([0.75, 0.25])
    o = None if off is None else np.asarray(OFF[off], np.int64)
    p_off = None if o is None else o.ctypes.data
    n = 2 * max(1, k) * 3
    if not spans:
        res = [np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(2, np.int32)]
        return _abi.lib().rl_search_rerank_ragged(None, None, q.ctypes.data, n_queries, 40, 16, None, None, None, 0, None, None, w.ctypes.data,
                                                  60, n_cand, v.ctypes.data, p_off, k, *[r.ctypes.data if outs else None for r in res],
                                                  _abi.MEM_HOST, None)
    offs = np.array([-1, 1], np.int32)
    res = [np.zeros(n, np.int32), np.zeros(2, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float64),
           np.zeros(2, np.int32), np.zeros(2, np.int32)]
    return _abi.lib().rl_search_rerank_spans_ragged(None, None, q.ctypes.data, n_queries, 40, 16, None, None, None, 0, None, None,
                                                    w.ctypes.data, 60, n_cand, v.ctypes.data, p_off, k, C.cast(FAKE, C.c_void_p),
                                                    offs.ctypes.data, 2, *[r.ctypes.data if outs else None for r in res], _abi.MEM_HOST, None)


ENTRIES = {"rl_maxsim_rerank_ragged": lambda off, **kw: _rerank(off, **kw),
           "rl_search_rerank_ragged": lambda off, **kw: _pipeline(off, **kw),
           "rl_search_rerank_spans_ragged": lambda off, **kw: _pipeline(off, spans=True, **kw)}


def _rejected(status, entry, text, code=None):
    assert status == (code or _abi.RL_ERR_INVALID), status
    msg = _abi.last_error()
    assert msg.startswith(entry) and text in msg, msg


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_table_is_checked_before_any_hip_call(entry):
    call = ENTRIES[entry]
    _rejected(call("ok"), entry, "null index")
    _rejected(call("first"), entry, "qv_off[0] must be 0")
    _rejected(call("empty"), entry, "query 1 has no vectors")
    _rejected(call("decreasing"), entry, "query 1 has no vectors")
    _rejected(call(None), entry, "null qv_off")
    _rejected(call("ok", n_queries=-1), entry, "")


@pytest.mark.parametrize("entry", ENTRIES)
def test_no_queries_is_ok(entry):
    assert ENTRIES[entry](None, n_queries=0) == _abi.RL_OK


@pytest.mark.parametrize("entry", ["rl_search_rerank_ragged", "rl_search_rerank_spans_ragged"])
def test_the_pipeline_entries_keep_the_size_checks(entry):
    call = ENTRIES[entry]
    _rejected(call("ok", n_cand=0), entry, "n_cand must be in [1, 4096]")
    _rejected(call("ok", n_cand=4097), entry, "n_cand must be in [1, 4096]")
    _rejected(call("ok", n_cand=4, k=5), entry, "k must be in [1, n_cand]")
    _rejected(call("ok", n_cand=4, k=0), entry, "")
    assert call("ok", n_queries=0, n_cand=4097) == _abi.RL_ERR_INVALID  # (the sizes come before "nothing to do")


def test_the_span_entry_checks_its_table_first():
    q, w = np.zeros((2, 8), np.float32), np.array([0.75, 0.25])
    st = _abi.lib().rl_search_rerank_spans_ragged(None, None, q.ctypes.data, 2, 40, 16, None, None, None, 0, None, None, w.ctypes.data, 60, 4,
                                                  q.ctypes.data, None, 2, None, None, 0, None, None, None, None, None, None, None,
                                                  _abi.MEM_HOST, None)
    _rejected(st, "rl_search_rerank_spans_ragged", "null span table")


def test_rerank_ragged_keeps_the_size_checks_of_maxsim_rerank():
    _rejected(_rerank("ok", n_cand=-1), "rl_maxsim_rerank_ragged", "bad sizes")
    _rejected(_rerank("ok", n_cand=0), "rl_maxsim_rerank_ragged", "null index")  # (n_cand == 0 is no error: the index is looked at next)
    _rejected(_rerank("ok", n_cand=4097), "rl_maxsim_rerank_ragged", "null index")


# ---- the routes of a batch ----------------------------------------------------------------------------------------------------------
class _StubDevice:
    """Stands where a DeviceIndex goes and only has `maxsim_rerank`: records the shape of every call."""

    def __init__(self):
        self.calls = []

    def maxsim_rerank(self, vecs, cand):
        self.calls.append(tuple(vecs.shape))
        return np.zeros(cand.shape, np.float32)


class _StubIndex:
    def __init__(self):
        self.index = _StubDevice()


class _F16Device(raglite_amd.DeviceIndex):
    """A DeviceIndex without a device: what `_routes` reads of one."""

    def __init__(self, storage):  # noqa: D107 - no handle is made
        self.storage = storage


def _vecs(lengths):
    return [np.zeros((n, 4), np.float32) for n in lengths]


@pytest.mark.parametrize("ragged", [True, False])
def test_a_stub_index_still_gets_one_call_per_distinct_length(ragged, monkeypatch):
    monkeypatch.setattr(_search._ops, "rerank_order",  # noqa: SLF001 - the ordering is a device call: stand in for it
                        lambda s, c, k: (None, None, np.tile(np.arange(k, dtype=np.int32), (len(s), 1)), np.full(len(s), k, np.int32)))
    gi = _StubIndex()
    ranker = raglite_amd.MaxSimRanker(gi, lambda q: np.zeros((2, 4), np.float32))
    assert raglite_amd.MaxSimRanker.ragged is True
    ranker.ragged = ragged
    lengths = [5, 9, 5, 40, 9, 5]
    out = ranker.score_batch([""] * 6, [[0, 1]] * 6, query_token_vectors=_vecs(lengths))
    assert sorted(gi.index.calls) == [(1, 40, 4), (2, 9, 4), (3, 5, 4)]
    assert [len(s) for s in out] == [2] * 6
    assert ranker._routes(_vecs(lengths)) == [([0, 2, 5], False), ([1, 4], False), ([3], False)]  # noqa: SLF001


def test_routes_over_a_device_index():
    gi = _StubIndex()
    ranker = raglite_amd.MaxSimRanker(gi, lambda q: np.zeros((2, 4), np.float32))
    routes = ranker._routes  # noqa: SLF001
    gi.index = _F16Device("f32")
    assert routes(_vecs([7, 7, 7])) == [([0, 1, 2], False)]                      # one length: the call as it was
    assert routes(_vecs([40, 40])) == [([0, 1], False)]                           # ... also beyond 32 on fp32 rows
    assert routes(_vecs([7, 9, 7, 32])) == [([0, 1, 2, 3], True)]                 # mixed: one ragged call
    assert routes(_vecs([7, 40, 9, 40, 33])) == [([1, 3], False), ([4], False), ([0, 2], True)]  # fp32 rows: long queries keep their groups
    ranker.ragged = False
    assert routes(_vecs([7, 9, 7])) == [([0, 2], False), ([1], False)]
    ranker.ragged = True
    gi.index = _F16Device("f16")
    assert routes(_vecs([7, 7])) == [([0, 1], False)]
    assert routes(_vecs([40, 40])) == [([0, 1], True)]                            # fp16 rows: the uniform call stops at 32 vectors
    assert routes(_vecs([7, 40, 9, 33])) == [([0, 1, 2, 3], True)]
    gi.index.storage = None  # (nothing for __del__ to close)


# ---- packing ------------------------------------------------------------------------------------------------------------------------
def test_pack_vectors():
    rng = np.random.default_rng(3)
    mats = [rng.standard_normal((n, 6)).astype(np.float32) for n in (3, 1, 40)]
    flat, off = _ragged.pack_vectors(mats)
    assert flat.dtype == np.float32 and flat.flags.c_contiguous and flat.shape == (44, 6)
    assert off.dtype == np.int64 and off.tolist() == [0, 3, 4, 44]
    for b, m in enumerate(mats):
        assert np.array_equal(flat[off[b]: off[b + 1]], m)
    flat64, _ = _ragged.pack_vectors([m.astype(np.float64) for m in mats])
    assert flat64.dtype == np.float32 and np.array_equal(flat64, flat)
    flat0, off0 = _ragged.pack_vectors([], 6)
    assert flat0.shape == (0, 6) and off0.tolist() == [0]


@pytest.mark.parametrize("bad", [np.zeros(6, np.float32), np.zeros((1, 2, 6), np.float32), [[0.0] * 6]])
def test_pack_vectors_rejects_what_is_not_a_matrix(bad):
    with pytest.raises(ValueError, match="2-D"):
        _ragged.pack_vectors([np.zeros((2, 6), np.float32), bad])


def test_pack_vectors_rejects_mixed_dims():
    with pytest.raises(ValueError, match="same dim"):
        _ragged.pack_vectors([np.zeros((2, 6), np.float32), np.zeros((2, 8), np.float32)])
    with pytest.raises(ValueError, match="same dim"):
        _ragged.pack_vectors([np.zeros((2, 6), np.float32)], 8)


def test_from_embedder_without_a_limit_keeps_every_vector():
    class _Embedder:
        def embed(self, query):
            return np.ones((len(query), 4), np.float32)

    gi = _StubIndex()
    long = "x" * 50
    assert raglite_amd.MaxSimRanker.from_embedder(gi, _Embedder()).query_encoder(long).shape == (32, 4)
    assert raglite_amd.MaxSimRanker.from_embedder(gi, _Embedder(), max_vectors=None).query_encoder(long).shape == (50, 4)
