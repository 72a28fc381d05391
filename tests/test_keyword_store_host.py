"""The keyword store's argument validation that returns before the first HIP call (include/raglite_hip.h "keyword store"): checked
without a GPU, through the C ABI."""

import ctypes as C

import numpy as np

from raglite_amd import _abi


def _store(lib):
    h = C.c_void_p()
    assert lib.rl_keyword_store_create(C.byref(h)) == _abi.RL_OK and h.value
    return h


def _invalid(status, word):
    return status == _abi.RL_ERR_INVALID and word in _abi.last_error()


def test_append_checks_host_offsets_and_ids_before_any_launch():
    lib = _abi.lib()
    h = _store(lib)
    try:
        ids = np.array([4, 0, 4, 9], np.int32)

        def append(off, ids=ids, mem=_abi.MEM_HOST):
            off = np.asarray(off, np.int64)
            return lib.rl_keyword_store_append(h, ids.ctypes.data, off.ctypes.data, off.size - 1, mem, None)

        assert _invalid(append([1, 4]), "offsets must start at 0")
        assert _invalid(append([0, 3, 2, 4]), "offsets must be ascending")
        assert _invalid(append([0, 2, 4], np.array([4, 0, -1, 9], np.int32)), "negative term id")
        assert _invalid(append([0, 4], mem=7), "bad mem")
        assert _invalid(lib.rl_keyword_store_append(h, None, np.array([0, 2], np.int64).ctypes.data, 1, _abi.MEM_HOST, None), "null term_ids")
        assert _invalid(lib.rl_keyword_store_append(h, ids.ctypes.data, None, 1, _abi.MEM_HOST, None), "null offsets")
        assert _invalid(lib.rl_keyword_store_append(h, ids.ctypes.data, None, -1, _abi.MEM_HOST, None), "negative size")
        assert _invalid(lib.rl_keyword_store_append(None, ids.ctypes.data, None, 1, _abi.MEM_HOST, None), "null store")
        assert lib.rl_keyword_store_append(h, None, None, 0, _abi.MEM_HOST, None) == _abi.RL_OK  # no chunk: nothing to do
        vals = [C.c_int64(-1) for _ in range(4)]
        assert lib.rl_keyword_store_info(h, *(C.byref(v) for v in vals)) == _abi.RL_OK and [v.value for v in vals] == [0, 0, 0, 0]
    finally:
        assert lib.rl_keyword_store_destroy(h) == _abi.RL_OK


def test_delete_count_and_build_check_their_arguments():
    lib = _abi.lib()
    h = _store(lib)
    try:
        ords = np.array([0], np.int64)
        assert _invalid(lib.rl_keyword_store_delete(h, ords.ctypes.data, 1, None), "chunk ordinal out of range")  # (an empty store)
        assert _invalid(lib.rl_keyword_store_delete(h, None, 1, None), "bad ordinals")
        assert lib.rl_keyword_store_delete(h, None, 0, None) == _abi.RL_OK
        for rank in ([0, 0, 1], [0, 1, 3], [-1, 0, 1]):
            r = np.asarray(rank, np.int32)
            assert _invalid(lib.rl_keyword_store_count(h, r.ctypes.data, 3, None, None, None, _abi.MEM_HOST, None), "permutation"), rank
        assert _invalid(lib.rl_keyword_store_count(h, None, -1, None, None, None, _abi.MEM_HOST, None), "negative size")
        assert _invalid(lib.rl_keyword_store_count(None, None, 1, None, None, None, _abi.MEM_HOST, None), "null store")
        kw = C.c_void_p(1)
        assert _invalid(lib.rl_keyword_store_build(h, None, None, C.byref(kw), _abi.MEM_HOST, None), "rl_keyword_store_count") and not kw.value
        assert _invalid(lib.rl_keyword_store_build(h, None, None, None, _abi.MEM_HOST, None), "null output handle")
        assert _invalid(lib.rl_keyword_index_read(None, None, None, None, _abi.MEM_HOST, None), "null index")
    finally:
        assert lib.rl_keyword_store_destroy(h) == _abi.RL_OK
    assert lib.rl_keyword_store_destroy(None) == _abi.RL_OK
