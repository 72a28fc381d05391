"""The C ABI is compiled from four files (api.hip, api_ingest.hip, api_keyword.hip, api_retrieval.hip: DESIGN.md 1.2) that share ONE
per-thread error slot: a failure in any of them is what rl_last_error returns on that thread, and on no other.  Every call below fails
an argument check that comes before the first HIP call, so no GPU is needed."""

import ctypes as C
import threading

from raglite_amd import _abi

INVALID = _abi.RL_ERR_INVALID


def _calls():
    lib = _abi.lib()
    one = (C.c_double * 1)(1.0)
    # (file, call, the text it leaves)
    return [
        ("api.hip", lambda: lib.rl_search_rows(None, None, 1, 1, None, None, 0, None), "rl_search_rows: null index"),
        ("api_ingest.hip", lambda: lib.rl_partition_chunks(None, None, None, 0, 0, 8, None, None, None, 7, None),
         "rl_partition_chunks: bad mem"),
        ("api_keyword.hip", lambda: lib.rl_keyword_index_create(None, None, 0, None, None, None, 0, None, None, 0, 0, None),
         "rl_keyword_index_create: null output handle"),
        ("api_keyword.hip", lambda: lib.rl_keyword_search(None, None, None, 1, 1, None, None, None, None, 0, None),
         "rl_keyword_search: null index"),
        ("api_retrieval.hip", lambda: lib.rl_rrf_fuse(None, 1, 1, 1, one, 60, 1, None, None, None, 7, None), "rl_rrf_fuse: bad mem"),
        ("api_retrieval.hip", lambda: lib.rl_span_table_create(None, None, None, 0), "rl_span_table_create: null output handle"),
        ("api_retrieval.hip", lambda: lib.rl_metadata_store_create(None, None, None, 0, 0, None),
         "rl_metadata_store_create: null output handle"),
    ]


def test_every_file_fails_into_the_same_slot():
    for file, call, text in _calls():
        assert call() == INVALID, file
        assert _abi.last_error() == text, file  # (this call's text, not the previous file's)


def test_the_slot_is_per_thread():
    _, call, text = _calls()[-1]
    assert call() == INVALID and _abi.last_error() == text
    seen = []
    t = threading.Thread(target=lambda: seen.append(_abi.last_error()))
    t.start()
    t.join()
    assert seen == [""]
    assert _abi.last_error() == text  # (and the fresh thread's read left this thread's alone)
