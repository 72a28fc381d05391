"""The binding's call trace: which symbol every wrapper of `raglite_amd._ops` calls, in which order and with which scalars.

The library is replaced by a recorder, so no GPU and no shared library is needed.  Every public wrapper is driven once with small
NumPy inputs (`_drive`), and what the recorder saw must equal `tests/golden/ops_call_trace.json`, which the same driver wrote
(`python -m tests.test_ops_calls_host > tests/golden/ops_call_trace.json`; the file names the commit it was written at).  A change of
the Python layer that is meant to leave the calls alone leaves this file alone.

What this does NOT prove: the recorder does not read through pointers, it records `ptr` or `null`.  Swapping two pointer arguments
of one call, or handing over the wrong array, passes here; the GPU suite, which compares results, catches that.  The wrappers that
only take CUDA tensors (`synth_fill`, `DeviceIndex.time_kernel`, `Communicator`) make no call from NumPy input and are left to it
too."""

import ctypes as C
import json
import re
import sys
import threading
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import raglite_amd
from raglite_amd import _abi, _chunking, _comm, _ops  # noqa: F401  (loaded, so that their `lib` is replaced too)

GOLDEN = Path(__file__).parent / "golden" / "ops_call_trace.json"
_HANDLE_OUT = C.POINTER(C.c_void_p)


def _poke(ptr: int, values, ctype) -> None:
    """Write `values` to the host address `ptr` (an output array of the wrapper's)."""
    arr = (ctype * len(values))(*values)
    C.memmove(ptr, arr, C.sizeof(arr))


class _Recorder:
    """Stands in for the loaded library: every declared symbol records (symbol, args) and returns RL_OK.  It writes into output
    arguments only where a wrapper reads them back."""

    def __init__(self) -> None:
        self.calls: list[tuple[str, tuple]] = []
        self.filter_set_shape = (0, 0)  # (n_filters, words) that rl_filter_set_bits reports: the driver sets it
        self._next_handle = 0x1000

    def __call__(self) -> "_Recorder":  # `lib()`
        return self

    def __getattr__(self, symbol: str):
        if symbol not in _abi._SIGNATURES:  # noqa: SLF001
            raise AttributeError(symbol)

        def call(*args):
            self.calls.append((symbol, args))
            self._write(symbol, args)
            return _abi.RL_OK

        return call

    def _write(self, symbol: str, args: tuple) -> None:
        for arg, ctype in zip(args, _abi._SIGNATURES[symbol]):  # noqa: SLF001
            if ctype is _HANDLE_OUT and arg is not None:  # a handle (or a device pointer) the library hands out
                self._next_handle += 0x100
                arg._obj.value = self._next_handle  # noqa: SLF001
        if symbol == "rl_keyword_index_info":
            for ref, v in zip(args[1:], (7, 9, 16)):  # (n_terms, n_postings, n_chunks)
                ref._obj.value = v  # noqa: SLF001
        elif symbol == "rl_keyword_store_info":
            for ref, v in zip(args[1:], (4, 4, 9, 1024)):  # (n_chunks, n_live, n_tokens, device_bytes)
                ref._obj.value = v  # noqa: SLF001
        elif symbol == "rl_keyword_analyze_begin":
            _poke(args[5], (3, 2, 4, 5, 4), C.c_int64)  # (tokens, distinct stems, stem bytes, symbols, all tokens)
        elif symbol == "rl_keyword_analyze_stems":
            _poke(args[1], tuple(b"abcd"), C.c_uint8)
            _poke(args[2], (0, 2, 4), C.c_int64)
        elif symbol == "rl_filter_set_bits":
            args[2]._obj.value, args[3]._obj.value = self.filter_set_shape  # noqa: SLF001
        elif symbol == "rl_index_arithmetic":
            args[1]._obj.value = 2  # noqa: SLF001


def _is_null(arg) -> bool:
    if arg is None:
        return True
    if isinstance(arg, int):
        return arg == 0
    if isinstance(arg, C.c_void_p):
        return not arg.value
    return False  # byref(...), a ctypes array, bytes


def _encode(symbol: str, args: tuple) -> list:
    """One recorded call as the golden file holds it: scalars by value, pointers as "ptr" / None."""
    out = []
    for arg, ctype in zip(args, _abi._SIGNATURES[symbol]):  # noqa: SLF001
        if ctype in (C.c_void_p, C.c_char_p) or hasattr(ctype, "contents"):
            out.append(None if _is_null(arg) else "ptr")
        elif ctype is C.c_double:
            out.append(float(arg))
        else:
            out.append(int(arg))
    return out


def _drive(rec: _Recorder) -> None:  # noqa: PLR0915
    """Every public wrapper of `_ops`, and `partition_similarities`, once or once per path."""
    rng = np.random.default_rng(0)
    n, dim, B, k, nq = 48, 32, 3, 4, 5  # noqa: N806
    emb = rng.standard_normal((n, dim)).astype(np.float32)
    off = np.arange(0, n + 1, 3, dtype=np.int64)
    n_chunks = int(off.size - 1)
    q = rng.standard_normal((B, dim)).astype(np.float32)
    qv = rng.standard_normal((B, nq, dim)).astype(np.float32)
    mask = rng.random(n_chunks) < 0.5
    query_filters = [mask, None, mask.copy()]  # (a repeated mask: sent once)
    limits = [5, None, 0]
    terms = [[3, 1, 3], [], [2]]

    # -- free functions --------------------------------------------------------------------------
    _ops.set_device(0)
    _ops.set_default_option("hi_search", 1)
    _ops.get_default_option("pp_schedule")
    with pytest.raises(ValueError, match="CUDA tensor"):
        _ops.synth_fill(np.zeros(4, np.float32), 1)
    _ops.pool_norm(emb, np.asarray([0, 5, 9]), np.asarray([5, 9, 48]), eps=0.25, want_f32=True)
    _ops.pool_norm(emb, [0], [48], normalize=False, want_f16=False, want_f32=True)
    _ops.adapter_apply(np.eye(dim, dtype=np.float32), q)
    _ops.adapter_apply(np.eye(dim, dtype=np.float32), q[0], want_f16=True)
    _ops.topk(rng.standard_normal((B, 40)).astype(np.float32), k)
    _ops.topk(rng.standard_normal(40).astype(np.float32), k)
    _ops.merge_topk(np.zeros((2, B, 6), np.float32), np.zeros((2, B, 6), np.int32), k)
    _ops.rrf_fuse([np.zeros((B, 6), np.int32), np.ones((B, 6), np.int32)], (0.75, 0.25), k=k)
    _ops.rrf_fuse(np.zeros((1, B, 6), np.int32), [1.0], rrf_k=10, k=k)
    _ops.rerank_order(np.zeros((B, 8), np.float32), np.zeros((B, 8), np.int32), k)
    _ops.shard_hybrid_fuse(np.zeros((2, B, 3 * 5 + 2 * 6), np.int32), num_hits=5, n_each=6, keywords=True, weights=(0.75, 0.25), k=k)
    _ops.shard_hybrid_fuse(np.zeros((2, B, 3 * 5), np.int32), num_hits=5, n_each=6, keywords=False, weights=(1.0,), rrf_k=7, k=k)

    # -- ingestion ---------------------------------------------------------------------------------
    doc_off = np.asarray([0, 20, 20, 48], np.int64)
    sizes = rng.integers(10, 90, size=n).astype(np.int64)
    _ops.pool_norm(emb, [0, 5], [5, 48])
    _chunking.partition_similarities(emb, doc_off, sizes)
    _ops.partition_chunks(np.zeros(n, np.float32), sizes, doc_off, 200)
    _ops.partition_chunklets(np.zeros(n), np.ones(n), sizes, doc_off, 200)
    _ops.partition_chunklets(np.zeros(n), np.ones(n), sizes, doc_off, 200, want_objective=False)
    cps = rng.integers(32, 127, size=n).astype(np.uint32)
    _ops.partition_sentences(cps, np.zeros(n, np.float32), doc_off)
    _ops.partition_sentences(cps, np.zeros(n, np.float16), doc_off, min_len=2, max_len=30, known=np.zeros(n), want_objective=False)
    flags = np.zeros(n, np.uint8)
    _ops.split_chunks_call(emb, doc_off, flags, flags, sizes, 200)
    _ops.split_chunks_call(emb, doc_off, None, None, sizes, 200, want_cost=True)
    cut, obj, status = _ops.partition_chunks(np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros(3, np.int64), 200)  # no call
    assert cut.shape == (0,) and obj.tolist() == [0.0, 0.0] and status.tolist() == [0, 0]

    # -- retrieval objects ---------------------------------------------------------------------------
    spans = _ops.SpanTable(np.arange(n_chunks) // 4, np.arange(n_chunks) % 4)
    spans.info()
    spans.chunk_spans(np.zeros((B, k), np.int32))
    spans.chunk_spans(np.zeros((B, k), np.int32), neighbors=None)

    index = _ops.DeviceIndex(emb, off, metric="dot")
    half = _ops.DeviceIndex(emb, storage="f16")
    half.maxsim_topk_batch(qv.astype(np.float16), k)
    half.close()

    tag_off = np.arange(n_chunks + 1, dtype=np.int64)
    store = _ops.MetadataStore(tag_off, np.zeros(n_chunks, np.int32))
    store.memory()
    device_filters, _, _ = store.filters(index, [0, 1, 2], [0, 1])
    rec.filter_set_shape = (device_filters.n_filters, device_filters.words)
    device_filters.read()
    per_query_set = device_filters.select([0, -1, 1])

    postings = SimpleNamespace(term_off=np.asarray([0, 2, 3, 3, 4]), post_chunk=np.asarray([0, 5, 2, 9]), post_tf=np.ones(4, np.int32),
                               post_term=np.asarray([0, 0, 1, 3]), idf=np.ones(4, np.float32), nrm=np.ones(n_chunks, np.float32))
    keyword = _ops.KeywordIndex(postings)
    keyword.read()
    keyword.search(terms, k)
    keyword.search(terms, k, chunk_filter=mask)
    keyword.search(terms, k, query_filters=query_filters)
    keyword.search(terms, k, query_filters=per_query_set)

    # -- the index -----------------------------------------------------------------------------------
    index.set_option("fused_topk", 0)
    index.get_option("fused_topk")
    with index.options(hi_search=0, pp_schedule=1) as same:
        assert same is index
    index.set_exact_fp32()
    assert index.arithmetic == "f16_split"
    index.live()
    index.filter_stats()
    index.memory()
    index.prepare()
    index.prepare("hi_image")

    index.search_rows(q, k)
    index.search_rows(q[0], k, chunk_filter=mask, rank_limit=9)
    assert index.rank_cut_begin(q) == B
    index.rank_cut_level(1, 9)
    index.rank_cut_level_done(1, np.zeros((B, 2048), np.int32))
    index.rank_cut_ties(9)
    index.rank_cut_finish(9, np.zeros(B, np.int32), k, chunk_filter=mask)

    index.search_chunks(q, 8, k)
    index.search_chunks(q[0], 8, k, chunk_filter=mask, rank_limit=9)
    index.search_chunks(q, 8, k, query_filters=query_filters)
    index.search_chunks(q, 8, k, chunk_filter=mask, rank_limit=limits)
    index.search_chunks(q, 8, k, rank_limit=limits, query_filters=per_query_set)
    for kw in ({}, {"keyword": keyword, "query_term_ids": terms}):
        index.hybrid_search(q, 8, 6, k, **kw)
        index.hybrid_search(q, 8, 6, k, chunk_filter=mask, rank_limit=9, **kw)
        index.hybrid_search(q, 8, 6, k, rank_limit=limits, query_filters=query_filters, rrf_k=30, **kw)
        index.hybrid_search(q, 8, 6, k, query_filters=per_query_set, **kw)
        index.search_rerank(q, 8, 6, 5, qv, k, **kw)
        index.search_rerank(q, 8, 6, 5, qv, k, chunk_filter=mask, **kw)
        index.search_rerank(q, 8, 6, 5, qv, k, rank_limit=9, **kw)
        index.search_rerank(q, 8, 6, 5, qv, k, rank_limit=limits, query_filters=query_filters, **kw)
        index.search_rerank(q, 8, 6, 5, qv, k, query_filters=per_query_set, **kw)
        index.search_rerank_spans(q, 8, 6, 5, qv, k, spans, **kw)
        index.search_rerank_spans(q, 8, 6, 5, qv, k, spans, neighbors=(), query_filters=query_filters, **kw)
        index.search_rerank_spans(q, 8, 6, 5, qv, k, spans, neighbors=(-2, -1, 1), rank_limit=limits, query_filters=per_query_set, **kw)
    index.hybrid_search(q, 8, 6, k, keyword=keyword, query_term_ids=[[], [], []])  # (no term at all)

    index.maxsim_scores(qv[0])
    index.maxsim_topk(qv[0], k)
    index.maxsim_topk(qv[0], k, chunk_filter=mask)
    index.maxsim_topk_batch(qv, k)
    index.maxsim_approx_scores(qv, kernel=1)
    index.maxsim_batch_begin(qv, k)
    index.maxsim_batch_finish(qv, np.zeros((2, B, k + 1), np.float32), 1, k)
    index.maxsim_rerank(qv, np.zeros((B, 6), np.int32))
    index.chunk_best_rows(q, np.zeros((B, 6), np.int32))
    index.chunk_best_rows(q[0], np.zeros(6, np.int32))
    index.gather_rows(np.asarray([0, 5, 7]))
    index.query_targets(q, np.zeros((B, 6), np.int32), np.ones((B, 6), bool), gap=0.125)
    with pytest.raises(ValueError, match="CUDA tensors"):
        index.time_kernel(0, qv[0], 3)

    index.append(emb[:6])
    index.append(emb[:6], chunk_sizes=[2, 4])
    store.append(np.asarray([0, 1, 1, 2], np.int64), np.zeros(2, np.int32))
    index.delete_chunks([1, 2])
    index.compact()

    # -- keyword ingestion ---------------------------------------------------------------------------
    analyzer = _ops.KeywordAnalyzer(np.arange(0x110000, dtype=np.uint32), ["the", "a"], hash_bits=8)
    n_tokens, stems, _ = analyzer.begin(cps, [0, 20, 48])
    assert (n_tokens, stems) == (3, ["ab", "cd"])
    term_ids = analyzer.finish([1, 0])
    term_ids.read()
    kstore = _ops.KeywordStore()
    kstore.append(term_ids)
    kstore.append([0, 1, 1], [0, 2, 3])
    kstore.delete([0])
    kstore.count(7, term_rank=np.arange(7))
    built = kstore.build(np.ones(7, np.float32), np.ones(4, np.float32))
    assert (built.n_terms, built.n_postings, built.n_chunks) == (7, 9, 16)
    kstore.count(7)

    for obj in (built, kstore, analyzer, keyword, per_query_set, device_filters, store, spans, index):
        obj.close()
        obj.close()  # (once is enough)


def record_trace() -> list:
    """[[symbol, [argument, ...]], ...] of one `_drive`, on a thread of its own so that its first call initialises the device."""
    rec = _Recorder()
    saved = {}
    for name, module in list(sys.modules.items()):
        if name.split(".")[0] == "raglite_amd" and "lib" in vars(module):
            saved[name] = module.lib
            module.lib = rec
    box: list = []

    def run() -> None:
        try:
            _drive(rec)
        except BaseException as exc:  # noqa: BLE001
            box.append(exc)

    try:
        t = threading.Thread(target=run)
        t.start()
        t.join()
    finally:
        for name, fn in saved.items():
            sys.modules[name].lib = fn
    if box:
        raise box[0]
    for symbol, args in rec.calls:
        sig = _abi._SIGNATURES[symbol]  # noqa: SLF001
        assert len(args) == len(sig), symbol
    return [[symbol, _encode(symbol, args)] for symbol, args in rec.calls]


@pytest.fixture(scope="module")
def trace():
    return record_trace()


def test_every_call_has_the_declared_argument_count_and_ends_in_mem_and_stream(trace):
    assert len(trace) > 100
    for symbol, args in trace:
        sig = _abi._SIGNATURES[symbol]  # noqa: SLF001
        assert len(args) == len(sig), symbol
        if len(sig) >= 2 and sig[-2:] == [C.c_int, C.c_void_p]:  # (..., int mem, hipStream_t stream)
            mem, stream = args[-2:]
            if symbol == "rl_keyword_store_append" and mem == _abi.MEM_DEVICE:  # (a `DeviceTermIds`: the analyzer's device memory)
                continue
            assert mem in (_abi.MEM_HOST, _abi.MEM_HOST | _abi.MEM_FILTERS_DEVICE), symbol  # NumPy arguments: host memory
            assert stream is None, symbol  # and the null stream


def test_every_public_wrapper_is_driven(trace):
    called = {symbol for symbol, _ in trace}
    cuda_only = {"rl_synth_fill", "rl_time_kernel"}
    wrapped = set()
    for name, module in sys.modules.items():
        if name.startswith("raglite_amd._ops"):
            wrapped |= set(re.findall(r"lib\(\)\.(rl_\w+)", Path(module.__file__).read_text()))
    assert wrapped - called == cuda_only


def test_the_trace_is_the_recorded_one(trace):
    golden = json.loads(GOLDEN.read_text())
    want = golden["calls"]
    assert [c[0] for c in trace] == [c[0] for c in want]
    for i, (got, exp) in enumerate(zip(trace, want)):
        assert got == exp, f"call {i}: {got[0]}"


if __name__ == "__main__":
    import subprocess

    commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    calls = record_trace()
    lines = ",\n".join("  " + json.dumps(c) for c in calls)
    print('{\n "written_by": ' + json.dumps(f"python -m tests.test_ops_calls_host at commit {commit}: symbols in call order; per argument "
                                            "the scalar value, or for a pointer null / \"ptr\"") + ',\n "calls": [\n' + lines + "\n ]\n}")
