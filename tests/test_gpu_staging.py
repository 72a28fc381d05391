"""The per-call staging frame ("The staging frame") at the limits of the pinned bounce buffer, where a frame can go wrong
without a score changing at ordinary sizes: a buffer just below, exactly at and just above the 256 KiB it bounces; a call whose
buffers ask for more than the 1 MiB there is, so that the last ones are copied directly; an optional output left out of a group; and
an argument error followed by a good call on the same thread.

Every case makes the same call twice, once with NumPy arguments and once with CUDA tensors.  Kernel, data and launch are the same, so
the outputs must be the same BITS; the input values are distinct, so no tie leaves an order open."""

import numpy as np
import pytest
import torch

import raglite_amd
from raglite_amd import _ops
from tests import rerank_ref as ref

pytestmark = pytest.mark.gpu


def _host(outs):
    return tuple(None if t is None else t.cpu().numpy() for t in outs)


def _same_bits(host, dev):
    assert len(host) == len(dev)
    for h, d in zip(host, dev):
        assert (h is None) == (d is None)
        if h is not None:
            assert h.dtype == d.dtype and h.shape == d.shape
            assert h.tobytes() == d.tobytes()


def _distinct(rng, shape):
    """float32 values that are all different (integers below 2^24, shuffled)."""
    return rng.permutation(int(np.prod(shape))).astype(np.float32).reshape(shape) - 1000.0


# k * 4 B = 8 KiB per query: the two outputs are 253,952 B, exactly 262,144 B (still bounced) and 270,336 B (copied directly); the
# input is above the limit in all three
@pytest.mark.parametrize("n_queries", [31, 32, 33])
def test_topk_outputs_around_the_bounce_limit(torch_cuda, n_queries):
    n, k = 4096, 2048
    scores = _distinct(np.random.default_rng(n_queries), (n_queries, n))
    host = _ops.topk(scores, k)
    dev = _ops.topk(torch.as_tensor(scores, device="cuda"), k)
    assert all(t.is_cuda for t in dev)
    _same_bits(host, _host(dev))
    want = np.argsort(-scores, axis=1, kind="stable")[:, :k]  # (distinct values: the order is the only one)
    assert np.array_equal(host[1], want)
    assert np.array_equal(host[0], np.take_along_axis(scores, want, axis=1))


def test_rerank_order_asks_for_more_bounce_space_than_there_is(torch_cuda):
    # two inputs and three outputs of 262,144 B each, and the counts: 1.25 MiB asked of a 1 MiB buffer, so the last output of full
    # size and the counts are copied directly in the middle of the call's copy-backs
    B, n_cand = 32, 2048
    rng = np.random.default_rng(5)
    scores = _distinct(rng, (B, n_cand))
    cand = rng.permutation(B * n_cand).astype(np.int32).reshape(B, n_cand)
    cand[rng.random((B, n_cand)) < 0.1] = -1  # padding: ordered last, not counted
    assert scores.nbytes == 262144
    host = _ops.rerank_order(scores, cand, n_cand)
    dev = _ops.rerank_order(torch.as_tensor(scores, device="cuda"), torch.as_tensor(cand, device="cuda"), n_cand)
    assert all(t.is_cuda for t in dev)
    _same_bits(host, _host(dev))
    ws, wc, wp, wn = ref.order(scores, cand, n_cand)
    s, c, p, n = host
    assert np.array_equal(n, wn) and np.array_equal(p, wp) and np.array_equal(c, wc)
    assert np.array_equal(ref.bits(s), ref.bits(ws))


def _partition_case():
    rng = np.random.default_rng(64)
    n, off = 64, np.asarray([0, 20, 41, 64], np.int64)
    cost = _distinct(rng, (n,)) / 64.0
    sizes = rng.integers(50, 400, size=n).astype(np.int64)
    return cost, sizes, off, 1000


def _partition_chunks(cost, sizes, off, max_size, want_objective):
    """raglite_amd.partition_chunks with the objective optional: the wrapper's own steps (it always asks for the objective)."""
    a = _ops._Args()
    _, p_cost = a.inp(cost, np.float32)
    _, p_sizes = _ops._same_side(a, sizes, np.int64)
    _, p_off = _ops._same_side(a, off, np.int64)
    n, n_docs = int(cost.shape[0]), int(off.shape[0]) - 1
    out, ptrs = _ops._partition_outputs(a, n, n_docs, want_objective)
    _ops.check(_ops.lib().rl_partition_chunks(p_cost, p_sizes, p_off, n, n_docs, int(max_size), *ptrs, a.mem, a.stream))
    return out


def _on_device(*arrays):
    return tuple(torch.as_tensor(x, device="cuda") for x in arrays)


def test_partition_with_and_without_the_optional_objective(torch_cuda):
    cost, sizes, off, max_size = _partition_case()
    runs = {}
    for want_objective in (False, True):
        host = _partition_chunks(cost, sizes, off, max_size, want_objective)
        dev = _partition_chunks(*_on_device(cost, sizes, off), max_size, want_objective)
        assert (host[1] is None) == (not want_objective)
        _same_bits(host, _host(dev))
        runs[want_objective] = host
    # leaving the objective out changes nothing else, and the public wrapper gives the run that has it
    assert runs[False][0].tobytes() == runs[True][0].tobytes() and runs[False][2].tobytes() == runs[True][2].tobytes()
    _same_bits(runs[True], raglite_amd.partition_chunks(cost, sizes, off, max_size))
    assert runs[True][0].any() and not runs[True][2].any()  # real cuts, every document solved


def test_a_good_call_after_an_argument_error_on_the_same_thread(torch_cuda):
    cost, sizes, off, max_size = _partition_case()
    want = _host(raglite_amd.partition_chunks(*_on_device(cost, sizes, off), max_size))
    with pytest.raises(ValueError, match="ascending"):  # an argument check: returns before any HIP call
        raglite_amd.partition_chunks(cost, sizes, np.asarray([0, 41, 20, 64], np.int64), max_size)
    _same_bits(raglite_amd.partition_chunks(cost, sizes, off, max_size), want)
