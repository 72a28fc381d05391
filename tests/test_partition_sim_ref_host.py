"""`tests/partition_sim_ref.py`, the float64 statement that tests/test_gpu_partition_sim.py holds the kernels against, is itself held
against the reference here: the oracle's float32 restatement of `_split_chunks.py:54-72` and the cost vectors the real
`split_chunks` produced (tests/golden/split_chunks.npz).  Also the one argument check of `rl_partition_similarity` that no other
host test makes: the width limit, refused before any HIP call."""

import numpy as np

from oracle import oracle
from raglite_amd import _abi
from tests import partition_sim_ref as ref
from tests.test_oracle_golden import _split_cases


def test_statement_agrees_with_the_oracle_and_the_reference_cost_on_the_golden_documents():
    seen = 0
    for chunklets, X, _max_size, cost, _sizes, _chunks in _split_cases():
        if len(cost) == 0:
            continue
        seen += 1
        lens = np.asarray([len(c) for c in chunklets])
        sel = oracle.nonoutlying_mask(lens)
        sim, branch, smallest, norms = ref.document(X, sel)
        assert branch == "mod" and smallest > 0.1 and int(sel.sum()) > 1, (branch, smallest)  # the golden documents are ordinary ones
        assert sim[-1] == 0.0
        tol = ref.tolerance(X.shape[1], [branch], [0, len(X)], norms)[:-1]
        want32 = oracle.partition_similarity(X, lens)
        assert np.all(np.abs(sim[:-1] - want32) <= tol), float(np.max(np.abs(sim[:-1] - want32) / tol))
        got = oracle.heading_adjusted(sim[:-1], chunklets)
        for want in (oracle.heading_adjusted(want32, chunklets), cost):
            assert np.all(np.abs(got - want) <= tol), float(np.max(np.abs(got - want) / tol))
    assert seen == 4


def test_branches_of_the_statement():
    rng = np.random.default_rng(0)
    X = rng.standard_normal((5, 24))
    plain, branch, smallest, norms = ref.document(X, None)
    assert branch == "no_selection" and np.isnan(smallest) and np.isnan(norms).all()
    Xh = X / np.linalg.norm(X, axis=1, keepdims=True)
    want = np.maximum((np.sum(Xh[:-1] * Xh[1:], axis=1) + 1) / 2, float(ref.SQRT_EPS32))
    assert np.allclose(plain[:-1], want, rtol=0, atol=1e-15) and plain[-1] == 0.0
    assert ref.document(X, np.zeros(5, np.uint8))[1] == "no_selection"
    # one selected row: degenerate by rule, the plain values
    one, branch, smallest, _ = ref.document(X, [0, 0, 1, 0, 0])
    assert branch == "degenerate" and smallest == 0.0 and np.array_equal(one, plain)
    # all selected rows one axis: exactly degenerate, whatever the other rows are
    Y = X.copy()
    Y[[1, 3]] = 0.0
    Y[[1, 3], 7] = [2.0, 0.5]
    axis, branch, smallest, _ = ref.document(Y, [0, 1, 0, 1, 0])
    assert branch == "degenerate" and smallest == 0.0 and np.array_equal(axis, ref.document(Y, None)[0])
    # several selected rows: the discourse vector is removed, and the result differs
    mod, branch, smallest, norms = ref.document(X, [1, 1, 0, 1, 0])
    assert branch == "mod" and smallest == norms.min() > 0.3 and not np.allclose(mod, plain)
    d = Xh[[0, 1, 3]].mean(axis=0)
    d /= np.linalg.norm(d)
    M = Xh - np.outer(Xh @ d, d)
    M /= np.linalg.norm(M, axis=1, keepdims=True)
    assert np.allclose(mod[:-1], (np.sum(M[:-1] * M[1:], axis=1) + 1) / 2, rtol=0, atol=1e-15)
    # opposite rows hit the floor, which is the float32 constant
    floor = ref.document(np.asarray([[1.0, 0.0], [-3.0, 0.0]]))[0]
    assert floor[0] == float(np.float32(np.sqrt(np.finfo(np.float32).eps))) and floor[1] == 0.0
    # batches: per document, empty ones included
    off = np.asarray([0, 0, 5, 5, 10])
    sim, branches, smallest, _ = ref.batch(np.concatenate((X, Y)), off, np.asarray([1, 1, 0, 1, 0, 0, 1, 0, 1, 0]))
    assert branches == ["no_selection", "mod", "no_selection", "degenerate"] and np.isnan(smallest[[0, 2]]).all()
    assert np.array_equal(sim[:5], mod) and np.array_equal(sim[5:], axis)
    assert ref.tol_plain(64) == 17 * 2.0 ** -24 and ref.tol_plain(65) == 18 * 2.0 ** -24 and ref.tol_plain(4096) == 80 * 2.0 ** -24


def test_partition_similarity_refuses_dim_4097_before_any_hip_call():
    n, dim = 3, 4097
    X = np.ones((n, dim), np.float32)
    sel = np.ones(n, np.uint8)
    out = np.full(n, -7.0, np.float32)
    off = np.asarray([0, 1, 3], np.int64)
    for p_off, n_docs in ((off.ctypes.data, 2), (None, 1)):
        rc = _abi.lib().rl_partition_similarity(X.ctypes.data, n, dim, p_off, n_docs, sel.ctypes.data, out.ctypes.data, _abi.MEM_HOST, None)
        assert rc == _abi.RL_ERR_UNSUPPORTED
        err = _abi.last_error()
        assert "rl_partition_similarity" in err and "4096" in err, err
    assert np.all(out == -7.0)
