"""`raglite_amd.merge_topk` (`rl_merge_topk`, csrc/select.hip `merge_topk_kernel`) as a public call, against `merge_ref` of
tests/long_lists_ref.py (an explicit Python sort on (key, id), itself checked against a brute-force sort on the CPU): every sort size
from 64 to 8192 records, `n_lists * k_in` off a power of two, k from 1 past the number of records, padding ids scattered through the
lists, empty lists, NaN / inf / subnormals, signed zeros (include/raglite_hip.h: +0.0 before -0.0 whatever the ids) and ties that
span lists and exceed k.  Every score bit and id of every slot is compared; host arrays and CUDA tensors must give the same bytes."""

import numpy as np
import pytest
import torch

import raglite_amd
from raglite_amd import _abi
from tests import long_lists_ref as ref

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 3, 64), (1, 3, 65), (2, 5, 100), (3, 7, 683), (4, 2, 2048), (8, 4, 1024), (64, 3, 128), (8192, 1, 1), (2, 300, 50)]


def _ks(total):
    """k in {1, 5, min(2048, total)} and, where the call allows one, a k past the number of records."""
    ks = {1, 5, min(ref.K_MAX, total)}
    if total < ref.K_MAX:
        ks.add(min(ref.K_MAX, total + 7))
    return sorted(ks)


def _check(s, i, ks, where, device=False, want=None):
    """merge_topk at every k against the restatement; returns the restatement's (scores, ids) at the largest k for a second call."""
    want_s, want_i = want or ref.merge_ref(s, i, max(ks))  # (a shorter list is its prefix, then padding: one Python sort per content)
    n_valid = (np.asarray(i) >= 0).sum(axis=(0, 2))
    for k in ks:
        if device:
            gs, gi = raglite_amd.merge_topk(torch.as_tensor(s, device="cuda"), torch.as_tensor(i, device="cuda"), k)
            assert gs.is_cuda and gi.is_cuda
            gs, gi = gs.cpu().numpy(), gi.cpu().numpy()
        else:
            gs, gi = raglite_amd.merge_topk(s, i, k)
        assert gs.shape == gi.shape == (s.shape[1], k) and gs.dtype == np.float32 and gi.dtype == np.int32
        ws, wi = want_s[:, :k], want_i[:, :k]
        bad = np.nonzero((gi != wi) | (ref.bits(gs) != ref.bits(ws)))
        assert bad[0].size == 0, (f"{where} k {k}: first difference at query {bad[0][0]} slot {bad[1][0]}: got "
                                  f"({ref.bits(gs)[bad[0][0], bad[1][0]]:#010x}, {gi[bad[0][0], bad[1][0]]}), expected "
                                  f"({ref.bits(ws)[bad[0][0], bad[1][0]]:#010x}, {wi[bad[0][0], bad[1][0]]})")
        real = np.arange(k)[None, :] < np.minimum(n_valid, k)[:, None]
        assert ((gi >= 0) == real).all() and np.isneginf(gs[~real]).all(), f"{where} k {k}: the (-inf, -1) tail"
    return want_s, want_i


@pytest.mark.parametrize("n_lists,B,k_in", SHAPES)
def test_merge_equals_the_restatement(torch_cuda, n_lists, B, k_in):
    rng = np.random.default_rng(n_lists * 100_003 + B * 1009 + k_in)
    total = n_lists * k_in
    ks = _ks(total)
    assert (max(ks) > total) == (total < ref.K_MAX)
    for name, (s, i) in ref.merge_contents(rng, n_lists, B, k_in).items():
        where = f"({n_lists}, {B}, {k_in}) {name}"
        want = _check(s, i, ks, where)
        _check(s, i, ks, where, device=True, want=want)
        want_i = want[1]
        if name == "three_values" and total >= 64:  # the ties span the lists and exceed k: the ids decide
            top = s.transpose(1, 0, 2).reshape(B, total).max(axis=1)
            tied = (s.transpose(1, 0, 2).reshape(B, total) == top[:, None]).sum(axis=1)
            assert (tied > 5).all() and all(np.all(np.diff(want_i[b, :5]) > 0) for b in range(B))
        if name == "all_padding":
            assert (want_i == -1).all()
    if total >= ref.K_MAX:  # no k past the records exists here: k stops at 2048
        s, i = ref.merge_contents(rng, n_lists, 1, k_in)["normal"]
        with pytest.raises(_abi.UnsupportedError, match="2048"):
            raglite_amd.merge_topk(s, i, ref.K_MAX + 1)


def test_signed_zero_block_and_the_stated_example(torch_cuda):
    """The rule of include/raglite_hip.h: +0.0 before -0.0 whatever the ids -- the kernel, the restatement and the host merge agree."""
    s = np.array([-0.0, 0.0], dtype=np.float32).reshape(1, 1, 2)
    i = np.array([3, 7], dtype=np.int32).reshape(1, 1, 2)
    gs, gi = raglite_amd.merge_topk(s, i, 2)
    assert gi.tolist() == [[7, 3]] and ref.bits(gs).tolist() == [[0x00000000, 0x80000000]]
    hs, hi = raglite_amd.merge_topk_host(s, i, 2)
    assert hi.tolist() == gi.tolist() and ref.bits(hs).tolist() == ref.bits(gs).tolist()
    # 4 lists x 600: the zeros of one sign interleave with the other sign's in id order, a few -1 / 0 / +1 around them
    rng = np.random.default_rng(8)
    s, i = ref.merge_contents(rng, 4, 3, 600)["signed_zeros"]
    want = _check(s, i, [1, 700, 2048], "signed zeros")
    _check(s, i, [2048], "signed zeros", device=True, want=want)
    want_i = want[1]
    flat_s, flat_i = s.transpose(1, 0, 2).reshape(3, -1), i.transpose(1, 0, 2).reshape(3, -1)
    for b in range(3):
        pos, neg = np.sort(flat_i[b][ref.bits(flat_s[b]) == 0]), np.sort(flat_i[b][ref.bits(flat_s[b]) == 0x80000000])
        ones = int((flat_s[b] == 1).sum())
        assert len(pos) > 100 and len(neg) > 100 and neg[0] < pos[-1]  # ids interleave: id order alone would mix the two signs
        assert np.array_equal(want_i[b, ones : ones + len(pos)], pos) and np.array_equal(want_i[b, ones + len(pos) : ones + len(pos) + len(neg)][:50], neg[:50])
    hs, hi = raglite_amd.merge_topk_host(s, i, 2048)
    gs, gi = raglite_amd.merge_topk(s, i, 2048)
    assert np.array_equal(hi, gi) and np.array_equal(ref.bits(hs), ref.bits(gs))


def test_more_than_8192_entries_is_refused(torch_cuda):
    for n_lists, k_in in ((8193, 1), (1, 8193), (3, 2731), (5, 2048)):
        s = np.zeros((n_lists, 1, k_in), dtype=np.float32)
        i = np.arange(n_lists * k_in, dtype=np.int32).reshape(n_lists, 1, k_in)
        with pytest.raises(_abi.UnsupportedError, match="8192"):
            raglite_amd.merge_topk(s, i, 10)
        with pytest.raises(_abi.UnsupportedError, match="8192"):
            raglite_amd.merge_topk(torch.as_tensor(s, device="cuda"), torch.as_tensor(i, device="cuda"), 10)
    s, i = np.zeros((2, 1, 4096), dtype=np.float32), np.arange(8192, dtype=np.int32).reshape(2, 1, 4096)
    gs, gi = raglite_amd.merge_topk(s, i, 3)  # exactly 8192 is the limit
    assert gi.tolist() == [[0, 1, 2]]
