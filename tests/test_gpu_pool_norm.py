"""The kernels of pool_norm.hip (`rl_pool_norm`) against float64 (`oracle.pool_norm_cast` through tests/pool_norm_ref.py): every
instantiation `launch_pool_norm` can dispatch, and the hand-made fp64 -> fp16 cast on every fp16 rounding midpoint.

  register-staged  pool_norm_kernel<NV, 4>, NV = 1, 2, 3, 4, 6, 8, 16 and pool_norm_kernel<NV, 1>, NV = 1, 2, 4, 8, 16, 32: at both ends of
                   their ranges of widths (`test_every_register_instantiation`), with more spans than waves (`test_more_spans_than_waves`);
  LDS-DMA          pool_norm_dma_kernel<1>, <2>, <4> (dim 256, 512, 1024 from 64 spans up): 1, 2, 3, 7, 8, 10 and 47 workgroups, span lengths
                   around the ring depth, empty spans at every place of a claim, a capped grid, non-finite rows next to healthy spans,
                   reuse of the span counters; and bit for bit against the register-staged kernel on the same spans.

Every comparison is exact (bits), or goes through `pool_norm_ref.assert_rounds_like` with the derived `pool_norm_ref.bound`: the output
is the reference rounded once, except where the reference lies within the bound of a rounding boundary, and such elements are at most
1e-6 of a batch (tests/test_pool_norm_ref_host.py shows the restated arithmetic has none on these batches).  No tolerance is tuned;
scripts/pool_norm_error.py prints how far inside the bound the kernels sit (profiles/pool_norm_error.txt).

The calls go to `lib().rl_pool_norm` with outputs that start as a sentinel (fp32 -7.0, fp16 bits 0x5555) and have one spare row: a row a
kernel never writes cannot hold the right answer from an earlier call, and nothing may be written past `n_spans` rows."""

import numpy as np
import pytest

from raglite_amd import _abi, _ops
from raglite_amd._abi import lib
from tests import pool_norm_ref as ref

pytestmark = pytest.mark.gpu

F16_SENTINEL = ref.SENTINEL_F16_BITS


def pool(tokens, begins, ends, normalize=True, eps=0.0, f32=True, f16=True, torch=None, status=_abi.RL_OK, f16_rows_only=False):
    """`rl_pool_norm` through the call frame -> (float32 [S, dim] or None, fp16 bits uint16 [S, dim] or None).  Host pointers, or CUDA
    tensors on torch's current stream where `torch` is given (`tokens` may already be one).  Asserts the status, that no sentinel
    survives in the S rows (`f16_rows_only`: no whole row of them, where 0x5555 is a possible result) and that the spare row is
    untouched; with a status other than RL_OK, that nothing was written at all."""
    a = _ops._Args()  # noqa: SLF001
    tok, p_tok = a.inp(tokens if torch is None or not isinstance(tokens, np.ndarray) else torch.tensor(tokens, device="cuda"), np.float32)
    n_rows, dim = int(tok.shape[0]), int(tok.shape[1])
    n = len(begins)
    p_b, p_e = a.same_side(np.array(begins), np.int64)[1], a.same_side(np.array(ends), np.int64)[1]
    o32 = o16 = p32 = p16 = None
    if f32:
        o32, p32 = a.inp(np.full((n + 1, dim), -7.0, np.float32) if torch is None else torch.full((n + 1, dim), -7.0, device="cuda"), np.float32)
    if f16:
        start = (np.full((n + 1, dim), F16_SENTINEL, np.uint16).view(np.float16) if torch is None
                 else torch.full((n + 1, dim), F16_SENTINEL, dtype=torch.int16, device="cuda").view(torch.float16))
        o16, p16 = a.inp(start, np.float16)
        assert o16 is start
    a.ensure_device()
    rc = lib().rl_pool_norm(p_tok, n_rows, dim, p_b, p_e, n, int(normalize), float(eps), p32, p16, a.mem, a.stream)
    if rc == _abi.RL_ERR_HIP:  # a device error: nothing more is started on this GPU by this session
        pytest.exit(f"rl_pool_norm: {_abi.last_error()}", returncode=3)
    assert rc == status, (rc, _abi.last_error())
    if torch is not None:
        try:
            o32 = None if o32 is None else o32.cpu().numpy()
            o16 = None if o16 is None else o16.view(torch.int16).cpu().numpy()
        except RuntimeError as exc:  # the kernel faulted: likewise
            pytest.exit(f"rl_pool_norm: {exc}", returncode=3)
    o16 = None if o16 is None else o16.view(np.uint16)
    written = slice(0, n) if status == _abi.RL_OK else slice(0, 0)
    if o32 is not None:
        assert np.all(o32[written.stop:] == ref.SENTINEL_F32), "fp32 written past n_spans rows"
        assert not np.any(o32[written] == ref.SENTINEL_F32), ("fp32 rows never written", np.flatnonzero(np.any(o32[written] == ref.SENTINEL_F32, axis=1))[:8])
    if o16 is not None:
        assert np.all(o16[written.stop:] == F16_SENTINEL), "fp16 written past n_spans rows"
        left = np.all(o16[written] == F16_SENTINEL, axis=1) if f16_rows_only else np.any(o16[written] == F16_SENTINEL, axis=1)
        assert not np.any(left), ("fp16 rows never written", np.flatnonzero(left)[:8])
    return (None if o32 is None else o32[:n]), (None if o16 is None else o16[:n])


def check(batch, got32, got16, normalize, eps=0.0, what=""):
    """Both outputs against the reference of `batch` under the comparator and the cap -> (excepted fp32, excepted fp16)."""
    r64, _r16, bnd = batch.ref(normalize, eps)
    n32 = ref.assert_rounds_like(got32, r64, bnd, np.float32, f"{what} fp32")
    n16 = ref.assert_rounds_like(got16, r64, bnd, np.float16, f"{what} fp16")
    print(f"{what}: {n32} fp32 and {n16} fp16 excepted elements of {r64.size}")
    assert n32 <= ref.cap(r64.size) and n16 <= ref.cap(r64.size), (what, n32, n16, r64.size)
    return n32, n16


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def single_outputs_match(batch, both32, both16, normalize, torch, eps=0.0):
    only32, none = pool(batch.tokens, batch.begins, batch.ends, normalize, eps, f16=False, torch=torch)
    assert none is None and same_bits(only32, both32), "out_f32 alone"
    none, only16 = pool(batch.tokens, batch.begins, batch.ends, normalize, eps, f32=False, torch=torch)
    assert none is None and same_bits(only16, both16), "out_f16 alone"


def kernel_id(dim):
    nv, vec = ref.instantiation(dim)
    return f"pool_norm_kernel<{nv},{vec}>-dim{dim}"


# ---- 1. every register-staged instantiation ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", ref.VEC4_DIMS + ref.SCALAR_DIMS, ids=kernel_id)
def test_every_register_instantiation(torch_cuda, dim):
    """14 spans (fewer than 64: dims 256, 512 and 1024 stay on this kernel) of 0, 1, 2, 3, 4, 5, 7, 8, 9 and 11 rows: every combination of
    the 4-row, 2-row and 1-row loops; one span overlapping others, one listed twice, the list out of order.  Both outputs, each alone,
    normalize on and off, the eps guard on ordinary spans; host pointers give the bits of CUDA tensors."""
    batch = ref.registers_batch(dim)
    for normalize, eps in ((True, 0.0), (False, 0.0), (True, 2.2e-16)):
        got32, got16 = pool(batch.tokens, batch.begins, batch.ends, normalize, eps, torch=torch_cuda)
        check(batch, got32, got16, normalize, eps, f"{kernel_id(dim)} normalize={normalize} eps={eps}")
        empty = batch.begins == batch.ends
        assert empty.sum() == 2 and np.all(np.isnan(got32[empty])) and np.all((got16[empty] & 0x7FFF) > 0x7C00)
        single_outputs_match(batch, got32, got16, normalize, torch_cuda, eps)
        host32, host16 = pool(batch.tokens, batch.begins, batch.ends, normalize, eps)
        assert same_bits(host32, got32) and same_bits(host16, got16), "host pointers"
    pairs = [(i, j) for i in range(batch.n_spans) for j in range(i + 1, batch.n_spans)
             if batch.begins[i] == batch.begins[j] and batch.ends[i] == batch.ends[j] and batch.ends[i] - batch.begins[i] > 1]
    assert pairs and all(same_bits(got32[i], got32[j]) for i, j in pairs)  # the span listed twice


@pytest.mark.parametrize("dim", [2049, 4100])
def test_unsupported_widths_write_nothing(torch_cuda, dim):
    """Above 2048 and no multiple of 4 (scalar lanes would need more than 32 values), above 4096: RL_ERR_UNSUPPORTED, named."""
    tokens = np.ones((3, dim), np.float32)
    for torch in (None, torch_cuda):
        pool(tokens, [0, 1], [1, 3], torch=torch, status=_abi.RL_ERR_UNSUPPORTED)
        err = _abi.last_error()
        assert "rl_pool_norm" in err and "4096" in err and "2048" in err, err


# ---- 2. the grid-stride loop ---------------------------------------------------------------------------------------------------------------

def test_more_spans_than_waves(torch_cuda):
    """`launch_t` starts at most 8 generations of what `persistent_grid` answers, workgroups of 4 waves, one span per wave and trip.
    For `pool_norm_kernel<1, 4>` `persistent_grid` answers 1 536 workgroups on the MI355X (256 CUs, 6 workgroups per CU): 12 288
    workgroups, 49 152 waves.  (8 per CU is the most the occupancy query can answer, 32 wave slots per CU: 65 536 waves.)  70 000 spans
    of 0 .. 2 rows at dim 4 are more than either: 20 848 waves take a second trip through `s += n_waves`.  Every span is checked."""
    batch = ref.stride_batch()
    assert batch.n_spans == ref.STRIDE_SPANS > 256 * 8 * 8 * 4
    for normalize in (True, False):
        got32, got16 = pool(batch.tokens, batch.begins, batch.ends, normalize, torch=torch_cuda)
        check(batch, got32, got16, normalize, what=f"70 000 spans normalize={normalize}")


# ---- 3. the DMA kernel ---------------------------------------------------------------------------------------------------------------------

def dma_id(dim):
    return f"pool_norm_dma_kernel<{dim // 256}>-dim{dim}"


@pytest.mark.parametrize("n_spans", ref.DMA_SPANS)
@pytest.mark.parametrize("dim", ref.DMA_DIMS, ids=dma_id)
def test_dma_kernel(torch_cuda, dim, n_spans):
    """One call per `n_spans`; the grid is ceil(n_spans / 64) workgroups of 8 waves and min(that, 8) span queues:
       64 -> 1 workgroup, 1 queue;  65, 130 -> 2, 3 workgroups (fewer queues than XCDs; queues of 32 + 33 and 43 + 43 + 44 spans);
       448, 512 -> 7, 8 workgroups;  577 -> 10 workgroups on 8 queues (two queues with 16 waves, six with 8; 72 or 73 spans each);
       3001 -> 47 workgroups (queues with 48 and 40 waves).
    With fewer than 8 spans per wave left in a queue the claims shrink (`want` < 8) and the last one is cut short (`count < want`): at 65
    spans a queue has 4 spans per wave, so every claim is of 4 or fewer.  Span lengths {0, 1, 2, RING - 1, RING, RING + 1, 2 RING + 1, 37},
    RING = 8, 8, 4 rows, one span of 300 rows and one of all 1 200.  Every span is checked: both outputs, each alone, normalize on and off."""
    batch = ref.dma_batch(dim, n_spans)
    for normalize in (True, False):
        got32, got16 = pool(batch.tokens, batch.begins, batch.ends, normalize, torch=torch_cuda)
        check(batch, got32, got16, normalize, what=f"{dma_id(dim)} {n_spans} spans normalize={normalize}")
        single_outputs_match(batch, got32, got16, normalize, torch_cuda)
        if n_spans == 130:  # host pointers: once per kernel
            host32, host16 = pool(batch.tokens, batch.begins, batch.ends, normalize)
            assert same_bits(host32, got32) and same_bits(host16, got16), "host pointers"


# ---- 4. empty spans on the DMA path --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ref.EMPTY_CASES)
@pytest.mark.parametrize("dim", [256, 1024], ids=dma_id)
def test_dma_empty_spans(torch_cuda, dim, case):
    """512 spans: 8 workgroups, 8 queues of 64 spans (`x_first` = 64 q) with 8 waves each, so `x_left / x_waves` is 8 at every wave's first
    claim; the waves start together, and their eight first claims take the whole queue: claim k of queue q is spans 64 q + 8 k .. + 7,
    whichever wave gets it.  (A wave that came back for a second claim before the others had made their first would take fewer spans
    from the same place; sixteen empty spans in a row hold a whole claim of 8 or fewer wherever the claims begin.)
       first       span 0: claim 0 of queue 0 opens on an empty span (`fetch_skip` before the first fetch);
       last        span 511: claim 7 of queue 7 ends on one (`fetch_skip` stops at the last span of the claim);
       sixteen     spans 72 .. 87: claims 1 and 2 of queue 1 are empty altogether (no row is ever fetched);
       scattered   spans 8, 11, 12, 15 (first, middle pair and last of claim 1 of queue 0), 131, 133, 135 (alternating, claim 0 of queue 2),
                   200 .. 206 (claim 1 of queue 3 keeps only its last span): `fetch_skip` inside `fetch_row`, while rows are in flight;
       last_queue  the last n_spans / 8 spans, 448 .. 511: queue 7 holds nothing but empty spans;
       all         every span is empty.
    An empty span is NaN in both outputs (np.mean of zero rows), every other span is what it is without them."""
    batch, emptied = ref.empties_batch(dim, case)
    assert batch.n_spans == 512 and np.array_equal(np.flatnonzero(batch.begins == batch.ends), emptied)
    for normalize in (True, False):
        got32, got16 = pool(batch.tokens, batch.begins, batch.ends, normalize, torch=torch_cuda)
        assert np.all(np.isnan(got32[emptied])) and np.all((got16[emptied] & 0x7FFF) > 0x7C00)
        check(batch, got32, got16, normalize, what=f"{dma_id(dim)} {case} normalize={normalize}")
        full, _ = ref.empties_batch(dim, "first")
        keep = np.setdiff1d(np.arange(1, 512), emptied)
        if len(keep):
            ref32, ref16 = pool(full.tokens, full.begins, full.ends, normalize, torch=torch_cuda)
            assert same_bits(got32[keep], ref32[keep]) and same_bits(got16[keep], ref16[keep])


# ---- 5. the capped DMA grid ----------------------------------------------------------------------------------------------------------------

def test_dma_grid_capped_at_the_cu_count(torch_cuda):
    """20 000 spans of 0 .. 3 rows at dim 256 (`pool_norm_dma_kernel<1>`): ceil(20 000 / 64) = 313 workgroups are asked for, the CU count
    (256) is launched, so every wave goes round the claim loop many times, down to claims of one span.  Every span is checked."""
    batch = ref.capped_grid_batch()
    n_cu = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    assert batch.n_spans == ref.CAPPED_SPANS > 64 * n_cu
    for normalize in (True, False):
        got32, got16 = pool(batch.tokens, batch.begins, batch.ends, normalize, torch=torch_cuda)
        check(batch, got32, got16, normalize, what=f"20 000 spans normalize={normalize}")


# ---- 6. DMA == register-staged, bit for bit ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", ref.DMA_DIMS, ids=dma_id)
def test_dma_and_register_kernels_give_the_same_bits(torch_cuda, dim):
    """The spans of `test_dma_kernel` in one call (`pool_norm_dma_kernel<dim / 256>`) and in calls of at most 63 spans
    (`pool_norm_kernel<dim / 256, 4>`, the same lane-to-column map, the same statements): the same bits in both outputs, normalize on and
    off.  Then the same tokens through a view that starts one float into its buffer, `flat[1:1 + T * dim].view(T, dim)`: 4-byte aligned
    only, so the call falls back to `pool_norm_kernel<dim / 64, 1>` (<4,1>, <8,1>, <16,1>) whatever the number of spans.  Its sums are the
    same sums (normalize off: the same bits); its norm is summed in another order, so normalize on goes through the comparator."""
    torch = torch_cuda
    tokens = torch.tensor(ref.dma_tokens(dim), device="cuda")
    flat = torch.zeros(ref.DMA_ROWS * dim + 4, device="cuda")
    flat[1:1 + ref.DMA_ROWS * dim] = tokens.flatten()
    shifted = flat[1:1 + ref.DMA_ROWS * dim].view(ref.DMA_ROWS, dim)
    assert tokens.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    for n_spans in ref.DMA_SPANS:
        batch = ref.dma_batch(dim, n_spans)
        for normalize in (True, False):
            dma32, dma16 = pool(tokens, batch.begins, batch.ends, normalize, torch=torch)
            parts = [pool(tokens, batch.begins[i:i + 63], batch.ends[i:i + 63], normalize, torch=torch) for i in range(0, n_spans, 63)]
            assert same_bits(np.concatenate([p[0] for p in parts]), dma32), (n_spans, normalize)
            assert same_bits(np.concatenate([p[1] for p in parts]), dma16), (n_spans, normalize)
            off32, off16 = pool(shifted, batch.begins, batch.ends, normalize, torch=torch)
            if normalize:
                check(batch, off32, off16, True, what=f"misaligned dim {dim} {n_spans} spans")
            else:
                assert same_bits(off32, dma32) and same_bits(off16, dma16), (n_spans, "misaligned")


# ---- 7. the cast ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [256, 512, 1024, 4096], ids=lambda d: dma_id(d) if d <= 1024 else kernel_id(d))
def test_cast_on_every_fp16_midpoint(torch_cuda, dim):
    """`f64_to_f16_bits` on all 31 744 positive fp16 rounding midpoints m (65520, the midpoint to overflow, included), on m - t/2 and
    m + t/2 with t = 2^(floor(log2 m) - 30), and on their negatives: 190 464 values, each the exact float64 mean of a two-row span
    (2 m, +-t), normalize off.  744 / 372 / 186 spans at dim 256 / 512 / 1024 (DMA kernels), 47 at 4096 (`pool_norm_kernel<16, 4>`).
    The fp16 output is astype(float16) of the mean, bit for bit, with no exception: subnormals, ties to even, overflow to +-inf, and the
    values that rounding through fp32 first gets wrong (a third of the set).  The fp32 output is the mean rounded once."""
    tokens, begins, ends, mean = ref.midpoint_spans(dim)
    with np.errstate(over="ignore"):
        want16, want32 = mean.astype(np.float16), mean.astype(np.float32)
    got32, got16 = pool(tokens, begins, ends, normalize=False, torch=torch_cuda, f16_rows_only=True)
    wrong = np.flatnonzero(got16.ravel() != want16.view(np.uint16).ravel())
    assert len(wrong) == 0, (len(wrong), [(float(mean.ravel()[i]).hex(), hex(int(got16.ravel()[i])), hex(int(want16.view(np.uint16).ravel()[i]))) for i in wrong[:4]])
    assert same_bits(got32, want32)
    assert int(np.isinf(got16.view(np.float16)).sum()) == 4
    _, alone16 = pool(tokens, begins, ends, normalize=False, f32=False, torch=torch_cuda, f16_rows_only=True)
    assert same_bits(alone16, got16)


# ---- 8. isolation and guards ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [256, 1024], ids=dma_id)
def test_dma_nonfinite_rows_stay_in_their_span(torch_cuda, dim):
    """96 spans (2 workgroups, claims of 6 and fewer): span 10 holds a NaN row, span 40 a +inf and a -inf row, span 41 (its neighbour in
    the ring) FLT_MAX rows, span 77 a +inf row.  The other 92 spans have the bits of the same call with those rows replaced by ones:
    the ring is shared, the sums are not.  The four spans give what NumPy gives: NaN; NaN (inf - inf); FLT_MAX in fp32 and inf in fp16
    without normalising, 1 / sqrt(dim) with; +inf without normalising, NaN (inf / inf) with."""
    bad, good = ref.isolation_batch(dim, False), ref.isolation_batch(dim, True)
    others = np.setdiff1d(np.arange(96), list(ref.SPECIAL))
    for normalize in (True, False):
        got32, got16 = pool(bad.tokens, bad.begins, bad.ends, normalize, torch=torch_cuda)
        want32, want16 = pool(good.tokens, good.begins, good.ends, normalize, torch=torch_cuda)
        assert same_bits(got32[others], want32[others]) and same_bits(got16[others], want16[others])
        check(good, want32, want16, normalize, what=f"healthy dim {dim} normalize={normalize}")
        check(bad, got32, got16, normalize, what=f"non-finite dim {dim} normalize={normalize}")
        f16 = got16.view(np.float16)
        assert np.all(np.isnan(got32[[10, 40]])) and np.all(np.isnan(f16[[10, 40]]))
        if normalize:
            assert np.all(got32[41] == np.float32(1 / np.sqrt(dim))) and np.all(np.isnan(got32[77])) and np.all(np.isnan(f16[77]))
        else:
            assert np.all(got32[41] == np.finfo(np.float32).max) and np.all(f16[41] == np.inf) and np.all(got32[77] == np.inf) and np.all(f16[77] == np.inf)


@pytest.mark.parametrize("n_spans", [12, 70], ids=["pool_norm_kernel<1,4>", "pool_norm_dma_kernel<1>"])
def test_eps_guard_on_zero_vectors(torch_cuda, n_spans):
    """Spans of zero rows (not empty spans: rows of zeros) at dim 256: the mean is 0, its norm 0.  eps = 2.2e-16: 0 / max(0, eps) = +0 in both
    outputs; eps = 0: 0 / 0 = NaN.  The other spans are what the reference gives under the same eps.  12 spans: register-staged; 70: DMA."""
    batch, zero = ref.zero_rows_batch(n_spans)
    for eps in (2.2e-16, 0.0):
        got32, got16 = pool(batch.tokens, batch.begins, batch.ends, True, eps, torch=torch_cuda)
        check(batch, got32, got16, True, eps, what=f"{n_spans} spans eps={eps}")
        if eps > 0:
            assert np.all(got32[zero].view(np.uint32) == 0) and np.all(got16[zero] == 0)
        else:
            assert np.all(np.isnan(got32[zero])) and np.all(np.isnan(got16[zero].view(np.float16)))
    got32, got16 = pool(batch.tokens, batch.begins, batch.ends, False, torch=torch_cuda)
    assert np.all(got32[zero].view(np.uint32) == 0) and np.all(got16[zero] == 0)  # +0.0, also from rows of -0.0 (include/raglite_hip.h)


# ---- 9. the span-counter pool --------------------------------------------------------------------------------------------------------------

def test_dma_counter_slots_are_reused(torch_cuda):
    """A DMA launch takes one of 64 slots of span counters and zeroes it on its stream.  140 launches back to back (dim 256, 64 spans),
    alternating between two streams, go round the pool more than twice: each gives the bits of the first."""
    torch = torch_cuda
    batch = ref.dma_batch(256, 64)
    first32, first16 = pool(batch.tokens, batch.begins, batch.ends, torch=torch)
    check(batch, first32, first16, True, what="first launch")
    tokens = torch.tensor(batch.tokens, device="cuda")
    begins, ends = torch.tensor(batch.begins, device="cuda"), torch.tensor(batch.ends, device="cuda")
    outs = [(torch.full((65, 256), -7.0, device="cuda"), torch.full((65, 256), F16_SENTINEL, dtype=torch.int16, device="cuda")) for _ in range(140)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for i, (o32, o16) in enumerate(outs):
        with torch.cuda.stream(streams[i % 2]):
            rc = lib().rl_pool_norm(tokens.data_ptr(), ref.DMA_ROWS, 256, begins.data_ptr(), ends.data_ptr(), 64, 1, 0.0, o32.data_ptr(), o16.data_ptr(),
                                    _abi.MEM_DEVICE, torch.cuda.current_stream().cuda_stream)
        assert rc == _abi.RL_OK, _abi.last_error()
    torch.cuda.synchronize()
    all32 = torch.stack([o[0] for o in outs]).cpu().numpy()
    all16 = torch.stack([o[1] for o in outs]).cpu().numpy().view(np.uint16)
    for i in range(140):
        assert same_bits(all32[i, :64], first32) and same_bits(all16[i, :64], first16), i
        assert np.all(all32[i, 64] == ref.SENTINEL_F32) and np.all(all16[i, 64] == F16_SENTINEL), i
