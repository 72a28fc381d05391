"""The native forward of a pack larger than one token block, and the batch of text queries built on it (`rl_encoder_linear_pack`,
`rl_encoder_forward_pack`, `rl_adapter_apply_rows`, `TorchTokenEmbedder.embed_pack`, `_search._embed_queries`).

The property under test is ONE: whatever goes through a pack has the bits it has in a call of its own.
  linear     a row of an M-row call (M over the 256-row block: 257, 288, 511, 512, 513, 769) equals the same row of `rl_encoder_linear`
             on the block that holds it, and of the call with that row alone; on normal data it keeps tests/encoder_ref.py's bounds.
  forward    a sequence of a 300 / 513 / 1 000-token pack equals `rl_encoder_forward` of that sequence alone, block edges included.
  queries    `_embed_queries` equals `_embed_one_by_one`, and the batched searches equal the loop of the single calls, ids and scores.
Shapes are small: a few seconds in all."""

import numpy as np
import pytest
import torch

import raglite_amd
from raglite_amd import _abi, _search
from raglite_amd import _encoder as enc
from raglite_amd._encoder import MAX_PACK_TOKENS, MAX_TOKENS, NativeEncoder
from raglite_amd._torch_embedder import EncoderShape, TorchTokenEmbedder, _build_encoder
from tests import encoder_ref as ref

pytestmark = pytest.mark.gpu

DEVICE = "cuda"
BLOCK = MAX_TOKENS  # the rows of one token block
GUARD, SENTINEL = 2, -7.0


def _bits(t):
    return t.cpu().contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


class Guarded:
    """An output of `shape` between GUARD rows (of the last dimension's width) of SENTINEL on either side."""

    def __init__(self, shape, dtype):
        n, pad = int(np.prod(shape)), GUARD * shape[-1]
        self.flat = torch.full((pad + n + pad,), SENTINEL, dtype=dtype, device=DEVICE)
        self.out, self.n, self.pad = self.flat[pad: pad + n].view(shape), n, pad

    def take(self):
        flat = self.flat.cpu()
        assert bool((flat[: self.pad] == SENTINEL).all()), "the rows in front of the output were written"
        assert bool((flat[self.pad + self.n:] == SENTINEL).all()), "the rows behind the output were written"
        return flat[self.pad: self.pad + self.n].view(self.out.shape).clone()


# ---- linear ----------------------------------------------------------------------------------------------------------------------------
# (N, K) from the small cases of tests/test_gpu_encoder_kernels.py: (32, 32) a tail-only chunk and three idle waves; (96, 96) a full chunk
# and a tail, two idle waves, three slabs; (96, 1344) 21 chunks, partial in 5 slices; (64, 2080) partial in 7 slices, the tail on wave 2
SHAPES = [(32, 32), (96, 96), (96, 1344), (64, 2080)]
MS = (257, 288, 511, 512, 513, 769)  # one row, one tile and all but one row of a second block; two whole blocks; a third of one row; three
LINEAR = [ref._make_linear(dtype, N, K, "real", (max(MS),), ref.EPILOGUES, 7000 + 10 * i + j)  # noqa: SLF001
          for j, dtype in enumerate(ref.DTYPES) for i, (N, K) in enumerate(SHAPES)]
_ids = lambda cases: [c.name for c in cases]  # noqa: E731


class LinearRun:
    def __init__(self, case, x=None):
        self.case = case
        self.x, self.W, self.bias = (case.x if x is None else x).to(DEVICE), case.W.to(DEVICE), case.bias.to(DEVICE)
        self.slices = enc.encoder_linear_slices(case.N, case.K)

    def __call__(self, lo, hi, epilogue, entry=None):
        """Rows [lo, hi) of x as a call of their own, through `entry` (the pack entry; `encoder_linear` up to a block), guards checked."""
        c, M = self.case, hi - lo  # noqa: N806
        entry = entry or (enc.encoder_linear if M <= BLOCK else enc.encoder_linear_pack)
        if epilogue == "partial":
            g = Guarded((self.slices, M, c.N), torch.float32)
            entry(self.x[lo:hi], self.W, None, "partial", out=g.out)
        else:
            g = Guarded((M, c.N), ref.tdtype(c.dtype))
            entry(self.x[lo:hi], self.W, self.bias, epilogue, out=g.out)
        return g.take()


@pytest.fixture(scope="module")
def gelu_c(torch_cuda):
    """The kernel's GELU allowance as tests/test_gpu_encoder_kernels.py derives it: twice the error of torch's own float32 erf-GELU on this
    GPU against float64, in units of u max(|v|, 1), over the pre-activations of these cases."""
    worst = max(ref.gelu_c(ref.linear_f64(c)[0].float(), torch.nn.functional.gelu(ref.linear_f64(c)[0].float().to(DEVICE))) for c in LINEAR)
    assert 0.0 < worst < 64.0, worst
    return 2.0 * worst


@pytest.mark.parametrize("case", LINEAR, ids=_ids(LINEAR))
def test_linear_rows_have_the_bits_of_their_own_block_and_of_their_own_call(torch_cuda, gelu_c, case):
    run = LinearRun(case)
    assert run.slices == ref.ksplit(case.N, case.K)
    v = ref.linear_f64(case)[0]
    per, total = ref.partial_bounds(case)
    slices64 = ref.linear_slices_f64(case)
    for epi in ref.EPILOGUES:
        blocks = {z: run(BLOCK * z, BLOCK * (z + 1), epi, enc.encoder_linear) for z in range(max(MS) // BLOCK)}  # whole blocks, the old entry
        ones = {}
        worst = 0.0
        for M in MS:  # noqa: N806
            got = run(0, M, epi)
            assert got.shape[-2:] == (M, case.N)
            for z in range(-(-M // BLOCK)):
                lo, hi = BLOCK * z, min(BLOCK * (z + 1), M)
                want = blocks[z][..., : hi - lo, :] if z in blocks else run(lo, hi, epi, enc.encoder_linear)
                if hi - lo < BLOCK:  # a partly filled block: the short call of the old entry, whatever its token tiles are
                    assert _same_bits(run(lo, hi, epi, enc.encoder_linear), want.contiguous()), (epi, M, z)
                assert _same_bits(got[..., lo:hi, :].contiguous(), want.contiguous()), (epi, M, z)
            for r in (0, BLOCK - 1, BLOCK, M - 1):
                if r not in ones:
                    ones[r] = run(r, r + 1, epi, enc.encoder_linear)
                assert _same_bits(got[..., r: r + 1, :].contiguous(), ones[r]), (epi, M, r)
            if epi == "partial":
                ratios = [ref.worst_ratio(got[s], p[:M], per[s][:M]) for s, (_, _, p, _) in enumerate(slices64)]
                acc = got[0].clone()
                for s in range(1, run.slices):
                    acc += got[s]
                ratios.append(ref.worst_ratio(acc, sum(p for _, _, p, _ in slices64)[:M], total[:M]))
                worst = max(worst, *ratios)
            elif epi == "bias":
                worst = max(worst, ref.worst_ratio(got, v[:M], ref.bias_bound(case)[:M]))
            else:
                worst = max(worst, ref.worst_ratio(got, ref.gelu64(v)[:M], ref.gelu_bound(case, gelu_c)[:M]))
        print(f"linear_pack {case.name} {epi} | worst error / bound {worst:.4f}")
        assert worst <= 1.0, (epi, worst)


@pytest.mark.parametrize("case", [c for c in LINEAR if (c.N, c.K) in ((96, 96), (96, 1344))], ids=_ids([c for c in LINEAR if (c.N, c.K) in ((96, 96), (96, 1344))]))
def test_a_nan_row_stays_in_its_row_across_a_block_edge(torch_cuda, case):
    clean = LinearRun(case)
    for M, row in ((257, 255), (257, 256), (513, 256), (513, 511), (513, 512), (769, 0)):  # noqa: N806 - either side of an edge; the clamped last row
        x = case.x.clone()
        x[row] = float("nan")
        run = LinearRun(case, x)
        others = [r for r in range(M) if r != row]
        for epi in ref.EPILOGUES:
            want, got = clean(0, M, epi), run(0, M, epi)
            assert bool(torch.isnan(got[..., row, :]).all()), (epi, M, row)
            assert _same_bits(got[..., others, :], want[..., others, :]), (epi, M, row)


def test_the_pack_entry_up_to_a_block_is_the_old_entry(torch_cuda):
    run = LinearRun(LINEAR[1])
    for M in (1, 33, 129, 256):  # noqa: N806
        for epi in ref.EPILOGUES:
            assert _same_bits(run(0, M, epi, enc.encoder_linear_pack), run(0, M, epi, enc.encoder_linear)), (M, epi)
    with pytest.raises(ValueError, match="rl_encoder_linear: M must be in"):
        run(0, 257, "bias", enc.encoder_linear)  # the old entry keeps its cap


# ---- forward ---------------------------------------------------------------------------------------------------------------------------
POSITIONS = 260
FORWARD_SHAPES = {
    "h64_f128": EncoderShape(vocab_size=1000, hidden=64, layers=2, heads=2, ffn=128, max_positions=POSITIONS, n_ctx=POSITIONS - 2),
    "bert_h64": EncoderShape(vocab_size=1000, hidden=64, layers=2, heads=2, ffn=128, max_positions=POSITIONS, n_ctx=POSITIONS, type_vocab=2,
                             position_offset=0, pad_id=0, bos_id=101, eos_id=102),
}


def pack_lengths(total, seed):
    """Sequence lengths of 2..40 tokens that add up to `total`, no sequence ending on a block edge (each edge is straddled), and a
    length-2 sequence on the rows 255 | 256."""
    rng = np.random.default_rng(seed)
    lens, pos = [], 0
    while pos < total:
        edge = (pos // BLOCK + 1) * BLOCK
        n = int(rng.integers(2, 41))
        if edge == BLOCK and pos + n >= BLOCK - 1 and total > BLOCK:  # close the first block one row short, then the split pair
            n = BLOCK - 1 - pos
            if n == 1:
                lens[-1] += 1  # (<= 41: still a short sequence)
            elif n > 0:
                lens.append(n)
            lens.append(2)
            pos = BLOCK + 1
            continue
        if pos + n == edge and edge < total:
            n += 1 if n < 40 else -1
        if total - (pos + n) < 2:  # the last sequence takes what is left
            n = total - pos
        lens.append(n)
        pos += n
    assert sum(lens) == total and min(lens) >= 2 and max(lens) <= 42
    starts = np.cumsum([0, *lens])
    assert not any(e % BLOCK == 0 for e in starts[1:-1]), "a sequence ends on a block edge"
    assert total <= BLOCK or (BLOCK - 1 in starts and lens[list(starts).index(BLOCK - 1)] == 2)
    return lens


class Case:
    def __init__(self, shape, dtype, seed=3):
        self.shape, self.dtype = shape, dtype
        state = torch.random.get_rng_state()
        torch.manual_seed(seed)
        self.module = _build_encoder(shape).to(device=DEVICE, dtype=dtype).eval()
        torch.random.set_rng_state(state)
        self.native = NativeEncoder(self.module, shape)

    def inputs(self, lens, seed=0):
        rng = np.random.default_rng(seed + 1000 * len(lens) + sum(lens))
        rows = [rng.integers(0, self.shape.vocab_size, size=n).tolist() for n in lens]
        types = [rng.integers(0, 2, size=n).tolist() for n in lens] if self.shape.type_vocab > 1 else None
        return rows, types

    def alone(self, rows, types, i):
        return self.native.forward_rows([rows[i]], None if types is None else [types[i]])  # rl_encoder_forward


@pytest.fixture(scope="module")
def cases(torch_cuda):
    made = {}

    def get(name, dtype):
        if (name, dtype) not in made:
            made[name, dtype] = Case(FORWARD_SHAPES[name], dtype)
        return made[name, dtype]

    yield get
    torch.cuda.synchronize()
    for c in made.values():
        c.native.close()


@pytest.fixture
def old_entry_calls(monkeypatch):
    calls = []
    real = _abi.lib().rl_encoder_forward
    monkeypatch.setattr(_abi.lib(), "rl_encoder_forward", lambda *a: calls.append(a[6]) or real(*a))  # (n_tokens of every call)
    return calls


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(FORWARD_SHAPES))
def test_a_sequence_has_the_bits_of_its_own_forward(cases, old_entry_calls, name, dtype):
    case = cases(name, dtype)
    for total in (300, 513, 1000):
        lens = pack_lengths(total, seed=total)
        rows, types = case.inputs(lens)
        before = case.native.pack_forwards
        got = case.native.forward_pack_rows(rows, types)
        assert case.native.pack_forwards == before + 1 and not old_entry_calls
        assert got.shape == (total, 64) and got.dtype == dtype and bool(torch.isfinite(got.float()).all())
        for i, part in enumerate(torch.split(got, lens)):
            assert torch.equal(part, case.alone(rows, types, i)), (total, i, lens[i])
        assert len(old_entry_calls) == len(lens)
        old_entry_calls.clear()
        assert torch.equal(case.native.forward_pack_rows(rows, types), got)  # run to run


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_a_long_sequence_behind_another_across_the_edge(cases, dtype):
    case = cases("h64_f128", dtype)
    rows, types = case.inputs([200, 250])  # the second: rows 200 .. 449, eight token tiles of its own when alone
    got = torch.split(case.native.forward_pack_rows(rows, types), [200, 250])
    for i in range(2):
        assert torch.equal(got[i], case.alone(rows, types, i)), i


def test_up_to_a_block_the_pack_is_the_old_forward(cases):
    for name in FORWARD_SHAPES:
        case = cases(name, torch.bfloat16)
        for lens in ([31], [2, 40, 23, 100, 91]):  # 31 and 256 tokens
            rows, types = case.inputs(lens)
            assert torch.equal(case.native.forward_pack_rows(rows, types), case.native.forward_rows(rows, types)), (name, lens)


def test_a_side_stream_and_the_arguments_of_forward_packed(cases):
    case = cases("bert_h64", torch.float16)
    lens = pack_lengths(513, seed=9)
    rows, types = case.inputs(lens)
    want = case.native.forward_pack_rows(rows, types)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = case.native.forward_pack_rows(rows, types)
    side.synchronize()
    assert torch.equal(got, want)
    flat = lambda rr: torch.tensor([t for r in rr for t in r], dtype=torch.long, device=DEVICE)  # noqa: E731
    off = torch.tensor(np.cumsum([0, *lens]), dtype=torch.int32, device=DEVICE)
    assert torch.equal(case.native.forward_pack(flat(rows), off, lens, flat(types)), want)
    with pytest.raises(ValueError, match="at most 8192 tokens"):
        case.native.forward_pack(torch.zeros(MAX_PACK_TOKENS + 1, dtype=torch.long, device=DEVICE), off, [MAX_PACK_TOKENS + 1])


def test_nothing_behind_the_workspace_in_use_is_written_and_a_small_one_is_refused(cases):
    case = cases("h64_f128", torch.bfloat16)
    lens = pack_lengths(300, seed=4)
    rows, types = case.inputs(lens)
    want = case.native.forward_pack_rows(rows, types)
    need = case.native.workspace_bytes(300)
    assert case.native.workspace_bytes(299) < need < case.native.workspace_bytes(301)
    buf, typ, n, lens = case.native._upload_rows(rows, types)  # noqa: SLF001
    args = (buf[:n], buf[n: 2 * n], buf[2 * n:], typ, len(lens), n, max(lens))
    big = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEVICE)
    out = torch.full((n + 3, 64), SENTINEL, dtype=torch.bfloat16, device=DEVICE)
    kept = case.native._workspace  # noqa: SLF001
    got = case.native.forward_pack_i32(*args, out=out[:n], workspace=big)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and bool((out[n:] == SENTINEL).all()), "rows behind out were written"
    after = big.cpu()
    assert bool((after[need:] == 0xA5).all()), "the workspace behind this pack's rows was written"
    assert float((after[:need] != 0xA5).float().mean()) > 0.9  # ... and the part in use was
    assert case.native._workspace is kept  # noqa: SLF001 - the object's own workspace was not involved
    with pytest.raises(ValueError, match="rl_encoder_forward_pack: workspace_bytes is less than"):
        case.native.forward_pack_i32(*args, workspace=big[: need - 16])
    with pytest.raises(ValueError, match="rl_encoder_forward_pack: workspace must be 16-byte aligned"):
        case.native.forward_pack_i32(*args, workspace=big[8:])
    assert torch.equal(case.native.forward_pack_i32(*args, workspace=big[:need]), want)  # exactly enough


# ---- the adapter for B rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [64, 102, 1024])
def test_adapter_rows_have_the_bits_of_the_single_call(torch_cuda, dim):
    """dim 102: the scalar lane map (no multiple of 4); 64 and 1024: the 16-byte one, a quarter of a wave and all of it four times.  B = 40 and 130: past `rl_adapter_apply`'s switch to other kernels at 5
    and at 96 queries, where its own rows are allowed to differ from the single call's."""
    rng = np.random.default_rng(dim)
    A = (rng.standard_normal((dim, dim)) / np.sqrt(dim)).astype(np.float32)  # noqa: N806
    Q = rng.standard_normal((130, dim)).astype(np.float32)  # noqa: N806
    single = np.stack([raglite_amd.adapter_apply(A, q) for q in Q[:40]])
    for B in (1, 3, 40):  # noqa: N806
        assert raglite_amd._ops.adapter_apply(A, Q[:B], rows=True).tobytes() == single[:B].tobytes(), B  # noqa: SLF001
    got = raglite_amd._ops.adapter_apply(torch.as_tensor(A, device=DEVICE), torch.as_tensor(Q, device=DEVICE), rows=True)  # noqa: SLF001
    assert got.is_cuda and got.cpu().numpy()[:40].tobytes() == single.tobytes()
    assert got.cpu().numpy()[129].tobytes() == raglite_amd.adapter_apply(A, Q[129]).tobytes()
    np.testing.assert_allclose(got.cpu().numpy(), Q.astype(np.float64) @ A.astype(np.float64).T, atol=1e-4 * np.sqrt(dim))
    half = raglite_amd._ops.adapter_apply(A, Q[:5], rows=True, want_f16=True)  # noqa: SLF001
    assert half.dtype == np.float16 and np.array_equal(half, single[:5].astype(np.float16))


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
TINY = EncoderShape(vocab_size=100_003, hidden=64, layers=2, heads=2, ffn=128, max_positions=MAX_TOKENS + 8, n_ctx=MAX_TOKENS + 6)
WORDS = ("kernel wave tile slab chunk bias gelu norm token query vector index store scan fuse rank span batch block lane "
         "stream graph cache heap").split()
N_CHUNKS = 60


def _queries(B):  # noqa: N803
    rng = np.random.default_rng(1000 + B)
    return [" ".join(rng.choice(WORDS, size=int(rng.integers(2, 7))).tolist()) + f" {b}" for b in range(B)]


@pytest.fixture(scope="module")
def world(torch_cuda):
    """A 60-chunk index (1 to 3 well separated unit rows per chunk, keyword texts, positions in 6 documents) with a query adapter, and
    two embedders with the same weights: short_forward "native" and "torch"."""
    rng = np.random.default_rng(5)
    mats = [rng.standard_normal((int(rng.integers(1, 4)), 64)).astype(np.float32) for _ in range(N_CHUNKS)]
    mats = [m / np.linalg.norm(m, axis=1, keepdims=True) for m in mats]
    ids = [f"chunk-{i}" for i in range(N_CHUNKS)]
    docs = [" ".join(rng.choice(WORDS, size=12).tolist()) + f" text {i}" for i in range(N_CHUNKS)]
    adapter = (np.eye(64) + 0.2 * rng.standard_normal((64, 64))).astype(np.float32)
    gi = raglite_amd.GpuIndex(ids, mats, docs=docs, keyword_texts=docs, positions=[(f"doc-{i // 10}", i % 10) for i in range(N_CHUNKS)],
                              query_adapter=adapter)
    native = TorchTokenEmbedder(TINY, device=DEVICE, seed=5, short_forward="native")
    plain = TorchTokenEmbedder(TINY, device=DEVICE, seed=5)
    raglite_amd.attach_index(gi)
    yield gi, native, plain
    raglite_amd.detach_index()
    raglite_amd.set_embedder_factory(None)
    gi.close()


def _use(emb):
    raglite_amd.set_embedder_factory(lambda config: emb)


@pytest.mark.parametrize("adapter", [False, True], ids=["plain", "adapter"])
@pytest.mark.parametrize("B", [1, 5, 40])
def test_the_query_matrix_is_the_loops(world, old_entry_calls, B, adapter):  # noqa: N803
    gi, native, _ = world
    _use(native)
    cfg = raglite_amd.HotPathConfig(vector_search_query_adapter=adapter)
    queries = _queries(B)
    want = _search._embed_one_by_one(queries, None, cfg, gi)  # noqa: SLF001
    assert len(old_entry_calls) == B and (B < 40 or sum(old_entry_calls) > MAX_TOKENS)  # 40 queries: more tokens than one block
    packs, calls = native._native.pack_forwards, native.embed_calls  # noqa: SLF001
    got = _search._embed_queries(queries, None, cfg, gi)  # noqa: SLF001
    assert native._native.pack_forwards == packs + 1 and native.embed_calls == calls + 1 and len(old_entry_calls) == B  # noqa: SLF001
    assert got.dtype == np.float32 and got.shape == (B, 64) and np.array_equal(got, want)
    if adapter:
        assert not np.array_equal(got, _search._embed_queries(queries, None, raglite_amd.HotPathConfig(vector_search_query_adapter=False), gi))  # noqa: SLF001
    mixed = [queries[0], want[0] * 2, *queries[1:]]
    assert np.array_equal(_search._embed_queries(mixed, None, cfg, gi), _search._embed_one_by_one(mixed, None, cfg, gi))  # noqa: SLF001


def _chunks_loop(gi, cfg, queries, fn):
    lookup = _search._ref_lookup(gi)  # noqa: SLF001
    return [[c.id for c in raglite_amd.search_and_rerank_chunks(q, num_results=4, search=fn, config=cfg, chunk_lookup=lookup)] for q in queries]


@pytest.mark.parametrize("adapter", [False, True], ids=["plain", "adapter"])
@pytest.mark.parametrize("B", [1, 5, 40])
def test_the_batched_searches_equal_the_loop_with_one_forward_per_batch(world, old_entry_calls, B, adapter):  # noqa: N803
    gi, native, _ = world
    _use(native)
    ranker = raglite_amd.MaxSimRanker.from_embedder(gi, native)
    cfg = raglite_amd.HotPathConfig(vector_search_query_adapter=adapter, reranker=ranker)
    queries = _queries(B)
    native.embed(queries[0])  # (the handle exists)
    n = native._native  # noqa: SLF001

    def one_forward(call):
        packs = n.pack_forwards
        old_entry_calls.clear()
        out = call()
        assert n.pack_forwards == packs + 1 and not old_entry_calls, (n.pack_forwards - packs, len(old_entry_calls))
        return out

    got = one_forward(lambda: raglite_amd.vector_search_batch(queries, num_results=5, config=cfg, index=gi))
    assert got == [raglite_amd.vector_search(q, num_results=5, config=cfg, index=gi) for q in queries]  # ids and float scores, ==
    assert all(len(ids) == 5 for ids, _ in got)
    got = one_forward(lambda: raglite_amd.hybrid_search_batch(queries, num_results=5, config=cfg, index=gi))
    assert got == [raglite_amd.hybrid_search(q, num_results=5, config=cfg, index=gi) for q in queries]
    for search, fn in (("hybrid", raglite_amd.hybrid_search), ("vector", raglite_amd.vector_search)):
        got = one_forward(lambda s=search: raglite_amd.search_and_rerank_chunks_batch(queries, num_results=4, search=s, config=cfg, index=gi))
        assert got == _chunks_loop(gi, cfg, queries, fn), search
        spans = one_forward(lambda s=search: raglite_amd.search_and_rerank_chunk_spans_batch(queries, num_results=4, search=s, config=cfg, index=gi))
        assert spans == [raglite_amd.search_and_rerank_chunk_spans(q, num_results=4, search=fn, config=cfg) for q in queries], search
        assert all(sp and sp[0].score >= sp[-1].score for sp in spans)
    vecs = one_forward(lambda: ranker._token_vectors(queries))  # noqa: SLF001
    assert all(np.array_equal(v, ranker.query_encoder(q)) for v, q in zip(vecs, queries))


def test_a_ranker_over_another_embedder_makes_its_own_forward(world, old_entry_calls):
    gi, native, _ = world
    _use(native)
    twin = TorchTokenEmbedder(TINY, device=DEVICE, seed=5, short_forward="native")
    cfg = raglite_amd.HotPathConfig(vector_search_query_adapter=False, reranker=raglite_amd.MaxSimRanker.from_embedder(gi, twin))
    queries = _queries(5)
    native.embed(queries[0])
    packs = native._native.pack_forwards  # noqa: SLF001
    got = raglite_amd.search_and_rerank_chunks_batch(queries, num_results=4, search="hybrid", config=cfg, index=gi)
    assert native._native.pack_forwards == packs + 1 and twin._native.pack_forwards == 1  # noqa: SLF001 - one each: two objects
    assert got == _chunks_loop(gi, cfg, queries, raglite_amd.hybrid_search)


def test_with_the_torch_route_the_calls_and_the_results_are_the_parents(world, old_entry_calls):
    gi, _, plain = world
    _use(plain)
    ranker = raglite_amd.MaxSimRanker.from_embedder(gi, plain)
    cfg = raglite_amd.HotPathConfig(vector_search_query_adapter=True, reranker=ranker)
    queries = _queries(5)
    assert plain.embed_pack(queries) is None
    calls = plain.embed_calls
    got = raglite_amd.hybrid_search_batch(queries, num_results=5, config=cfg, index=gi)
    assert plain.embed_calls == calls + 5  # one embed() per query, as before
    assert got == [raglite_amd.hybrid_search(q, num_results=5, config=cfg, index=gi) for q in queries]
    calls = plain.embed_calls
    got = raglite_amd.search_and_rerank_chunks_batch(queries, num_results=4, search="hybrid", config=cfg, index=gi)
    assert plain.embed_calls == calls + 10  # the encoder runs twice per query: the pooled vector and the token vectors
    assert got == _chunks_loop(gi, cfg, queries, raglite_amd.hybrid_search)
    assert not old_entry_calls and plain._native is None  # noqa: SLF001 - no native forward of either kind


def test_embed_pack_returns_embeds_matrices_and_keeps_the_cap_of_embed(world, old_entry_calls):
    _, native, _ = world
    queries = _queries(40)
    mats = native.embed_pack(queries)
    assert len(mats) == 40 and sum(len(m) for m in mats) > MAX_TOKENS
    for m, q in zip(mats, queries):
        alone = native.embed(q)
        assert m.dtype == torch.float32 and m.is_cuda and torch.equal(m, alone)
    assert native.embed_pack([]) == []
    long = " ".join(["ab"] * (MAX_TOKENS // 2))  # MAX_TOKENS + 1 rows: `embed()` takes torch's route for it, so the pack does not take it
    assert native.embed_pack([queries[0], long]) is None
    n_old = len(old_entry_calls)
    assert native.embed(long).shape == (MAX_TOKENS + 1, 64) and len(old_entry_calls) == n_old
