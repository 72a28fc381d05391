"""The native cross-encoder rerank on the GPU: `rl_encoder_classify_pack` behind `NativeEncoder.classify_rows`,
`TorchCrossEncoderRanker(forward="native")`, its `rank_batch`, and the batched search entries over it.

Accuracy: per (shape, dtype) the RMS error of the native logits against the float64 twin of the same 16-bit weights, pooled over more
than 200 pairs, must be at most 1.1 x the RMS error of torch's own `forward_packed` logits against that twin -- the margin
tests/test_gpu_encoder_native.py holds the trunk to; the figures go to profiles/cross_encoder_native_error.txt.  Everything else is
equality of bits: a pair's logit wherever it is packed, `rank_batch` against the loop of `rank`, the batched searches against the loop
of the single-query ones."""

import zlib
from pathlib import Path

import numpy as np
import pytest
import torch

import raglite_amd
from raglite_amd import _abi, _search
from raglite_amd._cross_encoder import CrossEncoderShape, TorchCrossEncoderRanker
from raglite_amd._encoder import MAX_PACK_TOKENS, NativeEncoder
from raglite_amd._torch_embedder import _build_encoder, pack_runs, packed_inputs

pytestmark = pytest.mark.gpu


def _shape(hidden, heads, ffn):
    return CrossEncoderShape(vocab_size=1000, hidden=hidden, layers=2, heads=heads, ffn=ffn, max_positions=512, n_ctx=512)


SHAPES = {"bert_h64": _shape(64, 2, 128), "bert_h192": _shape(192, 3, 320), "minilm_w": _shape(384, 12, 1536)}
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
SEVENTEEN = [3, 9, 30, 5, 17, 4, 21, 11, 3, 7, 33, 40, 19, 6, 44, 12, 38]  # 302 tokens; the minimum first, in the middle, and a long last
# one pair of 3 tokens ([CLS][SEP][SEP]); one of 512; first tokens on rows 255 and 256; seventeen mixed pairs
PACKS = [[3], [512], [255, 7, 9], [256, 5], SEVENTEEN]
MANY = 200  # and one pack of this many pairs of 3 .. 40 tokens: the RMS is over 226 logits, not over a handful


def _pairs(shape, lens, seed):
    """Encoded pairs of the given lengths: ([CLS] q [SEP] d [SEP], length of the first segment), random ids, every split of the segments."""
    rng = np.random.default_rng(seed)
    out = []
    for n in lens:
        body = rng.integers(103, shape.vocab_size, size=n - 3).tolist()
        nq = int(rng.integers(0, n - 2))
        out.append(([shape.bos_id, *body[:nq], shape.eos_id, *body[nq:], shape.eos_id], nq + 2))
    return out


def _types(pairs):
    return [[0] * first + [1] * (len(row) - first) for row, first in pairs]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


class Case:
    """One (shape, dtype): a native ranker on the GPU and the float64 twin of its module on the CPU."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = shape, dtype
        self.ranker = TorchCrossEncoderRanker(shape, device="cuda", dtype=dtype, forward="native", seed=3)
        self.twin = _build_encoder(shape).double().eval()
        self.twin.load_state_dict({k: v.double().cpu() for k, v in self.ranker.encoder.state_dict().items()})

    def native(self, pairs):
        return self.ranker._native_logits(pairs)  # noqa: SLF001

    def three(self, pairs):
        rows = [p[0] for p in pairs]
        ids, off, lens, typ = packed_inputs(rows, "cuda", _types(pairs))
        with torch.inference_mode():
            truth = self.twin.forward_packed(ids.cpu(), off.cpu(), lens, typ.cpu())
            ref = self.ranker.encoder.forward_packed(ids, off, lens, typ).float()
        got = self.native(pairs)
        assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (len(pairs),)
        return truth, ref.double().cpu(), got.double().cpu()


@pytest.fixture(scope="module")
def cases(torch_cuda):
    made = {}

    def get(name, dtype):
        if (name, dtype) not in made:
            made[name, dtype] = Case(SHAPES[name], DTYPES[dtype])
        return made[name, dtype]

    yield get
    for c in made.values():
        if c.ranker.native is not None:
            c.ranker.native.close()


@pytest.fixture(scope="module")
def error_log():
    lines = []
    yield lines
    try:  # (a read-only checkout keeps the committed figures)
        out = Path(__file__).resolve().parent.parent / "profiles" / "cross_encoder_native_error.txt"
        head = ("# tests/test_gpu_cross_encoder_native.py: RMS error of the logits against the float64 forward of the same 16-bit weights, pooled\n"
                "# over all pairs of a (shape, dtype)\n"
                "# shape dtype pairs | torch forward_packed (reference) | native | native / reference  (asserted <= 1.1)\n")
        out.write_text(head + "".join(sorted(lines)))
    except OSError:
        pass


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", list(SHAPES))
def test_native_logits_are_as_accurate_as_the_torch_route(cases, error_log, name, dtype):
    case = cases(name, dtype)
    rng = np.random.default_rng(7)
    packs = [*PACKS, rng.integers(3, 41, size=MANY).tolist()]
    err_ref, err_got = [], []
    for i, lens in enumerate(packs):
        before = case.ranker.native.pack_forwards if case.ranker.native is not None else 0
        truth, ref, got = case.three(_pairs(case.shape, lens, 100 + i))
        assert case.ranker.native.pack_forwards == before + 1, "a pack of at most 8192 tokens is one forward"
        assert bool(torch.isfinite(got).all())
        err_ref.append(ref - truth)
        err_got.append(got - truth)
    e_ref = float(torch.sqrt(torch.mean(torch.cat(err_ref) ** 2)))
    e_got = float(torch.sqrt(torch.mean(torch.cat(err_got) ** 2)))
    n = sum(len(p) for p in packs)
    assert n >= 200
    line = f"{name} {dtype} {n} | {e_ref:.4e} | {e_got:.4e} | {e_got / e_ref:.3f}\n"
    print(line, end="")
    error_log.append(line)
    assert e_got <= 1.1 * e_ref, line


@pytest.mark.parametrize("name,dtype", [("bert_h64", "bf16"), ("bert_h192", "fp16"), ("minilm_w", "bf16")])
def test_a_pair_has_the_same_bits_in_every_pack(cases, name, dtype):
    case = cases(name, dtype)
    sh = case.shape
    target = _pairs(sh, [20], 1)[0]
    mine = _pairs(sh, [9, 31, 14], 2)  # its query's other candidates
    others = _pairs(sh, [40, 3, 25, 60, 17], 3)  # other queries' pairs
    alone = case.native([target])
    assert torch.equal(_bits(alone), _bits(case.native([target]))), "run to run"
    among = case.native([mine[0], target, *mine[1:]])[1]
    middle = case.native([*others[:3], mine[0], target, *mine[1:], *others[3:]])[4]
    straddle = case.native([*_pairs(sh, [200, 46], 4), target])[2]  # rows 246 .. 265: across the edge of the first token block
    at_edge = case.native([*_pairs(sh, [200, 56], 5), target])[2]  # first token on row 256
    filler = _pairs(sh, [63] * 130, 6)  # 8190 tokens: the target no longer fits the first pack
    before = case.ranker.native.pack_forwards
    second = case.native([*filler, target, *mine])
    assert case.ranker.native.pack_forwards == before + 2
    for what, got in (("among", among), ("middle", middle), ("straddle", straddle), ("at_edge", at_edge), ("second pack", second[130])):
        assert torch.equal(_bits(got.reshape(1)), _bits(alone)), what
    assert torch.equal(_bits(second[:130]), _bits(case.native(filler))), "the first pack's pairs too"


def test_packs_just_under_and_just_over_the_cap(cases):
    case = cases("bert_h64", "bf16")
    under = _pairs(case.shape, [64] * 127 + [63], 8)  # 8191 tokens
    assert sum(len(r) for r, _ in under) == MAX_PACK_TOKENS - 1
    native = case.ranker._native_encoder()  # noqa: SLF001
    n0 = native.pack_forwards
    a = case.native(under)
    assert native.pack_forwards == n0 + 1
    full = [*under[:-1], *_pairs(case.shape, [64], 9)]  # exactly 8192
    case.native(full)
    assert native.pack_forwards == n0 + 2
    over = [*under, *_pairs(case.shape, [3], 10)]  # 8194: two forwards, of 8191 and 3 tokens
    b = case.native(over)
    assert native.pack_forwards == n0 + 4
    assert torch.equal(_bits(b[:-1]), _bits(a)) and torch.equal(_bits(b[-1:]), _bits(case.native([over[-1]])))
    with pytest.raises(ValueError, match="RL_ENCODER_MAX_PACK_TOKENS"):
        native.classify_rows([r for r, _ in over], _types(over))


# ---- rank_batch against the loop of rank -------------------------------------------------------------------------------------------
WORDS = [f"w{i}" for i in range(80)]


def _texts(rng, B):  # noqa: N803
    text = lambda n: " ".join(rng.choice(WORDS, size=n))  # noqa: E731
    queries = [text(int(rng.integers(1, 8))) + f" q{b}" for b in range(B)]
    docs = []
    for b in range(B):
        n = 0 if b % 7 == 2 else int(rng.integers(1, 10))
        ds = [text(int(rng.integers(1, 30))) for _ in range(n)]
        if n > 2:
            ds[-1] = ds[0]  # duplicates: equal scores, which must keep input order
        if n and b % 5 == 0:
            ds[n // 2] = text(150)  # longer than max_length: truncate_pair cuts it
        docs.append(ds)
    return queries, docs


def _same_results(got, want):
    assert got.query == want.query and len(got.results) == len(want.results)
    for g, w in zip(got.results, want.results):
        assert (g.doc_id, g.rank, g.text) == (w.doc_id, w.rank, w.text)
        assert np.float32(g.score).tobytes() == np.float32(w.score).tobytes()


@pytest.mark.parametrize("B", [1, 7, 40])
@pytest.mark.parametrize("name,dtype", [("bert_h64", "bf16"), ("minilm_w", "fp16")])
def test_rank_batch_equals_rank(cases, name, dtype, B):  # noqa: N803
    ranker = cases(name, dtype).ranker
    ranker.max_length = 96
    try:
        queries, docs = _texts(np.random.default_rng(B), B)
        if B > 1:
            assert any(not d for d in docs) and any(len(ranker.tokenizer.encode(x)) > 96 for d in docs for x in d)
        ids = [None if b % 2 else [1000 + 7 * i for i in range(len(d))] for b, d in enumerate(docs)]
        native = ranker._native_encoder()  # noqa: SLF001
        n0 = native.pack_forwards
        got = ranker.rank_batch(queries, docs, ids)
        lens = [len(p[0]) for q, d in zip(queries, docs) for p in ranker.encode_pairs(q, d)]
        assert native.pack_forwards - n0 == len(pack_runs(lens, MAX_PACK_TOKENS)) <= 2, "one forward per pack, not per query"
        for b in range(B):
            want = ranker.rank(queries[b], docs[b], ids[b])
            _same_results(got[b], want)
            if len(docs[b]) > 2:  # the duplicate pair: equal scores, the earlier one first
                order = [r.doc_id for r in want.results]
                first, last = (ids[b][0], ids[b][-1]) if ids[b] is not None else (0, len(docs[b]) - 1)
                assert order.index(first) < order.index(last)
                assert np.float32(want.results[order.index(first)].score).tobytes() == np.float32(want.results[order.index(last)].score).tobytes()
        for z, q, d in zip(ranker.logits_batch(queries, docs), queries, docs):
            assert torch.equal(_bits(z), _bits(ranker.logits(q, d)))
        for s, q, d in zip(ranker.score_batch(queries, docs), queries, docs):
            assert s.dtype == np.float32 and s.tobytes() == ranker.score(q, d).tobytes()
    finally:
        ranker.max_length = 512


def test_rank_batch_cuts_a_large_batch_into_packs(cases):
    ranker = cases("bert_h64", "bf16").ranker
    rng = np.random.default_rng(12)
    queries = [f"w{b} w{b + 1} q{b}" for b in range(24)]
    docs = [[" ".join(rng.choice(WORDS, size=40)) for _ in range(10)] for _ in queries]  # 240 pairs of 40-word docs: more than 8192 tokens
    native = ranker._native_encoder()  # noqa: SLF001
    lens = [len(p[0]) for q, d in zip(queries, docs) for p in ranker.encode_pairs(q, d)]
    runs = pack_runs(lens, MAX_PACK_TOKENS)
    assert 2 <= len(runs) < len(queries) and sum(lens) > MAX_PACK_TOKENS
    n0 = native.pack_forwards
    got = ranker.rank_batch(queries, docs)
    assert native.pack_forwards - n0 == len(runs), "one forward per pack, not per query"
    cut = runs[0][1] // 10  # the query whose pairs the first cut falls among (or in front of)
    for b in sorted({0, max(cut - 1, 0), cut, min(cut + 1, 23), 23}):
        _same_results(got[b], ranker.rank(queries[b], docs[b]))


# ---- the batched search entries -----------------------------------------------------------------------------------------------------
DIM, N_CHUNKS = 64, 200


def _hash_ints(text, shape):
    return np.random.default_rng(zlib.crc32(text.encode())).integers(-3, 4, size=shape).astype(np.float32)


@pytest.fixture(scope="module")
def corpus(torch_cuda):
    rng = np.random.default_rng(2025)
    mats = [rng.integers(-3, 4, size=(int(rng.integers(1, 4)), DIM)).astype(np.float32) for _ in range(N_CHUNKS)]
    bodies = [" ".join(rng.choice(WORDS[:24], size=int(rng.integers(3, 25)))) for _ in range(N_CHUNKS)]
    gi = raglite_amd.GpuIndex([f"chunk-{i:04d}" for i in range(N_CHUNKS)], mats, metric="dot", docs=bodies,
                              metadata=[{"topic": [f"t{i % 3}"]} for i in range(N_CHUNKS)], keyword_texts=bodies)
    yield gi
    gi.close()


@pytest.fixture
def pipeline(corpus, cases, monkeypatch):
    monkeypatch.setattr(_search, "embed_strings", lambda strings, config=None: np.stack([_hash_ints(s, (DIM,)) for s in strings]))
    raglite_amd.attach_index(corpus)
    ranker = cases("bert_h64", "bf16").ranker
    yield raglite_amd.HotPathConfig(vector_search_query_adapter=False, reranker=ranker), ranker
    raglite_amd.detach_index()


def _lookup(gi):
    return lambda ids: [gi.docs[gi.ordinal_of(cid)] for cid in ids]


@pytest.mark.parametrize("search", ["hybrid", "vector"])
def test_search_and_rerank_batch_equals_the_loop_in_one_forward_per_pack(corpus, pipeline, search):
    gi, (cfg, ranker) = corpus, pipeline
    rng = np.random.default_rng(4)
    B = 8  # noqa: N806  (six queries with results x 32 candidates of about 20 tokens: one pack)
    queries = [" ".join(rng.choice(WORDS[:24], size=int(rng.integers(1, 5)))) + f" q{b}" for b in range(B)]
    filters = [[None, {"topic": "t1"}, {"topic": "none"}, {"topic": ["t2"]}][b % 4] for b in range(B)]
    fn = raglite_amd.hybrid_search if search == "hybrid" else raglite_amd.vector_search
    native = ranker._native_encoder()  # noqa: SLF001
    n0 = native.pack_forwards
    got = raglite_amd.search_and_rerank_chunks_batch(queries, search=search, config=cfg, index=gi, metadata_filter=filters, chunk_lookup=_lookup(gi))
    batch_forwards = native.pack_forwards - n0
    want = [raglite_amd.search_and_rerank_chunks(q, search=fn, config=cfg, metadata_filter=f, chunk_lookup=_lookup(gi)) for q, f in zip(queries, filters)]
    loop_forwards = native.pack_forwards - n0 - batch_forwards
    assert got == want
    assert all(len(x) == 8 for b, x in enumerate(got) if b % 4 != 2) and all(x == [] for b, x in enumerate(got) if b % 4 == 2)
    assert batch_forwards == 1 and loop_forwards == sum(1 for x in want if x), "one forward per pack, not per query"
    plain = raglite_amd.HotPathConfig(vector_search_query_adapter=False)
    searched = raglite_amd.search_and_rerank_chunks_batch(queries, search=search, config=plain, index=gi, metadata_filter=filters, chunk_lookup=_lookup(gi))
    assert any(a != b for a, b in zip(got, searched)), "the rerank changed some query's order"
    # ids need a lookup, as in the loop
    with pytest.raises(ValueError, match="chunk_lookup"):
        raglite_amd.search_and_rerank_chunks_batch(queries, search=search, config=cfg, index=gi)
    with pytest.raises(ValueError, match="chunk_lookup"):
        raglite_amd.search_and_rerank_chunks(queries[0], search=fn, config=cfg)
    # rerank_chunks_batch over the searched ids
    found = raglite_amd.search_and_rerank_chunks_batch(queries, search=search, config=plain, index=gi, metadata_filter=filters, num_results=32)
    n0 = native.pack_forwards
    reranked = raglite_amd.rerank_chunks_batch(queries, found, config=cfg, chunk_lookup=_lookup(gi))
    assert native.pack_forwards - n0 == 1
    for q, ids, (got_ids, got_scores) in zip(queries, found, reranked):
        res = ranker.rank(q, _lookup(gi)(ids)) if ids else _search.RankedResults([], q)
        assert got_ids == [ids[r.doc_id] for r in res.results]
        assert [np.float32(s).tobytes() for s in got_scores] == [np.float32(r.score).tobytes() for r in res.results]
        assert _lookup(gi)(got_ids) == raglite_amd.rerank_chunks(q, ids, config=cfg, chunk_lookup=_lookup(gi))


def test_a_torch_cross_encoder_and_a_dict_go_per_query(corpus, pipeline):
    gi, (cfg, ranker) = corpus, pipeline
    torch_ranker = TorchCrossEncoderRanker(SHAPES["bert_h64"], device="cuda", seed=3)
    queries = ["w1 w2 q0", "w3 q1", "w4 w5 w6 q2"]
    native = ranker._native_encoder()  # noqa: SLF001
    for reranker in (torch_ranker, {"other": ranker}):
        c = raglite_amd.HotPathConfig(vector_search_query_adapter=False, reranker=reranker)
        n0 = native.pack_forwards
        got = raglite_amd.search_and_rerank_chunks_batch(queries, config=c, index=gi, chunk_lookup=_lookup(gi))
        assert native.pack_forwards - n0 == (0 if reranker is torch_ranker else len(queries))
        assert got == [raglite_amd.search_and_rerank_chunks(q, search=raglite_amd.hybrid_search, config=c, chunk_lookup=_lookup(gi)) for q in queries]
        with pytest.raises(ValueError, match="MaxSimRanker over the index"):
            raglite_amd.rerank_chunks_batch(queries, [[], [], []], config=c, index=gi, chunk_lookup=_lookup(gi))


# ---- forward="torch" gives today's bits ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batching", ["padded", "packed"])
def test_forward_torch_is_the_ranker_without_the_argument(torch_cuda, batching):
    a = TorchCrossEncoderRanker(SHAPES["bert_h64"], device="cuda", seed=5, batching=batching, forward="torch")
    b = TorchCrossEncoderRanker(SHAPES["bert_h64"], device="cuda", seed=5, batching=batching)
    queries, docs = _texts(np.random.default_rng(3), 7)
    for q, d in zip(queries, docs):
        assert torch.equal(_bits(a.logits(q, d)), _bits(b.logits(q, d)))
    for g, (q, d) in zip(a.rank_batch(queries, docs), zip(queries, docs)):
        _same_results(g, b.rank(q, d))
    assert a.native is None and b.native is None and b.forward == "torch"


# ---- stream, scratch, weights -------------------------------------------------------------------------------------------------------
def test_side_stream_and_guard_bytes(cases):
    case = cases("bert_h192", "fp16")
    pairs = _pairs(case.shape, [30, 3, 280, 17], 21)
    want = case.native(pairs)
    native = case.ranker._native_encoder()  # noqa: SLF001
    rows, types = [p[0] for p in pairs], _types(pairs)
    n, n_seqs = sum(map(len, rows)), len(rows)
    need, pack = native.classify_workspace_bytes(n, n_seqs), native.workspace_bytes(n)
    assert need >= pack + 2 * n * case.shape.hidden, "at least the pack bytes, and the final rows"
    assert native.classify_workspace_bytes(n + 1, n_seqs) > need >= native.classify_workspace_bytes(n - 1, n_seqs)
    assert native.classify_workspace_bytes(n, n_seqs + 1) >= need >= native.classify_workspace_bytes(n, 1)
    assert native.classify_workspace_bytes(0, 0) == 0
    guard = 256
    ws = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((n_seqs + 8,), -7.0, dtype=torch.float32, device="cuda")
    buf, typ, _, lens = native._upload_rows(rows, types)  # noqa: SLF001
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = native.classify_pack_i32(buf[:n], buf[n: 2 * n], buf[3 * n:], typ, n_seqs, n, max(lens), out=out, workspace=ws[:need])
    side.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(_bits(out[:n_seqs]), _bits(want))
    assert bool((out[n_seqs:] == -7.0).all()), "behind out_logits"
    assert bool((ws[need:] == 0xA5).all()), "behind workspace_bytes"
    with pytest.raises(ValueError, match="workspace_bytes"):
        native.classify_pack_i32(buf[:n], buf[n: 2 * n], buf[3 * n:], typ, n_seqs, n, max(lens), workspace=ws[: need - 16])
    torch.cuda.synchronize()


def test_a_handle_without_a_head_is_refused(torch_cuda):
    plain = CrossEncoderShape(vocab_size=1000, hidden=64, layers=1, heads=2, ffn=128, max_positions=64, n_ctx=64, classifier=False)
    native = NativeEncoder(_build_encoder(plain).to("cuda", torch.bfloat16), plain)
    try:
        with pytest.raises(ValueError, match="classifier"):
            native.classify_rows([[101, 102, 102]], [[0, 0, 1]])
        native._ensure_handle()  # noqa: SLF001
        ints = torch.zeros(16, dtype=torch.int32, device="cuda")
        out, ws = torch.zeros(4, device="cuda"), torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
        st = _abi.lib().rl_encoder_classify_pack(native._handle, ints.data_ptr(), ints.data_ptr(), None, ints.data_ptr(), 1, 3, 3, out.data_ptr(),  # noqa: SLF001
                                                 ws.data_ptr(), ws.numel(), _abi.MEM_DEVICE, None)
        assert st == _abi.RL_ERR_INVALID and "no head" in _abi.last_error()
    finally:
        native.close()


def test_new_weights_and_a_new_dtype_are_picked_up(torch_cuda):
    shape = SHAPES["bert_h64"]
    a = TorchCrossEncoderRanker(shape, device="cuda", dtype=torch.bfloat16, forward="native", seed=1)
    b = TorchCrossEncoderRanker(shape, device="cuda", dtype=torch.bfloat16, forward="native", seed=2)
    pairs = _pairs(shape, [12, 3, 40], 30)
    try:
        za, zb = a._native_logits(pairs), b._native_logits(pairs)  # noqa: SLF001
        assert not torch.equal(_bits(za), _bits(zb))
        a.encoder.load_state_dict(b.encoder.state_dict())
        assert torch.equal(_bits(a._native_logits(pairs)), _bits(zb))  # noqa: SLF001
        a.encoder.to(torch.float16)
        b16 = TorchCrossEncoderRanker(shape, device="cuda", dtype=torch.float16, forward="native", seed=9)
        b16.encoder.load_state_dict({k: v.to(torch.float16) for k, v in b.encoder.state_dict().items()})
        z16 = a._native_logits(pairs)  # noqa: SLF001
        assert torch.equal(_bits(z16), _bits(b16._native_logits(pairs))) and not torch.equal(_bits(z16), _bits(zb))  # noqa: SLF001
        a.encoder.to(torch.float32)  # no native route in fp32: the old one, silently
        assert not a._native_applies() and bool(torch.isfinite(a.logits("w1 w2", ["w3 w4", "w5"])).all())  # noqa: SLF001
        b16.native.close()
    finally:
        for r in (a, b):
            if r.native is not None:
                r.native.close()
