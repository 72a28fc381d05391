"""BM25 statistics across shards (raglite_amd/_keyword.py `shard_counts` / `build_shard_from_term_ids`): every shard's idf, nrm and
impacts are bitwise the slice of ONE build over the whole corpus, and the vocabulary ids agree with that build's."""

import numpy as np
import pytest

from raglite_amd import _keyword
from tests.keyword_ref import impacts_f32, zipf_corpus


def _split_check(flat, offsets, n_terms, live, cuts):
    full = _keyword.build_from_term_ids(flat, offsets, n_terms, live)
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        f = flat[offsets[lo] : offsets[hi]]
        o = offsets[lo : hi + 1] - offsets[lo]
        lv = None if live is None else live[lo:hi]
        parts.append((lo, hi, f, o, lv, _keyword.shard_counts(f, o, n_terms, lv)))
    corpus = _keyword.ShardCounts(sum(p[5].df for p in parts), sum(p[5].n_live for p in parts), sum(p[5].total_length for p in parts))
    assert np.array_equal(corpus.df, full.df) and corpus.n_live == full.n_live and corpus.total_length == int(full.length.sum())
    full_imp = impacts_f32(full)
    for lo, hi, f, o, lv, _ in parts:
        sh = _keyword.build_shard_from_term_ids(f, o, n_terms, lv, corpus)
        assert np.array_equal(sh.idf.view(np.uint32), full.idf.view(np.uint32))
        assert np.array_equal(sh.nrm.view(np.uint32), full.nrm[lo:hi].view(np.uint32))
        assert sh.n_live == full.n_live and sh.avgdl == full.avgdl
        sel = (full.post_chunk >= lo) & (full.post_chunk < hi)  # term-major, chunks ascending: the shard's own order
        assert np.array_equal(sh.post_term, full.post_term[sel])
        assert np.array_equal(sh.post_chunk, full.post_chunk[sel] - lo)
        assert np.array_equal(sh.post_tf, full.post_tf[sel])
        assert np.array_equal(impacts_f32(sh).view(np.uint32), full_imp[sel].view(np.uint32))
    return full


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_zipf_shards_equal_the_single_build(seed):
    rng = np.random.default_rng(seed)
    n_chunks, n_terms = 900, 400
    flat, offsets = zipf_corpus(rng, n_chunks, n_terms, 30)
    live = rng.random(n_chunks) > 0.1
    live[:200] = True  # dead chunks on some shards only
    for cuts in ([0, 900], [0, 7, 450, 450, 899, 900], [0, 100, 101, 600, 900], list(range(0, 901, 100))):
        _split_check(flat, offsets, n_terms, live, cuts)
        _split_check(flat, offsets, n_terms, None, cuts)


def test_a_term_on_one_shard_only_and_an_all_dead_shard():
    rng = np.random.default_rng(9)
    flat, offsets = zipf_corpus(rng, 300, 50, 10)
    flat = flat.copy()
    flat[offsets[250] : offsets[251]] = 50  # term 50: chunk 250 only (last shard)
    live = np.ones(300, bool)
    live[100:200] = False  # the middle shard holds no live chunk
    full = _split_check(flat, offsets, 51, live, [0, 100, 200, 300])
    assert full.df[50] == (1 if offsets[251] > offsets[250] else 0)


def test_texts_through_the_vocabulary_union():
    texts = ["The quick brown fox jumps over the lazy dog.", "Connected connections connecting", None, "Zebras graze; only here: quagga",
             "", "Foxes and dogs run", "Relational databases, relations", None, "The lazy connections of quick dogs"]
    stems = [None if t is None else _keyword.index_stems(t) for t in texts]
    vocab, full = _keyword.build_from_stems(stems)
    for cuts in ([0, 3, 9], [0, 4, 4, 7, 9], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]):
        union = sorted({s for lo, hi in zip(cuts[:-1], cuts[1:]) for ss in stems[lo:hi] if ss is not None for s in ss})
        assert union == vocab
        ids = {s: i for i, s in enumerate(union)}
        counts, parts = [], []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            f, o, lv = _keyword.stems_to_term_ids(stems[lo:hi], ids)
            parts.append((lo, hi, f, o, lv))
            counts.append(_keyword.shard_counts(f, o, len(union), lv))
        corpus = _keyword.ShardCounts(sum(c.df for c in counts), sum(c.n_live for c in counts), sum(c.total_length for c in counts))
        for lo, hi, f, o, lv in parts:
            sh = _keyword.build_shard_from_term_ids(f, o, len(union), lv, corpus)
            sel = (full.post_chunk >= lo) & (full.post_chunk < hi)
            assert np.array_equal(impacts_f32(sh).view(np.uint32), impacts_f32(full)[sel].view(np.uint32))
            assert np.array_equal(sh.nrm.view(np.uint32), full.nrm[lo:hi].view(np.uint32))


def test_build_shard_rejects_a_wrong_df_length():
    with pytest.raises(ValueError, match="one count per term"):
        _keyword.build_shard_from_term_ids(np.zeros(0, np.int64), np.zeros(1, np.int64), 3, None, _keyword.ShardCounts(np.zeros(2, np.int64), 0, 0))
