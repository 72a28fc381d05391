"""BM25 keyword search, host half (DESIGN.md "Keyword search"): the analyzer, the Porter stemmer, the postings and statistics, and
the float32 restatement the device is held to.  No GPU."""

import numpy as np
import pytest

from raglite_amd import _keyword
from tests import keyword_ref as ref


def test_analyzer_strips_accents_lowercases_and_splits():
    assert _keyword.tokenize("Café NAÏVE Ångström résumé") == ["cafe", "naive", "angstrom", "resume"]
    # digits, punctuation and any character outside a-z separate tokens
    assert _keyword.tokenize("gfx950 x86_64, MI355X! e-mail:foo@bar.com") == ["gfx", "x", "mi", "x", "e", "mail", "foo", "bar", "com"]
    # a backslash takes the character after it into the separator (DuckDB's `\\.` alternative): `\n` in text that was escaped
    # once too often splits "line\nbreak" into line / break, and the letter after a backslash is never part of a token
    assert _keyword.tokenize(r"line\nbreak tab\tstop back\\slash") == ["line", "break", "tab", "stop", "back", "slash"]
    assert _keyword.tokenize(r"foo\bar \xff\u00e9t\e") == ["foo", "ar", "ff", "e", "t"]
    assert _keyword.tokenize("") == [] and _keyword.tokenize(" 123 ... ") == []


def test_stopwords_removed_on_the_index_side_only():
    assert {"the", "and", "of", "would", "yourselves", "a", "z"} <= _keyword.STOPWORDS
    assert len(_keyword.STOPWORDS) == 570
    assert _keyword.index_stems("The ponies of the valley") == ["poni", "vallei"]
    # the query side keeps them (DuckDB's match_bm25 does not remove stopwords) and returns the distinct stems, sorted
    assert _keyword.query_stems("the ponies of THE valley, ponies") == ["of", "poni", "the", "vallei"]


@pytest.mark.parametrize("word, want", [
    ("caresses", "caress"), ("ponies", "poni"), ("ties", "ti"), ("caress", "caress"), ("cats", "cat"),
    ("feed", "feed"), ("agreed", "agre"), ("plastered", "plaster"), ("bled", "bled"), ("motoring", "motor"), ("sing", "sing"),
    ("conflated", "conflat"), ("troubled", "troubl"), ("sized", "size"), ("hopping", "hop"), ("tanned", "tan"), ("falling", "fall"),
    ("hissing", "hiss"), ("fizzed", "fizz"), ("failing", "fail"), ("filing", "file"), ("happy", "happi"), ("sky", "sky"),
    ("relational", "relat"), ("conditional", "condit"), ("rational", "ration"), ("valenci", "valenc"), ("digitizer", "digit"),
    ("triplicate", "triplic"), ("formative", "form"), ("electrical", "electr"), ("hopeful", "hope"), ("goodness", "good"),
    ("revival", "reviv"), ("allowance", "allow"), ("airliner", "airlin"), ("adjustable", "adjust"), ("replacement", "replac"),
    ("adoption", "adopt"), ("communism", "commun"), ("effective", "effect"), ("bowdlerize", "bowdler"), ("probate", "probat"),
    ("rate", "rate"), ("cease", "ceas"), ("controll", "control"), ("roll", "roll"), ("generalizations", "gener"),
])
def test_porter_stemmer_examples_of_the_paper(word, want):
    assert _keyword.stem(word) == want


def _texts():
    return ["The quick brown fox jumps over the lazy dog.",
            "Foxes are quick; dogs are lazy.  Quick, quick!",
            "",
            "A relational database stores relations between tables.",
            "The dog barks at the brown fox and the fox runs.",
            "the and of",  # only stopwords: a chunk of length 0
            "Résumé of the relational model, by a quick dog."]


def test_postings_and_statistics():
    texts = _texts()
    vocab, p = _keyword.build_from_texts(texts)
    stems = [_keyword.index_stems(t) for t in texts]
    assert vocab == sorted({s for st in stems for s in st})
    assert p.n_terms == len(vocab) and p.n_chunks == len(texts) and p.n_live == len(texts)
    assert p.length.tolist() == [len(st) for st in stems]
    assert p.avgdl == sum(len(st) for st in stems) / len(texts)
    assert p.term_off[0] == 0 and p.term_off[-1] == p.post_chunk.size and np.all(np.diff(p.term_off) >= 0)
    for t, s in enumerate(vocab):
        a, b = p.term_off[t], p.term_off[t + 1]
        chunks = p.post_chunk[a:b]
        assert np.all(np.diff(chunks) > 0) and np.all(p.post_term[a:b] == t)
        assert chunks.tolist() == [c for c, st in enumerate(stems) if s in st]
        assert p.post_tf[a:b].tolist() == [stems[c].count(s) for c in chunks]
        df = b - a
        assert p.idf[t] == np.float32(np.log1p((len(texts) - df + 0.5) / (df + 0.5)))
    assert np.all(p.idf > 0)
    for c, st in enumerate(stems):
        assert p.nrm[c] == np.float32(1.2 * (1 - 0.75 + 0.75 * len(st) / p.avgdl))


def test_rebuild_after_delete_changes_n_avgdl_and_df():
    texts = _texts()
    stems = [_keyword.index_stems(t) for t in texts]
    vocab, full = _keyword.build_from_stems(stems)
    gone = [1, 4]
    after = [None if i in gone else st for i, st in enumerate(stems)]
    vocab2, p = _keyword.build_from_stems(after)
    assert p.n_live == len(texts) - 2 and p.n_chunks == len(texts)
    assert p.avgdl == sum(len(st) for st in after if st is not None) / (len(texts) - 2) != full.avgdl
    assert p.length[1] == 0 and p.length[4] == 0
    assert not np.isin(p.post_chunk, gone).any()
    # "bark" only occurred in a deleted chunk: it leaves the vocabulary, and the ids of the stems after it move down
    assert "bark" in vocab and "bark" not in vocab2 and vocab2 == sorted({s for st in after if st for s in st})
    fox, fox2 = vocab.index("fox"), vocab2.index("fox")
    assert full.df[fox] == 3 and p.df[fox2] == 1
    assert p.idf[fox2] == np.float32(np.log1p((5 - 1 + 0.5) / (1 + 0.5)))


def test_term_id_builder_matches_the_text_builder():
    texts = _texts()
    vocab, p = _keyword.build_from_texts(texts)
    ids = {s: i for i, s in enumerate(vocab)}
    stems = [_keyword.index_stems(t) for t in texts]
    flat = np.array([ids[s] for st in stems for s in st], dtype=np.int64)
    off = np.concatenate(([0], np.cumsum([len(st) for st in stems])))
    q = _keyword.build_from_term_ids(flat, off, len(vocab))
    for f in ("term_off", "post_chunk", "post_tf", "post_term", "idf", "nrm", "length"):
        assert np.array_equal(getattr(p, f), getattr(q, f)), f
    with pytest.raises(ValueError):
        _keyword.build_from_term_ids(np.array([len(vocab)]), np.array([0, 1]), len(vocab))


def test_float32_restatement_against_float64_bm25():
    rng = np.random.default_rng(3)
    words = ["alpha", "beta", "gamma", "delta", "epsilon", "zeta", "theta", "iota", "kappa", "lambda", "running", "runs", "ran",
             "relational", "relations", "quickly", "quick", "fox", "foxes", "dog", "dogs", "the", "and", "of", "résumé"]
    texts = [" ".join(rng.choice(words, size=int(rng.integers(0, 40)))) for _ in range(300)]
    stems = [_keyword.index_stems(t) for t in texts]
    for dead in (None, set(rng.choice(300, size=60, replace=False).tolist())):
        chunk_stems = stems if dead is None else [None if i in dead else st for i, st in enumerate(stems)]
        vocab, p = _keyword.build_from_stems(chunk_stems)
        imp = ref.impacts_f32(p)
        assert imp.dtype == np.float32 and np.all(imp > 0)
        ids = {s: i for i, s in enumerate(vocab)}
        for query in ("quick fox", "the relational dogs ran", "alpha beta gamma delta epsilon zeta", "unknownword", "résumés"):
            qs = _keyword.query_stems(query)
            s32 = ref.scores_f32(p, imp, [ids[s] for s in qs if s in ids])
            s64 = ref.bm25_f64(chunk_stems, qs)
            assert sorted(np.nonzero(np.isfinite(s32))[0].tolist()) == sorted(s64)
            for c, v in s64.items():
                assert abs(float(s32[c]) - v) <= 2e-6 * v, (query, c)
            top_s, top_c = ref.topk_f32(s32, 10)
            assert np.all(np.diff(top_s) <= 0) and len(top_c) == min(10, len(s64))


def test_keyword_abi_validates_before_any_hip_call():
    import ctypes as C

    from raglite_amd import _abi

    lib = _abi.lib()
    h = C.c_void_p()
    off = np.array([0, 2, 3], dtype=np.int64)
    chunk = np.array([0, 1, 1], dtype=np.int32)
    tf = np.ones(3, dtype=np.int32)
    term = np.array([0, 0, 1], dtype=np.int32)
    idf = np.ones(2, dtype=np.float32)
    nrm = np.ones(2, dtype=np.float32)

    def create(off=off, chunk=chunk, tf=tf, term=term, n_terms=2, n_postings=3, n_chunks=2):
        return lib.rl_keyword_index_create(C.byref(h), off.ctypes.data, n_terms, chunk.ctypes.data, tf.ctypes.data, term.ctypes.data,
                                           n_postings, idf.ctypes.data, nrm.ctypes.data, n_chunks, _abi.MEM_HOST, None)

    assert create(n_chunks=1) == _abi.RL_ERR_INVALID and "out of range" in _abi.last_error() and not h.value
    assert create(chunk=np.array([1, 0, 1], np.int32)) == _abi.RL_ERR_INVALID and "ascending" in _abi.last_error()
    assert create(tf=np.array([1, 0, 1], np.int32)) == _abi.RL_ERR_INVALID and "frequencies" in _abi.last_error()
    assert create(term=np.array([0, 1, 1], np.int32)) == _abi.RL_ERR_INVALID and "post_term" in _abi.last_error()
    assert create(n_postings=2) == _abi.RL_ERR_INVALID and "term_off" in _abi.last_error()
    assert create(n_terms=-1) == _abi.RL_ERR_INVALID
    assert lib.rl_keyword_index_create(None, None, 0, None, None, None, 0, None, None, 0, _abi.MEM_HOST, None) == _abi.RL_ERR_INVALID
    assert lib.rl_keyword_search(None, None, None, 1, 10, None, None, None, None, _abi.MEM_HOST, None) == _abi.RL_ERR_INVALID
    assert lib.rl_keyword_index_info(None, None, None, None) == _abi.RL_ERR_INVALID
    assert lib.rl_keyword_index_destroy(None) == _abi.RL_OK
