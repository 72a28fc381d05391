"""Host half of BM25 keyword search: the analyzer, the Porter stemmer, the stopword list and the postings builder.

The reference ranks keywords with DuckDB's full-text search over `chunk.body` (`src/raglite/_search.py:156-230`; the index is
`PRAGMA create_fts_index('chunk', 'id', 'body')` with default settings, `_database.py:618`).  This module restates those defaults
(DESIGN.md "Keyword search" is the contract):

    index side   strip accents (NFKD, drop combining marks), lowercase, split on `(\\\\.|[^a-z])+`, drop English stopwords,
                 Porter-stem every token
    query side   the same without stopword removal, distinct stems; stems outside the vocabulary drop out
    statistics   over the LIVE chunks: N, avgdl (empty chunks count, length 0), df per stem
    score        sum over query stems t in chunk c of  idf_t * tf (k1 + 1) / (tf + nrm_c),  k1 = 1.2, b = 0.75,
                 idf_t = ln(1 + (N - df_t + 0.5) / (df_t + 0.5)),  nrm_c = k1 (1 - b + b len_c / avgdl)

Term ids are the ranks of the stems in the sorted vocabulary.  idf and nrm are computed in float64 and rounded to float32; the
device (`raglite_amd/csrc/keyword.hip`) does the float32 rest.
"""

from __future__ import annotations

import functools
import re
import unicodedata
from dataclasses import dataclass
from pathlib import Path
from typing import Sequence

import numpy as np

K1 = 1.2
B = 0.75

STOPWORDS: frozenset[str] = frozenset((Path(__file__).resolve().parent / "stopwords_english.txt").read_text().split())

# DuckDB's default `ignore='(\\.|[^a-z])+'`: a backslash with the character after it, or any character outside a-z, separates tokens
_SEPARATORS = re.compile(r"(?:\\.|[^a-z])+")


def normalize(text: str) -> str:
    """Strip accents (NFKD, then drop combining marks), then lowercase."""
    decomposed = unicodedata.normalize("NFKD", text)
    return "".join(ch for ch in decomposed if not unicodedata.combining(ch)).lower()


def tokenize(text: str) -> list[str]:
    return [tok for tok in _SEPARATORS.split(normalize(text)) if tok]


# ---- the Porter stemmer (M. F. Porter, "An algorithm for suffix stripping", Program 14(3), 1980) -----------------------------
def _consonant(w: str, i: int) -> bool:
    ch = w[i]
    if ch in "aeiou":
        return False
    if ch == "y":  # y is a consonant at the start of a word and after a vowel, a vowel after a consonant
        return i == 0 or not _consonant(w, i - 1)
    return True


def _measure(stem: str) -> int:
    """m of the stem's form [C](VC)^m[V]."""
    n, i, m = len(stem), 0, 0
    while i < n and _consonant(stem, i):
        i += 1
    while i < n:
        while i < n and not _consonant(stem, i):
            i += 1
        if i == n:
            break
        m += 1
        while i < n and _consonant(stem, i):
            i += 1
    return m


def _has_vowel(stem: str) -> bool:
    return any(not _consonant(stem, i) for i in range(len(stem)))


def _double_consonant(w: str) -> bool:
    return len(w) >= 2 and w[-1] == w[-2] and _consonant(w, len(w) - 1)


def _cvc(w: str) -> bool:
    """*o: the stem ends consonant-vowel-consonant, the last consonant not w, x or y."""
    n = len(w)
    return n >= 3 and _consonant(w, n - 3) and not _consonant(w, n - 2) and _consonant(w, n - 1) and w[-1] not in "wxy"


_STEP2 = {"ational": "ate", "tional": "tion", "enci": "ence", "anci": "ance", "izer": "ize", "abli": "able", "alli": "al", "entli": "ent",
          "eli": "e", "ousli": "ous", "ization": "ize", "ation": "ate", "ator": "ate", "alism": "al", "iveness": "ive", "fulness": "ful",
          "ousness": "ous", "aliti": "al", "iviti": "ive", "biliti": "ble"}
_STEP3 = {"icate": "ic", "ative": "", "alize": "al", "iciti": "ic", "ical": "ic", "ful": "", "ness": ""}
_STEP4 = ("al", "ance", "ence", "er", "ic", "able", "ible", "ant", "ement", "ment", "ent", "ion", "ou", "ism", "ate", "iti", "ous", "ive",
          "ize")


def _longest(w: str, suffixes) -> str | None:
    """Of a set of rules only the one with the longest matching suffix is tried (whether or not its condition then holds)."""
    best = None
    for suf in suffixes:
        if w.endswith(suf) and (best is None or len(suf) > len(best)):
            best = suf
    return best


@functools.lru_cache(maxsize=1 << 18)
def stem(word: str) -> str:
    w = word
    # step 1a
    if w.endswith("sses") or w.endswith("ies"):
        w = w[:-2]
    elif w.endswith("s") and not w.endswith("ss"):
        w = w[:-1]
    # step 1b
    again = False
    if w.endswith("eed"):
        if _measure(w[:-3]) > 0:
            w = w[:-1]
    elif w.endswith("ed") and _has_vowel(w[:-2]):
        w, again = w[:-2], True
    elif w.endswith("ing") and _has_vowel(w[:-3]):
        w, again = w[:-3], True
    if again:
        if w.endswith(("at", "bl", "iz")):
            w += "e"
        elif _double_consonant(w) and w[-1] not in "lsz":
            w = w[:-1]
        elif _measure(w) == 1 and _cvc(w):
            w += "e"
    # step 1c
    if w.endswith("y") and _has_vowel(w[:-1]):
        w = w[:-1] + "i"
    # step 2
    suf = _longest(w, _STEP2)
    if suf and _measure(w[: -len(suf)]) > 0:
        w = w[: -len(suf)] + _STEP2[suf]
    # step 3
    suf = _longest(w, _STEP3)
    if suf and _measure(w[: -len(suf)]) > 0:
        w = w[: -len(suf)] + _STEP3[suf]
    # step 4
    suf = _longest(w, _STEP4)
    if suf:
        base = w[: -len(suf)]
        if _measure(base) > 1 and (suf != "ion" or base.endswith(("s", "t"))):
            w = base
    # step 5a
    if w.endswith("e"):
        base = w[:-1]
        m = _measure(base)
        if m > 1 or (m == 1 and not _cvc(base)):
            w = base
    # step 5b
    if w.endswith("l") and _double_consonant(w) and _measure(w) > 1:
        w = w[:-1]
    return w


def index_stems(text: str) -> list[str]:
    """The stems a chunk body contributes to the index, in text order (stopwords removed)."""
    return [stem(tok) for tok in tokenize(text) if tok not in STOPWORDS]


def query_stems(text: str) -> list[str]:
    """The distinct stems of a query, sorted (no stopword removal: DuckDB's `match_bm25` keeps them)."""
    return sorted({stem(tok) for tok in tokenize(text)})


# ---- the analyzer as a table and a rule: what the device runs (`raglite_amd/csrc/keyword_analyze.hip`) --------------
# `tokenize` only ever compares tokens, so `normalize` can be applied per code point: a code point's image is a short sequence over
# {a-z, separator, backslash, newline}.  Symbols: 0 .. 25 = a .. z, then
SYM_SEPARATOR, SYM_BACKSLASH, SYM_NEWLINE = 26, 27, 28
FOLD_IMAGE_MAX = 6  # symbols per image (U+33AF, `rad/s2`, has six once its separator runs are collapsed)
FOLD_TABLE_SIZE = 0x110000


def _image_symbols(cp: int) -> list[int]:
    """The symbols of `normalize(chr(cp))`, a run of separators given as one."""
    out: list[int] = []
    for ch in normalize(chr(cp)):
        if "a" <= ch <= "z":
            out.append(ord(ch) - 97)
        elif ch == "\\":
            out.append(SYM_BACKSLASH)
        elif ch == "\n":
            out.append(SYM_NEWLINE)
        elif not out or out[-1] != SYM_SEPARATOR:
            out.append(SYM_SEPARATOR)
    return out


@functools.lru_cache(maxsize=1)
def fold_table() -> np.ndarray:
    """uint32 [0x110000]: the image of every code point under `normalize` (surrogates included: they are separators), built from
    `normalize` itself so the two cannot drift.  Up to FOLD_IMAGE_MAX fields of 5 bits from bit 0, field = symbol + 1, 0 = no further
    symbol; an empty image is 0.  What `rl_keyword_analyzer_create` takes."""
    table = np.empty(FOLD_TABLE_SIZE, dtype=np.uint32)
    for cp in range(FOLD_TABLE_SIZE):
        symbols = _image_symbols(cp)
        if len(symbols) > FOLD_IMAGE_MAX:
            raise ValueError(f"U+{cp:04X} folds to {len(symbols)} symbols; the table holds {FOLD_IMAGE_MAX}")
        entry = 0
        for j, s in enumerate(symbols):
            entry |= (s + 1) << (5 * j)
        table[cp] = entry
    table.setflags(write=False)
    return table


@functools.lru_cache(maxsize=1)
def _fold_entries() -> list[int]:
    return fold_table().tolist()


def fold_symbols(text: str) -> list[int]:
    """The folded stream of one text: the images of its code points, back to back (an empty image adds nothing)."""
    entries = _fold_entries()
    out: list[int] = []
    for ch in text:
        e = entries[ord(ch)]
        while e:
            out.append((e & 31) - 1)
            e >>= 5
    return out


def tokenize_by_table(text: str) -> list[str]:
    """`tokenize` restated without `unicodedata` or a regex, as the device runs it: fold through the table, then scan the symbols of the
    text from the left.  A backslash that is not itself consumed consumes the next symbol unless that is a newline; a consumed letter
    separates like anything else outside a-z.  So a symbol behind a run of r backslashes is consumed iff r is odd and it is no newline:
    the backslashes pair up from the left.  Nothing carries over from another text."""
    tokens: list[str] = []
    cur: list[str] = []
    run = 0  # backslashes directly in front of this symbol
    for s in fold_symbols(text):
        if s == SYM_BACKSLASH:
            run += 1
            letter = False
        else:
            letter = s < SYM_SEPARATOR and not (run & 1)  # (a newline is never consumed, and is no letter either way)
            run = 0
        if letter:
            cur.append(chr(97 + s))
        elif cur:
            tokens.append("".join(cur))
            cur = []
    if cur:
        tokens.append("".join(cur))
    return tokens


@functools.lru_cache(maxsize=1)
def default_analyzer():
    """The process-wide device analyzer over `fold_table()` and STOPWORDS (created on first use on the current device)."""
    from raglite_amd import _ops

    return _ops.KeywordAnalyzer(fold_table(), sorted(STOPWORDS))


DEFAULT_MAX_CHARS_PER_CALL = 1 << 24  # code points per device call: about 0.6 GB of device scratch at 6 letters per token


def analyze_texts_device(texts: Sequence[str | None], vocab: "Vocabulary", *, analyzer=None,
                         max_chars_per_call: int = DEFAULT_MAX_CHARS_PER_CALL, timings: dict | None = None):
    """Yields one `_ops.DeviceTermIds` per device call over consecutive runs of `texts` (None = a dead chunk: no tokens) of at most
    `max_chars_per_call` code points each (a longer text goes alone), every new stem added to `vocab` in order of first appearance.
    Each result is valid until the next one is asked for.  `timings`: seconds added up under encode / begin / vocabulary / finish, and the sizes of every call under calls."""
    import time

    if max_chars_per_call < 1:
        raise ValueError("max_chars_per_call must be >= 1")
    if analyzer is None:
        analyzer = default_analyzer()
    clock = time.perf_counter
    at, n_texts = 0, len(texts)
    while at < n_texts:
        t0 = clock()
        end, chars = at, 0
        while end < n_texts:
            size = len(texts[end]) if texts[end] is not None else 0
            if end > at and chars + size > max_chars_per_call:
                break
            chars += size
            end += 1
        run = texts[at:end]
        sizes = np.fromiter((len(t) if t is not None else 0 for t in run), dtype=np.int64, count=len(run))
        text_off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
        # (surrogatepass: a lone surrogate is a separator to `normalize`, and must not stop the encoder)
        codepoints = np.frombuffer("".join(t for t in run if t is not None).encode("utf-32-le", "surrogatepass"), dtype=np.uint32)
        t1 = clock()
        _, stems, _ = analyzer.begin(codepoints, text_off)
        t2 = clock()
        ids = vocab.add(stems)
        t3 = clock()
        result = analyzer.finish(ids)
        t4 = clock()
        if timings is not None:
            for key, dt in (("encode", t1 - t0), ("begin", t2 - t1), ("vocabulary", t3 - t2), ("finish", t4 - t3)):
                timings[key] = timings.get(key, 0.0) + dt
            timings.setdefault("calls", []).append(getattr(analyzer, "last_sizes", None))
        yield result
        at = end


def analyze_texts_batch(texts: Sequence[str | None], vocab: "Vocabulary", *, analyzer=None,
                        max_chars_per_call: int = DEFAULT_MAX_CHARS_PER_CALL, return_dead: bool = False, timings: dict | None = None):
    """(flat int32 ids, int64 offsets) of many chunk bodies, analyzed on the device: what
    `stems_to_store_ids([index_stems(t) for t in texts], vocab)` gives, with the same growth of `vocab` (None = a dead chunk: no
    tokens; `return_dead` adds the ordinals of those as a third value).  A bulk load is split into calls of at most
    `max_chars_per_call` code points; the vocabulary carries across them."""
    import time

    flats, offs, base = [], [np.zeros(1, dtype=np.int64)], 0
    for result in analyze_texts_device(texts, vocab, analyzer=analyzer, max_chars_per_call=max_chars_per_call, timings=timings):
        t0 = time.perf_counter()
        flat, offsets = result.read()
        if timings is not None:
            timings["read"] = timings.get("read", 0.0) + time.perf_counter() - t0
        flats.append(flat)
        offs.append(offsets[1:] + base)
        base += int(offsets[-1])
    flat = np.concatenate(flats) if flats else np.zeros(0, dtype=np.int32)
    offsets = np.concatenate(offs)
    if return_dead:
        return flat, offsets, np.asarray([i for i, t in enumerate(texts) if t is None], dtype=np.int64)
    return flat, offsets


# ---- postings and statistics --------------------------------------------------------------------------------------------------
@dataclass
class Postings:
    """Term-major CSR over chunk ordinals (what `rl_keyword_index_create` takes) and the statistics behind it."""

    term_off: np.ndarray    # int64 [n_terms + 1]
    post_chunk: np.ndarray  # int32, ascending within a term
    post_tf: np.ndarray     # int32 >= 1
    post_term: np.ndarray   # int32
    idf: np.ndarray         # float32 [n_terms]
    nrm: np.ndarray         # float32 [n_chunks] (every ordinal; a dead chunk has no postings)
    length: np.ndarray      # int64 [n_chunks]: stems per chunk (0 for a dead one)
    n_live: int             # N
    avgdl: float            # mean length over the live chunks (float64)

    @property
    def n_terms(self) -> int:
        return int(self.term_off.size - 1)

    @property
    def n_chunks(self) -> int:
        return int(self.nrm.size)

    @property
    def df(self) -> np.ndarray:
        return np.diff(self.term_off)


def bm25_weights(df: np.ndarray, length: np.ndarray, n_live: int, total_length: int) -> tuple[np.ndarray, np.ndarray, float]:
    """(idf float32 [n_terms], nrm float32 [n_chunks], avgdl) from the corpus statistics: df per term (int64), N = n_live and the total
    stem count of the live chunks; `length` holds the stems of the chunks the nrm values are for.  float64, rounded to float32 once.
    The one statement of the formulas: `build_from_term_ids` passes its own corpus, `build_shard_from_term_ids` the global one."""
    avgdl = float(total_length) / n_live if n_live else 0.0
    idf = np.log1p((n_live - df + 0.5) / (df + 0.5))
    rel = length / avgdl if avgdl > 0 else np.zeros(length.size)
    nrm = K1 * (1.0 - B + B * rel)
    return idf.astype(np.float32), nrm.astype(np.float32), avgdl


def _postings_csr(flat_ids: np.ndarray, offsets: np.ndarray, n_terms: int, live: np.ndarray | None):
    """(term_off, post_chunk, post_tf, post_term, length, n_live) of the chunks given (see `build_from_term_ids`)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    n_chunks = int(offsets.size - 1)
    flat_ids = np.asarray(flat_ids, dtype=np.int64)
    if flat_ids.size and (flat_ids.min() < 0 or flat_ids.max() >= n_terms):
        raise ValueError("term id out of range")
    chunk_of = np.repeat(np.arange(n_chunks, dtype=np.int64), np.diff(offsets))
    if live is not None:
        live = np.asarray(live, dtype=bool)
        keep = live[chunk_of]
        flat_ids, chunk_of = flat_ids[keep], chunk_of[keep]
    length = np.bincount(chunk_of, minlength=n_chunks).astype(np.int64)
    keys, tf = np.unique(flat_ids * max(n_chunks, 1) + chunk_of, return_counts=True)  # sorted: term-major, chunks ascending
    post_term = keys // max(n_chunks, 1)
    post_chunk = keys - post_term * max(n_chunks, 1)
    df = np.bincount(post_term, minlength=n_terms).astype(np.int64)
    term_off = np.concatenate(([0], np.cumsum(df))).astype(np.int64)
    n_live = n_chunks if live is None else int(live.sum())
    return term_off, post_chunk.astype(np.int32), tf.astype(np.int32), post_term.astype(np.int32), length, n_live


def build_from_term_ids(flat_ids: np.ndarray, offsets: np.ndarray, n_terms: int, live: np.ndarray | None = None) -> Postings:
    """Postings from pre-tokenised chunks: chunk c holds term ids flat_ids[offsets[c] : offsets[c + 1]] (any order, repeats = tf).
    `live`: bool per chunk (None = all); dead chunks add nothing and are not counted in N, avgdl or df."""
    term_off, post_chunk, post_tf, post_term, length, n_live = _postings_csr(flat_ids, offsets, n_terms, live)
    idf, nrm, avgdl = bm25_weights(np.diff(term_off), length, n_live, int(length.sum()))
    return Postings(term_off, post_chunk, post_tf, post_term, idf, nrm, length, n_live, avgdl)


@dataclass
class ShardCounts:
    """What one shard contributes to the corpus statistics (summed over the shards by `ShardedIndex.attach_keywords`)."""

    df: np.ndarray     # int64 [n_terms]: live local chunks holding each (global) term
    n_live: int        # live local chunks
    total_length: int  # stems over the live local chunks


def shard_counts(flat_ids: np.ndarray, offsets: np.ndarray, n_terms: int, live: np.ndarray | None = None) -> ShardCounts:
    term_off, _, _, _, length, n_live = _postings_csr(flat_ids, offsets, n_terms, live)
    return ShardCounts(np.diff(term_off), n_live, int(length.sum()))


def build_shard_from_term_ids(flat_ids: np.ndarray, offsets: np.ndarray, n_terms: int, live: np.ndarray | None, corpus: ShardCounts) -> Postings:
    """One shard's postings over its LOCAL chunk ordinals (term ids global), weighted by the statistics of the WHOLE corpus (`corpus`:
    df, N and the stem total summed over every shard): its idf, nrm and impacts are bitwise the slice of one build over everything.
    `n_live` / `avgdl` of the result are the corpus values; `df` (the postings' own) stays local."""
    term_off, post_chunk, post_tf, post_term, length, _ = _postings_csr(flat_ids, offsets, n_terms, live)
    df = np.asarray(corpus.df, dtype=np.int64)
    if df.size != n_terms:
        raise ValueError("corpus.df must hold one count per term")
    idf, nrm, avgdl = bm25_weights(df, length, int(corpus.n_live), int(corpus.total_length))
    return Postings(term_off, post_chunk, post_tf, post_term, idf, nrm, length, int(corpus.n_live), avgdl)


def stems_to_term_ids(chunk_stems: Sequence[Sequence[str] | None], ids: dict[str, int]):
    """(flat term ids, offsets, live or None) of chunks given as index stems (None = a dead chunk) under the vocabulary `ids`."""
    sizes = np.fromiter((len(stems) if stems is not None else 0 for stems in chunk_stems), dtype=np.int64, count=len(chunk_stems))
    flat = np.fromiter((ids[s] for stems in chunk_stems if stems is not None for s in stems), dtype=np.int64, count=int(sizes.sum()))
    live = np.fromiter((stems is not None for stems in chunk_stems), dtype=bool, count=len(chunk_stems))
    offsets = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    return flat, offsets, (None if live.all() else live)


def build_from_stems(chunk_stems: Sequence[Sequence[str] | None]) -> tuple[list[str], Postings]:
    """(vocabulary, postings) of chunks given as their index stems; None marks a dead chunk (an ordinal with no text)."""
    vocab = sorted({s for stems in chunk_stems if stems is not None for s in stems})
    flat, offsets, live = stems_to_term_ids(chunk_stems, {s: i for i, s in enumerate(vocab)})
    return vocab, build_from_term_ids(flat, offsets, len(vocab), live)


def build_from_texts(texts: Sequence[str | None]) -> tuple[list[str], Postings]:
    return build_from_stems([None if t is None else index_stems(t) for t in texts])


class Vocabulary:
    """Stable term ids for the device token store (`raglite_amd.KeywordStore`): a stem gets the next id the first time it is stored and
    keeps it, so the tokens on the device never have to be rewritten.  The postings' terms are the RANKS of the stems in the sorted
    vocabulary (`ranks()`, the permutation `KeywordStore.count` applies on the device).  Ranks are taken over every stem ever stored: a
    stem that lives only in dead chunks keeps its rank with df = 0, and the live stems keep the relative order the sorted live
    vocabulary gives them, so a score sums its impacts in the same order either way.  Host only."""

    def __init__(self) -> None:
        self._ids: dict[str, int] = {}
        self._stems: list[str] = []
        self._ranks = np.zeros(0, dtype=np.int32)

    def __len__(self) -> int:
        return len(self._stems)

    def __contains__(self, stem_: str) -> bool:
        return stem_ in self._ids

    @property
    def stems(self) -> list[str]:
        """The stems in id order."""
        return list(self._stems)

    def add(self, stems: Sequence[str]) -> np.ndarray:
        """The ids (int32) of `stems`, in their order; stems not seen before get the next ids in order of first appearance."""
        ids = self._ids
        out = np.empty(len(stems), dtype=np.int32)
        for i, s in enumerate(stems):
            t = ids.get(s)
            if t is None:
                t = ids[s] = len(self._stems)
                self._stems.append(s)
            out[i] = t
        return out

    def ranks(self) -> np.ndarray:
        """int32 [len(self)]: rank[id] = the position of the stem in the sorted vocabulary (recomputed only after growth)."""
        n = len(self._stems)
        if self._ranks.size != n:
            order = sorted(range(n), key=self._stems.__getitem__)
            ranks = np.empty(n, dtype=np.int32)
            ranks[np.asarray(order, dtype=np.int64)] = np.arange(n, dtype=np.int32)
            self._ranks = ranks
        return self._ranks

    def query_ranks(self, stems: Sequence[str], ranks: np.ndarray | None = None) -> list[int]:
        """The ranks of the distinct stems that are in the vocabulary, ascending (the term ids a query searches with).  `ranks`: an
        earlier result of `ranks()` -- the numbering of the index that was built with it; stems added since then are unknown to it."""
        if ranks is None:
            ranks = self.ranks()
        ids = self._ids
        return sorted({int(ranks[ids[s]]) for s in stems if s in ids and ids[s] < ranks.size})


def stems_to_store_ids(chunk_stems: Sequence[Sequence[str] | None], vocab: Vocabulary):
    """(flat int32 ids, int64 offsets, ordinals of the dead chunks) of chunks given as index stems (None = dead: no tokens), every
    stem added to `vocab`: what `KeywordStore.append` and `.delete` take."""
    sizes = np.fromiter((len(stems) if stems is not None else 0 for stems in chunk_stems), dtype=np.int64, count=len(chunk_stems))
    flat = vocab.add([s for stems in chunk_stems if stems is not None for s in stems])
    dead = np.asarray([i for i, stems in enumerate(chunk_stems) if stems is None], dtype=np.int64)
    return flat, np.concatenate(([0], np.cumsum(sizes))).astype(np.int64), dead
