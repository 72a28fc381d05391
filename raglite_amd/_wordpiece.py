"""BERT WordPiece on the device: the cross-encoder's tokenizer, from text to the four int32 arrays of
`NativeEncoder.classify_pack_i32` with no Python between the UTF-32 encode and the read-back of the pairs' offsets.

The tables come from the tokenizer being mirrored -- a `tokenizers.Tokenizer` whose model is WordPiece -- not from Unicode data in this
package: `WordPieceTables.from_tokenizer` probes its normalizer and pre-tokenizer once per code point and reads its vocabulary.  The
library is imported lazily; importing this module does not need it.

The contract: for every text, the ids equal `tok.encode(text, add_special_tokens=False).ids`.  Two kinds of text cannot be answered from
per-code-point tables, and both go to the mirrored tokenizer itself on the host (rare; torch splices the answers in):
  - a text that holds a code point with the CONTEXT flag: a combining mark that survives normalisation, whose image may depend on its
    neighbours through canonical reordering (status 1 from the kernels);
  - a text that contains the content of one of the tokenizer's added tokens (`[SEP]` written out in a passage): the library cuts those
    out before it normalises.

`WordPieceTables.encode_tables` is the algorithm over the tables in plain Python: the specification of csrc/wordpiece.hip and the
reference of tests/test_wordpiece_host.py.  `pairs_host` is the same for the pair assembly (`rl_wordpiece_pairs`).
"""

from __future__ import annotations

import ctypes as C
import unicodedata
from dataclasses import dataclass, field
from typing import Any, Sequence

import numpy as np

from raglite_amd._abi import MEM_DEVICE, MEM_HOST, check, lib
from raglite_amd._ops_frame import _Args, _Handle

N_TABLE = 0x110000
IMAGE_MAX = 3  # WP_IMAGE_MAX: the longest image, in code points
FIELD = (1 << 21) - 1
CLS_WORD, CLS_SPACE, CLS_PUNCT, CLS_CONTEXT = 0, 1, 2, 4
MAX_WORD_CHARS = 200  # WP_MAX_WORD_CHARS: the largest max_input_chars_per_word the kernels take


def text_codepoints(texts: Sequence[str]) -> tuple[np.ndarray, np.ndarray]:
    """(codepoints uint32 [n], text_off int64 [len(texts) + 1]) of texts: one UTF-32 encode of their concatenation."""
    codepoints = np.frombuffer("".join(texts).encode("utf-32-le", "surrogatepass"), dtype=np.uint32)
    text_off = np.zeros(len(texts) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in texts], out=text_off[1:])
    return codepoints, text_off


def _truncate_pair(n_query: int, n_doc: int, budget: int) -> tuple[int, int]:
    from raglite_amd._cross_encoder import truncate_pair

    return truncate_pair(n_query, n_doc, budget)


def pairs_host(ids: Any, tok_off: Any, query_text: Sequence[int], doc_text: Sequence[int], max_length: int, cls_id: int, sep_id: int,
               position_offset: int = 0) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """The host statement of `rl_wordpiece_pairs`: (ids, positions, type_ids, seq_offsets), all int32, of the rows
    `cls_id, q[:nq], sep_id, d[:nd], sep_id` with (nq, nd) = truncate_pair(len(q), len(d), max_length - 3)."""
    ids, tok_off = np.asarray(ids, dtype=np.int32), np.asarray(tok_off, dtype=np.int64)
    rows, pos, typ, off = [], [], [], [0]
    for a, b in zip(query_text, doc_text):
        q, d = ids[tok_off[a]: tok_off[a + 1]], ids[tok_off[b]: tok_off[b + 1]]
        nq, nd = _truncate_pair(len(q), len(d), max_length - 3)
        row = [cls_id, *q[:nq].tolist(), sep_id, *d[:nd].tolist(), sep_id]
        rows += row
        pos += [position_offset + j for j in range(len(row))]
        typ += [0] * (nq + 2) + [1] * (len(row) - nq - 2)
        off.append(len(rows))
    as32 = lambda x: np.asarray(x, dtype=np.int32)  # noqa: E731
    return as32(rows), as32(pos), as32(typ), as32(off)


@dataclass
class WordPieceTables:
    """What `rl_wordpiece_create` takes, and the tokenizer it was probed from (as its JSON: `load` needs no second probe)."""

    image: np.ndarray        # uint64 [n_table]: three 21-bit fields, field = code point + 1, 0 = none
    cls: np.ndarray          # uint8 [n_table]: bits 0-1 the class (word / white space / punctuation), bit 2 the context flag
    piece_cp: np.ndarray     # uint32: the pieces as UTF-32 back to back, the continuation prefix stripped
    piece_off: np.ndarray    # int64 [n_pieces + 1]
    piece_flags: np.ndarray  # uint8 [n_pieces]: 1 = a continuation
    piece_ids: np.ndarray    # int32 [n_pieces]
    unk_id: int
    max_input_chars_per_word: int
    tokenizer_json: str = ""
    added_tokens: tuple = ()  # contents of the tokenizer's added tokens: a text that contains one goes to the host
    _tokenizer: Any = field(default=None, repr=False, compare=False)
    _pieces: Any = field(default=None, repr=False, compare=False)

    # ---- construction -------------------------------------------------------------------------------------------------------
    @classmethod
    def from_tokenizer(cls, tok: Any) -> "WordPieceTables":
        """Probe a `tokenizers.Tokenizer` (model WordPiece): its normalizer and pre-tokenizer once per code point 0 .. 0x10FFFF without
        the surrogates, then its vocabulary.  Raises where a code point's image is longer than three code points."""
        model = tok.model
        if type(model).__name__ != "WordPiece":
            raise ValueError("WordPieceTables.from_tokenizer: the tokenizer's model must be WordPiece")
        norm, pre = tok.normalizer, tok.pre_tokenizer
        image = np.zeros(N_TABLE, dtype=np.uint64)
        klass = np.zeros(N_TABLE, dtype=np.uint8)
        kinds = {1: CLS_WORD, 2: CLS_SPACE, 3: CLS_PUNCT}
        for c in range(N_TABLE):
            if 0xD800 <= c < 0xE000:
                continue  # (surrogates: the empty image)
            ch = chr(c)
            s = ch if norm is None else norm.normalize_str(ch)
            if len(s) > IMAGE_MAX:
                raise ValueError(f"WordPieceTables.from_tokenizer: the image of U+{c:04X} has {len(s)} code points, more than {IMAGE_MAX}")
            e = 0
            for j, x in enumerate(s):
                e |= (ord(x) + 1) << (21 * j)
            image[c] = e
            n_split = 1 if pre is None else len(pre.pre_tokenize_str("a" + ch + "a"))
            if n_split not in kinds:
                raise ValueError(f"WordPieceTables.from_tokenizer: the pre-tokenizer cuts 'a' + U+{c:04X} + 'a' into {n_split} pieces")
            k = kinds[n_split]
            if s and unicodedata.combining(ch) != 0:
                k |= CLS_CONTEXT  # the only code points whose image can depend on a neighbour: marks that survive, reordered canonically
            klass[c] = k
        prefix = model.continuing_subword_prefix or ""
        vocab = sorted(tok.get_vocab(with_added_tokens=False).items(), key=lambda kv: kv[1])
        texts, flags, ids = [], [], []
        for token, i in vocab:
            texts.append(token)  # every entry is what a word's first piece can equal ...
            flags.append(0)
            ids.append(i)
            if prefix and token.startswith(prefix) and len(token) > len(prefix):
                texts.append(token[len(prefix):])  # ... and behind the prefix, what a later piece can
                flags.append(1)
                ids.append(i)
        piece_cp, piece_off = text_codepoints(texts)
        unk = tok.token_to_id(model.unk_token)
        if unk is None:
            raise ValueError("WordPieceTables.from_tokenizer: the unknown token is not in the vocabulary")
        added = tuple(sorted({t.content for t in tok.get_added_tokens_decoder().values() if t.content}))
        return cls(image, klass, piece_cp.copy(), piece_off, np.asarray(flags, dtype=np.uint8), np.asarray(ids, dtype=np.int32), int(unk),
                   int(model.max_input_chars_per_word), tok.to_str(), added)

    @classmethod
    def from_vocab(cls, vocab: dict, lowercase: bool = True, unk_token: str = "[UNK]") -> "WordPieceTables":
        """The tables of BERT's own pipeline over `vocab` (token -> id): BertNormalizer(lowercase=), BertPreTokenizer, WordPiece."""
        return cls.from_tokenizer(bert_tokenizer(vocab, lowercase=lowercase, unk_token=unk_token))

    def save(self, path: Any) -> None:
        np.savez_compressed(path, image=self.image, cls=self.cls, piece_cp=self.piece_cp, piece_off=self.piece_off, piece_flags=self.piece_flags,
                            piece_ids=self.piece_ids, scalars=np.asarray([self.unk_id, self.max_input_chars_per_word], dtype=np.int64),
                            tokenizer_json=np.asarray(self.tokenizer_json), added_tokens=np.asarray(list(self.added_tokens), dtype=np.str_))

    @classmethod
    def load(cls, path: Any) -> "WordPieceTables":
        with np.load(path, allow_pickle=False) as z:
            return cls(z["image"], z["cls"], z["piece_cp"], z["piece_off"], z["piece_flags"], z["piece_ids"], int(z["scalars"][0]),
                       int(z["scalars"][1]), str(z["tokenizer_json"]), tuple(str(t) for t in z["added_tokens"]))

    # ---- the mirrored tokenizer -----------------------------------------------------------------------------------------------
    def tokenizer(self) -> Any:
        """The mirrored tokenizer, rebuilt from its JSON on first use (no truncation, no padding)."""
        if self._tokenizer is None:
            from tokenizers import Tokenizer

            tok = Tokenizer.from_str(self.tokenizer_json)
            tok.no_truncation()
            tok.no_padding()
            self._tokenizer = tok
        return self._tokenizer

    def encode_mirrored(self, texts: Sequence[str]) -> list[list[int]]:
        return [e.ids for e in self.tokenizer().encode_batch(list(texts), add_special_tokens=False)]

    def holds_added_token(self, text: str) -> bool:
        return any(a in text for a in self.added_tokens)

    # ---- the specification ----------------------------------------------------------------------------------------------------
    def _piece_dict(self) -> tuple[dict, int]:
        if self._pieces is None:
            joined = self.piece_cp.astype("<u4").tobytes().decode("utf-32-le", "surrogatepass")
            table, longest = {}, 0
            for i in range(len(self.piece_ids)):
                b, e = int(self.piece_off[i]), int(self.piece_off[i + 1])
                if 1 <= e - b <= self.max_input_chars_per_word:
                    table.setdefault((joined[b:e], int(self.piece_flags[i]) & 1), int(self.piece_ids[i]))
                    longest = max(longest, e - b)
            self._pieces = (table, longest)
        return self._pieces

    def encode_tables(self, texts: Sequence[str]) -> dict:
        """The kernels' algorithm, text by text: {"ids": int32, "offsets": int64 [n + 1], "status": uint8 [n], "counts": (n_tokens, n_words,
        n_unk, n_flagged_texts, n_symbols)} -- what `rl_wordpiece_encode` leaves, flagged texts included as the tables see them."""
        table, longest = self._piece_dict()
        n_table = len(self.image)
        ids, offsets, status = [], [0], []
        n_words = n_unk = n_symbols = 0
        for text in texts:
            sym, flagged = [], False
            for ch in text:
                c = ord(ch)
                if c >= n_table:
                    continue
                flagged |= bool(self.cls[c] & CLS_CONTEXT)
                e = int(self.image[c])
                while e & FIELD:
                    sym.append((e & FIELD) - 1)
                    e >>= 21
            n_symbols += len(sym)
            kinds = [int(self.cls[s]) & 3 if s < n_table else CLS_WORD for s in sym]
            words, p = [], 0
            while p < len(sym):  # a maximal run of word characters, or one punctuation symbol; white space is dropped
                if kinds[p] == CLS_SPACE:
                    p += 1
                elif kinds[p] == CLS_PUNCT:
                    words.append(chr(sym[p]))
                    p += 1
                else:
                    q = p
                    while q < len(sym) and kinds[q] == CLS_WORD:
                        q += 1
                    words.append("".join(map(chr, sym[p:q])))
                    p = q
            n_words += len(words)
            for word in words:
                out, at = [], 0
                bad = len(word) > self.max_input_chars_per_word
                while at < len(word) and not bad:
                    end, found = min(len(word), at + longest), None
                    while end > at:  # greedy: the longest [at, end) in the vocabulary, as a continuation behind the first piece
                        found = table.get((word[at:end], 1 if at else 0))
                        if found is not None:
                            break
                        end -= 1
                    if found is None:
                        bad = True
                    else:
                        out.append(found)
                        at = end
                if bad:
                    out = [self.unk_id]
                    n_unk += 1
                ids += out
            offsets.append(len(ids))
            status.append(1 if flagged else 0)
        return {"ids": np.asarray(ids, dtype=np.int32), "offsets": np.asarray(offsets, dtype=np.int64), "status": np.asarray(status, dtype=np.uint8),
                "counts": (len(ids), n_words, n_unk, int(sum(status)), n_symbols)}

    def encode_host(self, texts: Sequence[str]) -> list[list[int]]:
        """The ids of every text on the host: `encode_tables`, and the mirrored tokenizer for the texts the tables cannot answer."""
        texts = list(texts)
        r = self.encode_tables(texts)
        off = r["offsets"]
        out = [r["ids"][off[i]: off[i + 1]].tolist() for i in range(len(texts))]
        redo = [i for i, t in enumerate(texts) if r["status"][i] or self.holds_added_token(t)]
        for i, ids in zip(redo, self.encode_mirrored([texts[i] for i in redo])):
            out[i] = ids
        return out


def bert_tokenizer(vocab: dict, lowercase: bool = True, unk_token: str = "[UNK]") -> Any:
    """A `tokenizers.Tokenizer` of BERT's pipeline over `vocab`, without added tokens or a post-processor."""
    from tokenizers import Tokenizer, models, normalizers, pre_tokenizers

    tok = Tokenizer(models.WordPiece(dict(vocab), unk_token=unk_token))
    tok.normalizer = normalizers.BertNormalizer(lowercase=lowercase)
    tok.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    return tok


class DeviceWordPiece(_Handle):
    """The tokenizer on the device (`rl_wordpiece_*`).  `encode(text) -> list[int]` makes it a drop-in for `tokenizer=` of
    `TorchCrossEncoderRanker`; with `forward="native"` the ranker takes `encode_pairs_device` instead and no id list is ever made."""

    _destroy = "rl_wordpiece_destroy"

    def __init__(self, tables: WordPieceTables, *, device: Any = "cuda", hash_bits: int = 0) -> None:
        import torch

        self.tables = tables
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        a = _Args.on(MEM_DEVICE, self.device)
        a.ensure_device()
        arrays = [np.ascontiguousarray(x, dtype=t) for x, t in ((tables.image, np.uint64), (tables.cls, np.uint8), (tables.piece_cp, np.uint32),
                                                                (tables.piece_off, np.int64), (tables.piece_flags, np.uint8),
                                                                (tables.piece_ids, np.int32))]
        if len(arrays[0]) != len(arrays[1]) or len(arrays[3]) != len(arrays[5]) + 1 or len(arrays[4]) != len(arrays[5]):
            raise ValueError("DeviceWordPiece: image and cls need one length, piece_off one entry more than piece_flags and piece_ids")
        h = C.c_void_p()
        check(lib().rl_wordpiece_create(C.byref(h), *(x.ctypes.data for x in arrays[:2]), len(arrays[0]), *(x.ctypes.data for x in arrays[2:]),
                                        len(arrays[5]), int(tables.unk_id), int(tables.max_input_chars_per_word), int(hash_bits)))
        self._handle = h

    def info(self) -> dict:
        out = (C.c_int64 * 4)()
        check(lib().rl_wordpiece_info(self._handle, out))
        return {"pieces": out[0], "longest_piece": out[1], "slots": out[2], "device_bytes": out[3]}

    # ---- texts -> ids ---------------------------------------------------------------------------------------------------------
    def encode_batch(self, texts: Sequence[str]) -> tuple[Any, Any, dict]:
        """(ids int32 [n_tokens], offsets int64 [len(texts) + 1], counts) with both tensors on the device: text i's ids are
        ids[offsets[i]: offsets[i + 1]].  counts: tokens, words, unk, flagged (texts answered by the mirrored tokenizer), symbols."""
        import torch

        texts = list(texts)
        codepoints, text_off = text_codepoints(texts)
        a = _Args.on(MEM_DEVICE, self.device)
        a.ensure_device()
        up = torch.empty(2 * (len(text_off)) + len(codepoints), dtype=torch.int32).pin_memory()  # offsets (as int32 pairs) | code points
        staged = up.numpy()  # (shares the pinned memory)
        staged[: 2 * len(text_off)] = text_off.view(np.int32)
        staged[2 * len(text_off):] = codepoints.view(np.int32)
        dev = up.to(self.device, non_blocking=True)
        counts = (C.c_int64 * 5)()
        a.hold(up, dev)
        check(lib().rl_wordpiece_encode(self._handle, dev[2 * len(text_off):].data_ptr() if len(codepoints) else None, dev.data_ptr(), len(codepoints),
                                        len(texts), counts, MEM_DEVICE, a.stream))
        n_tokens, flagged = int(counts[0]), int(counts[3])
        ids = torch.empty(n_tokens, dtype=torch.int32, device=self.device)
        offsets = torch.empty(len(texts) + 1, dtype=torch.int64, device=self.device)
        status = torch.empty(len(texts), dtype=torch.uint8, device=self.device) if flagged else None
        a.hold(ids, offsets, status)
        check(lib().rl_wordpiece_result(self._handle, ids.data_ptr() if n_tokens else None, offsets.data_ptr(),
                                        status.data_ptr() if flagged else None, MEM_DEVICE, a.stream))
        redo = set(status.cpu().nonzero().flatten().tolist()) if flagged else set()
        if self.tables.added_tokens:
            redo |= {i for i, t in enumerate(texts) if self.tables.holds_added_token(t)}
        if redo:
            ids, offsets = self._splice(texts, ids, offsets, sorted(redo))
        names = ("tokens", "words", "unk", "flagged", "symbols")
        out = dict(zip(names, (int(c) for c in counts)))
        out["tokens"], out["flagged"] = int(ids.numel()), len(redo)
        return ids, offsets, out

    def _splice(self, texts: list, ids: Any, offsets: Any, redo: list) -> tuple[Any, Any]:
        """The texts `redo` answered by the mirrored tokenizer, the others' ids as they are (torch is plumbing here: the rare path)."""
        import torch

        off = offsets.cpu().tolist()
        answers = self.tables.encode_mirrored([texts[i] for i in redo])
        parts, lens, at = [], [off[i + 1] - off[i] for i in range(len(texts))], 0
        for i, got in zip(redo, answers):
            parts.append(ids[off[at]: off[i]])
            parts.append(torch.tensor(got, dtype=torch.int32).to(self.device))
            lens[i], at = len(got), i + 1
        parts.append(ids[off[at]:])
        new_off = np.zeros(len(texts) + 1, dtype=np.int64)
        np.cumsum(lens, out=new_off[1:])
        return torch.cat(parts), torch.from_numpy(new_off).to(self.device)

    def encode(self, text: str) -> list[int]:
        return self.encode_batch([text])[0].cpu().tolist()

    # ---- text pairs -> the arrays of classify_pack_i32 -------------------------------------------------------------------------
    def encode_pairs_device(self, queries: Sequence[str], docs_per_query: Sequence[Sequence[str]], max_length: int, shape: Any) -> tuple:
        """(ids, positions, type_ids, seq_offsets, seq_offsets_host) of the pairs (query b, each of docs_per_query[b]) in query and then
        doc order: four int32 device tensors and the offsets once more as a NumPy array (the one read-back).  The distinct strings of the
        call are encoded once."""
        import torch

        index: dict[str, int] = {}
        q_idx, d_idx = [], []
        for q, docs in zip(queries, docs_per_query):
            qi = index.setdefault(q, len(index))
            for d in docs:
                q_idx.append(qi)
                d_idx.append(index.setdefault(d, len(index)))
        n_pairs = len(q_idx)
        empty = torch.empty(0, dtype=torch.int32, device=self.device)
        if n_pairs == 0:
            return empty, empty, empty, torch.zeros(1, dtype=torch.int32, device=self.device), np.zeros(1, dtype=np.int32)
        ids, tok_off, _ = self.encode_batch(list(index))
        if ids.numel() == 0:
            ids = torch.zeros(1, dtype=torch.int32, device=self.device)  # (no token at all: a pointer the call may hold, never read)
        a = _Args.on(MEM_DEVICE, self.device)
        a.ensure_device()
        pair_idx = torch.tensor([q_idx, d_idx], dtype=torch.int32).pin_memory().to(self.device, non_blocking=True)
        seq = torch.empty(n_pairs + 1, dtype=torch.int32, device=self.device)
        total = C.c_int64()
        args = (ids.data_ptr(), tok_off.data_ptr(), len(index), pair_idx[0].data_ptr(), pair_idx[1].data_ptr(), n_pairs, int(max_length),
                int(shape.bos_id), int(shape.eos_id), int(shape.position_offset))
        a.hold(ids, tok_off, pair_idx, seq)
        check(lib().rl_wordpiece_pairs(*args, None, None, None, seq.data_ptr(), C.byref(total), MEM_DEVICE, a.stream))  # the sizes
        out = torch.empty(3 * total.value, dtype=torch.int32, device=self.device)
        n = total.value
        a.hold(out)
        check(lib().rl_wordpiece_pairs(*args, out.data_ptr(), out[n:].data_ptr(), out[2 * n:].data_ptr(), seq.data_ptr(), C.byref(total), MEM_DEVICE,
                                       a.stream))
        return out[:n], out[n: 2 * n], out[2 * n:], seq, seq.cpu().numpy()


def pairs_arrays(ids: Any, tok_off: Any, query_text: Any, doc_text: Any, max_length: int, cls_id: int, sep_id: int, position_offset: int = 0) -> tuple:
    """`rl_wordpiece_pairs` over NumPy arrays (host memory): (ids, positions, type_ids, seq_offsets) int32, equal to `pairs_host`."""
    from raglite_amd._ops_frame import _ensure_thread

    _ensure_thread()
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    tok_off = np.ascontiguousarray(tok_off, dtype=np.int64)
    q, d = np.ascontiguousarray(query_text, dtype=np.int32), np.ascontiguousarray(doc_text, dtype=np.int32)
    if len(q) != len(d) or len(tok_off) < 1:
        raise ValueError("pairs_arrays: one doc text per query text, and tok_off [n_texts + 1], are required")
    seq = np.zeros(len(q) + 1, dtype=np.int32)
    total = C.c_int64()
    args = (ids.ctypes.data, tok_off.ctypes.data, len(tok_off) - 1, q.ctypes.data, d.ctypes.data, len(q), int(max_length), int(cls_id), int(sep_id),
            int(position_offset))
    check(lib().rl_wordpiece_pairs(*args, None, None, None, seq.ctypes.data, C.byref(total), MEM_HOST, None))
    out = np.zeros((3, max(total.value, 1)), dtype=np.int32)
    check(lib().rl_wordpiece_pairs(*args, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, seq.ctypes.data, C.byref(total), MEM_HOST, None))
    n = total.value
    return out[0, :n].copy(), out[1, :n].copy(), out[2, :n].copy(), seq
