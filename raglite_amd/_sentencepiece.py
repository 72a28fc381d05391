"""SentencePiece Unigram on the device: the embedder's tokenizer, from text to the int32 arrays of
`NativeEncoder.forward_pack_i32` with no Python between the UTF-32 encode and the read-back of the texts' offsets.

The tables come from the model file being mirrored -- a SentencePiece `ModelProto` whose trainer made a UNIGRAM model -- not from Unicode
data in this package: `UnigramTables.from_model` walks the normaliser's precompiled character map (a Darts-clone double array) and reads
the pieces with their scores.  The `sentencepiece` library is imported lazily; importing this module does not need it.

The contract: for every text, the ids equal `SentencePieceProcessor.encode(text)` (raw layout) or `SentencePieceTokenizer.encode(text)`
(XLM-R layout: every id + 1, the unknown piece 3).  One kind of text cannot be answered from per-code-point tables and goes to the
mirrored processor on the host: a text that holds a code point of the TRAILING SET -- one that stands at position >= 1 of a key of
several code points in the character map (Hangul jamo, kana voicing marks, Indic vowel signs, combining marks ...), where the
normaliser's longest-prefix match may consume it together with its predecessor (status 1 from the kernels).  A text without any of
them can only match keys of one code point, which is what the per-code-point image states.

`normalize_host` and `encode_host` are the algorithm over the tables in plain Python: the specification of csrc/sentencepiece.hip and
the reference of tests/test_sentencepiece_host.py.  `rows_host` is the same for the row assembly (`rl_sentencepiece_rows`).
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Any, Sequence

import numpy as np

from raglite_amd._abi import MEM_DEVICE, MEM_HOST, check, lib
from raglite_amd._ops_frame import _Args, _Handle

N_TABLE = 0x110000
SPACE, MARK = 0x20, 0x2581  # U+0020 in the expanded stream becomes U+2581 in the normalised one
MAX_PIECE = 64  # SP_MAX_PIECE: the longest piece, in code points, the search kernel's lanes cover
UNK_PENALTY = np.float32(10.0)
XLMR_OFFSET, XLMR_UNK = 1, 3
NORMAL, UNKNOWN, CONTROL, USER_DEFINED, UNUSED, BYTE = 1, 2, 3, 4, 5, 6  # ModelProto.SentencePiece.Type
UNIGRAM = 1  # TrainerSpec.ModelType
_MODEL_TYPES = {1: "UNIGRAM", 2: "BPE", 3: "WORD", 4: "CHAR"}


def text_codepoints(texts: Sequence[str]) -> tuple[np.ndarray, np.ndarray]:
    """(codepoints uint32 [n], text_off int64 [len(texts) + 1]) of texts: one UTF-32 encode of their concatenation."""
    codepoints = np.frombuffer("".join(texts).encode("utf-32-le", "surrogatepass"), dtype=np.uint32)
    text_off = np.zeros(len(texts) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in texts], out=text_off[1:])
    return codepoints, text_off


def _encodable(text: str) -> bool:
    """Can the mirrored processor and the kernels see the same code points?  Not with a lone surrogate in the text."""
    try:
        text.encode("utf-8")
    except UnicodeEncodeError:
        return False
    return True


# ---- the precompiled character map ----------------------------------------------------------------------------------------------------
def charsmap_parts(blob: bytes) -> tuple[np.ndarray, bytes]:
    """(the double array's uint32 units, the pool of NUL-terminated UTF-8 replacements) of a `precompiled_charsmap`."""
    if len(blob) < 4:
        raise ValueError("normalizer_spec.precompiled_charsmap: too short for its header")
    trie_bytes = int(np.frombuffer(blob, dtype="<u4", count=1)[0])
    if trie_bytes % 4 or trie_bytes < 4 or 4 + trie_bytes > len(blob):
        raise ValueError("normalizer_spec.precompiled_charsmap: the double array does not fit its blob")
    return np.frombuffer(blob, dtype="<u4", count=trie_bytes // 4, offset=4).copy(), bytes(blob[4 + trie_bytes:])


def charsmap_walk(blob: bytes):  # noqa: ANN201 - a generator of (key bytes, replacement bytes)
    """Every (key, replacement) of the map, depth first over the labels 1 .. 255 in ascending order.  The structure is a DAWG: the keys
    outnumber the units, and the children of a state are worked out once per state."""
    arr, pool = charsmap_parts(blob)
    n = len(arr)
    labels = np.arange(1, 256, dtype=np.uint32)

    def offset(u: int) -> int:
        return (u >> 10) << ((u & 512) >> 6)

    children: dict[int, list[tuple[int, int]]] = {}

    def kids(pos: int) -> list[tuple[int, int]]:
        got = children.get(pos)
        if got is None:
            cand = labels ^ np.uint32(pos)
            ok = cand < n
            units = arr[np.where(ok, cand, 0)]
            hit = ok & ((units & np.uint32(0x800000FF)) == labels)
            got = [(int(c), int(cand[c - 1])) for c in labels[hit].tolist()]
            children[pos] = got
        return got

    def leaf(at: int) -> bytes | None:
        u = int(arr[at])
        if not (u >> 8) & 1:
            return None
        v = int(arr[at ^ offset(u)]) & 0x7FFFFFFF
        end = pool.index(b"\0", v)
        return pool[v:end]

    stack = [(offset(int(arr[0])), b"")]
    while stack:
        pos, key = stack.pop()
        for c, at in reversed(kids(pos)):
            k = key + bytes([c])
            value = leaf(at)
            if value is not None:
                yield k, value
            stack.append((at ^ offset(int(arr[at])), k))


def charsmap_summary(blob: bytes) -> dict:
    """The counts of the map: units, keys, keys of one code point, keys of several, the longest key and replacement in code points, the
    trailing set (code points at position >= 1 of a key of several) and the images of the keys of one code point."""
    arr, _ = charsmap_parts(blob)
    single: dict[int, str] = {}
    trailing: set[int] = set()
    n_keys = n_multi = longest_key = longest_value = 0
    for key, value in charsmap_walk(blob):
        k, v = key.decode("utf-8"), value.decode("utf-8")
        n_keys += 1
        longest_key, longest_value = max(longest_key, len(k)), max(longest_value, len(v))
        if len(k) == 1:
            single[ord(k)] = v
        else:
            n_multi += 1
            trailing.update(ord(x) for x in k[1:])
    return {"units": len(arr), "keys": n_keys, "single": len(single), "multi": n_multi, "longest_key": longest_key,
            "longest_value": longest_value, "trailing": trailing, "images": single}


def rows_host(ids: Any, tok_off: Any, max_len: int, bos_id: int, eos_id: int, position_offset: int = 0) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The host statement of `rl_sentencepiece_rows`: (ids, positions, seq_offsets), all int32, of the rows `bos, ids[:max_len - 2], eos`."""
    ids, tok_off = np.asarray(ids, dtype=np.int32), np.asarray(tok_off, dtype=np.int64)
    rows, pos, off = [], [], [0]
    for t in range(len(tok_off) - 1):
        row = [bos_id, *ids[tok_off[t]: tok_off[t + 1]][: max(max_len - 2, 0)].tolist(), eos_id]
        rows += row
        pos += [position_offset + j for j in range(len(row))]
        off.append(len(rows))
    as32 = lambda x: np.asarray(x, dtype=np.int32)  # noqa: E731
    return as32(rows), as32(pos), as32(off)


@dataclass
class UnigramTables:
    """What `rl_sentencepiece_create` takes, and the model it was read from (as its bytes: `load` needs no second walk)."""

    image_off: np.ndarray     # int32 [n_table]: where the image of a code point begins in image_pool; -1 = the code point itself
    image_len: np.ndarray     # uint8 [n_table]: its length in code points (0 = it vanishes); bit 7 = the code point is in the trailing set
    image_pool: np.ndarray    # uint32: the replacements' code points back to back
    piece_cp: np.ndarray      # uint32: the NORMAL pieces as UTF-32 back to back
    piece_off: np.ndarray     # int64 [n_pieces + 1]
    piece_ids: np.ndarray     # int32 [n_pieces]: SentencePiece ids
    piece_scores: np.ndarray  # float32 [n_pieces]: as stored
    unk_id: int               # the SentencePiece id of the unknown piece
    unk_score: float          # float32(min NORMAL score) - float32(10), computed in float32
    vocab_size: int           # pieces of the model, every type
    xlmr: bool = True         # the id layout of `encode`: every id + 1, unknown 3 (False: raw SentencePiece ids)
    model_proto: bytes = b""
    _processor: Any = field(default=None, repr=False, compare=False)
    _pieces: Any = field(default=None, repr=False, compare=False)

    FLAG = 0x80  # image_len bit 7

    @property
    def longest_piece(self) -> int:
        return int(np.diff(self.piece_off).max()) if len(self.piece_ids) else 0

    # ---- construction -------------------------------------------------------------------------------------------------------
    @classmethod
    def from_model(cls, model_file: Any = None, *, model_proto: bytes | None = None, xlmr: bool = True) -> "UnigramTables":
        """Read a SentencePiece model (exactly one of the file and the bytes).  Raises ValueError, naming the field, for everything the
        kernels do not state: see the module's text and DESIGN.md 4.25."""
        from sentencepiece import sentencepiece_model_pb2 as pb

        who = "UnigramTables.from_model"
        if (model_file is None) == (model_proto is None):
            raise ValueError(f"{who} needs exactly one of model_file / model_proto")
        if model_proto is None:
            with open(model_file, "rb") as f:
                model_proto = f.read()
        m = pb.ModelProto()
        m.ParseFromString(model_proto)
        ts, ns = m.trainer_spec, m.normalizer_spec
        if ts.model_type != UNIGRAM:
            raise ValueError(f"{who}: trainer_spec.model_type is {_MODEL_TYPES.get(ts.model_type, ts.model_type)}, only UNIGRAM is built")
        if ts.byte_fallback:
            raise ValueError(f"{who}: trainer_spec.byte_fallback is not built")
        if ts.treat_whitespace_as_suffix:
            raise ValueError(f"{who}: trainer_spec.treat_whitespace_as_suffix is not built")
        if not ns.precompiled_charsmap:
            raise ValueError(f"{who}: normalizer_spec.precompiled_charsmap is empty")
        for name in ("add_dummy_prefix", "remove_extra_whitespaces", "escape_whitespaces"):
            if not getattr(ns, name):
                raise ValueError(f"{who}: normalizer_spec.{name} must be true")
        texts, ids, scores, unk = [], [], [], None
        mark_ok = False
        for i, p in enumerate(m.pieces):
            if p.type in (USER_DEFINED, BYTE):
                raise ValueError(f"{who}: pieces[{i}].type is {'USER_DEFINED' if p.type == USER_DEFINED else 'BYTE'}, which is not built")
            if p.type == UNKNOWN:
                unk = i if unk is None else unk
            if p.type != NORMAL:
                continue
            if chr(MARK) in p.piece[1:]:
                raise ValueError(f"{who}: pieces[{i}].piece has U+2581 after its first code point")
            mark_ok |= p.piece == chr(MARK)
            if not p.piece:
                continue
            if len(p.piece) > MAX_PIECE:
                raise ValueError(f"{who}: pieces[{i}].piece has {len(p.piece)} code points, more than {MAX_PIECE}")
            texts.append(p.piece)
            ids.append(i)
            scores.append(p.score)
        if not mark_ok:
            raise ValueError(f"{who}: pieces: U+2581 itself must be a NORMAL piece")
        if unk is None:
            raise ValueError(f"{who}: pieces: no piece of type UNKNOWN")
        if xlmr and unk != 0:
            raise ValueError(f"{who}: trainer_spec.unk_id is {unk}, the XLM-R layout needs 0")
        piece_scores = np.asarray(scores, dtype=np.float32)
        if not np.isfinite(piece_scores).all():
            raise ValueError(f"{who}: pieces: a score is not finite")
        summary = charsmap_summary(ns.precompiled_charsmap)
        image_off = np.full(N_TABLE, -1, dtype=np.int32)
        image_len = np.ones(N_TABLE, dtype=np.uint8)
        pool: list[int] = []
        for c, v in summary["images"].items():
            if "  " in v:
                raise ValueError(f"{who}: normalizer_spec.precompiled_charsmap: the image of U+{c:04X} holds two spaces in a row")
            image_off[c], image_len[c] = len(pool), len(v)
            pool += [ord(x) for x in v]
        for c in summary["trailing"]:
            image_len[c] |= cls.FLAG
        piece_cp, piece_off = text_codepoints(texts)
        unk_score = np.float32(piece_scores.min()) - UNK_PENALTY
        return cls(image_off, image_len, np.asarray(pool, dtype=np.uint32), piece_cp.copy(), piece_off, np.asarray(ids, dtype=np.int32), piece_scores,
                   int(unk), float(np.float32(unk_score)), len(m.pieces), bool(xlmr), bytes(model_proto))

    def save(self, path: Any) -> None:
        np.savez_compressed(path, image_off=self.image_off, image_len=self.image_len, image_pool=self.image_pool, piece_cp=self.piece_cp,
                            piece_off=self.piece_off, piece_ids=self.piece_ids, piece_scores=self.piece_scores,
                            scalars=np.asarray([self.unk_id, self.vocab_size, int(self.xlmr)], dtype=np.int64),
                            unk_score=np.asarray(self.unk_score, dtype=np.float32), model_proto=np.frombuffer(self.model_proto, dtype=np.uint8))

    @classmethod
    def load(cls, path: Any) -> "UnigramTables":
        with np.load(path, allow_pickle=False) as z:
            s = z["scalars"]
            return cls(z["image_off"], z["image_len"], z["image_pool"], z["piece_cp"], z["piece_off"], z["piece_ids"], z["piece_scores"], int(s[0]),
                       float(z["unk_score"]), int(s[1]), bool(s[2]), z["model_proto"].tobytes())

    # ---- the mirrored processor -------------------------------------------------------------------------------------------------
    def processor(self) -> Any:
        """The mirrored `SentencePieceProcessor`, rebuilt from the model's bytes on first use."""
        if self._processor is None:
            import sentencepiece as spm

            self._processor = spm.SentencePieceProcessor(model_proto=self.model_proto)
        return self._processor

    def layout(self, raw_ids: Sequence[int], xlmr: bool | None = None) -> list[int]:
        """SentencePiece ids in the tables' id layout."""
        if not (self.xlmr if xlmr is None else xlmr):
            return list(raw_ids)
        return [i + XLMR_OFFSET if i != self.unk_id else XLMR_UNK for i in raw_ids]

    def encode_mirrored(self, texts: Sequence[str], xlmr: bool | None = None) -> list[list[int]]:
        """The library's own answer (a lone surrogate is not UTF-8: it is replaced as `str.encode(errors="replace")` does first)."""
        clean = [t if _encodable(t) else t.encode("utf-8", "replace").decode("utf-8") for t in texts]
        return [self.layout(ids, xlmr) for ids in self.processor().encode(clean)] if clean else []

    # ---- the specification ------------------------------------------------------------------------------------------------------
    def flagged(self, text: str) -> bool:
        """Does the text hold a code point of the trailing set (status 1)?"""
        cp = np.frombuffer(text.encode("utf-32-le", "surrogatepass"), dtype=np.uint32)
        return bool((self.image_len[cp[cp < N_TABLE]] & self.FLAG).any())

    def expand(self, text: str) -> list[int]:
        """The expanded stream: the image of every code point (itself without a key), nothing else done."""
        out: list[int] = []
        for ch in text:
            c = ord(ch)
            o = int(self.image_off[c])
            if o < 0:
                out.append(c)
            else:
                out += self.image_pool[o: o + (int(self.image_len[c]) & 0x7F)].tolist()
        return out

    def normalize_symbols(self, text: str) -> list[int]:
        """The normalised symbols of a text, by the kernels' per-symbol rule: a space is kept (as U+2581) iff the next symbol of the text
        exists and is no space; a non-space symbol that is the text's first is preceded by one U+2581 of its own."""
        raw = self.expand(text)
        out: list[int] = []
        for p, c in enumerate(raw):
            if c == SPACE:
                if p + 1 < len(raw) and raw[p + 1] != SPACE:
                    out.append(MARK)
            else:
                if p == 0:
                    out.append(MARK)
                out.append(c)
        return out

    def normalize_host(self, text: str) -> str:
        """What `SentencePieceProcessor.normalize(text)` returns, for a text that is not flagged: the image per code point, leading and
        trailing spaces dropped, runs of spaces collapsed, space -> U+2581, one U+2581 in front, empty -> empty."""
        return "".join(map(chr, self.normalize_symbols(text)))

    def _piece_dict(self) -> dict:
        if self._pieces is None:
            joined = self.piece_cp.astype("<u4").tobytes().decode("utf-32-le", "surrogatepass")
            table: dict[str, tuple[int, np.float32]] = {}
            for i in range(len(self.piece_ids)):
                b, e = int(self.piece_off[i]), int(self.piece_off[i + 1])
                table.setdefault(joined[b:e], (int(self.piece_ids[i]), np.float32(self.piece_scores[i])))
            self._pieces = table
        return self._pieces

    def viterbi(self, s: str) -> list[int]:
        """The raw ids of the best path over the normalised symbols `s`: `unigram::Model::EncodeOptimized` in float32, then the merge
        of consecutive unknowns into one."""
        table, longest, n = self._piece_dict(), self.longest_piece, len(s)
        if n == 0:
            return []
        unk_score = np.float32(self.unk_score)
        best = [np.float32(0)] * (n + 1)
        start = [-1] * (n + 1)
        ident = [-1] * (n + 1)
        for i in range(n):
            single = False
            for ln in range(1, min(longest, n - i) + 1):
                hit = table.get(s[i: i + ln])
                if hit is None:
                    continue
                c = np.float32(hit[1] + best[i])
                if start[i + ln] < 0 or c > best[i + ln]:
                    best[i + ln], start[i + ln], ident[i + ln] = c, i, hit[0]
                single |= ln == 1
            if not single:
                c = np.float32(unk_score + best[i])
                if start[i + 1] < 0 or c > best[i + 1]:
                    best[i + 1], start[i + 1], ident[i + 1] = c, i, -1
        out, j = [], n
        while j > 0:
            if not (ident[j] < 0 and out and out[-1] < 0):
                out.append(ident[j])
            j = start[j]
        return [self.unk_id if i < 0 else i for i in reversed(out)]

    def encode_tables(self, texts: Sequence[str], xlmr: bool | None = None) -> dict:
        """The kernels' algorithm, text by text: {"ids": int32, "offsets": int64 [n + 1], "status": uint8 [n], "symbols": uint32,
        "sym_off": int64 [n + 1], "counts": (n_tokens, n_symbols, n_unk, n_flagged_texts, longest text in symbols)} -- what
        `rl_sentencepiece_encode` leaves, flagged texts included as the tables see them."""
        ids, offsets, status, symbols, sym_off = [], [0], [], [], [0]
        n_unk = longest = 0
        for text in texts:
            sym = self.normalize_symbols(text)
            raw = self.viterbi("".join(map(chr, sym)))
            n_unk += sum(1 for i in raw if i == self.unk_id)
            ids += self.layout(raw, xlmr)
            offsets.append(len(ids))
            symbols += sym
            sym_off.append(len(symbols))
            longest = max(longest, len(sym))
            status.append(1 if self.flagged(text) else 0)
        return {"ids": np.asarray(ids, dtype=np.int32), "offsets": np.asarray(offsets, dtype=np.int64), "status": np.asarray(status, dtype=np.uint8),
                "symbols": np.asarray(symbols, dtype=np.uint32), "sym_off": np.asarray(sym_off, dtype=np.int64),
                "counts": (len(ids), len(symbols), n_unk, int(sum(status)), longest)}

    def needs_mirror(self, text: str) -> bool:
        return self.flagged(text) or not _encodable(text)

    def encode_host(self, texts: Sequence[str], xlmr: bool | None = None) -> list[list[int]]:
        """The ids of every text on the host: the recurrence, and the mirrored processor for the texts the tables cannot answer."""
        texts = list(texts)
        out: list[list[int]] = []
        for t in texts:
            if self.needs_mirror(t):
                out.append(self.encode_mirrored([t], xlmr)[0])
            else:
                out.append(self.layout(self.viterbi(self.normalize_host(t)), xlmr))
        return out


class DeviceSentencePiece(_Handle):
    """The tokenizer on the device (`rl_sentencepiece_*`).  `encode(text) -> list[int]`, `decode` and `vocab_size` make it a drop-in for
    `tokenizer=` of `TorchTokenEmbedder`; the embedder takes `rows_device` instead where it offers it, and no id list is ever made."""

    _destroy = "rl_sentencepiece_destroy"

    def __init__(self, tables: UnigramTables, *, device: Any = "cuda", hash_bits: int = 0) -> None:
        import torch

        self.tables = tables
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        a = _Args.on(MEM_DEVICE, self.device)
        a.ensure_device()
        self._handle = create_handle(tables, hash_bits)

    def info(self) -> dict:
        out = (C.c_int64 * 4)()
        check(lib().rl_sentencepiece_info(self._handle, out))
        return {"pieces": out[0], "longest_piece": out[1], "slots": out[2], "device_bytes": out[3]}

    @property
    def vocab_size(self) -> int:
        return self.tables.vocab_size + (XLMR_OFFSET if self.tables.xlmr else 0)

    # ---- texts -> ids -----------------------------------------------------------------------------------------------------------
    def encode_batch(self, texts: Sequence[str], *, xlmr: bool | None = None) -> tuple[Any, Any, dict]:
        """(ids int32 [n_tokens], offsets int64 [len(texts) + 1], counts) with both tensors on the device: text i's ids are
        ids[offsets[i]: offsets[i + 1]].  counts: tokens, symbols, unk, flagged (texts answered by the mirrored processor), longest."""
        import torch

        texts = list(texts)
        layout = self.tables.xlmr if xlmr is None else bool(xlmr)
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
        check(lib().rl_sentencepiece_encode(self._handle, dev[2 * len(text_off):].data_ptr() if len(codepoints) else None, dev.data_ptr(),
                                            len(codepoints), len(texts), 0 if layout else 1, counts, MEM_DEVICE, a.stream))
        n_tokens, flagged = int(counts[0]), int(counts[3])
        ids = torch.empty(n_tokens, dtype=torch.int32, device=self.device)
        offsets = torch.empty(len(texts) + 1, dtype=torch.int64, device=self.device)
        status = torch.empty(len(texts), dtype=torch.uint8, device=self.device) if flagged else None
        a.hold(ids, offsets, status)
        check(lib().rl_sentencepiece_result(self._handle, ids.data_ptr() if n_tokens else None, offsets.data_ptr(),
                                            status.data_ptr() if flagged else None, MEM_DEVICE, a.stream))
        redo = set(status.cpu().nonzero().flatten().tolist()) if flagged else set()
        if ((codepoints >= 0xD800) & (codepoints < 0xE000)).any():  # lone surrogates: Python cannot hand them to the library as UTF-8
            redo |= {i for i, t in enumerate(texts) if not _encodable(t)}
        if redo:
            ids, offsets = self._splice(texts, ids, offsets, sorted(redo), layout)
        names = ("tokens", "symbols", "unk", "flagged", "longest")
        out = dict(zip(names, (int(c) for c in counts)))
        out["tokens"], out["flagged"] = int(ids.numel()), len(redo)
        return ids, offsets, out

    def _splice(self, texts: list, ids: Any, offsets: Any, redo: list, xlmr: bool) -> tuple[Any, Any]:
        """The texts `redo` answered by the mirrored processor, the others' ids as they are (torch is plumbing here: the rare path)."""
        import torch

        off = offsets.cpu().tolist()
        answers = self.tables.encode_mirrored([texts[i] for i in redo], xlmr)
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

    def decode(self, ids: Sequence[int]) -> str:
        if not self.tables.xlmr:
            return self.tables.processor().decode(list(ids))
        return self.tables.processor().decode([i - XLMR_OFFSET for i in ids if i > XLMR_UNK])

    # ---- texts -> the arrays of forward_pack_i32 ------------------------------------------------------------------------------------
    def rows_device(self, texts: Sequence[str], shape: Any) -> tuple:
        """(ids, positions, seq_offsets, seq_offsets_host) of the rows `bos, ids[: n_ctx - 2], eos` of every text: three int32 device
        tensors and the offsets once more as a NumPy array (the one read-back)."""
        import torch

        texts = list(texts)
        if not texts:
            empty = torch.empty(0, dtype=torch.int32, device=self.device)
            return empty, empty, torch.zeros(1, dtype=torch.int32, device=self.device), np.zeros(1, dtype=np.int32)
        ids, tok_off, _ = self.encode_batch(texts)
        if ids.numel() == 0:
            ids = torch.zeros(1, dtype=torch.int32, device=self.device)  # (no token at all: a pointer the call may hold, never read)
        a = _Args.on(MEM_DEVICE, self.device)
        a.ensure_device()
        seq = torch.empty(len(texts) + 1, dtype=torch.int32, device=self.device)
        total = C.c_int64()
        args = (ids.data_ptr(), tok_off.data_ptr(), len(texts), int(shape.n_ctx), int(shape.bos_id), int(shape.eos_id), int(shape.position_offset))
        a.hold(ids, tok_off, seq)
        check(lib().rl_sentencepiece_rows(*args, None, None, seq.data_ptr(), C.byref(total), MEM_DEVICE, a.stream))  # the sizes
        n = total.value
        out = torch.empty(2 * n, dtype=torch.int32, device=self.device)
        a.hold(out)
        check(lib().rl_sentencepiece_rows(*args, out.data_ptr(), out[n:].data_ptr(), seq.data_ptr(), C.byref(total), MEM_DEVICE, a.stream))
        return out[:n], out[n:], seq, seq.cpu().numpy()


def create_handle(tables: UnigramTables, hash_bits: int = 0) -> C.c_void_p:
    """`rl_sentencepiece_create` over the tables' arrays (all host memory, copied by the call)."""
    arrays = [np.ascontiguousarray(x, dtype=t) for x, t in ((tables.image_off, np.int32), (tables.image_len, np.uint8), (tables.image_pool, np.uint32),
                                                            (tables.piece_cp, np.uint32), (tables.piece_off, np.int64), (tables.piece_ids, np.int32),
                                                            (tables.piece_scores, np.float32))]
    if len(arrays[0]) != len(arrays[1]) or len(arrays[4]) != len(arrays[5]) + 1 or len(arrays[6]) != len(arrays[5]):
        raise ValueError("DeviceSentencePiece: image_off and image_len need one length, piece_off one entry more than piece_ids and piece_scores")
    h = C.c_void_p()
    check(lib().rl_sentencepiece_create(C.byref(h), arrays[0].ctypes.data, arrays[1].ctypes.data, len(arrays[0]), arrays[2].ctypes.data, len(arrays[2]),
                                        arrays[3].ctypes.data, arrays[4].ctypes.data, arrays[5].ctypes.data, arrays[6].ctypes.data, len(arrays[5]),
                                        int(tables.unk_id), C.c_float(tables.unk_score), int(hash_bits)))
    return h


def rows_arrays(ids: Any, tok_off: Any, max_len: int, bos_id: int, eos_id: int, position_offset: int = 0) -> tuple:
    """`rl_sentencepiece_rows` over NumPy arrays (host memory): (ids, positions, seq_offsets) int32, equal to `rows_host`."""
    from raglite_amd._ops_frame import _ensure_thread

    _ensure_thread()
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    tok_off = np.ascontiguousarray(tok_off, dtype=np.int64)
    if len(tok_off) < 1:
        raise ValueError("rows_arrays: tok_off [n_texts + 1] is required")
    n_texts = len(tok_off) - 1
    seq = np.zeros(n_texts + 1, dtype=np.int32)
    total = C.c_int64()
    args = (ids.ctypes.data, tok_off.ctypes.data, n_texts, int(max_len), int(bos_id), int(eos_id), int(position_offset))
    check(lib().rl_sentencepiece_rows(*args, None, None, seq.ctypes.data, C.byref(total), MEM_HOST, None))
    out = np.zeros((2, max(total.value, 1)), dtype=np.int32)
    check(lib().rl_sentencepiece_rows(*args, out[0].ctypes.data, out[1].ctypes.data, seq.ctypes.data, C.byref(total), MEM_HOST, None))
    n = total.value
    return out[0, :n].copy(), out[1, :n].copy(), seq
