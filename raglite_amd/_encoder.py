"""The native encoder forward for short packs through the C ABI (`rl_encoder_*`, raglite_amd/csrc/encoder.hip): the
whole forward of `_torch_embedder`'s `Encoder` over a packed batch of at most `MAX_TOKENS` tokens, enqueued by one call -- what a text
query needs, where the torch route is bound by launches and Python -- and, for all text queries of a batched search at once, over a pack of
up to `MAX_PACK_TOKENS` tokens in token blocks of `MAX_TOKENS` rows (`forward_pack`), every sequence with the bits of a
call of its own.  CUDA tensors only, like `_attention.py`, which is why the wrapper lives here and not among the `_ops*` modules."""

from __future__ import annotations

import ctypes as C
from typing import Any, Sequence

from raglite_amd._abi import ATTN_DTYPES, ENCODER_EPILOGUES, ENCODER_MAX_PACK_TOKENS, ENCODER_MAX_TOKENS, MEM_DEVICE, check, lib
from raglite_amd._attention import HEAD_DIMS
from raglite_amd._ops_frame import _Args, _Handle

MAX_TOKENS = ENCODER_MAX_TOKENS
MAX_PACK_TOKENS = ENCODER_MAX_PACK_TOKENS  # `forward_pack`: token blocks of MAX_TOKENS rows, a sequence's bits as in a call of its own
HIDDEN_MAX, FFN_MAX = 8192, 32768
_HEAD_PARAMS = ("pooler.weight", "pooler.bias", "head.weight", "head.bias")  # the order of rl_encoder_set_head
_LAYER_PARAMS = ("qkv.weight", "qkv.bias", "out.weight", "out.bias", "ln1.weight", "ln1.bias", "up.weight", "up.bias", "down.weight",
                 "down.bias", "ln2.weight", "ln2.bias")  # the order of rl_encoder_create's layer_params


def _dtype_name(dtype: Any) -> str:
    return str(dtype).split(".")[-1]


class NativeEncoder(_Handle):
    """`Encoder.forward_packed` in HIP: `forward` returns the (n_tokens, hidden) rows in the module's 16-bit dtype (no classifier
    head); for a `shape.classifier` module, `classify_rows` returns the head's float32 logits, one per sequence.  The handle borrows the module's parameters; it is made on the first call and made again whenever a parameter's
    `data_ptr()` or the dtype has changed (`.to(dtype)`, a `load_state_dict` that reallocates).  A parameter rewritten IN PLACE is
    simply read: the library keeps no copy."""

    _destroy = "rl_encoder_destroy"

    def __init__(self, encoder_module: Any, shape: Any) -> None:
        self.module, self.shape = encoder_module, shape
        self._key: tuple | None = None
        self._held: list = []
        self._workspace: Any | None = None  # `forward_pack`'s scratch: a uint8 CUDA tensor, grown when a larger pack arrives
        self.pack_forwards = 0  # `rl_encoder_forward_pack` / `rl_encoder_classify_pack` calls made (what a batch that fits a pack should cost: one)
        self._collect()

    def _collect(self) -> None:
        """The module's Parameter objects in the order of rl_encoder_create.  They are looked up once: `.to(dtype)` and `load_state_dict`
        swap or rewrite their storage and keep the objects; a conversion that makes new ones (a move between devices) is noticed by
        `_ensure_handle` on the first and the last of them."""
        names = ["tok.weight", "pos.weight", "typ.weight", "ln.weight", "ln.bias"]
        names += [f"layers.{i}.{n}" for i in range(self.shape.layers) for n in _LAYER_PARAMS]
        params = dict(self.module.named_parameters())
        self._n_head = len(_HEAD_PARAMS) if getattr(self.shape, "classifier", False) else 0
        names += list(_HEAD_PARAMS[: self._n_head])  # (behind the trunk's: `_ensure_handle` hands the trunk's to rl_encoder_create by position)
        self._params = [params[n] for n in names]

    @staticmethod
    def supports(shape: Any, dtype: Any, n_tokens: int, device: Any = "cuda", classify: bool = False) -> bool:
        """Does the native forward take a pack of `n_tokens` tokens of this shape, element type and device?  `classify`: the caller
        wants the classifier head's logits (`classify_rows`), which needs a `shape.classifier`; without it the answer is about the rows,
        whatever head the module has."""
        import torch

        if classify and not getattr(shape, "classifier", False):
            return False
        if torch.device(device).type != "cuda" or _dtype_name(dtype) not in ATTN_DTYPES:
            return False
        if shape.heads < 1 or shape.hidden % shape.heads or shape.hidden // shape.heads not in HEAD_DIMS:
            return False
        if shape.hidden % 32 or shape.ffn % 32 or shape.hidden > HIDDEN_MAX or shape.ffn > FFN_MAX or shape.layers < 1:
            return False
        return 1 <= n_tokens <= MAX_TOKENS

    @staticmethod
    def supports_pack(shape: Any, dtype: Any, n_tokens: int, device: Any = "cuda", classify: bool = False) -> bool:
        """Does `forward_pack` (`classify`: `classify_rows`) take a pack of `n_tokens` tokens of this shape, element type and device?
        `supports` with the cap of `MAX_PACK_TOKENS`."""
        return 1 <= n_tokens <= MAX_PACK_TOKENS and NativeEncoder.supports(shape, dtype, 1, device, classify)

    def _ensure_handle(self) -> None:
        last = self.module.head.bias if self._n_head else self.module.layers[-1].ln2.bias
        if self.module.tok.weight is not self._params[0] or last is not self._params[-1]:
            self._collect()
        key =(self._params[0].dtype, *(p.data_ptr() for p in self._params))
        if key == self._key and self._handle:
            return
        self.close()
        sh, tensors = self.shape, [p.data for p in self._params]
        if any(not t.is_cuda or not t.is_contiguous() or t.dtype != tensors[0].dtype for t in tensors):
            raise ValueError("NativeEncoder: the encoder's parameters must be contiguous CUDA tensors of one dtype")
        name = _dtype_name(tensors[0].dtype)
        if name not in ATTN_DTYPES:
            raise ValueError("NativeEncoder: the encoder must be bfloat16 or float16")
        n_trunk = len(tensors) - self._n_head
        layer_ptrs = (C.c_void_p * (n_trunk - 5))(*(t.data_ptr() for t in tensors[5:n_trunk]))
        h = C.c_void_p()
        check(lib().rl_encoder_create(C.byref(h), sh.vocab_size, sh.hidden, sh.layers, sh.heads, sh.ffn, sh.max_positions, sh.type_vocab,
                                      float(sh.layer_norm_eps), ATTN_DTYPES[name], *(t.data_ptr() for t in tensors[:5]), layer_ptrs))
        self._handle, self._key, self._held = h, key, tensors  # (the storages the handle reads stay alive with it)
        if self._n_head:
            check(lib().rl_encoder_set_head(h, *(t.data_ptr() for t in tensors[n_trunk:])))

    def close(self) -> None:
        super().close()
        self._key, self._held = None, []

    def info(self, n_tokens: int = 0) -> dict:
        """The handle's cap, its scratch block (device pointer and bytes), the prefix a forward of `n_tokens` rows writes, and the kernel
        launches of a forward."""
        a = _Args.on(MEM_DEVICE, self._params[0].device)
        a.ensure_device()
        self._ensure_handle()
        cap, launches, total, used, ptr = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_void_p()
        check(lib().rl_encoder_info(self._handle, int(n_tokens), C.byref(cap), C.byref(total), C.byref(used), C.byref(ptr), C.byref(launches)))
        return {"max_tokens": cap.value, "scratch_bytes": total.value, "used_bytes": used.value, "scratch": ptr.value or 0,
                "launches": launches.value}

    def forward_i32(self, ids: Any, positions: Any, seq_offsets: Any, type_ids: Any | None, n_seqs: int, n_tokens: int, max_len: int,
                    out: Any | None = None) -> Any:
        """The C call on int32 CUDA tensors as it takes them (ids, positions, type_ids or None: n_tokens each; seq_offsets: n_seqs + 1),
        enqueued on torch's current stream; nothing waits for the device."""
        import torch

        dev = self._params[0].device
        a = _Args.on(MEM_DEVICE, dev)
        a.ensure_device()
        self._ensure_handle()
        for t in (ids, positions, seq_offsets, type_ids):
            if t is not None and not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
                raise ValueError("NativeEncoder: ids, positions, seq_offsets and type_ids must be contiguous int32 CUDA tensors")
        if ids.numel() < n_tokens or positions.numel() < n_tokens or seq_offsets.numel() < n_seqs + 1 or (type_ids is not None and type_ids.numel() < n_tokens):
            raise ValueError("NativeEncoder: an argument is shorter than n_tokens / n_seqs + 1")
        if out is None:
            out = torch.empty((n_tokens, self.shape.hidden), dtype=self._params[0].dtype, device=dev)
        a.hold(ids, positions, seq_offsets, type_ids, out)
        check(lib().rl_encoder_forward(self._handle, ids.data_ptr(), positions.data_ptr(), type_ids.data_ptr() if type_ids is not None else None,
                                       seq_offsets.data_ptr(), int(n_seqs), int(n_tokens), int(max_len), out.data_ptr(), MEM_DEVICE, a.stream))
        return out

    def workspace_bytes(self, n_tokens: int) -> int:
        """The device bytes `rl_encoder_forward_pack` needs for a pack of `n_tokens` rows (host only once the handle exists)."""
        a = _Args.on(MEM_DEVICE, self._params[0].device)
        a.ensure_device()
        self._ensure_handle()
        n = C.c_int64()
        check(lib().rl_encoder_pack_workspace_bytes(self._handle, int(n_tokens), C.byref(n)))
        return n.value

    def forward_pack_i32(self, ids: Any, positions: Any, seq_offsets: Any, type_ids: Any | None, n_seqs: int, n_tokens: int, max_len: int,
                         out: Any | None = None, workspace: Any | None = None) -> Any:
        """`forward_i32` for up to `MAX_PACK_TOKENS` tokens (`rl_encoder_forward_pack`).  `workspace`: a contiguous uint8 CUDA tensor of
        at least `workspace_bytes(n_tokens)` bytes; None: the one kept on this object, grown when the pack needs more (calls that share
        it are ordered by torch's current stream, as torch's own allocator expects of a tensor's users)."""
        import torch

        dev = self._params[0].device
        a = _Args.on(MEM_DEVICE, dev)
        a.ensure_device()
        self._ensure_handle()
        for t in (ids, positions, seq_offsets, type_ids):
            if t is not None and not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
                raise ValueError("NativeEncoder: ids, positions, seq_offsets and type_ids must be contiguous int32 CUDA tensors")
        if ids.numel() < n_tokens or positions.numel() < n_tokens or seq_offsets.numel() < n_seqs + 1 or (type_ids is not None and type_ids.numel() < n_tokens):
            raise ValueError("NativeEncoder: an argument is shorter than n_tokens / n_seqs + 1")
        if workspace is None:
            need = self.workspace_bytes(n_tokens) if 0 <= n_tokens <= MAX_PACK_TOKENS else 0  # (past the cap the C call says so)
            if self._workspace is None or self._workspace.device != dev or self._workspace.numel() < need:
                self._workspace = torch.empty(need, dtype=torch.uint8, device=dev)
            workspace = self._workspace
        elif not (workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.is_contiguous()):
            raise ValueError("NativeEncoder: workspace must be a contiguous uint8 CUDA tensor")
        if out is None:
            out = torch.empty((n_tokens, self.shape.hidden), dtype=self._params[0].dtype, device=dev)
        a.hold(ids, positions, seq_offsets, type_ids, out, workspace)
        check(lib().rl_encoder_forward_pack(self._handle, ids.data_ptr(), positions.data_ptr(), type_ids.data_ptr() if type_ids is not None else None,
                                            seq_offsets.data_ptr(), int(n_seqs), int(n_tokens), int(max_len), out.data_ptr(),
                                            workspace.data_ptr(), int(workspace.numel()), MEM_DEVICE, a.stream))
        self.pack_forwards += 1
        return out

    def classify_workspace_bytes(self, n_tokens: int, n_seqs: int) -> int:
        """The device bytes `rl_encoder_classify_pack` needs for `n_tokens` rows in `n_seqs` sequences (host only once the handle exists)."""
        a = _Args.on(MEM_DEVICE, self._params[0].device)
        a.ensure_device()
        self._ensure_handle()
        n = C.c_int64()
        check(lib().rl_encoder_classify_workspace_bytes(self._handle, int(n_tokens), int(n_seqs), C.byref(n)))
        return n.value

    def classify_pack_i32(self, ids: Any, positions: Any, seq_offsets: Any, type_ids: Any | None, n_seqs: int, n_tokens: int, max_len: int,
                          out: Any | None = None, workspace: Any | None = None) -> Any:
        """`forward_pack_i32` through the classifier head (`rl_encoder_classify_pack`): (n_seqs,) float32 logits.  `workspace`: at least
        `classify_workspace_bytes(n_tokens, n_seqs)` bytes; None: the one kept on this object, which `forward_pack_i32` shares."""
        import torch

        if not self._n_head:
            raise ValueError("NativeEncoder: classify needs an encoder with a classifier head (shape.classifier)")
        dev = self._params[0].device
        a = _Args.on(MEM_DEVICE, dev)
        a.ensure_device()
        self._ensure_handle()
        for t in (ids, positions, seq_offsets, type_ids):
            if t is not None and not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
                raise ValueError("NativeEncoder: ids, positions, seq_offsets and type_ids must be contiguous int32 CUDA tensors")
        if ids.numel() < n_tokens or positions.numel() < n_tokens or seq_offsets.numel() < n_seqs + 1 or (type_ids is not None and type_ids.numel() < n_tokens):
            raise ValueError("NativeEncoder: an argument is shorter than n_tokens / n_seqs + 1")
        if workspace is None:
            need = self.classify_workspace_bytes(n_tokens, n_seqs) if 0 <= n_tokens <= MAX_PACK_TOKENS and 0 <= n_seqs <= 65535 else 0
            if self._workspace is None or self._workspace.device != dev or self._workspace.numel() < need:
                self._workspace = torch.empty(need, dtype=torch.uint8, device=dev)
            workspace = self._workspace
        elif not (workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.is_contiguous()):
            raise ValueError("NativeEncoder: workspace must be a contiguous uint8 CUDA tensor")
        if out is None:
            out = torch.empty((n_seqs,), dtype=torch.float32, device=dev)
        elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= n_seqs):
            raise ValueError("NativeEncoder: out must be a contiguous float32 CUDA tensor of at least n_seqs elements")
        a.hold(ids, positions, seq_offsets, type_ids, out, workspace)
        check(lib().rl_encoder_classify_pack(self._handle, ids.data_ptr(), positions.data_ptr(), type_ids.data_ptr() if type_ids is not None else None,
                                             seq_offsets.data_ptr(), int(n_seqs), int(n_tokens), int(max_len), out.data_ptr(),
                                             workspace.data_ptr(), int(workspace.numel()), MEM_DEVICE, a.stream))
        self.pack_forwards += 1
        return out

    def classify_rows(self, rows: Sequence[Sequence[int]], type_rows: Sequence[Sequence[int]] | None = None) -> Any:
        """The logits of token-id lists (each with its `[CLS]` / `[SEP]`s), (len(rows),) float32 on the device: ONE copy from pinned
        memory, then the one C call.  A sequence's logit bits do not depend on what else is in `rows`."""
        buf, typ, n, lens = self._upload_rows(rows, type_rows)
        return self.classify_pack_i32(buf[:n], buf[n: 2 * n], buf[(3 if typ is not None else 2) * n:], typ, len(lens), n, max(lens))

    def forward_pack(self, ids: Any, seq_offsets: Any, lengths_host: Sequence[int], type_ids: Any | None = None) -> Any:
        """`forward` for a pack of up to `MAX_PACK_TOKENS` tokens: every sequence's rows are bit for bit the rows `forward` gives for
        that sequence alone."""
        import torch

        n = int(ids.shape[0])
        if n == 0 or n != sum(lengths_host):
            raise ValueError("NativeEncoder.forward_pack: needs at least one token, and lengths that add up to the number of tokens")
        if n > MAX_PACK_TOKENS:
            raise ValueError(f"NativeEncoder.forward_pack: at most {MAX_PACK_TOKENS} tokens per pack")
        pos = torch.tensor([t + self.shape.position_offset for ln in lengths_host for t in range(ln)], dtype=torch.int32)
        pos = pos.pin_memory().to(ids.device, non_blocking=True)
        typ = None if type_ids is None else type_ids.to(torch.int32).contiguous()
        return self.forward_pack_i32(ids.to(torch.int32).contiguous(), pos, seq_offsets.to(torch.int32).contiguous(), typ, len(lengths_host),
                                     n, max(lengths_host))

    def forward_pack_rows(self, rows: Sequence[Sequence[int]], type_rows: Sequence[Sequence[int]] | None = None) -> Any:
        """`forward_rows` for up to `MAX_PACK_TOKENS` tokens: still ONE copy from pinned memory."""
        buf, typ, n, lens = self._upload_rows(rows, type_rows)
        return self.forward_pack_i32(buf[:n], buf[n: 2 * n], buf[(3 if typ is not None else 2) * n:], typ, len(lens), n, max(lens))

    def forward(self, ids: Any, seq_offsets: Any, lengths_host: Sequence[int], type_ids: Any | None = None) -> Any:
        """`Encoder.forward_packed`'s arguments: ids (n_tokens,) CUDA integers, the sequences one after another; seq_offsets int32
        (n_seqs + 1) on the device; lengths_host their lengths as Python integers (the positions are made from them on the host)."""
        import torch

        n = int(ids.shape[0])
        if n == 0 or n != sum(lengths_host):
            raise ValueError("NativeEncoder.forward: needs at least one token, and lengths that add up to the number of tokens")
        if n > MAX_TOKENS:
            raise ValueError(f"NativeEncoder.forward: at most {MAX_TOKENS} tokens per pack")
        pos = torch.tensor([t + self.shape.position_offset for ln in lengths_host for t in range(ln)], dtype=torch.int32)
        pos = pos.pin_memory().to(ids.device, non_blocking=True)
        typ = None if type_ids is None else type_ids.to(torch.int32).contiguous()
        return self.forward_i32(ids.to(torch.int32).contiguous(), pos, seq_offsets.to(torch.int32).contiguous(), typ, len(lengths_host), n,
                                max(lengths_host))

    def forward_rows(self, rows: Sequence[Sequence[int]], type_rows: Sequence[Sequence[int]] | None = None) -> Any:
        """The forward of token-id lists (each with its `<s>` / `</s>`): ids, positions, type ids and offsets go up in ONE copy from
        pinned memory."""
        buf, typ, n, lens = self._upload_rows(rows, type_rows)
        return self.forward_i32(buf[:n], buf[n: 2 * n], buf[(3 if typ is not None else 2) * n:], typ, len(lens), n, max(lens))

    def _upload_rows(self, rows: Sequence[Sequence[int]], type_rows: Sequence[Sequence[int]] | None) -> tuple:
        """(the int32 device buffer ids | positions | [type ids] | offsets, its type-id part or None, n_tokens, lengths) of token-id
        lists: one pinned upload."""
        import itertools

        import torch

        lens = [len(r) for r in rows]
        n, off = sum(lens), self.shape.position_offset
        flat = list(itertools.chain.from_iterable(rows))
        flat += [t + off for ln in lens for t in range(ln)]
        if type_rows is not None:
            flat += list(itertools.chain.from_iterable(type_rows))
        flat += list(itertools.accumulate(lens, initial=0))
        buf = torch.tensor(flat, dtype=torch.int32).pin_memory().to(self._params[0].device, non_blocking=True)
        return buf, (buf[2 * n: 3 * n] if type_rows is not None else None), n, lens


# ---- the forward's three launches one at a time (rl_encoder_embed / _linear / _layer_norm): the same kernels, on the caller's tensors ----
def _take(who: str, dtype: Any, *tensors: Any) -> tuple:
    """(ATTN_DTYPES code, frame) for a call whose 16-bit CUDA tensors are `tensors` (None allowed): all contiguous, of `dtype`."""
    name = _dtype_name(dtype)
    if name not in ATTN_DTYPES:
        raise ValueError(f"{who}: the tensors must be bfloat16 or float16")
    for t in tensors:
        if t is not None and not (t.is_cuda and t.is_contiguous() and t.dtype == dtype):
            raise ValueError(f"{who}: every 16-bit argument must be a contiguous CUDA tensor of one dtype")
    first = next(t for t in tensors if t is not None)
    a = _Args.on(MEM_DEVICE, first.device)
    a.ensure_device()
    return ATTN_DTYPES[name], a


def _ptr(t: Any) -> Any:
    return None if t is None else t.data_ptr()


def encoder_linear_slices(N: int, K: int) -> int:  # noqa: N803 - the header's names
    """The K slices the partial epilogue of `encoder_linear` writes at (N, K): `part` is (slices, M, N) float32.  Host only."""
    s = C.c_int32()
    check(lib().rl_encoder_linear_slices(int(N), int(K), C.byref(s)))
    return s.value


def encoder_linear(x: Any, W: Any, bias: Any | None = None, epilogue: str = "bias", *, out: Any | None = None) -> Any:  # noqa: N803
    """x (M, K) . W (N, K)^T through the skinny linear kernel.  epilogue "bias" / "gelu": (M, N) in x's dtype, `+ bias` or
    `gelu_erf(. + bias)` rounded once; "partial": (encoder_linear_slices(N, K), M, N) float32, the raw K slices (bias is not read).
    `out`, if given, is the tensor written (its shape and dtype as above)."""
    return _linear("rl_encoder_linear", "encoder_linear", x, W, bias, epilogue, out)


def _linear(entry: str, who: str, x: Any, W: Any, bias: Any | None, epilogue: str, out: Any | None) -> Any:  # noqa: N803
    import torch

    if epilogue not in ENCODER_EPILOGUES:
        raise ValueError(f'{who}: epilogue must be "bias", "gelu" or "partial"')
    partial = epilogue == "partial"
    if x.dim() != 2 or W.dim() != 2 or x.shape[1] != W.shape[1]:
        raise ValueError(f"{who}: x must be (M, K) and W (N, K)")
    if not partial and (bias is None or tuple(bias.shape) != (W.shape[0],)):
        raise ValueError(f"{who}: the bias and GELU epilogues take a bias of N elements")
    dt, a = _take(who, x.dtype, x, W, None if partial else bias)
    M, K, N = int(x.shape[0]), int(x.shape[1]), int(W.shape[0])  # noqa: N806
    shape = (encoder_linear_slices(N, K), M, N) if partial else (M, N)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32 if partial else x.dtype, device=x.device)
    elif not (out.is_cuda and out.is_contiguous() and tuple(out.shape) == shape and out.dtype == (torch.float32 if partial else x.dtype)):
        raise ValueError(f"{who}: out must be a contiguous CUDA tensor of shape {shape}")
    a.hold(x, W, bias, out)
    check(getattr(lib(), entry)(x.data_ptr(), M, K, W.data_ptr(), N, None if partial else bias.data_ptr(), ENCODER_EPILOGUES[epilogue], dt,
                                  None if partial else out.data_ptr(), out.data_ptr() if partial else None, MEM_DEVICE, a.stream))
    return out


def encoder_linear_pack(x: Any, W: Any, bias: Any | None = None, epilogue: str = "bias", *, out: Any | None = None) -> Any:  # noqa: N803
    """`encoder_linear` for M up to `MAX_PACK_TOKENS` rows (`rl_encoder_linear_pack`): above `MAX_TOKENS` one workgroup per token block
    of 256 rows, every row with the bits `encoder_linear` gives it."""
    return _linear("rl_encoder_linear_pack", "encoder_linear_pack", x, W, bias, epilogue, out)


def encoder_head(x: Any, seq_offsets: Any, pooler_w: Any, pooler_b: Any, head_w: Any, head_b: Any, *, out: Any | None = None) -> Any:
    """The cross-encoder's head on its own (`rl_encoder_head`): x (n_tokens, hidden) final hidden states, seq_offsets int32 (n_seqs + 1) on
    the device; pooler_w (hidden, hidden), pooler_b (hidden,), head_w (1, hidden) or (hidden,), head_b (1,), all of x's 16-bit dtype.
    Returns (n_seqs,) float32: head_w . tanh(pooler_w x[first token] + pooler_b) + head_b, every step in f32; NaN for an empty sequence."""
    import torch

    if x.dim() != 2 or tuple(pooler_w.shape) != (x.shape[1], x.shape[1]) or tuple(pooler_b.shape) != (x.shape[1],) or head_w.numel() != x.shape[1] \
            or head_b.numel() != 1:
        raise ValueError("encoder_head: x must be (n_tokens, hidden), pooler_w (hidden, hidden), pooler_b (hidden,), head_w of hidden elements, head_b of one")
    if not (seq_offsets.is_cuda and seq_offsets.dtype == torch.int32 and seq_offsets.is_contiguous() and seq_offsets.dim() == 1 and seq_offsets.numel() >= 1):
        raise ValueError("encoder_head: seq_offsets must be a contiguous int32 CUDA tensor of n_seqs + 1 elements")
    dt, a = _take("encoder_head", x.dtype, x, pooler_w, pooler_b, head_w, head_b)
    n_seqs = int(seq_offsets.numel()) - 1
    if out is None:
        out = torch.empty((n_seqs,), dtype=torch.float32, device=x.device)
    elif not (out.is_cuda and out.is_contiguous() and tuple(out.shape) == (n_seqs,) and out.dtype == torch.float32):
        raise ValueError("encoder_head: out must be a contiguous float32 CUDA tensor (n_seqs,)")
    a.hold(x, seq_offsets, pooler_w, pooler_b, head_w, head_b, out)
    check(lib().rl_encoder_head(x.data_ptr(), seq_offsets.data_ptr(), n_seqs, int(x.shape[0]), int(x.shape[1]), pooler_w.data_ptr(),
                                pooler_b.data_ptr(), head_w.data_ptr(), head_b.data_ptr(), dt, out.data_ptr(), MEM_DEVICE, a.stream))
    return out


def encoder_layer_norm(part: Any, bias: Any, resid: Any, ln_w: Any, ln_b: Any, eps: float, *, out: Any | None = None) -> Any:
    """LN(part[0] + .. + part[slices - 1] + bias + resid) per row: part (slices, M, hidden) float32, resid (M, hidden), the vectors
    (hidden,), all 16-bit tensors of one dtype; returns (M, hidden) in it."""
    import torch

    if part.dim() != 3 or part.dtype != torch.float32 or not (part.is_cuda and part.is_contiguous()):
        raise ValueError("encoder_layer_norm: part must be a contiguous float32 CUDA tensor (slices, M, hidden)")
    slices, M, hidden = (int(v) for v in part.shape)  # noqa: N806
    if tuple(resid.shape) != (M, hidden) or any(tuple(v.shape) != (hidden,) for v in (bias, ln_w, ln_b)):
        raise ValueError("encoder_layer_norm: resid must be (M, hidden) and bias, ln_w, ln_b (hidden,)")
    dt, a = _take("encoder_layer_norm", resid.dtype, bias, resid, ln_w, ln_b)
    if out is None:
        out = torch.empty((M, hidden), dtype=resid.dtype, device=resid.device)
    elif not (out.is_cuda and out.is_contiguous() and tuple(out.shape) == (M, hidden) and out.dtype == resid.dtype):
        raise ValueError("encoder_layer_norm: out must be a contiguous CUDA tensor (M, hidden) of resid's dtype")
    a.hold(part, bias, resid, ln_w, ln_b, out)
    check(lib().rl_encoder_layer_norm(part.data_ptr(), slices, M, hidden, bias.data_ptr(), resid.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(),
                                      float(eps), dt, out.data_ptr(), MEM_DEVICE, a.stream))
    return out


def encoder_embed(ids: Any, positions: Any, type_ids: Any | None, tok: Any, pos: Any, typ: Any, ln_w: Any, ln_b: Any, eps: float, *,
                  out: Any | None = None) -> Any:
    """LN(tok[ids] + pos[positions] + typ[type_ids or 0]) per token, every index clamped into its table: ids, positions, type_ids
    (or None) int32 CUDA tensors of n_tokens; tok, pos, typ (rows, hidden); returns (n_tokens, hidden) in the tables' dtype."""
    import torch

    n = int(ids.numel())
    for t in (ids, positions, type_ids):
        if t is not None and not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n):
            raise ValueError("encoder_embed: ids, positions and type_ids must be contiguous int32 CUDA tensors of one length")
    hidden = int(tok.shape[-1])
    if any(m.dim() != 2 or m.shape[1] != hidden for m in (tok, pos, typ)) or any(tuple(v.shape) != (hidden,) for v in (ln_w, ln_b)):
        raise ValueError("encoder_embed: tok, pos, typ must be (rows, hidden) and ln_w, ln_b (hidden,)")
    dt, a = _take("encoder_embed", tok.dtype, tok, pos, typ, ln_w, ln_b)
    if out is None:
        out = torch.empty((n, hidden), dtype=tok.dtype, device=tok.device)
    elif not (out.is_cuda and out.is_contiguous() and tuple(out.shape) == (n, hidden) and out.dtype == tok.dtype):
        raise ValueError("encoder_embed: out must be a contiguous CUDA tensor (n_tokens, hidden) of the tables' dtype")
    a.hold(ids, positions, type_ids, tok, pos, typ, ln_w, ln_b, out)
    check(lib().rl_encoder_embed(ids.data_ptr(), positions.data_ptr(), _ptr(type_ids), n, tok.data_ptr(), int(tok.shape[0]), pos.data_ptr(),
                                 int(pos.shape[0]), typ.data_ptr(), int(typ.shape[0]), ln_w.data_ptr(), ln_b.data_ptr(), hidden, float(eps), dt,
                                 out.data_ptr(), MEM_DEVICE, a.stream))
    return out
