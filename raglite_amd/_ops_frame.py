"""What every wrapper of the C ABI starts from: the per-call frame (`_Args`), the per-thread device initialisation and the base of
the objects that own a library handle."""

from __future__ import annotations

import threading
from typing import Any

import numpy as np

from raglite_amd import _abi
from raglite_amd._abi import MEM_DEVICE, MEM_HOST, lib


def _is_torch(x: Any) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


def _torch():
    import torch

    return torch


def _is_half(x: Any) -> bool:
    """IEEE fp16 data (NumPy float16 or torch.float16)?"""
    if _is_torch(x):
        return x.dtype == _torch().float16
    return getattr(x, "dtype", None) == np.float16


_tls = threading.local()


def _current_device() -> int:
    return getattr(_tls, "device", 0)


def _ensure_init(device: int) -> None:
    if getattr(_tls, "initialised", None) != device:
        _abi.init(device)
        _tls.initialised = device
        _tls.device = device


def _ensure_thread() -> None:
    """Make this thread's device current: what a call does that takes host memory only."""
    _ensure_init(_current_device())


def set_device(device: int) -> None:
    """Select the GPU used by host-array calls made from this thread."""
    _tls.device = device
    _ensure_init(device)


class _Args:
    """The frame of one call into the library: converts the array arguments, enforces that they all live on the same side (NumPy
    arrays: host pointers, `mem` MEM_HOST; CUDA tensors: device pointers, `mem` MEM_DEVICE, torch's current stream), allocates the
    outputs on that side and keeps all of it alive.

    Lifetime: the frame must outlive the `lib()` call its pointers go to -- a wrapper holds it in a local until it returns, and
    nothing may shorten that.  A converted array (a cast or contiguous copy made by `inp` / `same_side`) is referenced by the frame
    alone; on the host side the call is synchronous, so it may go when the frame does; on the device side it came from torch's
    caching allocator on the stream the call was enqueued on, so releasing it when the frame dies is safe: the block can only be
    handed out again to work that is ordered behind the call on that stream."""

    def __init__(self) -> None:
        self.mem: int | None = None
        self.device = None
        self._keep: list[Any] = []
        self.filters_flag = 0  # MEM_FILTERS_DEVICE once the call's filter table is a `FilterSet` (device memory whatever the rest is)

    @classmethod
    def on(cls, mem: int, device=None) -> "_Args":
        """The frame of a call whose side is given, not taken from its first array: one that takes no array (`mem` and `device` of the
        object it is made on), or host memory only."""
        a = cls()
        a._side(mem, device)
        return a

    @property
    def call_mem(self) -> int:
        """`mem` of a call that takes filters."""
        return self.mem | self.filters_flag

    def _side(self, mem: int, device=None) -> None:
        if self.mem is None:
            self.mem, self.device = mem, device
        elif self.mem != mem:
            raise ValueError("all array arguments of one call must be NumPy arrays or all CUDA tensors")

    def inp(self, x: Any, dtype: np.dtype) -> tuple[Any, int]:
        """An input argument -> (array, pointer): `array` is `x` as contiguous `dtype` (`x` itself where it already is), the object
        whose pointer goes to the library.  A NumPy cast rounds as `astype(dtype)` does."""
        if _is_torch(x):
            torch = _torch()
            if not x.is_cuda:
                raise ValueError("torch tensors passed to raglite_amd must live on a CUDA (HIP) device")
            t = x.to(getattr(torch, np.dtype(dtype).name)).contiguous()
            self._side(MEM_DEVICE, t.device)
            self._keep.append(t)
            return t, t.data_ptr()
        a = np.ascontiguousarray(x, dtype=dtype)
        self._side(MEM_HOST)
        self._keep.append(a)
        return a, a.ctypes.data

    def same_side(self, x: Any, dtype: np.dtype) -> tuple[Any, int]:
        """`inp` for the small host-derived arrays of a call (offsets, sizes, flags, bitsets): NumPy input follows the call to the
        device."""
        if self.mem != MEM_DEVICE or _is_torch(x):
            return self.inp(x, dtype)
        t = _torch().from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(self.device)
        self._keep.append(t)
        return t, t.data_ptr()

    def out(self, shape: tuple[int, ...], dtype: np.dtype) -> tuple[Any, int]:
        if self.mem == MEM_DEVICE:
            torch = _torch()
            t = torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device=self.device)
            self._keep.append(t)
            return t, t.data_ptr()
        a = np.empty(shape, dtype=dtype)
        self._keep.append(a)
        return a, a.ctypes.data

    def hold(self, *objects: Any) -> None:
        """Keep alive, for as long as the frame, something the call reads that is not one of its converted arguments."""
        self._keep += objects

    @property
    def stream(self) -> int:
        if self.mem == MEM_DEVICE:
            return _torch().cuda.current_stream(self.device).cuda_stream
        return 0

    def ensure_device(self) -> None:
        """Make the HIP device current for this thread (ctypes calls run on the caller's thread)."""
        dev = self.device.index if (self.mem == MEM_DEVICE and self.device.index is not None) else _current_device()
        _ensure_init(dev)


_same_side = _Args.same_side  # (`_same_side(a, x, dtype)`, as the tests of the staging frame spell it)


class _Handle:
    """Base of the objects that own one handle of the library: `_handle`, an idempotent `close()` and a silent `__del__`.  A subclass
    names the symbol that destroys its handle."""

    _destroy: str
    _handle = None  # (until `__init__` has created it: closing an object whose `__init__` raised does nothing)

    def close(self) -> None:
        h, self._handle = self._handle, None
        if h:
            getattr(lib(), self._destroy)(h)

    def __del__(self) -> None:  # noqa: D105
        try:
            self.close()
        except Exception:  # noqa: BLE001,S110 - interpreter shutdown
            pass
