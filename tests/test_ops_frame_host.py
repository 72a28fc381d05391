"""The per-call frame and the handle base of the binding (`raglite_amd._ops_frame`) on their own: no library call, no GPU."""

import ctypes as C
import gc
import weakref

import numpy as np
import pytest

from raglite_amd import _abi, _ops
from raglite_amd._ops_frame import _Handle


def test_inp_returns_the_converted_array_and_its_pointer():
    a = _ops._Args()  # noqa: SLF001
    arr, ptr = a.inp([[1, 2, 3], [4, 5, 6]], np.float32)
    assert isinstance(arr, np.ndarray) and arr.dtype == np.float32 and arr.flags.c_contiguous
    assert arr.tolist() == [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]] and ptr == arr.ctypes.data
    assert a.mem == _abi.MEM_HOST and a.call_mem == _abi.MEM_HOST and a.stream == 0
    strided = np.arange(12, dtype=np.float32).reshape(3, 4)[:, ::2]
    arr, ptr = a.inp(strided, np.float32)
    assert arr.flags.c_contiguous and np.array_equal(arr, strided) and ptr == arr.ctypes.data and ptr != strided.ctypes.data


def test_inp_passes_a_contiguous_array_of_the_right_dtype_through():
    x = np.arange(6, dtype=np.int64).reshape(2, 3)
    a = _ops._Args()  # noqa: SLF001
    arr, ptr = a.inp(x, np.int64)
    assert arr is x and ptr == x.ctypes.data
    arr, ptr = a.same_side(x, np.int64)  # (on the host side `same_side` is `inp`)
    assert arr is x and ptr == x.ctypes.data
    assert _ops._same_side(a, x, np.int64)[0] is x  # noqa: SLF001


def test_inp_rounds_to_fp16_as_astype_does():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(4096).astype(np.float32), np.float32([0.0, -0.0, 65504.0, 65520.0, 1e-8, 6e-8, 2.0 ** -24, np.inf, -1e9]),
                        (1.0 + np.arange(1, 64, dtype=np.float32) * np.float32(2.0 ** -12))])  # (and ties of the 11-bit significand)
    with np.errstate(over="ignore"):
        arr, _ = _ops._Args().inp(x, np.float16)  # noqa: SLF001
        want = np.ascontiguousarray(np.asarray(x).astype(np.float16, copy=False))
    assert arr.dtype == np.float16 and arr.view(np.uint16).tolist() == want.view(np.uint16).tolist()
    h = want.copy()
    assert _ops._Args().inp(h, np.float16)[0] is h  # noqa: SLF001  (fp16 input is taken as it is)


class _FakeTensor:
    """Enough of a torch tensor to reach the frame's checks without a GPU: its type lives in a module named torch..."""

    is_cuda = False
    device = "cuda:0"

    def to(self, _dtype):
        return self

    def contiguous(self):
        return self

    def data_ptr(self):
        return 0x40


class _FakeCudaTensor(_FakeTensor):
    is_cuda = True


_FakeTensor.__module__ = _FakeCudaTensor.__module__ = "torch._fake"


def test_arguments_of_one_call_live_on_one_side():
    assert _ops._is_torch(_FakeTensor())  # noqa: SLF001
    with pytest.raises(ValueError, match=r"torch tensors passed to raglite_amd must live on a CUDA \(HIP\) device"):
        _ops._Args().inp(_FakeTensor(), np.float32)  # noqa: SLF001
    one_side = "all array arguments of one call must be NumPy arrays or all CUDA tensors"
    a = _ops._Args()  # noqa: SLF001
    t = _FakeCudaTensor()
    assert a.inp(t, np.float32) == (t, 0x40) and a.mem == _abi.MEM_DEVICE and a.device == "cuda:0"
    with pytest.raises(ValueError, match=one_side):
        a.inp(np.zeros(3, np.float32), np.float32)
    b = _ops._Args()  # noqa: SLF001
    b.inp(np.zeros(3, np.float32), np.float32)
    with pytest.raises(ValueError, match=one_side):
        b.inp(t, np.int32)
    with pytest.raises(ValueError, match=one_side):
        _ops._Args.on(_abi.MEM_DEVICE, "cuda:0").inp(np.zeros(3, np.float32), np.float32)  # noqa: SLF001  (the frame of a call without an array)


def test_out_on_the_host_side():
    a = _ops._Args()  # noqa: SLF001
    a.inp(np.zeros(3, np.float32), np.float32)
    for shape, dtype in (((2, 5), np.float64), ((0,), np.int32), ((3,), np.uint8)):
        arr, ptr = a.out(shape, dtype)
        assert isinstance(arr, np.ndarray) and arr.shape == shape and arr.dtype == dtype and ptr == arr.ctypes.data


def test_the_frame_holds_what_it_converted_until_it_is_dropped():
    a = _ops._Args()  # noqa: SLF001
    x = np.arange(8, dtype=np.int64)
    copies = [a.inp(x, np.float32)[0], a.same_side(x[::2], np.int64)[0], a.out((4,), np.int32)[0]]
    held = np.arange(3)
    a.hold(held, None)
    refs = [weakref.ref(c) for c in (*copies, held)]
    assert all(c is not x for c in copies)
    del copies, held
    gc.collect()
    assert all(r() is not None for r in refs)  # the frame alone keeps them
    del a
    gc.collect()
    assert all(r() is None for r in refs)


class _Recorder:
    def __init__(self):
        self.destroyed = []

    def rl_thing_destroy(self, handle):
        self.destroyed.append(handle)
        return _abi.RL_OK


class _Thing(_Handle):
    _destroy = "rl_thing_destroy"

    def __init__(self, handle, fail=False):
        if fail:
            raise ValueError("no handle yet")
        self._handle = handle


@pytest.fixture
def destroy(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr("raglite_amd._ops_frame.lib", lambda: rec)
    return rec


def test_close_destroys_once(destroy):
    t = _Thing(0x1234)
    t.close()
    t.close()
    assert destroy.destroyed == [0x1234] and t._handle is None  # noqa: SLF001
    del t
    gc.collect()
    assert destroy.destroyed == [0x1234]


def test_del_destroys_what_was_not_closed_and_swallows_errors(destroy, monkeypatch):
    t = _Thing(7)
    del t
    gc.collect()
    assert destroy.destroyed == [7]
    monkeypatch.setattr("raglite_amd._ops_frame.lib", None)  # (as at interpreter shutdown: calling it raises)
    t = _Thing(8)
    del t  # silent
    gc.collect()


def test_del_after_a_failed_init_and_close_on_a_null_handle_call_nothing(destroy):
    with pytest.raises(ValueError, match="no handle yet"):
        _Thing(1, fail=True)
    t = _Thing.__new__(_Thing)  # (what a failed __init__ leaves behind)
    t.__del__()
    t.close()
    for null in (None, 0, C.c_void_p(), C.c_void_p(0)):
        _Thing(null).close()
    gc.collect()
    assert destroy.destroyed == []


def test_every_owner_of_a_handle_uses_the_base():
    from raglite_amd import _comm

    owners = (_ops.SpanTable, _ops.MetadataStore, _ops.DeviceIndex, _ops.KeywordIndex, _ops.KeywordAnalyzer, _ops.KeywordStore, _comm.Communicator)
    for cls in owners:
        assert issubclass(cls, _Handle) and "__del__" not in vars(cls) and cls._destroy in _abi._SIGNATURES  # noqa: SLF001
        assert ("close" in vars(cls)) == (cls is _ops.DeviceIndex)  # (its close also drops the borrowed tensor)
    assert issubclass(_ops.FilterSet, _Handle) and "close" in vars(_ops.FilterSet) and "__del__" not in vars(_ops.FilterSet)
