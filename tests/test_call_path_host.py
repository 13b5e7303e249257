"""CPU tests of the one way from Python into the library (realtimeobjectdetection_amd/_ffi.py): the pointer parameter type,
the least-recently-used cache, and the workspace key.  No device is touched."""
import ctypes as C

import numpy as np
import pytest
import torch

from realtimeobjectdetection_amd import _ffi


def _memcpy():
    fn = C.CDLL(None).memcpy
    fn.restype, fn.argtypes = C.c_void_p, [_ffi.Ptr, _ffi.Ptr, C.c_size_t]
    return fn


def test_pointer_type_passes_the_address_of_every_kind_it_accepts():
    """A tensor, a numpy array, an int, a c_void_p and a byref as the source of a memcpy: the bytes arrive, so the address did."""
    memcpy = _memcpy()
    want = np.arange(1, 9, dtype=np.float32)
    tensor, array, carray = torch.from_numpy(want.copy()), want.copy(), (C.c_float * 8)(*want.tolist())
    for kind, src in (("tensor", tensor), ("numpy", array), ("int", array.ctypes.data), ("c_void_p", C.c_void_p(array.ctypes.data)),
                      ("byref", C.byref(carray)), ("ctypes array", carray)):
        for dst in (torch.zeros(8), np.zeros(8, np.float32)):         # ... and as its destination, a tensor and an array
            back = memcpy(dst, src, want.nbytes)
            got = dst.numpy() if isinstance(dst, torch.Tensor) else dst
            assert np.array_equal(got, want), kind
            assert back == (dst.data_ptr() if isinstance(dst, torch.Tensor) else dst.ctypes.data), kind
    # a view that starts inside its storage passes its own first element
    dst = np.zeros(2, np.float32)
    memcpy(dst, tensor[3:5], 8)
    assert dst.tolist() == [4.0, 5.0]
    # None is NULL
    assert _ffi.Ptr.from_param(None) is None
    assert memcpy(dst, None, 0) == dst.ctypes.data


def test_pointer_type_refuses_what_is_not_one_block_of_memory():
    memcpy = _memcpy()
    t = torch.zeros(4, 6)
    dst = np.zeros(24, np.float32)
    for bad in (t.t(), t[:, ::2], np.zeros((4, 6), np.float32).T):
        with pytest.raises(ValueError, match="non-contiguous"):
            _ffi.Ptr.from_param(bad)
        with pytest.raises(C.ArgumentError, match="non-contiguous"):  # (ctypes reports a refusal of from_param under its own type)
            memcpy(dst, bad, 4)
    with pytest.raises(C.ArgumentError):
        memcpy(dst, 1.5, 4)
    assert not dst.any()


def test_every_data_pointer_of_the_table_has_the_pointer_type():
    """The table holds ``c_void_p`` only where a parameter is a plan handle, a stream or a pointer array; the entries the package
    hands tensors to take them."""
    for name in ("rtod_forward", "rtod_conv_wgrad", "rtod_conv1x1_wgrad", "rtod_conv_dgrad_s2", "rtod_bn_grad", "rtod_yolo_loss", "rtod_write_results"):
        args = _ffi.SIGNATURES[name][1]
        assert _ffi.Ptr in args and args[-1] is C.c_void_p, name       # (the stream stays a plain handle)
    assert _ffi.SIGNATURES["rtod_forward"][1] == [C.c_void_p, _ffi.Ptr, C.c_int, _ffi.Ptr, C.c_void_p]
    assert not hasattr(_ffi, "SIGNATURES_DIGIT_NAMES")
    lib = _ffi.lib()
    assert all(getattr(lib, name).argtypes == args for name, (_, args) in _ffi.SIGNATURES.items())


def _counting(log):
    def build_for(key):
        def build():
            log.append(key)
            return ("value of", key)
        return build
    return build_for


def test_cache_evicts_the_least_recently_used_entry_and_nothing_else():
    log = []
    build_for = _counting(log)
    cap = 5
    c = _ffi.LruCache(cap)
    for k in range(cap):
        assert c.get(k, build_for(k)) == ("value of", k)
    assert log == list(range(cap)) and len(c) == cap and c.keys() == list(range(cap - 1, -1, -1))
    for k in range(cap):                                              # hits: nothing is built
        c.get(k, build_for(k))
    assert log == list(range(cap))
    assert c.get(1, build_for(1)) == ("value of", 1)                  # a hit moves its key to the front
    assert c.keys() == [1, 4, 3, 2, 0] and log == list(range(cap))
    c.get(cap, build_for(cap))                                        # capacity + 1 keys: exactly the least recently used one goes
    assert log == list(range(cap)) + [cap] and len(c) == cap
    assert 0 not in c and all(k in c for k in (1, 2, 3, 4, cap)) and c.keys() == [cap, 1, 4, 3, 2]
    sizes = []
    for k in range(100, 140):                                         # the cache is never emptied as a whole: it stays full
        c.get(k, build_for(k))
        sizes.append(len(c))
    assert sizes == [cap] * 40 and c.keys() == [139, 138, 137, 136, 135]
    c.get(0, build_for(0))                                            # the evicted key is built again
    assert log.count(0) == 2


def test_the_capacity_is_one_constant_above_what_a_step_needs():
    assert _ffi.CACHE_CAPACITY >= 64 and _ffi.cache.capacity == _ffi.CACHE_CAPACITY


def test_workspace_key_holds_device_stream_entry_and_shape(monkeypatch):
    """``workspace`` on a CPU device (the size query is host code): one query and one tensor per (device, stream, entry, shape);
    two stream handles with the same shape are two entries."""
    lib = _ffi.lib()
    real, queries = lib.rtod_conv_wgrad_workspace, []

    def counted(*args):
        queries.append(args[:-1])
        return real(*args)
    monkeypatch.setattr(lib, "rtod_conv_wgrad_workspace", counted)
    monkeypatch.setattr(_ffi, "cache", _ffi.LruCache(8))
    stream = [0x1000]
    monkeypatch.setattr(_ffi, "stream_key", lambda dev: (0, stream[0]))
    cpu = torch.device("cpu")
    shape = (1, 32, 32, 1, 5, 1)
    ws, n = _ffi.workspace("rtod_conv_wgrad", cpu, *shape)
    want = C.c_size_t()
    assert real(*shape, C.byref(want)) == 0
    assert n == want.value > 0 and ws.dtype == torch.uint8 and ws.numel() == (n + 15) // 16 * 16 and ws.data_ptr() % 16 == 0
    again, _ = _ffi.workspace("rtod_conv_wgrad", cpu, *shape)
    assert again is ws and queries == [shape]
    stream[0] = 0x2000                                                # the same shape on another stream: its own entry
    other, _ = _ffi.workspace("rtod_conv_wgrad", cpu, *shape)
    assert other is not ws and other.data_ptr() != ws.data_ptr() and queries == [shape, shape] and len(_ffi.cache) == 2
    assert (0, 0x1000, "rtod_conv_wgrad", shape) in _ffi.cache and (0, 0x2000, "rtod_conv_wgrad", shape) in _ffi.cache
    stream[0] = 0x1000
    assert _ffi.workspace("rtod_conv_wgrad", cpu, *shape)[0] is ws and len(queries) == 2
    assert _ffi.workspace("rtod_conv_wgrad", cpu, 1, 32, 32, 1, 6, 1)[0] is not ws and len(queries) == 3     # another shape
    with pytest.raises(_ffi.RtodError):                               # a shape the entry refuses is an error, and nothing is cached
        _ffi.workspace("rtod_conv_wgrad", cpu, 1, 32, 31, 1, 5, 1)
    assert len(_ffi.cache) == 3
