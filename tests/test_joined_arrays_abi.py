"""The joined-array entry points (dsa_batch_joined_arrays and its companions) as the library exports them, without a GPU: struct
layouts, symbols, the calls on no batch, and a loud failure instead of a host-side fallback."""
import ctypes as C

import pytest

import draco_sharp_amd as dsa
from draco_sharp_amd import encoder, native

SYMBOLS = ("dsa_batch_joined_arrays_bytes", "dsa_batch_joined_arrays", "dsa_batch_joined_arrays_layout", "dsa_batch_joined_member",
           "dsa_batch_host_joined_arrays", "dsa_batch_device_joined_arrays")


def test_struct_layouts_match_header():
    assert C.sizeof(native.JoinGroup) == 8
    assert C.sizeof(native.JoinRequest) == 64
    assert C.sizeof(native.JoinedArrays) == 400
    assert native.JoinRequest.order.offset == 32 and native.JoinedArrays.attributes.offset == 16
    assert (native.DSA_JOIN_STREAM_ORDER, native.DSA_JOIN_INPUT_ORDER) == (0, 1)


def test_symbols_are_exported():
    L = native.lib()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in native.EXPORTS
    assert L.dsa_abi_version() == 4           # added without changing the ABI: callers detect the feature by the symbol


def test_null_batch_is_answered_not_dereferenced():
    L = native.lib()
    req = native.JoinRequest(native.VertexRequest(native.DSA_VA_QUANTIZED, 0, 0), native.DSA_JOIN_STREAM_ORDER)
    group = native.JoinGroup(0, 1)
    assert L.dsa_batch_joined_arrays_bytes(None, C.byref(req), 1, C.byref(group)) == 0
    assert L.dsa_batch_joined_arrays(None, C.byref(req), 1, C.byref(group), None, None, None, 0) == native.DSA_ERR_INVALID_ARGUMENT
    assert L.dsa_batch_joined_arrays_layout(None, 0, C.byref(native.JoinedArrays())) == native.DSA_ERR_INVALID_ARGUMENT
    g, f, r = C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert L.dsa_batch_joined_member(None, 0, C.byref(g), C.byref(f), C.byref(r)) == native.DSA_ERR_INVALID_ARGUMENT
    assert not L.dsa_batch_host_joined_arrays(None) and not L.dsa_batch_device_joined_arrays(None)


def test_no_gpu_means_loud_failure_not_fallback():
    L = native.lib()
    assert callable(dsa.Batch.joined_arrays) and callable(dsa.Batch.joined_views) and callable(dsa.Batch.device_joined_views) and callable(encoder.join_plan)
    if L.dsa_device_count() > 0:
        ctx = dsa.Context(0)                  # with a GPU the same call has a device to run on: a bad order is still refused
        b = dsa.Batch(ctx, [b"DRACO"])
        b.decode()
        with pytest.raises(ValueError):
            b.joined_arrays([(0, 1)], order="sorted")
        b.close(); ctx.close()
        return
    with pytest.raises(dsa.DeviceException):
        dsa.Batch(dsa.Context(0), [b"DRACO"]).joined_arrays([(0, 1)])
    closed = dsa.Batch.__new__(dsa.Batch)     # a batch without a device behind it has nothing to gather with
    closed._h, closed._L, closed.ctx = None, L, None
    with pytest.raises(dsa.DeviceException):
        closed.joined_arrays([(0, 1)])
