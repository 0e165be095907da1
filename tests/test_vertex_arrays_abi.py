"""The vertex-array entry points (dsa_batch_vertex_arrays and its companions) as the library exports them, without a GPU: struct
layouts, symbols, the size query on no batch, and a loud failure instead of a host-side fallback."""
import ctypes as C

import pytest

import draco_sharp_amd as dsa
from draco_sharp_amd import native


def test_struct_layouts_match_header():
    assert C.sizeof(native.VertexRequest) == 32
    assert C.sizeof(native.VertexAttribute) == 24
    assert C.sizeof(native.MeshVertexArrays) == 408
    assert native.MeshVertexArrays.attributes.offset == 24 and native.VertexAttribute.stride.offset == 8


def test_symbols_are_exported():
    L = native.lib()
    for name in ("dsa_batch_vertex_arrays_bytes", "dsa_batch_vertex_arrays", "dsa_batch_vertex_arrays_layout", "dsa_batch_host_vertex_arrays",
                 "dsa_batch_device_vertex_arrays"):
        assert hasattr(L, name), name
        assert name in native.EXPORTS
    assert L.dsa_abi_version() == 4           # added without changing the ABI: callers detect the feature by the symbol


def test_null_batch_is_answered_not_dereferenced():
    L = native.lib()
    req = native.VertexRequest(native.DSA_VA_QUANTIZED, 0, 0)
    assert L.dsa_batch_vertex_arrays_bytes(None, C.byref(req)) == 0
    assert L.dsa_batch_vertex_arrays(None, C.byref(req), None, 0) == native.DSA_ERR_INVALID_ARGUMENT
    assert L.dsa_batch_vertex_arrays_layout(None, 0, C.byref(native.MeshVertexArrays())) == native.DSA_ERR_INVALID_ARGUMENT
    assert not L.dsa_batch_host_vertex_arrays(None, 0) and not L.dsa_batch_device_vertex_arrays(None, 0)


def test_no_gpu_means_loud_failure_not_fallback():
    L = native.lib()
    assert callable(dsa.Batch.vertex_arrays) and callable(dsa.Batch.vertex_views) and callable(dsa.Batch.device_vertex_views)
    if L.dsa_device_count() > 0:
        ctx = dsa.Context(0)                  # with a GPU the same call has a device to run on: a bad format is still refused
        b = dsa.Batch(ctx, [b"DRACO"])
        b.decode()
        with pytest.raises(ValueError):
            b.vertex_arrays(format="floats")
        b.close(); ctx.close()
        return
    with pytest.raises(dsa.DeviceException):
        dsa.Batch(dsa.Context(0), [b"DRACO"]).vertex_arrays()
    closed = dsa.Batch.__new__(dsa.Batch)     # a batch without a device behind it has nothing to gather with
    closed._h, closed._L, closed.ctx = None, L, None
    with pytest.raises(dsa.DeviceException):
        closed.vertex_arrays()
