"""dsa_encode_ordered_sequential_batch (the points of a sequential stream in Morton order): the ctypes mirror and the C#
declaration of its option struct against the header as a C compiler lays it out, the defaults, the exports, the tile constant,
every option the call refuses before anything is touched, and how Config routes.  No GPU needed (the texts of the refusals need a
context: tests/test_gpu_encode_order.py reads them)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ordercases
import draco_sharp_amd as dsa
from draco_sharp_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("sequential", "point_order", "reserved")


def test_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    body = '  printf(" %zu", sizeof(dsa_encode_order_options));\n' + "".join('  printf(" %%zu", offsetof(dsa_encode_order_options, %s));\n' % f for f in FIELDS)
    body += '  printf(" %u", (unsigned)DSA_ENCODE_ORDER_TILE);\n'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "draco_mi355x.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    mirror = native.EncodeOrderOptions
    assert [n for n, _ in mirror._fields_] == list(FIELDS)
    assert got[:-1] == [C.sizeof(mirror)] + [getattr(mirror, f).offset for f in FIELDS]
    assert C.sizeof(mirror) == C.sizeof(native.EncodeSequentialOptions) + 32 == 96 and mirror.point_order.offset == 64
    assert got[-1] == native.ENCODE_ORDER_TILE == dsa.ENCODE_ORDER_TILE == ordercases.TILE


def test_abi_version_exports_and_constants():
    L = native.lib()
    for name in ("dsa_encode_default_order_options", "dsa_encode_ordered_sequential_batch"):
        assert name in native.EXPORTS
        assert hasattr(L, name)
    assert L.dsa_abi_version() == 4
    assert (dsa.POINT_ORDER_CALLER, dsa.POINT_ORDER_MORTON) == (0, 1)


def options(**kw):
    o = native.EncodeOrderOptions()
    native.lib().dsa_encode_default_order_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_default_options_are_those_of_the_sequential_call():
    L = native.lib()
    oo, so = native.EncodeOrderOptions(), native.EncodeSequentialOptions()
    C.memset(C.byref(oo), 0xFF, C.sizeof(oo))
    L.dsa_encode_default_order_options(C.byref(oo))
    L.dsa_encode_sequential_default_options(C.byref(so))
    assert bytes(oo.sequential) == bytes(so) and oo.point_order == 0 and list(oo.reserved) == [0] * 7
    L.dsa_encode_default_order_options(None)


def test_every_invalid_option_fails_the_call():
    """The options are checked before anything else is touched: no context, no meshes."""
    L = native.lib()
    h = C.c_void_p()

    def refused(o, field):
        assert L.dsa_encode_ordered_sequential_batch(None, 0, None, None, C.byref(o), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT, field
    for value in (2, -1, 7):
        refused(options(point_order=value), "point_order")
    for k in range(7):
        o = options()
        o.reserved[k] = 1
        refused(o, "reserved")
    # what the sequential call refuses, through this one
    o = options(point_order=1)
    o.sequential.geometry = 2
    refused(o, "geometry")
    o = options(point_order=1)
    o.sequential.base.position_bits = 21
    refused(o, "position_bits")
    o = options()
    o.sequential.reserved[5] = 1
    refused(o, "reserved")
    refused(options(point_order=1), "no context")
    assert L.dsa_encode_ordered_sequential_batch(None, 0, None, None, None, C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT


def test_csharp_declarations_agree_with_the_header():
    cs = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "NativeMethods.cs")).read()
    m = re.search(r"struct DsaEncodeOrderOptions\s*\{(.*?)\n\}", cs, re.S)
    assert m, "DsaEncodeOrderOptions is not declared"
    assert [" ".join(f.split()) for f in re.sub(r"//[^\n]*", "", m.group(1)).split(";") if f.strip()] == \
        ["public DsaEncodeSequentialOptions Sequential", "public int PointOrder", "public fixed int Reserved[7]"]
    for name in ("dsa_encode_default_order_options(out DsaEncodeOrderOptions options)",
                 "dsa_encode_ordered_sequential_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, DsaMeshGrids* grids, in DsaEncodeOrderOptions options, out IntPtr encoded)"):
        assert name in cs
    header = open(os.path.join(ROOT, "include", "draco_mi355x.h")).read()
    h = re.search(r"typedef struct dsa_encode_order_options \{(.*?)\} dsa_encode_order_options;", header, re.S)
    assert h and [" ".join(f.split()) for f in re.sub(r"/\*.*?\*/", "", h.group(1), flags=re.S).split(";") if f.strip()] == \
        ["dsa_encode_sequential_options sequential", "int32_t point_order", "int32_t reserved[7]"]
    enc = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "GpuDracoEncoder.cs")).read()
    for word in ("public int PointOrder", "dsa_encode_ordered_sequential_batch", "oo.PointOrder = PointOrder"):
        assert word in enc


def test_config_switch():
    assert dsa.Config().point_order == 0
    assert dsa.Config(point_order=dsa.POINT_ORDER_MORTON, encoding_method=0).point_order == 1
    with pytest.raises(ValueError, match="point_order 2"):
        dsa.Config(point_order=2)
    o = dsa.Config(point_order=1, encoding_method=0, position_bits=14, compress_connectivity=True)._native_order(1)
    assert o.point_order == 1 and o.sequential.geometry == 1 and o.sequential.compress_connectivity == 1 and o.sequential.base.position_bits == 14
    assert list(o.reserved) == [0] * 7


class _Recorder:
    """native.lib() with every encode entry point replaced by a recorder: which call EncodeBatch chooses, and with what."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        real = getattr(self._real, name)
        if not name.startswith("dsa_encode_") or "default" in name:
            return real

        def record(*args):
            self.calls.append((name, args))
            return 0
        return record


def test_encode_batch_takes_the_new_entry_point_only_when_asked(monkeypatch):
    r = _Recorder(native.lib())
    monkeypatch.setattr(native, "lib", lambda: r)

    class Ctx:
        _h = None
    enc = dsa.DracoEncoder(Ctx())
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)
    mesh, cloud = dsa.MeshData(pos, np.array([[0, 1, 2], [2, 1, 3]], np.uint32)), dsa.PointCloudData(pos)
    # the plain case keeps arriving through the call it always took
    enc.EncodeBatch([cloud], dsa.Config(), handle=True)
    enc.EncodeBatch([mesh], dsa.Config(encoding_method=0), handle=True)
    assert [c[0] for c in r.calls] == ["dsa_encode_grid_sequential_batch"] * 2
    del r.calls[:]
    enc.EncodeBatch([cloud, cloud], dsa.Config(point_order=1), handle=True)
    enc.EncodeBatch([mesh], dsa.Config(point_order=1, encoding_method=0, compress_connectivity=True), handle=True)
    assert [c[0] for c in r.calls] == ["dsa_encode_ordered_sequential_batch"] * 2
    _, n, _, grids, opt, _ = r.calls[0][1]
    assert n == 2 and grids is None and opt._obj.point_order == 1 and opt._obj.sequential.geometry == 0
    o = r.calls[1][1][4]._obj
    assert o.point_order == 1 and o.sequential.geometry == 1 and o.sequential.compress_connectivity == 1
    # Edgebreaker orders its own entries
    with pytest.raises(ValueError, match="point_order needs a sequential stream"):
        enc.EncodeBatch([mesh], dsa.Config(point_order=1), handle=True)
