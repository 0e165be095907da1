"""dsa_encode_merged_sequential_batch (one point per occupied quantisation cell of a point cloud): the ctypes mirror and the C#
declaration of its option struct against the header as a C compiler lays it out, the defaults, the exports in every layer, every
option the call refuses before anything is touched, and how Config routes.  No GPU needed (the texts of the refusals need a
context to be read from: tests/test_gpu_encode_merge.py asserts them)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import draco_sharp_amd as dsa
from draco_sharp_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("order", "merge_points", "reserved")
SYMBOLS = ("dsa_encode_default_merge_options", "dsa_encode_merged_sequential_batch", "dsa_encoded_row_entries")


def test_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    body = '  printf(" %zu", sizeof(dsa_encode_merge_options));\n' + "".join('  printf(" %%zu", offsetof(dsa_encode_merge_options, %s));\n' % f for f in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "draco_mi355x.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    mirror = native.EncodeMergeOptions
    assert [n for n, _ in mirror._fields_] == list(FIELDS)
    assert got == [C.sizeof(mirror)] + [getattr(mirror, f).offset for f in FIELDS]
    assert C.sizeof(mirror) == C.sizeof(native.EncodeOrderOptions) + 32 == 128 and mirror.merge_points.offset == 96


def test_symbols_in_every_layer():
    L = native.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "draco_mi355x.h")).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "NativeMethods.cs")).read()
    for name in SYMBOLS:
        assert name in native.EXPORTS and hasattr(L, name)
        assert re.search(r"\b%s\s*\(" % name, header) and re.search(r"extern \w+ %s\(" % name, cs)
    assert L.dsa_abi_version() == 4
    assert (dsa.MERGE_NONE, dsa.MERGE_CELLS) == (native.MERGE_NONE, native.MERGE_CELLS) == (0, 1)


def options(point_order=0, geometry=None, **kw):
    o = native.EncodeMergeOptions()
    native.lib().dsa_encode_default_merge_options(C.byref(o))
    o.order.point_order = point_order
    if geometry is not None:
        o.order.sequential.geometry = geometry
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_default_options_are_those_of_the_ordered_call():
    L = native.lib()
    mo, oo = native.EncodeMergeOptions(), native.EncodeOrderOptions()
    C.memset(C.byref(mo), 0xFF, C.sizeof(mo))
    L.dsa_encode_default_merge_options(C.byref(mo))
    L.dsa_encode_default_order_options(C.byref(oo))
    assert bytes(mo.order) == bytes(oo) and mo.merge_points == 0 and list(mo.reserved) == [0] * 7
    L.dsa_encode_default_merge_options(None)


def test_every_invalid_option_fails_the_call():
    """The options are checked before anything else is touched: no context, no meshes."""
    L = native.lib()
    h = C.c_void_p()

    def refused(o, field):
        assert L.dsa_encode_merged_sequential_batch(None, 0, None, None, C.byref(o), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT, field
    for value in (2, -1, 7):
        refused(options(1, 0, merge_points=value), "merge_points")
    refused(options(0, 0, merge_points=1), "merge_points without point_order")
    refused(options(1, 1, merge_points=1), "merge_points with geometry 1")
    refused(options(1, None, merge_points=1), "merge_points with the default geometry (meshes)")
    for k in range(7):
        o = options(1, 0, merge_points=1)
        o.reserved[k] = 1
        refused(o, "reserved")
    # what the nested calls refuse, through this one
    refused(options(2, 0), "point_order")
    o = options(1, 0, merge_points=1)
    o.order.reserved[2] = 1
    refused(o, "order.reserved")
    o = options(1, 0, merge_points=1)
    o.order.sequential.base.position_bits = 21
    refused(o, "position_bits")
    o = options(1, 0)
    o.order.sequential.reserved[5] = 1
    refused(o, "sequential.reserved")
    refused(options(1, 0, merge_points=1), "no context")
    assert L.dsa_encode_merged_sequential_batch(None, 0, None, None, None, C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT
    count = C.c_uint32()
    assert L.dsa_encoded_row_entries(None, 0, None, 0, C.byref(count)) == native.DSA_ERR_INVALID_ARGUMENT


def test_csharp_declarations_agree_with_the_header():
    cs = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "NativeMethods.cs")).read()
    m = re.search(r"struct DsaEncodeMergeOptions\s*\{(.*?)\n\}", cs, re.S)
    assert m, "DsaEncodeMergeOptions is not declared"
    assert [" ".join(f.split()) for f in re.sub(r"//[^\n]*", "", m.group(1)).split(";") if f.strip()] == \
        ["public DsaEncodeOrderOptions Order", "public int MergePoints", "public fixed int Reserved[7]"]
    for name in ("dsa_encode_default_merge_options(out DsaEncodeMergeOptions options)",
                 "dsa_encode_merged_sequential_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, DsaMeshGrids* grids, in DsaEncodeMergeOptions options, out IntPtr encoded)",
                 "dsa_encoded_row_entries(IntPtr encoded, uint mesh, uint* dst, nuint capacity, out uint count)"):
        assert name in cs
    header = open(os.path.join(ROOT, "include", "draco_mi355x.h")).read()
    h = re.search(r"typedef struct dsa_encode_merge_options \{(.*?)\} dsa_encode_merge_options;", header, re.S)
    assert h and [" ".join(f.split()) for f in re.sub(r"/\*.*?\*/", "", h.group(1), flags=re.S).split(";") if f.strip()] == \
        ["dsa_encode_order_options order", "int32_t merge_points", "int32_t reserved[7]"]
    enc = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "GpuDracoEncoder.cs")).read()
    for word in ("public int MergePoints", "public uint[] RowEntries(int i)", "dsa_encode_merged_sequential_batch", "mo.MergePoints = MergePoints", "dsa_encoded_row_entries"):
        assert word in enc


def test_config_switch():
    assert dsa.Config().merge_points == 0
    cfg = dsa.Config(merge_points=dsa.MERGE_CELLS, point_order=dsa.POINT_ORDER_MORTON, encoding_method=0, position_bits=13)
    assert cfg.merge_points == 1
    with pytest.raises(ValueError, match="merge_points 2"):
        dsa.Config(merge_points=2, point_order=1, encoding_method=0)
    with pytest.raises(ValueError, match="merge_points.*point_order=POINT_ORDER_MORTON"):
        dsa.Config(merge_points=dsa.MERGE_CELLS, encoding_method=0)                      # the caller's order
    with pytest.raises(ValueError, match="merge_points.*sequential"):
        dsa.Config(merge_points=dsa.MERGE_CELLS, point_order=dsa.POINT_ORDER_MORTON)      # an Edgebreaker config
    o = cfg._native_merge(0)
    assert o.merge_points == 1 and o.order.point_order == 1 and o.order.sequential.geometry == 0 and o.order.sequential.base.position_bits == 13
    assert list(o.reserved) == [0] * 7 and list(o.order.reserved) == [0] * 7


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
    # the calls without the option keep arriving where they always did
    enc.EncodeBatch([cloud], dsa.Config(), handle=True)
    enc.EncodeBatch([cloud], dsa.Config(point_order=1, encoding_method=0), handle=True)
    assert [c[0] for c in r.calls] == ["dsa_encode_grid_sequential_batch", "dsa_encode_ordered_sequential_batch"]
    del r.calls[:]
    merged = dsa.Config(merge_points=dsa.MERGE_CELLS, point_order=dsa.POINT_ORDER_MORTON, encoding_method=0)
    enc.EncodeBatch([cloud, cloud], merged, handle=True)
    assert [c[0] for c in r.calls] == ["dsa_encode_merged_sequential_batch"]
    _, n, _, grids, opt, _ = r.calls[0][1]
    assert n == 2 and grids is None and opt._obj.merge_points == 1 and opt._obj.order.point_order == 1 and opt._obj.order.sequential.geometry == 0
    # merging the points of a mesh would collapse its faces
    with pytest.raises(ValueError, match="merge_points takes point clouds"):
        enc.EncodeBatch([mesh], merged, handle=True)
    assert len(r.calls) == 1
