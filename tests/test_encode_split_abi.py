"""dsa_encode_split_sequential_batch (the Morton order of a point cloud in parts of bounded size): the ctypes mirrors and the C#
declarations of its structs against the header as a C compiler lays them out, the defaults, DSA_ENCODE_MAX_PARTS, the exports in
every layer, every option the call refuses before anything is touched, and how Config routes.  No GPU needed (the texts of the
refusals need a context to be read from: tests/test_gpu_encode_split.py asserts them)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import draco_sharp_amd as dsa
from draco_sharp_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION_FIELDS = ("merge", "part_points", "reserved")
INFO_FIELDS = ("input", "part", "parts", "first_entry", "num_points", "position_bits", "qmin", "qmax", "box_min", "box_max", "reserved")
SYMBOLS = ("dsa_encode_default_split_options", "dsa_encode_split_sequential_batch", "dsa_encoded_parts", "dsa_encoded_part_info")


def test_struct_layouts_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    body = '  printf(" %zu", sizeof(dsa_encode_split_options));\n' + "".join('  printf(" %%zu", offsetof(dsa_encode_split_options, %s));\n' % f for f in OPTION_FIELDS)
    body += '  printf(" %zu", sizeof(dsa_part_info));\n' + "".join('  printf(" %%zu", offsetof(dsa_part_info, %s));\n' % f for f in INFO_FIELDS)
    body += '  printf(" %u", DSA_ENCODE_MAX_PARTS);\n'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "draco_mi355x.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    opt, info = native.EncodeSplitOptions, native.PartInfo
    assert [n for n, _ in opt._fields_] == list(OPTION_FIELDS) and [n for n, _ in info._fields_] == list(INFO_FIELDS)
    assert got == [C.sizeof(opt)] + [getattr(opt, f).offset for f in OPTION_FIELDS] + [C.sizeof(info)] + [getattr(info, f).offset for f in INFO_FIELDS] + [65536]
    assert C.sizeof(opt) == C.sizeof(native.EncodeMergeOptions) + 32 == 160 and opt.part_points.offset == 128
    # six words, two integer triples, two float triples, two reserved words
    assert C.sizeof(info) == 80 and info.qmin.offset == 24 and info.box_min.offset == 48 and info.reserved.offset == 72
    assert native.ENCODE_MAX_PARTS == dsa.ENCODE_MAX_PARTS == 65536


def test_symbols_in_every_layer():
    L = native.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "draco_mi355x.h")).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "NativeMethods.cs")).read()
    for name in SYMBOLS:
        assert name in native.EXPORTS and hasattr(L, name)
        assert re.search(r"\b%s\s*\(" % name, header) and re.search(r"extern \w+ %s\(" % name, cs)
    assert re.search(r"#define DSA_ENCODE_MAX_PARTS 65536u", header)
    assert L.dsa_abi_version() == 4


def options(point_order=0, geometry=None, merge_points=0, **kw):
    o = native.EncodeSplitOptions()
    native.lib().dsa_encode_default_split_options(C.byref(o))
    o.merge.order.point_order, o.merge.merge_points = point_order, merge_points
    if geometry is not None:
        o.merge.order.sequential.geometry = geometry
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_default_options_are_those_of_the_merged_call():
    L = native.lib()
    so, mo = native.EncodeSplitOptions(), native.EncodeMergeOptions()
    C.memset(C.byref(so), 0xFF, C.sizeof(so))
    L.dsa_encode_default_split_options(C.byref(so))
    L.dsa_encode_default_merge_options(C.byref(mo))
    assert bytes(so.merge) == bytes(mo) and so.part_points == 0 and list(so.reserved) == [0] * 7
    L.dsa_encode_default_split_options(None)


def test_every_invalid_option_fails_the_call():
    """The options are checked before anything else is touched: no context, no meshes."""
    L = native.lib()
    h = C.c_void_p()

    def refused(o, field):
        assert L.dsa_encode_split_sequential_batch(None, 0, None, None, C.byref(o), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT, field
    for value in (-1, -2**31):
        refused(options(1, 0, part_points=value), "part_points")
    refused(options(0, 0, part_points=5), "part_points without point_order")
    refused(options(1, 1, part_points=5), "part_points with geometry 1")
    refused(options(1, None, part_points=5), "part_points with the default geometry (meshes)")
    refused(options(1, 0, merge_points=1, part_points=5), "part_points with merge_points")
    for k in range(7):
        o = options(1, 0, part_points=5)
        o.reserved[k] = 1
        refused(o, "reserved")
    # what the nested calls refuse, through this one
    refused(options(1, 0, merge_points=2), "merge_points")
    refused(options(2, 0), "point_order")
    o = options(1, 0, part_points=5)
    o.merge.reserved[2] = 1
    refused(o, "merge.reserved")
    o = options(1, 0, part_points=5)
    o.merge.order.sequential.base.position_bits = 21
    refused(o, "position_bits")
    refused(options(1, 0, part_points=5), "no context")
    assert L.dsa_encode_split_sequential_batch(None, 0, None, None, None, C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT
    first, count, info = C.c_uint32(), C.c_uint32(), native.PartInfo()
    assert L.dsa_encoded_parts(None, 0, C.byref(first), C.byref(count)) == native.DSA_ERR_INVALID_ARGUMENT
    assert L.dsa_encoded_part_info(None, 0, C.byref(info)) == native.DSA_ERR_INVALID_ARGUMENT


def test_csharp_declarations_agree_with_the_header():
    cs = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "NativeMethods.cs")).read()
    header = open(os.path.join(ROOT, "include", "draco_mi355x.h")).read()

    def fields(text):
        return [" ".join(f.split()) for f in re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S).split(";") if f.strip()]
    m = re.search(r"struct DsaEncodeSplitOptions\s*\{(.*?)\n\}", cs, re.S)
    assert m and fields(m.group(1)) == ["public DsaEncodeMergeOptions Merge", "public int PartPoints", "public fixed int Reserved[7]"]
    m = re.search(r"struct DsaPartInfo\s*\{(.*?)\n\}", cs, re.S)
    assert m and fields(m.group(1)) == ["public uint Input, Part, Parts", "public uint FirstEntry, NumPoints", "public uint PositionBits", "public fixed int QMin[3]",
                                        "public fixed int QMax[3]", "public fixed float BoxMin[3]", "public fixed float BoxMax[3]", "public fixed uint Reserved[2]"]
    h = re.search(r"typedef struct dsa_encode_split_options \{(.*?)\} dsa_encode_split_options;", header, re.S)
    assert h and fields(h.group(1)) == ["dsa_encode_merge_options merge", "int32_t part_points", "int32_t reserved[7]"]
    h = re.search(r"typedef struct dsa_part_info \{(.*?)\} dsa_part_info;", header, re.S)
    assert h and fields(h.group(1)) == ["uint32_t input, part, parts", "uint32_t first_entry, num_points", "uint32_t position_bits", "int32_t qmin[3], qmax[3]",
                                        "float box_min[3], box_max[3]", "uint32_t reserved[2]"]
    for name in ("dsa_encode_default_split_options(out DsaEncodeSplitOptions options)",
                 "dsa_encode_split_sequential_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, DsaMeshGrids* grids, in DsaEncodeSplitOptions options, out IntPtr encoded)",
                 "dsa_encoded_parts(IntPtr encoded, uint input, out uint firstStream, out uint count)",
                 "dsa_encoded_part_info(IntPtr encoded, uint stream, out DsaPartInfo info)"):
        assert name in cs
    enc = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "GpuDracoEncoder.cs")).read()
    for word in ("public int PartPoints", "Parts(int i)", "PartInfo(int s)", "dsa_encode_split_sequential_batch", "po.PartPoints = PartPoints", "dsa_encoded_part_info"):
        assert word in enc


def test_config_switch():
    assert dsa.Config().part_points == 0
    cfg = dsa.Config(part_points=4096, point_order=dsa.POINT_ORDER_MORTON, encoding_method=0, position_bits=13)
    assert cfg.part_points == 4096
    with pytest.raises(ValueError, match="part_points -1"):
        dsa.Config(part_points=-1, point_order=1, encoding_method=0)
    with pytest.raises(ValueError, match="part_points.*point_order=POINT_ORDER_MORTON"):
        dsa.Config(part_points=5, encoding_method=0)                                      # the caller's order
    with pytest.raises(ValueError, match="part_points.*sequential"):
        dsa.Config(part_points=5, point_order=dsa.POINT_ORDER_MORTON)                     # an Edgebreaker config
    with pytest.raises(ValueError, match="part_points.*no merge_points"):
        dsa.Config(part_points=5, point_order=dsa.POINT_ORDER_MORTON, merge_points=dsa.MERGE_CELLS, encoding_method=0)
    o = cfg._native_split(0)
    assert o.part_points == 4096 and o.merge.merge_points == 0 and o.merge.order.point_order == 1 and o.merge.order.sequential.geometry == 0
    assert o.merge.order.sequential.base.position_bits == 13 and list(o.reserved) == [0] * 7 and list(o.merge.reserved) == [0] * 7


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
    enc.EncodeBatch([cloud], dsa.Config(point_order=1, merge_points=1, encoding_method=0), handle=True)
    assert [c[0] for c in r.calls] == ["dsa_encode_grid_sequential_batch", "dsa_encode_ordered_sequential_batch", "dsa_encode_merged_sequential_batch"]
    del r.calls[:]
    split = dsa.Config(part_points=2, point_order=dsa.POINT_ORDER_MORTON, encoding_method=0)
    enc.EncodeBatch([cloud, cloud], split, handle=True)
    assert [c[0] for c in r.calls] == ["dsa_encode_split_sequential_batch"]
    _, n, _, grids, opt, _ = r.calls[0][1]
    assert n == 2 and grids is None and opt._obj.part_points == 2 and opt._obj.merge.merge_points == 0 and opt._obj.merge.order.point_order == 1
    assert opt._obj.merge.order.sequential.geometry == 0
    # a part of a mesh would need its faces cut
    with pytest.raises(ValueError, match="part_points takes point clouds"):
        enc.EncodeBatch([mesh], split, handle=True)
    assert len(r.calls) == 1
