"""dsa_encode_lod_sequential_batch (additive levels of detail of merged point clouds, on the device): the ctypes mirror and the C#
declaration of its structs against the header as a C compiler lays them out, the defaults, the exports in every layer, every option
the call refuses before anything is touched, the errors of Config and how it routes.  No GPU needed (the texts of the refusals need
a context to be read from: tests/test_gpu_encode_lod.py asserts them)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import draco_sharp_amd as dsa
from draco_sharp_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION_FIELDS = ("cell_parts", "lod_base_bits", "reserved")
INFO_FIELDS = ("input", "level", "levels", "cell_bits", "level_first_stream", "level_streams", "level_points", "part_in_level", "reserved")
SYMBOLS = ("dsa_encode_default_lod_options", "dsa_encode_lod_sequential_batch", "dsa_encoded_lod_info")


def test_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    body = '  printf(" %zu", sizeof(dsa_encode_lod_options));\n' + "".join('  printf(" %%zu", offsetof(dsa_encode_lod_options, %s));\n' % f for f in OPTION_FIELDS)
    body += '  printf(" %zu", sizeof(dsa_lod_info));\n' + "".join('  printf(" %%zu", offsetof(dsa_lod_info, %s));\n' % f for f in INFO_FIELDS)
    body += '  printf(" %zu %zu %zu", sizeof(dsa_encode_cell_parts_options), sizeof(dsa_encode_split_options), sizeof(dsa_part_info));\n'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "draco_mi355x.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    opt, info = native.EncodeLodOptions, native.LodInfo
    assert [n for n, _ in opt._fields_] == list(OPTION_FIELDS) and [n for n, _ in info._fields_] == list(INFO_FIELDS)
    assert got == ([C.sizeof(opt)] + [getattr(opt, f).offset for f in OPTION_FIELDS] + [C.sizeof(info)] + [getattr(info, f).offset for f in INFO_FIELDS]
                   + [192, 160, 80])             # (the existing structs stay)
    assert C.sizeof(opt) == C.sizeof(native.EncodeCellPartsOptions) + 32 == 224 and opt.lod_base_bits.offset == 192 and opt.reserved.offset == 196
    assert C.sizeof(info) == 48 and info.reserved.offset == 32


def test_symbols_in_every_layer():
    L = native.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "draco_mi355x.h")).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "NativeMethods.cs")).read()
    for name in SYMBOLS:
        assert name in native.EXPORTS and hasattr(L, name)
        assert re.search(r"\b%s\s*\(" % name, header) and re.search(r"extern \w+ %s\(" % name, cs)
    assert L.dsa_abi_version() == 4                       # the feature is detected by the symbol


def options(point_order=1, geometry=0, merge_points=1, part_cells=5, **kw):
    o = native.EncodeLodOptions()
    native.lib().dsa_encode_default_lod_options(C.byref(o))
    m = o.cell_parts.split.merge
    m.order.point_order, m.merge_points, o.cell_parts.part_cells = point_order, merge_points, part_cells
    if geometry is not None:
        m.order.sequential.geometry = geometry
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_default_options_are_those_of_the_cell_parts_call():
    L = native.lib()
    lo, co = native.EncodeLodOptions(), native.EncodeCellPartsOptions()
    C.memset(C.byref(lo), 0xFF, C.sizeof(lo))
    L.dsa_encode_default_lod_options(C.byref(lo))
    L.dsa_encode_default_cell_parts_options(C.byref(co))
    assert bytes(lo.cell_parts) == bytes(co) and lo.lod_base_bits == 0 and list(lo.reserved) == [0] * 7
    L.dsa_encode_default_lod_options(None)


def test_every_invalid_option_fails_the_call():
    """The options are checked before anything else is touched: no context, no meshes."""
    L = native.lib()
    h = C.c_void_p()

    def refused(o, field):
        assert L.dsa_encode_lod_sequential_batch(None, 0, None, None, C.byref(o), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT, field
    for value in (-1, -2**31):
        refused(options(lod_base_bits=value), "lod_base_bits")
    bits = options().cell_parts.split.merge.order.sequential.base.position_bits
    refused(options(lod_base_bits=bits + 1), "lod_base_bits above position_bits")
    refused(options(lod_base_bits=21), "lod_base_bits above every position_bits")
    refused(options(part_cells=0, lod_base_bits=3), "lod_base_bits without part_cells")
    refused(options(merge_points=0, part_cells=0, lod_base_bits=3), "lod_base_bits without merge_points")
    refused(options(merge_points=0, lod_base_bits=3), "lod_base_bits without merge_points, with part_cells")
    refused(options(point_order=0, lod_base_bits=3), "lod_base_bits without point_order")
    refused(options(geometry=1, lod_base_bits=3), "lod_base_bits with geometry 1")
    refused(options(geometry=None, lod_base_bits=3), "lod_base_bits with the default geometry (meshes)")
    for k in range(7):
        o = options(lod_base_bits=3)
        o.reserved[k] = 1
        refused(o, "reserved")
    # what the nested calls refuse, through this one
    refused(options(part_cells=-1), "part_cells")
    refused(options(merge_points=2), "merge_points")
    o = options(lod_base_bits=3)
    o.cell_parts.reserved[2] = 1
    refused(o, "cell_parts.reserved")
    o = options(lod_base_bits=3)
    o.cell_parts.split.part_points = 7
    refused(o, "part_points")
    o = options(lod_base_bits=3)
    o.cell_parts.split.merge.order.sequential.base.position_bits = 21
    refused(o, "position_bits")
    refused(options(lod_base_bits=3), "no context")
    refused(options(lod_base_bits=0), "no context, no levels")
    assert L.dsa_encode_lod_sequential_batch(None, 0, None, None, None, C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT
    assert L.dsa_encoded_lod_info(None, 0, C.byref(native.LodInfo())) == native.DSA_ERR_INVALID_ARGUMENT


def test_csharp_declarations_agree_with_the_header():
    cs = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "NativeMethods.cs")).read()
    header = open(os.path.join(ROOT, "include", "draco_mi355x.h")).read()

    def fields(text):
        return [" ".join(f.split()) for f in re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S).split(";") if f.strip()]
    m = re.search(r"struct DsaEncodeLodOptions\s*\{(.*?)\n\}", cs, re.S)
    assert m and fields(m.group(1)) == ["public DsaEncodeCellPartsOptions CellParts", "public int LodBaseBits", "public fixed int Reserved[7]"]
    h = re.search(r"typedef struct dsa_encode_lod_options \{(.*?)\} dsa_encode_lod_options;", header, re.S)
    assert h and fields(h.group(1)) == ["dsa_encode_cell_parts_options cell_parts", "int32_t lod_base_bits", "int32_t reserved[7]"]
    m = re.search(r"struct DsaLodInfo\s*\{(.*?)\n\}", cs, re.S)
    assert m and fields(m.group(1)) == ["public uint Input", "public uint Level, Levels", "public uint CellBits", "public uint LevelFirstStream, LevelStreams",
                                        "public uint LevelPoints", "public uint PartInLevel", "public fixed uint Reserved[4]"]
    h = re.search(r"typedef struct dsa_lod_info \{(.*?)\} dsa_lod_info;", header, re.S)
    assert h and fields(h.group(1)) == ["uint32_t input", "uint32_t level, levels", "uint32_t cell_bits", "uint32_t level_first_stream, level_streams",
                                        "uint32_t level_points", "uint32_t part_in_level", "uint32_t reserved[4]"]
    for name in ("dsa_encode_default_lod_options(out DsaEncodeLodOptions options)",
                 "dsa_encode_lod_sequential_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, DsaMeshGrids* grids, in DsaEncodeLodOptions options, out IntPtr encoded)",
                 "dsa_encoded_lod_info(IntPtr encoded, uint stream, out DsaLodInfo info)"):
        assert name in cs
    enc = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "GpuDracoEncoder.cs")).read()
    for word in ("public int LodBaseBits", "public LodLevel LodInfo(int s)", "dsa_encode_lod_sequential_batch", "lo.LodBaseBits = LodBaseBits", "lo.CellParts.PartCells = PartCells",
                 "LodBaseBits needs PartCells", "LodBaseBits takes point clouds"):
        assert word in enc
    # what the header says is not built
    for word in ("nearest the cell centre", "levels of sequential meshes", "levels\n * without the merge", "joined decode-side layout of the levels"):
        assert word in header, word


def test_config_switch():
    assert dsa.Config().lod_base_bits == 0
    base = dict(merge_points=dsa.MERGE_CELLS, point_order=dsa.POINT_ORDER_MORTON, encoding_method=0)
    cfg = dsa.Config(lod_base_bits=9, part_cells=4096, position_bits=13, **base)
    assert cfg.lod_base_bits == 9 and cfg.part_cells == 4096
    assert dsa.Config(lod_base_bits=13, part_cells=1, position_bits=13, **base).lod_base_bits == 13
    with pytest.raises(ValueError, match="lod_base_bits -1"):
        dsa.Config(lod_base_bits=-1, part_cells=5, **base)
    with pytest.raises(ValueError, match="lod_base_bits 14 is above position_bits 13"):
        dsa.Config(lod_base_bits=14, part_cells=5, position_bits=13, **base)
    with pytest.raises(ValueError, match="lod_base_bits.*part_cells >= 1"):
        dsa.Config(lod_base_bits=5, **base)
    with pytest.raises(ValueError, match="part_cells"):
        dsa.Config(lod_base_bits=5, part_cells=5, point_order=dsa.POINT_ORDER_MORTON, encoding_method=0)        # no merge: part_cells refuses first
    with pytest.raises(ValueError):
        dsa.Config(lod_base_bits=5, part_cells=5, merge_points=dsa.MERGE_CELLS, point_order=dsa.POINT_ORDER_MORTON)      # an Edgebreaker config
    o = cfg._native_lod(0)
    assert o.lod_base_bits == 9 and o.cell_parts.part_cells == 4096 and o.cell_parts.split.part_points == 0 and o.cell_parts.split.merge.merge_points == 1
    assert o.cell_parts.split.merge.order.point_order == 1 and o.cell_parts.split.merge.order.sequential.geometry == 0
    assert o.cell_parts.split.merge.order.sequential.base.position_bits == 13 and list(o.reserved) == [0] * 7 and list(o.cell_parts.reserved) == [0] * 7


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
    enc.EncodeBatch([cloud], dsa.Config(point_order=1, merge_points=1, encoding_method=0), handle=True)
    enc.EncodeBatch([cloud], dsa.Config(point_order=1, part_points=2, encoding_method=0), handle=True)
    enc.EncodeBatch([cloud], dsa.Config(point_order=1, merge_points=1, part_cells=2, encoding_method=0), handle=True)
    assert [c[0] for c in r.calls] == ["dsa_encode_grid_sequential_batch", "dsa_encode_merged_sequential_batch", "dsa_encode_split_sequential_batch",
                                       "dsa_encode_cell_parts_sequential_batch"]
    del r.calls[:]
    levels = dsa.Config(lod_base_bits=3, part_cells=2, merge_points=dsa.MERGE_CELLS, point_order=dsa.POINT_ORDER_MORTON, encoding_method=0)
    enc.EncodeBatch([cloud, cloud], levels, handle=True)
    assert [c[0] for c in r.calls] == ["dsa_encode_lod_sequential_batch"]
    _, n, _, grids, opt, _ = r.calls[0][1]
    o = opt._obj
    assert n == 2 and grids is None and o.lod_base_bits == 3 and o.cell_parts.part_cells == 2 and o.cell_parts.split.merge.merge_points == 1
    assert o.cell_parts.split.merge.order.point_order == 1 and o.cell_parts.split.merge.order.sequential.geometry == 0
    with pytest.raises(ValueError, match="part_cells takes point clouds"):
        enc.EncodeBatch([mesh], levels, handle=True)
    assert len(r.calls) == 1
