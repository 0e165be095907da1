"""dsa_encode_cell_parts_sequential_batch (the kept order of merge_points in parts of bounded size, sized on the device): the
ctypes mirror and the C# declaration of its struct against the header as a C compiler lays it out, the defaults, the exports in
every layer, every option the call refuses before anything is touched, the errors of Config and how it routes.  No GPU needed (the
texts of the refusals need a context to be read from: tests/test_gpu_encode_cell_parts.py asserts them)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import draco_sharp_amd as dsa
from draco_sharp_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION_FIELDS = ("split", "part_cells", "reserved")
SYMBOLS = ("dsa_encode_default_cell_parts_options", "dsa_encode_cell_parts_sequential_batch")


def test_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    body = '  printf(" %zu", sizeof(dsa_encode_cell_parts_options));\n' + "".join('  printf(" %%zu", offsetof(dsa_encode_cell_parts_options, %s));\n' % f for f in OPTION_FIELDS)
    body += '  printf(" %zu %zu", sizeof(dsa_encode_split_options), sizeof(dsa_part_info));\n'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "draco_mi355x.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    opt = native.EncodeCellPartsOptions
    assert [n for n, _ in opt._fields_] == list(OPTION_FIELDS)
    assert got == [C.sizeof(opt)] + [getattr(opt, f).offset for f in OPTION_FIELDS] + [160, 80]          # (the existing structs stay)
    assert C.sizeof(opt) == C.sizeof(native.EncodeSplitOptions) + 32 == 192 and opt.part_cells.offset == 160 and opt.reserved.offset == 164


def test_symbols_in_every_layer():
    L = native.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "draco_mi355x.h")).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "NativeMethods.cs")).read()
    for name in SYMBOLS:
        assert name in native.EXPORTS and hasattr(L, name)
        assert re.search(r"\b%s\s*\(" % name, header) and re.search(r"extern \w+ %s\(" % name, cs)
    assert L.dsa_abi_version() == 4                       # the feature is detected by the symbol


def options(point_order=1, geometry=0, merge_points=1, part_points=0, **kw):
    o = native.EncodeCellPartsOptions()
    native.lib().dsa_encode_default_cell_parts_options(C.byref(o))
    o.split.merge.order.point_order, o.split.merge.merge_points, o.split.part_points = point_order, merge_points, part_points
    if geometry is not None:
        o.split.merge.order.sequential.geometry = geometry
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_default_options_are_those_of_the_split_call():
    L = native.lib()
    co, so = native.EncodeCellPartsOptions(), native.EncodeSplitOptions()
    C.memset(C.byref(co), 0xFF, C.sizeof(co))
    L.dsa_encode_default_cell_parts_options(C.byref(co))
    L.dsa_encode_default_split_options(C.byref(so))
    assert bytes(co.split) == bytes(so) and co.part_cells == 0 and list(co.reserved) == [0] * 7
    L.dsa_encode_default_cell_parts_options(None)


def test_every_invalid_option_fails_the_call():
    """The options are checked before anything else is touched: no context, no meshes."""
    L = native.lib()
    h = C.c_void_p()

    def refused(o, field):
        assert L.dsa_encode_cell_parts_sequential_batch(None, 0, None, None, C.byref(o), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT, field
    for value in (-1, -2**31):
        refused(options(part_cells=value), "part_cells")
    refused(options(merge_points=0, part_cells=5), "part_cells without merge_points")
    refused(options(point_order=0, part_cells=5), "part_cells without point_order")
    refused(options(geometry=1, part_cells=5), "part_cells with geometry 1")
    refused(options(geometry=None, part_cells=5), "part_cells with the default geometry (meshes)")
    refused(options(part_points=7, part_cells=5), "part_cells with part_points")
    refused(options(merge_points=0, part_points=7, part_cells=5), "part_cells with part_points and no merge_points")
    for k in range(7):
        o = options(part_cells=5)
        o.reserved[k] = 1
        refused(o, "reserved")
    # what the nested calls refuse, through this one
    refused(options(part_points=7), "part_points with merge_points")
    refused(options(merge_points=2), "merge_points")
    refused(options(point_order=2), "point_order")
    o = options(part_cells=5)
    o.split.reserved[2] = 1
    refused(o, "split.reserved")
    o = options(part_cells=5)
    o.split.merge.reserved[4] = 1
    refused(o, "split.merge.reserved")
    o = options(part_cells=5)
    o.split.merge.order.sequential.base.position_bits = 21
    refused(o, "position_bits")
    refused(options(part_cells=5), "no context")
    assert L.dsa_encode_cell_parts_sequential_batch(None, 0, None, None, None, C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT


def test_csharp_declarations_agree_with_the_header():
    cs = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "NativeMethods.cs")).read()
    header = open(os.path.join(ROOT, "include", "draco_mi355x.h")).read()

    def fields(text):
        return [" ".join(f.split()) for f in re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S).split(";") if f.strip()]
    m = re.search(r"struct DsaEncodeCellPartsOptions\s*\{(.*?)\n\}", cs, re.S)
    assert m and fields(m.group(1)) == ["public DsaEncodeSplitOptions Split", "public int PartCells", "public fixed int Reserved[7]"]
    h = re.search(r"typedef struct dsa_encode_cell_parts_options \{(.*?)\} dsa_encode_cell_parts_options;", header, re.S)
    assert h and fields(h.group(1)) == ["dsa_encode_split_options split", "int32_t part_cells", "int32_t reserved[7]"]
    for name in ("dsa_encode_default_cell_parts_options(out DsaEncodeCellPartsOptions options)",
                 "dsa_encode_cell_parts_sequential_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, DsaMeshGrids* grids, in DsaEncodeCellPartsOptions options, out IntPtr encoded)"):
        assert name in cs
    enc = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "GpuDracoEncoder.cs")).read()
    for word in ("public int PartCells", "dsa_encode_cell_parts_sequential_batch", "co.PartCells = PartCells", "co.Split = po", "PartCells takes point clouds"):
        assert word in enc
    # the sentences of the split call that say what it does not build keep their text
    assert "Not built: parts with merge_points = 1 (the number of kept points, and so of parts, is known only on the device" in header


def test_config_switch():
    assert dsa.Config().part_cells == 0
    cfg = dsa.Config(part_cells=4096, merge_points=dsa.MERGE_CELLS, point_order=dsa.POINT_ORDER_MORTON, encoding_method=0, position_bits=13)
    assert cfg.part_cells == 4096 and cfg.part_points == 0
    with pytest.raises(ValueError, match="part_cells -1"):
        dsa.Config(part_cells=-1, merge_points=1, point_order=1, encoding_method=0)
    with pytest.raises(ValueError, match="part_cells.*merge_points=MERGE_CELLS"):
        dsa.Config(part_cells=5, point_order=dsa.POINT_ORDER_MORTON, encoding_method=0)   # no merge
    with pytest.raises(ValueError):
        dsa.Config(part_cells=5, merge_points=dsa.MERGE_CELLS, encoding_method=0)         # the caller's order (merge_points refuses first)
    with pytest.raises(ValueError):
        dsa.Config(part_cells=5, merge_points=dsa.MERGE_CELLS, point_order=dsa.POINT_ORDER_MORTON)      # an Edgebreaker config
    with pytest.raises(ValueError, match="part_points"):
        dsa.Config(part_cells=5, part_points=7, merge_points=dsa.MERGE_CELLS, point_order=dsa.POINT_ORDER_MORTON, encoding_method=0)
    with pytest.raises(ValueError, match="part_cells"):
        dsa.Config(part_cells=5, part_points=7, point_order=dsa.POINT_ORDER_MORTON, encoding_method=0)
    o = cfg._native_cell_parts(0)
    assert o.part_cells == 4096 and o.split.part_points == 0 and o.split.merge.merge_points == 1 and o.split.merge.order.point_order == 1
    assert o.split.merge.order.sequential.geometry == 0 and o.split.merge.order.sequential.base.position_bits == 13
    assert list(o.reserved) == [0] * 7 and list(o.split.reserved) == [0] * 7 and list(o.split.merge.reserved) == [0] * 7


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
    enc.EncodeBatch([cloud], dsa.Config(point_order=1, part_points=2, encoding_method=0), handle=True)
    assert [c[0] for c in r.calls] == ["dsa_encode_grid_sequential_batch", "dsa_encode_ordered_sequential_batch", "dsa_encode_merged_sequential_batch",
                                       "dsa_encode_split_sequential_batch"]
    del r.calls[:]
    parts = dsa.Config(part_cells=2, merge_points=dsa.MERGE_CELLS, point_order=dsa.POINT_ORDER_MORTON, encoding_method=0)
    enc.EncodeBatch([cloud, cloud], parts, handle=True)
    assert [c[0] for c in r.calls] == ["dsa_encode_cell_parts_sequential_batch"]
    _, n, _, grids, opt, _ = r.calls[0][1]
    o = opt._obj
    assert n == 2 and grids is None and o.part_cells == 2 and o.split.part_points == 0 and o.split.merge.merge_points == 1 and o.split.merge.order.point_order == 1
    assert o.split.merge.order.sequential.geometry == 0
    # a part of a mesh would need its faces cut
    with pytest.raises(ValueError, match="part_cells takes point clouds"):
        enc.EncodeBatch([mesh], parts, handle=True)
    assert len(r.calls) == 1
