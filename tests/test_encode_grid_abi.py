"""dsa_encode_grid_batch / dsa_encode_grid_sequential_batch (quantisation grids given by the caller or shared within a group): the
ctypes mirrors and the C# declarations of dsa_quantization_grid, dsa_mesh_grids and dsa_encode_grid_options against the header as
a C compiler lays it out, the exports, the ABI version, the argument failures that need no device, and what Grid / MeshData /
Attribute refuse before the device is touched.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import draco_sharp_amd as dsa
from draco_sharp_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = (("dsa_quantization_grid", native.QuantizationGrid, ("origin", "range", "mode", "reserved")),
           ("dsa_mesh_grids", native.MeshGrids, ("position", "texcoord", "attributes", "group", "reserved")),
           ("dsa_encode_grid_options", native.EncodeGridOptions, ("repair", "weld_points", "reserved")))


def test_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    body = ""
    for name, _, fields in STRUCTS:
        body += '  printf(" %%zu", sizeof(%s));\n' % name + "".join('  printf(" %%zu", offsetof(%s, %s));\n' % (name, f) for f in fields)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "draco_mi355x.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for _, mirror, fields in STRUCTS:
        assert [n for n, _ in mirror._fields_] == list(fields)
        want += [C.sizeof(mirror)] + [getattr(mirror, f).offset for f in fields]
    assert got == want
    assert C.sizeof(native.QuantizationGrid) == 32 and C.sizeof(native.MeshGrids) == 80
    assert C.sizeof(native.EncodeGridOptions) == C.sizeof(native.EncodeRepairOptions) + 32


def test_abi_version_and_exports():
    L = native.lib()
    for name in ("dsa_encode_default_grid_options", "dsa_encode_grid_batch", "dsa_encode_grid_sequential_batch"):
        assert name in native.EXPORTS
        assert hasattr(L, name)
    assert L.dsa_abi_version() == 4


def test_default_options_are_those_of_the_repair_call():
    L = native.lib()
    go, ro = native.EncodeGridOptions(), native.EncodeRepairOptions()
    C.memset(C.byref(go), 0xFF, C.sizeof(go))
    L.dsa_encode_default_grid_options(C.byref(go))
    L.dsa_encode_default_repair_options(C.byref(ro))
    assert bytes(go.repair) == bytes(ro) and go.weld_points == 0 and list(go.reserved) == [0] * 7
    L.dsa_encode_default_grid_options(None)


def test_argument_failures_that_need_no_device():
    """The options are checked before anything else is touched; a null context or result pointer fails either call."""
    L = native.lib()
    h = C.c_void_p()

    def options(**kw):
        o = native.EncodeGridOptions()
        L.dsa_encode_default_grid_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o
    for weld in (2, -1):
        assert L.dsa_encode_grid_batch(None, 0, None, None, C.byref(options(weld_points=weld)), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT
    for k in range(7):
        o = options()
        o.reserved[k] = 1
        assert L.dsa_encode_grid_batch(None, 0, None, None, C.byref(o), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT
    o = options()
    o.repair.topology = 2
    assert L.dsa_encode_grid_batch(None, 0, None, None, C.byref(o), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT
    o = options()
    o.repair.reserved[3] = 1
    assert L.dsa_encode_grid_batch(None, 0, None, None, C.byref(o), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT
    assert L.dsa_encode_grid_batch(None, 0, None, None, C.byref(options()), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT      # no context
    assert L.dsa_encode_grid_batch(None, 0, None, None, None, C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT
    so = native.EncodeSequentialOptions()
    L.dsa_encode_sequential_default_options(C.byref(so))
    assert L.dsa_encode_grid_sequential_batch(None, 0, None, None, C.byref(so), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT


def test_csharp_declarations_agree_with_the_header():
    cs = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "NativeMethods.cs")).read()

    def fields(struct):
        m = re.search(r"struct %s\s*\{(.*?)\n\}" % struct, cs, re.S)
        assert m, "%s is not declared" % struct
        return [" ".join(f.split()) for f in re.sub(r"//[^\n]*", "", m.group(1)).split(";") if f.strip()]
    assert fields("DsaQuantizationGrid") == ["public fixed float Origin[4]", "public float Range", "public int Mode", "public fixed uint Reserved[2]"]
    assert fields("DsaMeshGrids") == ["public DsaQuantizationGrid Position, Texcoord", "public DsaQuantizationGrid* Attributes", "public uint Group", "public uint Reserved"]
    assert fields("DsaEncodeGridOptions") == ["public DsaEncodeRepairOptions Repair", "public int WeldPoints", "public fixed int Reserved[7]"]
    for name in ("dsa_encode_default_grid_options(out DsaEncodeGridOptions options)",
                 "dsa_encode_grid_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, DsaMeshGrids* grids, in DsaEncodeGridOptions options, out IntPtr encoded)",
                 "dsa_encode_grid_sequential_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, DsaMeshGrids* grids, in DsaEncodeSequentialOptions options, out IntPtr encoded)"):
        assert name in cs
    enc = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "GpuDracoEncoder.cs")).read()
    for word in ("QuantizationOrigin", "QuantizationRange", "Groups", "dsa_encode_grid_batch"):
        assert word in enc


def test_what_grid_and_meshdata_refuse():
    pos = np.zeros((4, 3), np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    for origin, rng in (([0, 0, 0], 0.0), ([0, 0, 0], -1.0), ([0, 0, 0], float("inf")), ([0, float("nan"), 0], 1.0), ([], 1.0), ([0] * 5, 1.0)):
        with pytest.raises(ValueError):
            dsa.Grid(origin, rng)
    g = dsa.Grid([0, 0, 0], 2.0)
    assert g.mode == 1 and dsa.Grid.shared().mode == 2
    n = g._native(3)
    assert list(n.origin) == [0, 0, 0, 0] and n.range == 2.0 and n.mode == 1 and list(n.reserved) == [0, 0]
    with pytest.raises(ValueError, match="origin components"):
        g._native(2)
    with pytest.raises(ValueError, match="position_grid"):
        dsa.MeshData(pos, faces, position_grid=([0, 0, 0], 1.0))
    with pytest.raises(ValueError, match="texcoord_grid without texcoords"):
        dsa.MeshData(pos, faces, texcoord_grid=dsa.Grid([0, 0], 1.0))
    with pytest.raises(ValueError, match="group"):
        dsa.MeshData(pos, faces, group=-1)
    with pytest.raises(ValueError, match="group"):
        dsa.PointCloudData(pos, group=1 << 32)
    with pytest.raises(ValueError, match="integer attributes have no grid"):
        dsa.Attribute(np.zeros(4, np.uint8), grid=dsa.Grid([0], 1.0))
    m = dsa.MeshData(pos, faces, texcoords=np.zeros((4, 2), np.float32), position_grid=g, texcoord_grid=dsa.Grid.shared(), group=7,
                     attributes=[dsa.Attribute(np.zeros((4, 2), np.float32), grid=dsa.Grid([0, 1], 3.0)), dsa.Attribute(np.zeros(4, np.uint8))])
    assert m.group == 7 and m.position_grid is g and m.attributes[0].grid.range == 3.0 and m.attributes[1].grid is None
    plain = dsa.MeshData(pos, faces)
    assert plain.position_grid is None and plain.texcoord_grid is None and plain.group == 0
