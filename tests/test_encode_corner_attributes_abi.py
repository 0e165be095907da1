"""dsa_encode_corner_attributes_batch (row ids per corner for the attributes of the list; the listed attributes welded alone): the
ctypes mirrors and the C# declarations of its three structs against the header as a C compiler lays them out, the defaults, the
exports, the ABI version, every option the call refuses before anything is touched, and how Config / Attribute route.  No GPU
needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import draco_sharp_amd as dsa
from draco_sharp_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = (("dsa_attribute_corners", "AttributeCorners", ("corners", "num_rows", "reserved")),
           ("dsa_mesh_attribute_corners", "MeshAttributeCorners", ("attributes", "reserved")),
           ("dsa_encode_corner_attributes_options", "EncodeCornerAttributesOptions", ("seam_repair", "weld_attributes", "reserved")))


def test_struct_layouts_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    body = ""
    for cname, _, fields in STRUCTS:
        body += '  printf(" %%zu", sizeof(%s));\n' % cname + "".join('  printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f in fields)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "draco_mi355x.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for _, pyname, fields in STRUCTS:
        mirror = getattr(native, pyname)
        assert [n for n, _ in mirror._fields_] == list(fields)
        want += [C.sizeof(mirror)] + [getattr(mirror, f).offset for f in fields]
    assert got == want
    assert C.sizeof(native.AttributeCorners) == 16 and C.sizeof(native.MeshAttributeCorners) == 16
    assert C.sizeof(native.EncodeCornerAttributesOptions) == C.sizeof(native.EncodeSeamRepairOptions) + 32


def test_abi_version_and_exports():
    L = native.lib()
    for name in ("dsa_encode_default_corner_attributes_options", "dsa_encode_corner_attributes_batch"):
        assert name in native.EXPORTS
        assert hasattr(L, name)
    assert L.dsa_abi_version() == 4


def options(**kw):
    o = native.EncodeCornerAttributesOptions()
    native.lib().dsa_encode_default_corner_attributes_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_default_options_are_those_of_the_seam_repair_call():
    L = native.lib()
    co, so = native.EncodeCornerAttributesOptions(), native.EncodeSeamRepairOptions()
    C.memset(C.byref(co), 0xFF, C.sizeof(co))
    L.dsa_encode_default_corner_attributes_options(C.byref(co))
    L.dsa_encode_default_seam_repair_options(C.byref(so))
    assert bytes(co.seam_repair) == bytes(so) and co.weld_attributes == 0 and list(co.reserved) == [0] * 7
    L.dsa_encode_default_corner_attributes_options(None)


def test_every_invalid_option_fails_the_call():
    """The options are checked before anything else is touched: no context, no meshes."""
    L = native.lib()
    h = C.c_void_p()

    def refused(o, field):
        assert L.dsa_encode_corner_attributes_batch(None, 0, None, None, None, C.byref(o), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT, field
    for value in (2, -1, 7):
        refused(options(weld_attributes=value), "weld_attributes")
    for k in range(7):
        o = options()
        o.reserved[k] = 1
        refused(o, "reserved")
    o = options(weld_attributes=1)               # weld_points 0 (the default): the listed attributes of a welded mesh are the caller's
    assert o.seam_repair.grid.weld_points == 0
    refused(o, "weld_points")
    # what the sibling calls refuse, through this one
    o = options()
    o.seam_repair.corner_repair = 2
    refused(o, "corner_repair")
    o = options()
    o.seam_repair.corner_repair = 1              # (topology 0)
    refused(o, "topology")
    o = options()
    o.seam_repair.reserved[3] = 1
    refused(o, "reserved")
    o = options()
    o.seam_repair.grid.weld_points = 2
    refused(o, "weld_points")
    o = options()
    o.seam_repair.grid.repair.reserved[0] = 1
    refused(o, "reserved")
    assert L.dsa_encode_corner_attributes_batch(None, 0, None, None, None, C.byref(options()), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT      # no context
    assert L.dsa_encode_corner_attributes_batch(None, 0, None, None, None, None, C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT


def test_csharp_declarations_agree_with_the_header():
    cs = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "NativeMethods.cs")).read()
    want = {"DsaAttributeCorners": ["public uint* Corners", "public uint NumRows", "public uint Reserved"],
            "DsaMeshAttributeCorners": ["public DsaAttributeCorners* Attributes", "public fixed uint Reserved[2]"],
            "DsaEncodeCornerAttributesOptions": ["public DsaEncodeSeamRepairOptions SeamRepair", "public int WeldAttributes", "public fixed int Reserved[7]"]}
    for name, fields in want.items():
        m = re.search(r"struct %s\s*\{(.*?)\n\}" % name, cs, re.S)
        assert m, "%s is not declared" % name
        assert [" ".join(f.split()) for f in re.sub(r"//[^\n]*", "", m.group(1)).split(";") if f.strip()] == fields
    for name in ("dsa_encode_default_corner_attributes_options(out DsaEncodeCornerAttributesOptions options)",
                 "dsa_encode_corner_attributes_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, DsaMeshGrids* grids, DsaMeshAttributeCorners* corners, "
                 "in DsaEncodeCornerAttributesOptions options, out IntPtr encoded)"):
        assert name in cs
    header = open(os.path.join(ROOT, "include", "draco_mi355x.h")).read()
    for cname, fields in (("dsa_attribute_corners", ["const uint32_t *corners", "uint32_t num_rows", "uint32_t reserved"]),
                          ("dsa_mesh_attribute_corners", ["const dsa_attribute_corners *attributes", "uint32_t reserved[2]"]),
                          ("dsa_encode_corner_attributes_options", ["dsa_encode_seam_repair_options seam_repair", "int32_t weld_attributes", "int32_t reserved[7]"])):
        h = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), header, re.S)
        assert h and [" ".join(f.split()) for f in re.sub(r"/\*.*?\*/", "", h.group(1), flags=re.S).split(";") if f.strip()] == fields
    enc = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "GpuDracoEncoder.cs")).read()
    for word in ("public bool WeldAttributes", "public bool CornerAttributes", "dsa_encode_corner_attributes_batch", "co.WeldAttributes = 1", "a.MappedIndex((uint)face[c])"):
        assert word in enc


def test_config_switch():
    assert dsa.Config().weld_attributes is False
    assert dsa.Config(weld_points=True).weld_attributes is False
    assert dsa.Config(weld_points=True, weld_attributes=True).weld_attributes is True
    with pytest.raises(ValueError, match="weld_points"):
        dsa.Config(weld_attributes=True)
    with pytest.raises(ValueError):
        dsa.Config(weld_points=True, weld_attributes=True, encoding_method=0)      # (a sequential stream takes no weld at all)


def _mesh(ids=False, points=False):
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)
    faces = np.array([[0, 1, 2], [2, 1, 3]], np.uint32)
    if ids:
        return dsa.MeshData(pos, faces, attributes=[dsa.Attribute(np.arange(12, dtype=np.float32).reshape(6, 2), attribute_type=3, corners=np.arange(6).reshape(2, 3))])
    return dsa.MeshData(pos, faces, attributes=[dsa.Attribute(np.zeros((4, 2), np.float32), attribute_type=3)])


def test_attribute_ids_are_checked_like_the_built_in_ones():
    pos = np.zeros((4, 3), np.float32)
    faces = np.array([[0, 1, 2], [2, 1, 3]], np.uint32)
    rows = np.zeros((5, 2), np.float32)
    m = dsa.MeshData(pos, faces, attributes=[dsa.Attribute(rows, corners=[[0, 1, 2], [2, 1, 4]])])
    assert m.attributes[0].corners.dtype == np.uint32 and m.attributes[0].corners.shape == (2, 3) and m.per_corner
    with pytest.raises(ValueError, match="attribute 0 corners: id 5 out of range \\(5 rows\\)"):
        dsa.MeshData(pos, faces, attributes=[dsa.Attribute(rows, corners=[[0, 1, 2], [2, 1, 5]])])
    with pytest.raises(ValueError, match="attribute 0 corners: one id per face corner"):
        dsa.MeshData(pos, faces, attributes=[dsa.Attribute(rows, corners=[[0, 1, 2]])])
    with pytest.raises(ValueError, match="attribute 0 corners: ids are row numbers, not negative"):
        dsa.MeshData(pos, faces, attributes=[dsa.Attribute(rows, corners=[[0, 1, 2], [2, 1, -1]])])
    with pytest.raises(ValueError, match="attribute 0: one row per vertex"):
        dsa.MeshData(pos, faces, attributes=[dsa.Attribute(rows)])                  # without ids: one row per vertex, as ever
    with pytest.raises(ValueError, match="a point cloud has one value per point"):
        dsa.PointCloudData(pos, attributes=[dsa.Attribute(rows, corners=[[0, 1, 2], [2, 1, 4]])])


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


@pytest.fixture
def recorder(monkeypatch):
    r = _Recorder(native.lib())
    monkeypatch.setattr(native, "lib", lambda: r)

    class Ctx:
        _h = None
    return r, Ctx()


def test_encode_batch_takes_the_new_entry_point_only_when_asked(recorder):
    r, ctx = recorder
    enc = dsa.DracoEncoder(ctx)
    # nothing asked for: exactly as today
    enc.EncodeBatch([_mesh()], dsa.Config(), handle=True)
    enc.EncodeBatch([_mesh()], dsa.Config(weld_points=True), handle=True)
    assert [c[0] for c in r.calls] == ["dsa_encode_seam_repair_batch"] * 2
    # ids on an attribute of the list
    del r.calls[:]
    enc.EncodeBatch([_mesh(), _mesh(ids=True)], dsa.Config(repair_topology=True, repair_seams=True), handle=True)
    assert [c[0] for c in r.calls] == ["dsa_encode_corner_attributes_batch"]
    _, n, _, grids, corners, opt, _ = r.calls[0][1]
    o = opt._obj
    assert n == 2 and grids is None and o.weld_attributes == 0 and list(o.reserved) == [0] * 7
    assert o.seam_repair.corner_repair == 1 and o.seam_repair.grid.repair.topology == 1 and o.seam_repair.grid.weld_points == 0
    assert not corners[0].attributes and corners[1].attributes[0].num_rows == 6 and corners[1].attributes[0].corners
    assert list(corners[1].reserved) == [0, 0] and corners[1].attributes[0].reserved == 0
    # the listed attributes welded alone
    del r.calls[:]
    enc.EncodeBatch([_mesh()], dsa.Config(weld_points=True, weld_attributes=True), handle=True)
    assert [c[0] for c in r.calls] == ["dsa_encode_corner_attributes_batch"]
    o = r.calls[0][1][5]._obj
    assert o.weld_attributes == 1 and o.seam_repair.grid.weld_points == 1 and o.seam_repair.corner_repair == 0
    # per-point input takes no ids; a sequential stream has one value per point
    with pytest.raises(ValueError, match="weld_points takes one row per point"):
        enc.EncodeBatch([_mesh(ids=True)], dsa.Config(weld_points=True, weld_attributes=True), handle=True)
    with pytest.raises(ValueError, match="a sequential stream has one value per point"):
        enc.EncodeBatch([_mesh(ids=True)], dsa.Config(encoding_method=0), handle=True)
