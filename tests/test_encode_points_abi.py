"""dsa_encode_points_batch / dsa_weld_batch (meshes given as one row per point, welded in front of the Edgebreaker coder): the
ctypes mirror and the C# declaration of dsa_welded_info against the header as a C compiler lays it out, the exports, the ABI
version, the argument failures that need no device, and what Config / EncodeBatch / WeldBatch refuse before the device is
touched.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import draco_sharp_amd as dsa
from draco_sharp_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("status", "num_points", "num_vertices", "num_normals", "num_texcoords", "normals_per_vertex", "texcoords_per_vertex", "reserved",
          "vertex_of_point", "vertex_point", "normal_of_point", "normal_point", "texcoord_of_point", "texcoord_point")


def test_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "draco_mi355x.h"\nint main(void) {\n'
                   '  printf("%zu %zu", sizeof(dsa_welded_info), sizeof(dsa_mesh_attr_input));\n' +
                   "".join('  printf(" %%zu", offsetof(dsa_welded_info, %s));\n' % f for f in FIELDS) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(native.WeldedInfo), C.sizeof(native.MeshAttrInput)] + [getattr(native.WeldedInfo, f).offset for f in FIELDS]
    assert got == want
    assert got[0] == 80 and got[1] == 96
    assert [n for n, _ in native.WeldedInfo._fields_] == list(FIELDS)


def test_abi_version_and_exports():
    L = native.lib()
    for name in ("dsa_encode_points_batch", "dsa_weld_batch", "dsa_welded_size", "dsa_welded_mesh", "dsa_welded_free"):
        assert name in native.EXPORTS
        assert hasattr(L, name)
    assert L.dsa_abi_version() == 4


def test_argument_failures_that_need_no_device():
    """The options are those of dsa_encode_repair_batch and are checked before anything else is touched; a null context or result
    pointer fails either call; the accessors answer a null handle."""
    L = native.lib()
    h = C.c_void_p()
    for field, value in (("topology", 2), ("topology", -1)):
        o = native.EncodeRepairOptions()
        L.dsa_encode_default_repair_options(C.byref(o))
        setattr(o, field, value)
        assert L.dsa_encode_points_batch(None, 0, None, C.byref(o), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT
    for k in range(7):
        o = native.EncodeRepairOptions()
        L.dsa_encode_default_repair_options(C.byref(o))
        o.reserved[k] = 1
        assert L.dsa_encode_points_batch(None, 0, None, C.byref(o), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT
    o = native.EncodeRepairOptions()
    L.dsa_encode_default_repair_options(C.byref(o))
    assert L.dsa_encode_points_batch(None, 0, None, C.byref(o), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT      # no context
    assert L.dsa_weld_batch(None, 0, None, C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT
    assert L.dsa_welded_size(None) == 0
    info = native.WeldedInfo()
    assert L.dsa_welded_mesh(None, 0, C.byref(info)) == native.DSA_ERR_INVALID_ARGUMENT
    L.dsa_welded_free(None)


def test_csharp_declarations_agree_with_the_header():
    cs = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "NativeMethods.cs")).read()
    m = re.search(r"struct DsaWeldedInfo\s*\{(.*?)\n\}", cs, re.S)
    assert m, "DsaWeldedInfo is not declared"
    body = re.sub(r"//[^\n]*", "", m.group(1))
    fields = [" ".join(f.split()) for f in body.split(";") if f.strip()]
    assert fields == ["public int Status", "public uint NumPoints, NumVertices, NumNormals, NumTexcoords", "public uint NormalsPerVertex, TexcoordsPerVertex",
                      "public uint Reserved", "public uint* VertexOfPoint, VertexPoint", "public uint* NormalOfPoint, NormalPoint",
                      "public uint* TexcoordOfPoint, TexcoordPoint"]
    for name in ("dsa_encode_points_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, in DsaEncodeRepairOptions options, out IntPtr encoded)",
                 "dsa_weld_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, out IntPtr welded)",
                 "dsa_welded_mesh(IntPtr welded, uint mesh, out DsaWeldedInfo info)", "dsa_welded_free(IntPtr welded)"):
        assert name in cs
    enc = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "GpuDracoEncoder.cs")).read()
    assert "public bool WeldPoints" in enc and "dsa_encode_points_batch(_ctx" in enc


def test_config_carries_the_option():
    assert dsa.Config().weld_points is False
    cfg = dsa.Config(weld_points=True, repair_topology=True, traversal_method=1)
    assert cfg.weld_points and cfg._native_repair().topology == 1
    assert dsa.Config(weld_points=True)._native_repair().topology == 0
    with pytest.raises(ValueError, match="weld_points"):
        dsa.Config(weld_points=True, encoding_method=0)
    with pytest.raises(ValueError, match="weld_points"):
        dsa.Config(weld_points=True, encoding_method=-1, speed=10)


class NoDevice:
    """A context that fails the test when anything reaches for the device."""
    @property
    def _h(self):
        raise AssertionError("the device was touched")


def test_what_the_python_surface_refuses_before_the_device():
    pos = np.random.default_rng(0).random((4, 3)).astype(np.float32)
    faces = np.array([[0, 1, 2], [2, 1, 3]], np.uint32)
    uv = pos[:, :2].copy()
    enc = dsa.DracoEncoder(NoDevice())
    corners = dsa.MeshData(pos, faces, texcoords=uv, texcoord_corners=faces)
    with pytest.raises(ValueError, match="weld_points"):
        enc.EncodeBatch([corners], dsa.Config(weld_points=True))
    with pytest.raises(ValueError, match="weld_points"):
        enc.EncodeBatch([dsa.PointCloudData(pos)], dsa.Config(weld_points=True))
    cfg = dsa.Config(weld_points=True)
    cfg.encoding_method = 0                                   # (set behind the constructor's back)
    with pytest.raises(ValueError, match="weld_points"):
        enc.EncodeBatch([dsa.MeshData(pos, faces)], cfg)
    with pytest.raises(ValueError, match="welded already"):
        enc.WeldBatch([corners])
    with pytest.raises(ValueError, match="point cloud"):
        enc.WeldBatch([dsa.PointCloudData(pos)])
