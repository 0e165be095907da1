"""dsa_attribute_input / dsa_mesh_attr_input and the two entry points that take them (the encoder's attribute list): the ctypes
mirrors against the header as a C compiler lays it out, the exports, the ABI version, and what the Python surface (Attribute,
MeshData / PointCloudData attributes=) accepts.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import draco_sharp_amd as dsa
from draco_sharp_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATTRIBUTE_FIELDS = ("attribute_type", "data_type", "num_components", "normalized", "unique_id", "quantization_bits", "values", "reserved")
MESH_FIELDS = ("mesh", "attributes", "num_attributes", "reserved")


def layout(tmp_path, struct, fields):
    src = tmp_path / ("layout_%s.c" % struct)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "draco_mi355x.h"\nint main(void) {\n'
                   '  printf("%%zu", sizeof(%s));\n' % struct +
                   "".join('  printf(" %%zu", offsetof(%s, %s));\n' % (struct, f) for f in fields) + "  return 0;\n}\n")
    exe = str(tmp_path / ("layout_" + struct))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    return [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]


def test_attribute_input_layout_matches_the_header(tmp_path):
    got = layout(tmp_path, "dsa_attribute_input", ATTRIBUTE_FIELDS)
    assert got == [C.sizeof(native.AttributeInput)] + [getattr(native.AttributeInput, f).offset for f in ATTRIBUTE_FIELDS]
    assert got == [40, 0, 4, 8, 12, 16, 20, 24, 32]


def test_mesh_attr_input_layout_matches_the_header(tmp_path):
    got = layout(tmp_path, "dsa_mesh_attr_input", MESH_FIELDS)
    assert got == [C.sizeof(native.MeshAttrInput)] + [getattr(native.MeshAttrInput, f).offset for f in MESH_FIELDS]
    assert got == [96, 0, 80, 88, 92]
    # the structs before it keep their layout
    assert C.sizeof(native.MeshInput) == 56 and C.sizeof(native.MeshCornerInput) == 80
    assert C.sizeof(native.EncodeOptionsEx) == 64 and C.sizeof(native.EncodeSequentialOptions) == 64


def test_abi_version_and_exports():
    L = native.lib()
    for name in ("dsa_encode_attributes_batch", "dsa_encode_attributes_sequential_batch"):
        assert name in native.EXPORTS
        assert hasattr(L, name)
    assert L.dsa_abi_version() == 4
    text = open(os.path.join(ROOT, "include", "draco_mi355x.h")).read()
    assert "#define DSA_ABI_VERSION 4" in text and "#define DSA_UNIQUE_ID_DEFAULT 0xFFFFFFFFu" in text
    assert native.UNIQUE_ID_DEFAULT == 0xFFFFFFFF


@pytest.mark.parametrize("dtype,data_type", [(np.int8, 1), (np.uint8, 2), (np.int16, 3), (np.uint16, 4), (np.int32, 5), (np.uint32, 6), (np.float32, 9)])
def test_attribute_takes_its_type_from_the_array(dtype, data_type):
    a = dsa.Attribute(np.zeros((5, 3), dtype))
    assert a.data_type == data_type and a.values.shape == (5, 3) and a.values.dtype == dtype
    assert (a.attribute_type, a.normalized, a.unique_id, a.quantization_bits) == (4, False, None, 0)
    assert dsa.Attribute(np.zeros(5, dtype)).values.shape == (5, 1)


@pytest.mark.parametrize("dtype", [np.float64, np.int64, np.uint64, bool, np.float16])
def test_attribute_refuses_other_types(dtype):
    with pytest.raises(ValueError, match="dtype"):
        dsa.Attribute(np.zeros((5, 2), dtype))


def test_attribute_refuses_other_shapes():
    with pytest.raises(ValueError, match="components"):
        dsa.Attribute(np.zeros((5, 5), np.uint8))
    with pytest.raises(ValueError):
        dsa.Attribute(np.zeros((5, 2, 2), np.uint8))


def test_mesh_data_and_point_cloud_data_take_a_list():
    pos = np.zeros((4, 3), np.float32)
    faces = np.array([[0, 1, 2], [2, 1, 3]], np.uint32)
    m = dsa.MeshData(pos, faces, attributes=[np.zeros((4, 4), np.uint16), dsa.Attribute(np.zeros(4, np.float32), attribute_type=3, quantization_bits=12)])
    assert [a.data_type for a in m.attributes] == [4, 9] and m.attributes[1].quantization_bits == 12
    assert dsa.MeshData(pos, faces).attributes == [] and dsa.PointCloudData(pos).attributes == []
    with pytest.raises(ValueError, match="one row per vertex"):
        dsa.MeshData(pos, faces, attributes=[np.zeros(3, np.uint8)])
    with pytest.raises(ValueError, match="one row per vertex"):
        dsa.PointCloudData(pos, attributes=[np.zeros((5, 2), np.int16)])
    # generic= keeps casting to uint8
    assert dsa.MeshData(pos, faces, generic=np.arange(4, dtype=np.int32)).generic.dtype == np.uint8
