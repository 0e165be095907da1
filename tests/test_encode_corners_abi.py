"""dsa_mesh_corner_input / dsa_encode_batch_corners (attributes given per corner): the ctypes mirror against the header as a C
compiler lays it out, the export, and MeshData's checks of corner ids.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import draco_sharp_amd as dsa
from draco_sharp_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("mesh", "normal_corners", "texcoord_corners", "num_normals", "num_texcoords")


def test_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "draco_mi355x.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(dsa_mesh_corner_input));\n' +
                   "".join('  printf(" %%zu", offsetof(dsa_mesh_corner_input, %s));\n' % f for f in FIELDS) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(native.MeshCornerInput)] + [getattr(native.MeshCornerInput, f).offset for f in FIELDS]
    assert got == want
    if C.sizeof(C.c_void_p) == 8:
        assert got[0] == 80


def test_abi_version_and_export():
    L = native.lib()
    assert "dsa_encode_batch_corners" in native.EXPORTS
    assert hasattr(L, "dsa_encode_batch_corners")
    assert L.dsa_abi_version() == 4


def grid():
    pos = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    return pos, faces


def test_meshdata_accepts_corner_ids():
    pos, faces = grid()
    uv = np.zeros((6, 2), np.float32)
    m = dsa.MeshData(pos, faces, texcoords=uv, texcoord_corners=[[0, 1, 2], [3, 4, 5]])
    assert m.per_corner and m.texcoord_corners.dtype == np.uint32 and m.texcoord_corners.shape == (2, 3)
    assert m.normal_corners is None
    assert not dsa.MeshData(pos, faces, texcoords=np.zeros((4, 2), np.float32)).per_corner


@pytest.mark.parametrize("kw, match", [
    (dict(texcoord_corners=[[0, 1, 2], [0, 2, 3]]), "needs texcoords"),
    (dict(texcoords=np.zeros((4, 2)), texcoord_corners=[[0, 1, 2]]), "one id per face corner"),
    (dict(texcoords=np.zeros((4, 2)), texcoord_corners=[[0, 1, 2], [0, 2, 4]]), "out of range"),
    (dict(texcoords=np.zeros((4, 2)), texcoord_corners=[[0, 1, 2], [0, -2, 3]]), "not negative"),
    (dict(normals=np.zeros((4, 3)), normal_corners=[[0, 1, 2], [0, 2, 9]]), "out of range"),
    (dict(normals=np.zeros((4, 2)), normal_corners=[[0, 1, 2], [0, 2, 3]]), "3 components"),
])
def test_meshdata_rejects_bad_ids(kw, match):
    pos, faces = grid()
    with pytest.raises(ValueError, match=match):
        dsa.MeshData(pos, faces, **kw)
