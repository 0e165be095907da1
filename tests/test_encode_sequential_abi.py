"""dsa_encode_sequential_options / dsa_encode_sequential_batch (sequential meshes and point clouds): the ctypes mirror against
the header as a C compiler lays it out, the exports, the ABI version, the defaults, Config's encoding_method and the rules of
EncodeBatch about what a batch may mix.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import draco_sharp_amd as dsa
from draco_sharp_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("base", "geometry", "compress_connectivity", "reserved")


def test_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "draco_mi355x.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(dsa_encode_sequential_options));\n' +
                   "".join('  printf(" %%zu", offsetof(dsa_encode_sequential_options, %s));\n' % f for f in FIELDS) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(native.EncodeSequentialOptions)] + [getattr(native.EncodeSequentialOptions, f).offset for f in FIELDS]
    assert got == want
    assert got == [64, 0, 32, 36, 40]


def test_abi_version_and_exports():
    L = native.lib()
    for name in ("dsa_encode_sequential_batch", "dsa_encode_sequential_default_options"):
        assert name in native.EXPORTS
        assert hasattr(L, name)
    assert L.dsa_abi_version() == 4


def test_default_options():
    o = native.EncodeSequentialOptions()
    o.geometry, o.compress_connectivity, o.reserved[0], o.reserved[5] = 7, 7, 7, 7
    native.lib().dsa_encode_sequential_default_options(C.byref(o))
    d = native.EncodeOptions()
    native.lib().dsa_encode_default_options(C.byref(d))
    assert bytes(o.base) == bytes(d)
    assert o.geometry == 1 and o.compress_connectivity == 0 and list(o.reserved) == [0] * 6


@pytest.mark.parametrize("method", [1, 0, -1])
def test_config_accepts_the_encoding_methods(method):
    assert dsa.Config(encoding_method=method).encoding_method == method


@pytest.mark.parametrize("method", [2, -2, 10, None, "sequential"])
def test_config_refuses_other_encoding_methods(method):
    with pytest.raises(ValueError, match="encoding_method"):
        dsa.Config(encoding_method=method)


def test_config_resolves_the_method():
    assert not dsa.Config().sequential and dsa.Config().encoding_method == 1
    assert not dsa.Config(speed=10).sequential                     # the default stays Edgebreaker whatever the speed
    assert dsa.Config(encoding_method=0).sequential and dsa.Config(encoding_method=0, speed=3).sequential
    assert dsa.Config(encoding_method=-1, speed=10).sequential     # DracoEncoder.cs:43-57: sequential exactly at speed 10
    assert not dsa.Config(encoding_method=-1, speed=9).sequential
    assert not dsa.Config(encoding_method=1, compress_connectivity=True).sequential


def test_config_fills_the_native_options():
    o = dsa.Config(encoding_method=0, compress_connectivity=True, position_bits=14, speed=2, symbol_scheme=0)._native_sequential(1)
    assert (o.geometry, o.compress_connectivity, o.base.position_bits, o.base.compression_level, o.base.symbol_scheme) == (1, 1, 14, 8, 0)
    assert list(o.reserved) == [0] * 6
    o = dsa.Config(encoding_method=0, compress_connectivity=True)._native_sequential(0)
    assert (o.geometry, o.compress_connectivity) == (0, 0)         # a point cloud has no connectivity to compress
    assert dsa.Config(encoding_method=0)._native_sequential(1).compress_connectivity == 0


def _mesh(**kw):
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)
    return dsa.MeshData(pos, np.array([[0, 1, 2], [2, 1, 3]], np.uint32), **kw)


def test_point_cloud_data_checks_its_rows():
    pos = np.zeros((5, 3), np.float32)
    pc = dsa.PointCloudData(pos, normals=np.ones((5, 3)), texcoords=np.zeros((5, 2)), generic=np.zeros(5, np.uint8))
    assert len(pc.faces) == 0 and pc.generic.shape == (5, 1)
    with pytest.raises(ValueError, match="normals"):
        dsa.PointCloudData(pos, normals=np.ones((4, 3)))
    with pytest.raises(ValueError, match="texcoords"):
        dsa.PointCloudData(pos, texcoords=np.ones((5, 3)))
    with pytest.raises(ValueError, match="generic"):
        dsa.PointCloudData(pos, generic=np.zeros((5, 5), np.uint8))


def test_encode_batch_refuses_meshes_beside_point_clouds():
    pc = dsa.PointCloudData(np.zeros((3, 3), np.float32))
    for cfg in (None, dsa.Config(encoding_method=0)):
        with pytest.raises(ValueError, match="meshes or point clouds"):
            dsa.DracoEncoder().EncodeBatch([_mesh(), pc], cfg)


@pytest.mark.parametrize("cfg", [dict(encoding_method=0), dict(encoding_method=-1, speed=10)])
def test_encode_batch_refuses_corner_ids_with_a_sequential_config(cfg):
    uv = np.zeros((6, 2), np.float32)
    m = _mesh(texcoords=uv, texcoord_corners=np.arange(6, dtype=np.uint32).reshape(2, 3))
    with pytest.raises(ValueError, match="per corner"):
        dsa.DracoEncoder().EncodeBatch([_mesh(), m], dsa.Config(**cfg))
