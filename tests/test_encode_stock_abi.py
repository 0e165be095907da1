"""dsa_encode_options_ex / dsa_encode_batch_ex (valence Edgebreaker, TexCoordsPortable, GeometricNormal): the ctypes mirror
against the header as a C compiler lays it out, the exports, the ABI version, and Config's checks of the method ids.  No GPU
needed."""
import ctypes as C
import os
import subprocess

import pytest

import draco_sharp_amd as dsa
from draco_sharp_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("base", "edgebreaker_method", "normal_prediction", "reserved")


def test_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "draco_mi355x.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(dsa_encode_options_ex));\n' +
                   "".join('  printf(" %%zu", offsetof(dsa_encode_options_ex, %s));\n' % f for f in FIELDS) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(native.EncodeOptionsEx)] + [getattr(native.EncodeOptionsEx, f).offset for f in FIELDS]
    assert got == want
    assert got[0] == 64


def test_abi_version_and_exports():
    L = native.lib()
    for name in ("dsa_encode_batch_ex", "dsa_encode_default_options_ex"):
        assert name in native.EXPORTS
        assert hasattr(L, name)
    assert L.dsa_abi_version() == 4


def test_default_options_ex():
    o = native.EncodeOptionsEx()
    o.edgebreaker_method, o.normal_prediction, o.reserved[5] = 7, 7, 7
    native.lib().dsa_encode_default_options_ex(C.byref(o))
    d = native.EncodeOptions()
    native.lib().dsa_encode_default_options(C.byref(d))
    assert bytes(o.base) == bytes(d)
    assert o.edgebreaker_method == 0 and o.normal_prediction == 0 and list(o.reserved) == [0] * 6


@pytest.mark.parametrize("kw", [dict(edgebreaker_method=1), dict(edgebreaker_method=3), dict(edgebreaker_method=-2),
                                dict(normal_prediction=1), dict(normal_prediction=5), dict(texcoord_prediction=4),
                                dict(texcoord_prediction=6), dict(position_prediction=4), dict(position_prediction=5)])
def test_config_rejects_methods_the_encoder_cannot_write(kw):
    with pytest.raises(ValueError, match=list(kw)[0]):
        dsa.Config(**kw)


def test_config_accepts_the_stock_methods():
    cfg = dsa.Config(edgebreaker_method=2, texcoord_prediction=5, normal_prediction=6)
    assert cfg.extended
    o = cfg._native_ex()
    assert (o.edgebreaker_method, o.normal_prediction, o.base.texcoord_prediction) == (2, 6, 5)
    assert dsa.Config(edgebreaker_method=-1, speed=3)._native_ex().base.compression_level == 7
    assert not dsa.Config(texcoord_prediction=5).extended          # the standard entry points write it too
    assert not dsa.Config().extended
