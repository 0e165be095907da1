"""dsa_encode_level_options / dsa_encode_level_batch (MultiParallelogram, ConstrainedMultiParallelogram, prediction-degree order):
the ctypes mirror against the header as a C compiler lays it out, the exports, the ABI version, the defaults, and Config's checks of
the two options.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import draco_sharp_amd as dsa
from draco_sharp_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("ex", "multi_parallelogram", "traversal_method", "reserved")


def test_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "draco_mi355x.h"\nint main(void) {\n'
                   '  printf("%zu %zu", sizeof(dsa_encode_level_options), sizeof(dsa_encode_options_ex));\n' +
                   "".join('  printf(" %%zu", offsetof(dsa_encode_level_options, %s));\n' % f for f in FIELDS) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(native.EncodeLevelOptions), C.sizeof(native.EncodeOptionsEx)] + [getattr(native.EncodeLevelOptions, f).offset for f in FIELDS]
    assert got == want
    assert got[0] == 64 + 32 == 96 and got[1] == 64


def test_abi_version_and_exports():
    L = native.lib()
    for name in ("dsa_encode_level_batch", "dsa_encode_default_level_options"):
        assert name in native.EXPORTS
        assert hasattr(L, name)
    assert L.dsa_abi_version() == 4


def test_default_level_options():
    o = native.EncodeLevelOptions()
    o.multi_parallelogram, o.traversal_method, o.reserved[0], o.reserved[5], o.ex.reserved[1], o.ex.edgebreaker_method = 7, 7, 7, 7, 7, 7
    native.lib().dsa_encode_default_level_options(C.byref(o))
    d = native.EncodeOptionsEx()
    native.lib().dsa_encode_default_options_ex(C.byref(d))
    assert bytes(o.ex) == bytes(d)
    assert o.multi_parallelogram == 0 and o.traversal_method == 0 and list(o.reserved) == [0] * 6


@pytest.mark.parametrize("mp", [0, 2, 4, -1])
@pytest.mark.parametrize("tm", [0, 1, 2])
def test_config_accepts_the_levels(mp, tm):
    cfg = dsa.Config(multi_parallelogram=mp, traversal_method=tm, speed=1)
    assert cfg.leveled == (mp != 0 or tm != 0)
    o = cfg._native_level()
    assert (o.multi_parallelogram, o.traversal_method, o.ex.base.compression_level) == (mp, tm, 9)
    assert bytes(o.ex) == bytes(cfg._native_ex())


@pytest.mark.parametrize("kw", [dict(multi_parallelogram=1), dict(multi_parallelogram=3), dict(multi_parallelogram=-2), dict(multi_parallelogram=5),
                                dict(traversal_method=3), dict(traversal_method=-1)])
def test_config_rejects_other_values(kw):
    with pytest.raises(ValueError, match=list(kw)[0]):
        dsa.Config(**kw)


def test_the_method_ids_underneath_stay():
    with pytest.raises(ValueError, match="position_prediction"):
        dsa.Config(position_prediction=4)
    with pytest.raises(ValueError, match="position_prediction"):
        dsa.Config(position_prediction=2, multi_parallelogram=4)
    assert not dsa.Config().leveled


@pytest.mark.parametrize("kw", [dict(multi_parallelogram=4), dict(traversal_method=1), dict(multi_parallelogram=-1, traversal_method=2)])
def test_sequential_configs_and_point_clouds_refuse_the_levels(kw):
    with pytest.raises(ValueError, match="sequential"):
        dsa.Config(encoding_method=0, **kw)
    with pytest.raises(ValueError, match="sequential"):
        dsa.Config(encoding_method=-1, speed=10, **kw)
    cloud = dsa.PointCloudData(np.zeros((5, 3), np.float32))
    with pytest.raises(ValueError, match="point clouds"):
        dsa.DracoEncoder(context=object()).EncodeBatch([cloud], dsa.Config(**kw))       # (refused before the context is touched)
