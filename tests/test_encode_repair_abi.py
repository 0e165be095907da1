"""dsa_encode_repair_options / dsa_encode_repair_batch (the reference's corner table for meshes that are not clean): the ctypes
mirror and the C# declaration against the header as a C compiler lays it out, the exports, the ABI version, the defaults, the
argument failures that need no device, and Config's handling of the option.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import draco_sharp_amd as dsa
import draco_sharp_amd.synth as synth
from draco_sharp_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("level", "topology", "reserved")


def test_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "draco_mi355x.h"\nint main(void) {\n'
                   '  printf("%zu %zu", sizeof(dsa_encode_repair_options), sizeof(dsa_encode_level_options));\n' +
                   "".join('  printf(" %%zu", offsetof(dsa_encode_repair_options, %s));\n' % f for f in FIELDS) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(native.EncodeRepairOptions), C.sizeof(native.EncodeLevelOptions)] + [getattr(native.EncodeRepairOptions, f).offset for f in FIELDS]
    assert got == want
    assert got[0] == 96 + 4 + 28 == 128 and got[1] == 96


def test_abi_version_and_exports():
    L = native.lib()
    for name in ("dsa_encode_repair_batch", "dsa_encode_default_repair_options"):
        assert name in native.EXPORTS
        assert hasattr(L, name)
    assert L.dsa_abi_version() == 4


def test_default_repair_options():
    o = native.EncodeRepairOptions()
    o.topology, o.reserved[0], o.reserved[6], o.level.reserved[1], o.level.multi_parallelogram, o.level.ex.edgebreaker_method = 7, 7, 7, 7, 7, 7
    native.lib().dsa_encode_default_repair_options(C.byref(o))
    d = native.EncodeLevelOptions()
    native.lib().dsa_encode_default_level_options(C.byref(d))
    assert bytes(o.level) == bytes(d)
    assert o.topology == 0 and list(o.reserved) == [0] * 7


def test_argument_failures_that_need_no_device():
    """The options are checked before anything else is touched: topology outside {0, 1} and a non-zero reserved word fail the call."""
    L = native.lib()
    h = C.c_void_p()
    for field, value in (("topology", 2), ("topology", -1)):
        o = native.EncodeRepairOptions()
        L.dsa_encode_default_repair_options(C.byref(o))
        setattr(o, field, value)
        assert L.dsa_encode_repair_batch(None, 0, None, C.byref(o), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT
    for k in range(7):
        o = native.EncodeRepairOptions()
        L.dsa_encode_default_repair_options(C.byref(o))
        o.reserved[k] = 1
        assert L.dsa_encode_repair_batch(None, 0, None, C.byref(o), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT
    o = native.EncodeRepairOptions()
    L.dsa_encode_default_repair_options(C.byref(o))
    assert L.dsa_encode_repair_batch(None, 0, None, C.byref(o), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT      # no context


def test_csharp_declaration_agrees_with_the_header():
    cs = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "NativeMethods.cs")).read()
    m = re.search(r"struct DsaEncodeRepairOptions\s*\{(.*?)\n\}", cs, re.S)
    assert m, "DsaEncodeRepairOptions is not declared"
    body = re.sub(r"//[^\n]*", "", m.group(1))
    fields = [" ".join(f.split()) for f in body.split(";") if f.strip()]
    assert fields == ["public DsaEncodeLevelOptions Level", "public int Topology", "public fixed int Reserved[7]"]
    hdr = open(os.path.join(ROOT, "include", "draco_mi355x.h")).read()
    m = re.search(r"typedef struct dsa_encode_repair_options \{(.*?)\} dsa_encode_repair_options;", hdr, re.S)
    c_fields = [" ".join(f.split()) for f in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";") if f.strip()]
    assert c_fields == ["dsa_encode_level_options level", "int32_t topology", "int32_t reserved[7]"]
    assert [n for n, _ in native.EncodeRepairOptions._fields_] == ["level", "topology", "reserved"]
    for name in ("dsa_encode_default_repair_options(out DsaEncodeRepairOptions options)",
                 "dsa_encode_repair_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, in DsaEncodeRepairOptions options, out IntPtr encoded)"):
        assert name in cs
    enc = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "GpuDracoEncoder.cs")).read()
    assert "public bool RepairTopology" in enc and "dsa_encode_repair_batch(_ctx" in enc


def test_config_carries_the_option():
    assert dsa.Config().repair_topology is False
    cfg = dsa.Config(repair_topology=True, multi_parallelogram=4, traversal_method=1, speed=3)
    o = cfg._native_repair()
    assert o.topology == 1 and list(o.reserved) == [0] * 7
    assert bytes(o.level) == bytes(cfg._native_level())
    assert dsa.Config(multi_parallelogram=2)._native_repair().topology == 0
    with pytest.raises(ValueError, match="repair_topology"):
        dsa.Config(repair_topology=True, encoding_method=0)


def test_synth_options_mirror_the_host_coder():
    o = synth.options()
    assert o.repair_topology == 0 and synth.Options._fields_[-1][0] == "repair_topology"      # appended last, off by default
    assert synth.options(repair_topology=1).repair_topology == 1
    pos = np.random.default_rng(0).random((3, 3)).astype(np.float32)
    twice = np.array([[0, 1, 2], [0, 1, 2]], np.uint32)
    with pytest.raises(RuntimeError, match="non-manifold edge"):
        synth.encode_mesh(pos, twice)
    assert synth.encode_mesh(pos, twice, opt=synth.options(repair_topology=1))[:5] == b"DRACO"
