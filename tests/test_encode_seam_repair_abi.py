"""dsa_encode_seam_repair_batch (attributes given per corner coded over a mesh whose topology needs the repair): the ctypes mirror
and the C# declaration of dsa_encode_seam_repair_options against the header as a C compiler lays it out, the defaults, the exports,
the ABI version, every option the call refuses before anything is touched, and how Config routes.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import draco_sharp_amd as dsa
from draco_sharp_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("grid", "corner_repair", "reserved")


def test_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    body = '  printf(" %zu", sizeof(dsa_encode_seam_repair_options));\n' + "".join('  printf(" %%zu", offsetof(dsa_encode_seam_repair_options, %s));\n' % f for f in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "draco_mi355x.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    mirror = native.EncodeSeamRepairOptions
    assert [n for n, _ in mirror._fields_] == list(FIELDS)
    assert got == [C.sizeof(mirror)] + [getattr(mirror, f).offset for f in FIELDS]
    assert C.sizeof(mirror) == C.sizeof(native.EncodeGridOptions) + 32


def test_abi_version_and_exports():
    L = native.lib()
    for name in ("dsa_encode_default_seam_repair_options", "dsa_encode_seam_repair_batch"):
        assert name in native.EXPORTS
        assert hasattr(L, name)
    assert L.dsa_abi_version() == 4


def options(**kw):
    o = native.EncodeSeamRepairOptions()
    native.lib().dsa_encode_default_seam_repair_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_default_options_are_those_of_the_grid_call():
    L = native.lib()
    so, go = native.EncodeSeamRepairOptions(), native.EncodeGridOptions()
    C.memset(C.byref(so), 0xFF, C.sizeof(so))
    L.dsa_encode_default_seam_repair_options(C.byref(so))
    L.dsa_encode_default_grid_options(C.byref(go))
    assert bytes(so.grid) == bytes(go) and so.corner_repair == 0 and list(so.reserved) == [0] * 7
    L.dsa_encode_default_seam_repair_options(None)


def test_every_invalid_option_fails_the_call():
    """The options are checked before anything else is touched: no context, no meshes."""
    L = native.lib()
    h = C.c_void_p()

    def refused(o, field):
        assert L.dsa_encode_seam_repair_batch(None, 0, None, None, C.byref(o), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT, field
    for value in (2, -1, 7):
        refused(options(corner_repair=value), "corner_repair")
    for k in range(7):
        o = options()
        o.reserved[k] = 1
        refused(o, "reserved")
    o = options(corner_repair=1)                 # topology 0 (the default): corner_repair needs the repaired table
    assert o.grid.repair.topology == 0
    refused(o, "topology")
    o = options(corner_repair=1)
    o.grid.repair.topology = 2
    refused(o, "topology")
    # what the sibling calls refuse, through this one
    o = options()
    o.grid.weld_points = 2
    refused(o, "weld_points")
    o = options()
    o.grid.reserved[6] = 1
    refused(o, "reserved")
    o = options()
    o.grid.repair.reserved[0] = 1
    refused(o, "reserved")
    assert L.dsa_encode_seam_repair_batch(None, 0, None, None, C.byref(options()), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT      # no context
    assert L.dsa_encode_seam_repair_batch(None, 0, None, None, None, C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT


def test_csharp_declarations_agree_with_the_header():
    cs = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "NativeMethods.cs")).read()
    m = re.search(r"struct DsaEncodeSeamRepairOptions\s*\{(.*?)\n\}", cs, re.S)
    assert m, "DsaEncodeSeamRepairOptions is not declared"
    fields = [" ".join(f.split()) for f in re.sub(r"//[^\n]*", "", m.group(1)).split(";") if f.strip()]
    assert fields == ["public DsaEncodeGridOptions Grid", "public int CornerRepair", "public fixed int Reserved[7]"]
    for name in ("dsa_encode_default_seam_repair_options(out DsaEncodeSeamRepairOptions options)",
                 "dsa_encode_seam_repair_batch(IntPtr ctx, uint n, DsaMeshAttrInput* meshes, DsaMeshGrids* grids, in DsaEncodeSeamRepairOptions options, out IntPtr encoded)"):
        assert name in cs
    header = open(os.path.join(ROOT, "include", "draco_mi355x.h")).read()
    h = re.search(r"typedef struct dsa_encode_seam_repair_options \{(.*?)\} dsa_encode_seam_repair_options;", header, re.S)
    assert h and [" ".join(f.split()) for f in re.sub(r"/\*.*?\*/", "", h.group(1), flags=re.S).split(";") if f.strip()] == \
        ["dsa_encode_grid_options grid", "int32_t corner_repair", "int32_t reserved[7]"]
    enc = open(os.path.join(ROOT, "draco-sharp_amd", "csharp", "GpuDracoEncoder.cs")).read()
    for word in ("public bool RepairSeams", "dsa_encode_seam_repair_batch", "CornerRepair = 1"):
        assert word in enc


def test_config_switch():
    assert dsa.Config().repair_seams is False
    assert dsa.Config(repair_topology=True).repair_seams is False
    assert dsa.Config(repair_topology=True, repair_seams=True).repair_seams is True
    with pytest.raises(ValueError, match="repair_topology"):
        dsa.Config(repair_seams=True)
    with pytest.raises(ValueError):
        dsa.Config(repair_topology=True, repair_seams=True, encoding_method=0)      # (a sequential stream takes no repair at all)


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


def _mesh(corners=False):
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)
    faces = np.array([[0, 1, 2], [2, 1, 3]], np.uint32)
    uv = np.zeros((6, 2), np.float32)
    if corners:
        return dsa.MeshData(pos, faces, texcoords=uv, texcoord_corners=np.arange(6).reshape(2, 3))
    return dsa.MeshData(pos, faces, texcoords=uv[:4])


def test_encode_batch_takes_the_new_entry_point_only_when_asked(recorder):
    """EncodeBatch reaches every Edgebreaker batch through dsa_encode_seam_repair_batch: what is asked for is what the options
    say, and nothing that is not asked for is switched on."""
    r, ctx = recorder
    enc = dsa.DracoEncoder(ctx)

    def the_call():
        assert [c[0] for c in r.calls] == ["dsa_encode_seam_repair_batch"]
        _, n, _, grids, opt, _ = r.calls[0][1]
        o = opt._obj
        assert n == 1 and list(o.reserved) == [0] * 7 and list(o.grid.reserved) == [0] * 7 and list(o.grid.repair.reserved) == [0] * 7
        return grids, o
    for weld in (False, True):
        for corners in ((False, True) if not weld else (False,)):
            # without the switch: the request of dsa_encode_repair_batch / dsa_encode_points_batch
            del r.calls[:]
            enc.EncodeBatch([_mesh(corners)], dsa.Config(repair_topology=True, weld_points=weld), handle=True)
            grids, o = the_call()
            assert grids is None and o.corner_repair == 0 and o.grid.repair.topology == 1 and o.grid.weld_points == (1 if weld else 0)
            # the new switch
            del r.calls[:]
            enc.EncodeBatch([_mesh(corners)], dsa.Config(repair_topology=True, weld_points=weld, repair_seams=True), handle=True)
            grids, o = the_call()
            assert grids is None and o.corner_repair == 1 and o.grid.repair.topology == 1 and o.grid.weld_points == (1 if weld else 0)
    # a grid rides along
    del r.calls[:]
    m = _mesh(True)
    m.position_grid = dsa.Grid([0, 0, 0], 2.0)
    enc.EncodeBatch([m], dsa.Config(repair_topology=True, repair_seams=True), handle=True)
    grids, o = the_call()
    assert grids is not None and o.corner_repair == 1
    del r.calls[:]
    enc.EncodeBatch([m], dsa.Config(repair_topology=True), handle=True)
    grids, o = the_call()
    assert grids is not None and o.corner_repair == 0 and o.grid.repair.topology == 1      # (the request of dsa_encode_grid_batch)
    # nothing set: every added field at its default, the request of the per-vertex call as ever
    del r.calls[:]
    enc.EncodeBatch([_mesh()], dsa.Config(), handle=True)
    grids, o = the_call()
    assert grids is None and (o.corner_repair, o.grid.weld_points, o.grid.repair.topology) == (0, 0, 0)
    lv = o.grid.repair.level
    assert (lv.multi_parallelogram, lv.traversal_method, lv.ex.edgebreaker_method, lv.ex.normal_prediction) == (0, 0, 0, 0)
