"""dsa_encode_rows_batch (track_rows: which row of the caller's arrays every entry of a stream carries) and
dsa_encoded_entry_rows: the ctypes mirror of the options against the header as a C compiler lays it out, the defaults, the
exports, the ABI version, every option the call refuses before anything is touched, and how Config routes.  No GPU needed (the
texts of the refusals need a context: tests/test_gpu_source_rows.py reads them)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import draco_sharp_amd as dsa
from draco_sharp_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("corner_attributes", "track_rows", "reserved")


def test_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    body = '  printf(" %zu", sizeof(dsa_encode_rows_options));\n' + "".join('  printf(" %%zu", offsetof(dsa_encode_rows_options, %s));\n' % f for f in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "draco_mi355x.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    mirror = native.EncodeRowsOptions
    assert [n for n, _ in mirror._fields_] == list(FIELDS)
    assert got == [C.sizeof(mirror)] + [getattr(mirror, f).offset for f in FIELDS]
    assert C.sizeof(mirror) == C.sizeof(native.EncodeCornerAttributesOptions) + 32
    header = open(os.path.join(ROOT, "include", "draco_mi355x.h")).read()
    h = re.search(r"typedef struct dsa_encode_rows_options \{(.*?)\} dsa_encode_rows_options;", header, re.S)
    assert h and [" ".join(f.split()) for f in re.sub(r"/\*.*?\*/", "", h.group(1), flags=re.S).split(";") if f.strip()] == [
        "dsa_encode_corner_attributes_options corner_attributes", "int32_t track_rows", "int32_t reserved[7]"]


def test_abi_version_and_exports():
    L = native.lib()
    for name in ("dsa_encode_default_rows_options", "dsa_encode_rows_batch", "dsa_encoded_entry_rows", "dsa_encoded_attributes"):
        assert name in native.EXPORTS
        assert hasattr(L, name)
    assert L.dsa_abi_version() == 4


def options(**kw):
    o = native.EncodeRowsOptions()
    native.lib().dsa_encode_default_rows_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_default_options_are_those_of_the_corner_attributes_call():
    L = native.lib()
    ro, co = native.EncodeRowsOptions(), native.EncodeCornerAttributesOptions()
    C.memset(C.byref(ro), 0xFF, C.sizeof(ro))
    L.dsa_encode_default_rows_options(C.byref(ro))
    L.dsa_encode_default_corner_attributes_options(C.byref(co))
    assert bytes(ro.corner_attributes) == bytes(co) and ro.track_rows == 0 and list(ro.reserved) == [0] * 7
    L.dsa_encode_default_rows_options(None)


def test_every_invalid_option_fails_the_call():
    """The options are checked before anything else is touched: no context, no meshes."""
    L = native.lib()
    h = C.c_void_p()

    def refused(o, field):
        assert L.dsa_encode_rows_batch(None, 0, None, None, None, C.byref(o), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT, field
    for value in (2, -1, 7):
        refused(options(track_rows=value), "track_rows")
    for k in range(7):
        o = options(track_rows=1)
        o.reserved[k] = 1
        refused(o, "reserved")
    # what the calls below refuse, through this one
    o = options()
    o.corner_attributes.weld_attributes = 1          # (weld_points 0)
    refused(o, "weld_points")
    o = options()
    o.corner_attributes.reserved[6] = 1
    refused(o, "reserved")
    o = options()
    o.corner_attributes.seam_repair.corner_repair = 1      # (topology 0)
    refused(o, "topology")
    o = options()
    o.corner_attributes.seam_repair.grid.repair.level.traversal_method = 3
    refused(o, "traversal_method")
    assert L.dsa_encode_rows_batch(None, 0, None, None, None, C.byref(options()), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT      # no context
    assert L.dsa_encode_rows_batch(None, 0, None, None, None, None, C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT
    count = C.c_uint32()
    assert L.dsa_encoded_entry_rows(None, 0, 0, None, 0, C.byref(count)) == native.DSA_ERR_INVALID_ARGUMENT
    assert L.dsa_encoded_attributes(None, 0, C.byref(count)) == native.DSA_ERR_INVALID_ARGUMENT


def test_config_switch():
    assert dsa.Config().track_rows is False
    assert dsa.Config(track_rows=1).track_rows is True
    assert dsa.Config(track_rows=True, weld_points=True, weld_attributes=True, repair_topology=True, repair_seams=True).track_rows is True
    assert dsa.Config(track_rows=True, encoding_method=0).sequential          # (a sequential stream answers with the identity: nothing to refuse)


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


def test_encode_batch_takes_the_new_entry_point_only_when_asked(monkeypatch):
    r = _Recorder(native.lib())
    monkeypatch.setattr(native, "lib", lambda: r)

    class Ctx:
        _h = None
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)
    mesh = dsa.MeshData(pos, np.array([[0, 1, 2], [2, 1, 3]], np.uint32))
    enc = dsa.DracoEncoder(Ctx())
    enc.EncodeBatch([mesh], dsa.Config(), handle=True)
    enc.EncodeBatch([mesh], dsa.Config(weld_points=True, weld_attributes=True), handle=True)
    enc.EncodeBatch([mesh], dsa.Config(track_rows=True, encoding_method=0), handle=True)
    assert [c[0] for c in r.calls] == ["dsa_encode_seam_repair_batch", "dsa_encode_corner_attributes_batch", "dsa_encode_grid_sequential_batch"]
    del r.calls[:]
    enc.EncodeBatch([mesh], dsa.Config(track_rows=True, weld_points=True, weld_attributes=True, repair_topology=True, traversal_method=2), handle=True)
    assert [c[0] for c in r.calls] == ["dsa_encode_rows_batch"]
    _, n, _, grids, corners, opt, _ = r.calls[0][1]
    o = opt._obj
    assert n == 1 and grids is None and o.track_rows == 1 and list(o.reserved) == [0] * 7
    assert o.corner_attributes.weld_attributes == 1 and o.corner_attributes.seam_repair.grid.weld_points == 1
    assert o.corner_attributes.seam_repair.grid.repair.topology == 1 and o.corner_attributes.seam_repair.grid.repair.level.traversal_method == 2
    assert not corners[0].attributes
