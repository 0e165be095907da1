"""The encoder's arena layout for attributes of the list given per corner (draco-sharp_amd/csrc/dsa_encode_layout.h: enc_take_extras
with a dsa_attribute_corners array, the id checks of enc_plan_mesh, enc_extra_caps over the rows the ids index, EncChunk::rows_of /
att_corners, enc_layout, and the weld view of enc_weld_check / enc_weld_view) compiled for the host under AddressSanitizer + UBSan
(tests/hostcheck/enclayoutlist_host.cpp) and run on the meshes of tests/cornerattrcases.py: float and integer attributes, fewer
rows than vertices, more, one per corner, more than 65 536 (the wide id form), beside per-vertex ones; per-point meshes whose weld
gives ids and whose weld gives none.  Every array handed in is a heap block of exactly the stated size, so a read past a row
count fails the run; the regions are held to the assertions of the layout host check.  A check of the product source on CPU, not a
CPU encode path."""
import os
import struct
import subprocess

import numpy as np
import pytest

import cornerattrcases as K
import draco_sharp_amd.synth as synth

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostcheck", "enclayoutlist_host.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("enclayoutlist") / "enclayoutlist_host")      # always rebuilt: the sources under test change
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=signed-integer-overflow",
                    "-fno-sanitize-recover=undefined", "-o", out, SRC], check=True)
    return out


def _extras(f, extras, nf):
    f.write(struct.pack("<I", len(extras)))
    for e in extras:
        f.write(struct.pack("<IIIII", e.attribute_type, e.data_type, e.num_components, int(e.corners is not None), len(e.values)))
        if e.corners is not None:
            assert e.corners.size == 3 * nf
            f.write(np.ascontiguousarray(e.corners, np.uint32).tobytes())
        f.write(np.ascontiguousarray(e.values).tobytes())


def run(exe, tmp_path, built, per_point):
    """built: cornerattrcases.Built with ids; per_point: [(pos, faces, [synth.Extra with one row per point])]"""
    path = tmp_path / "meshes.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(built) + len(per_point)))
        for b in built:
            f.write(struct.pack("<III", len(b.pos), len(b.faces), 0))
            f.write(np.ascontiguousarray(b.pos, np.float32).tobytes() + np.ascontiguousarray(b.faces, np.uint32).tobytes())
            f.write(struct.pack("<I", (1 if b.nid is not None else 0) | (2 if b.uid is not None else 0)))
            for rows, ids in ((b.nrm, b.nid), (b.uv, b.uid)):
                if ids is not None:
                    f.write(struct.pack("<I", len(rows)) + np.ascontiguousarray(ids, np.uint32).tobytes())
            _extras(f, b.extras, len(b.faces))
        for pos, faces, extras in per_point:
            f.write(struct.pack("<III", len(pos), len(faces), 1))
            f.write(np.ascontiguousarray(pos, np.float32).tobytes() + np.ascontiguousarray(faces, np.uint32).tobytes())
            f.write(struct.pack("<I", 0))
            _extras(f, extras, len(faces))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def per_point_of(b, seed):
    pos, faces, _, _, arrays = K.unweld(b._replace(nrm=None, nid=None, uv=None, uid=None), np.random.default_rng(seed))
    return pos, faces, K.point_extras(b, arrays)


NAMES = ["grid5x4/fid16-one-row", "grid6x5/fid32-none", "grid7x7/uv1-checker+colour-random", "grid16x9/fid32-stripes+vertex+uv1-island",
         "grid33x17/uv1-stripes+colour-checker+fid16-island+fid32-single", "grid33x17/uv1-corner", "grid33x17/no-ids", "grid4x3/colour-corner",
         "fan-closed/fid16-single", "components/colour-corner"]


def test_small_cases_and_weld_views(exe, tmp_path):
    built = [K.build(next(c for c in K.CASES if c.name == n)) for n in NAMES]
    # what the cases are taken for: float and integer attributes with ids; fewer rows than vertices, more, one per corner; and none
    with_ids = [(e, b) for b in built for e in b.extras if e.corners is not None]
    assert {e.values.dtype for e, _ in with_ids} >= {np.dtype(np.float32), np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.int32)}
    assert any(len(e.values) < len(b.pos) for e, b in with_ids) and any(len(b.pos) < len(e.values) < 3 * len(b.faces) for e, b in with_ids)
    assert any(len(e.values) == 3 * len(b.faces) for e, b in with_ids) and any(e.corners is None for b in built for e in b.extras)
    # (cuts that leave the positions a table the strict coder takes also with the attributes in the vertex key; the last two: no
    # attribute splits a vertex, so the weld gives no ids)
    per_point = [per_point_of(built[k], 40 + k) for k in (3, 8, 1, 6)]
    out = run(exe, tmp_path, built, per_point)
    # 16 settings x 2 chunks with ids; 2 x 2 weld views
    assert "enclayoutlist: %d chunks laid out" % (16 * 2 + 4) in out, out
    counts = dict(zip(("with", "without"), [int(x) for x in out.split("weld views with ids ")[1].replace(", without", "").split()]))
    assert counts["with"] == 2 * 2 and counts["without"] == 2 * 4 + 2 * 2, out      # weld_attributes 1: two meshes get ids; 0: none does


def test_more_than_65536_rows(exe, tmp_path):
    """One row per corner on 25 600 faces: 76 800 rows, the wide id form, beside a small mesh with the narrow one."""
    big = K.build(K.Case("grid129x101/fid16-corner+uv1-corner", lambda: synth.make_mesh(synth.GRID, 128, 100, 2), (None, None), [("fid16", "corner"), ("uv1", "corner")]))
    assert len(big.extras[0].values) == 76800 > 65536
    small = K.build(next(c for c in K.CASES if c.name == "grid7x7/uv1-checker+colour-random"))
    out = run(exe, tmp_path, [small, big, small], [])
    assert "enclayoutlist: %d chunks laid out" % (16 * 2) in out, out
