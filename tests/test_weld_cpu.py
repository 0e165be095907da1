"""The weld of per-point input by the CPU coder (synth.weld_points, dsa_encode_host.h weld_points -- the specification the device
kernels are held against): equal to the numpy pin of tests/weldcases.py on every case, array for array; the streams of
synth.encode_mesh_points decode (independent oracle) to the face multiset of quantised corner values computed straight from the
per-point input, so the weld lost and moved nothing; a two-sided sheet is refused strict and coded on the repaired table when its
attributes collapse to one row per vertex."""
import numpy as np
import pytest

import draco_sharp_amd.synth as synth
import meshutil
import oracle
import weldcases

CASES = weldcases.cases()


def weld(c):
    return synth.weld_points(c.pos, c.faces, c.normals, c.uvs, c.generic, weldcases.extras_of(c))


def encode(c, **opt):
    return synth.encode_mesh_points(c.pos, c.faces, c.normals, c.uvs, c.generic, weldcases.extras_of(c), synth.options(**opt) if opt else None)


def test_the_weld_equals_the_pin():
    for c in CASES:
        if c.refused == "face index out of range":
            with pytest.raises(RuntimeError, match="face index out of range"):
                weld(c)
            continue
        assert weldcases.same_welded(weld(c), weldcases.pin(c.pos, c.faces, c.normals, c.uvs, c.generic, c.extra)) is None, c.name


def test_the_cases_weld_to_what_they_say():
    by = {c.name: c for c in CASES}
    w = weld(by["all-equal"])
    assert (w.num_vertices, w.num_normals, w.num_texcoords) == (1, 1, 1)
    w = weld(by["40000-points-2-positions"])
    assert w.num_vertices == 2 and w.vertex_point.tolist() == [0, 1]
    assert weld(by["40000-distinct"]).num_vertices == 40000
    for name in ("differ-in-z", "differ-in-last-bit", "differ-in-sign-of-zero"):
        assert weld(by[name]).num_vertices == 4, name
    w = weld(by["nan-rows"])
    assert w.num_vertices == 5 and w.vertex_of_point[0] == w.vertex_of_point[3] != w.vertex_of_point[6]
    w = weld(by["unused-points"])
    assert (w.vertex_of_point[[0, 1, 12, 13, 14]] == weldcases.INVALID).all() and (w.vertex_of_point[-2:] == weldcases.INVALID).all() and w.vertex_point[0] == 2
    c = by["colours-split"]
    assert weld(c).num_vertices > synth.weld_points(c.pos, c.faces, c.normals, c.uvs).num_vertices
    for P in (65535, 65536, 65537):
        assert weld(by["P=%d" % P]).num_points == P
    w = weld(by["no-faces"])
    assert w.num_vertices == 0 and (w.vertex_of_point == weldcases.INVALID).all()


def test_the_seamed_topologies_weld_back_to_manifolds_and_smaller_streams():
    """The 35 inputs of the 12 x 9 topologies: coded, and never larger than the same points given as they are (where those encode)."""
    for c in CASES[:35]:
        welded = encode(c)
        try:
            torn = synth.encode_mesh(c.pos, c.faces, c.normals, c.uvs)
        except RuntimeError:
            continue
        assert len(welded) <= len(torn), c.name


def test_streams_decode_to_the_source_corner_values():
    for c in CASES:
        if c.weld_only or c.generic is not None or c.extra:
            continue
        if c.refused:
            with pytest.raises(RuntimeError) as e:
                encode(c)
            assert str(e.value) == c.refused, c.name
            continue
        ref = oracle.decode(encode(c))
        want, _ = meshutil.source_corner_faces(c.pos, c.normals, c.uvs, c.faces)
        got = meshutil.face_multiset_fast(ref.faces, meshutil.decoded_point_keys(ref))
        assert got.shape == want.shape and (got == want).all(), c.name


def test_attributes_that_split_vertices_are_coded_per_vertex():
    for name in ("colours-split", "generic-splits"):
        c = next(x for x in CASES if x.name == name)
        w = weld(c)
        data = encode(c)
        assert data == synth.encode_mesh_corners(w.pos, w.faces, w.normals, w.normal_corners, w.uvs, w.uv_corners, generic=w.generic,
                                                 extra=[synth.Extra(e, attribute_type=2, normalized=True) for e in w.extra]), name
        ref = oracle.decode(data)
        assert ref.num_points >= w.num_vertices and len(ref.faces) == len(c.faces)


def test_a_two_sided_sheet():
    sheet = next(c for c in CASES if c.name == "two-sided-sheet")
    w = weld(sheet)
    assert w.normals_per_vertex and w.texcoords_per_vertex and w.normal_corners is None and w.num_vertices * 2 == len(sheet.pos)
    with pytest.raises(RuntimeError, match="non-manifold edge"):
        encode(sheet)
    ref = oracle.decode(encode(sheet, repair_topology=1))
    assert len(ref.faces) == len(sheet.faces)
    two = next(c for c in CASES if c.name == "two-sided-sheet-two-normals")
    assert not weld(two).normals_per_vertex
    with pytest.raises(RuntimeError):          # seams over a table that needs repair are not written
        encode(two, repair_topology=1)
