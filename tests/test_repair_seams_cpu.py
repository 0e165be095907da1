"""The CPU coder with repair_topology = 2 (dsa_encode_host.h plan_mesh: as 1, and attributes given per corner are coded over the
repaired table -- the ids of the faces that are not degenerate, AttrConn / the attribute walks / the seam bits over
CornerTable::from_repaired), decoded through the oracle against the pin of tests/seamdefects.py, which is written from the contract
and not from the coder.  This is the coder the device encoder is held against (tests/test_gpu_encode_repair_seams.py).
No GPU needed."""
import numpy as np
import pytest

import defects
import oracle
import seamdefects as sd
import weldcases
import draco_sharp_amd.synth as synth

SMALL = defects.named() + defects.placed()
SOURCES = (("grid", synth.GRID, 6, 5), ("torus", synth.TORUS, 9, 8), ("holes", synth.HOLES, 14, 12))


def coded_points(m):
    """V' - isolated of the mesh's position table: what the coder without corner attributes (repair_topology = 1, held against hand
    counts by tests/test_repair_cpu.py) writes into its header for the same faces."""
    return sd.header_counts(synth.encode_mesh(m.pos, m.faces, opt=synth.options(repair_topology=1)))[0]


@pytest.mark.parametrize("c", SMALL, ids=lambda c: c.name)
def test_named_and_placed_cases_with_ids_of_three_kinds(c):
    for j, kind in enumerate(sd.ID_KINDS):
        m = sd.with_ids(c, kind, j)
        for opt in sd.OPTIONS:
            d = sd.check(oracle, sd.encode(synth, m, repair_topology=2, **opt), m, c.points)
            assert d.traversal_type == opt.get("predictive_connectivity", 0) and len(d.attributes) == 3
    # one row per (face, corner) over a table with an interior edge: the stream carries corner-attribute decoders
    m = sd.with_ids(c, "corner")
    d = oracle.decode(sd.encode(synth, m, repair_topology=2))
    interior = bool((d.opposite != 0xFFFFFFFF).any())
    assert [x["element_type"] for x in d.decoders] == ([0, 1, 1] if interior else [0, 0, 0]), c.name


@pytest.mark.parametrize("source", SOURCES, ids=lambda s: s[0])
def test_seamed_sources_with_injected_defects(source):
    name, kind, nx, ny = source
    corner_decoders = 0
    for j, charts in enumerate(sd.CHARTS):
        clean = sd.seamed_source(synth, name, kind, nx, ny, charts, 4 + j)
        for k, defect in enumerate(defects.KINDS):
            for count in (1, 5):
                m = sd.inject(clean, defect, count, np.random.default_rng(100 * j + 10 * k + count))
                points = coded_points(m)
                for opt in sd.OPTIONS:
                    d = sd.check(oracle, sd.encode(synth, m, repair_topology=2, **opt), m, points)
                    corner_decoders += any(x["element_type"] == 1 for x in d.decoders)
    assert corner_decoders > 0


def test_every_soup_with_ids_encodes_and_round_trips():
    """None is left out but the soups without a face that is not degenerate, which both values refuse in the same words."""
    coded = refused = needed_repair = corner_decoder = 0
    for k, c in enumerate(defects.soups(4000)):
        m = sd.soup_with_ids(c, k)
        if defects.is_degenerate(c.faces).all():
            for value in (1, 2):
                with pytest.raises(RuntimeError, match="all triangles are degenerate"):
                    sd.encode(synth, m, repair_topology=value)
            refused += 1
            continue
        opt = sd.OPTIONS[(k // 4) % len(sd.OPTIONS)] if k % 4 == 0 else {}
        d = sd.check(oracle, sd.encode(synth, m, repair_topology=2, **opt), m, coded_points(m) if k % 8 == 0 else None)
        coded += 1
        corner_decoder += any(x["element_type"] == 1 for x in d.decoders)
        try:
            sd.encode(synth, m)
        except RuntimeError:
            needed_repair += 1
    assert coded + refused == 4000
    assert needed_repair >= 1000, needed_repair      # (a condition on the generator)
    assert corner_decoder >= 1000, corner_decoder


def _doubled_face_case():
    """the mesh of tests/test_repair_cpu.py::test_per_corner_attributes_over_a_table_that_needs_repair_are_refused"""
    from meshutil import seamed_mesh
    pos, faces, nrm, nid, uv, uid = seamed_mesh(synth, synth.GRID, 6, 5, 4)
    faces2, uid2 = np.concatenate([faces, faces[2:3]]), np.concatenate([uid.reshape(-1, 3), uid.reshape(-1, 3)[2:3]])
    nid2 = None if nid is None else np.concatenate([nid.reshape(-1, 3), nid.reshape(-1, 3)[2:3]])
    return sd.Seamed("grid-6x5-face-doubled", pos, faces2.astype(np.uint32), nrm, nid2, uv, uid2.astype(np.uint32))


def test_value_1_still_refuses_and_value_2_codes_the_same_mesh():
    m = _doubled_face_case()
    with pytest.raises(RuntimeError) as e:
        sd.encode(synth, m, repair_topology=1)
    assert str(e.value) == "attributes given per corner over a mesh whose topology needs repair are not implemented"
    sd.check(oracle, sd.encode(synth, m, repair_topology=2), m, coded_points(m))


def test_clean_meshes_give_the_bytes_of_value_0():
    import irregular
    for j, charts in enumerate(sd.CHARTS):
        for name, kind, nx, ny in SOURCES:
            m = sd.seamed_source(synth, name, kind, nx, ny, charts, 4 + j)
            for opt in sd.OPTIONS:
                want = sd.encode(synth, m, **opt)
                assert want == sd.encode(synth, m, repair_topology=2, **opt) == sd.encode(synth, m, repair_topology=1, **opt), (m.name, opt)
    for k, c in enumerate(irregular.SMALL[:4]):      # per vertex, no ids at all
        pos, nrm, uv, faces = irregular.mesh(c)
        assert synth.encode_mesh(pos, faces, nrm, uv) == synth.encode_mesh(pos, faces, nrm, uv, opt=synth.options(repair_topology=2)), c.name


def test_per_vertex_meshes_that_need_repair_give_the_bytes_of_value_1():
    for k, c in enumerate(SMALL):
        pos, nrm, uv, generic, extra = defects.attributes(c.nv, k)
        for opt in sd.OPTIONS:
            a = synth.encode_mesh(pos, c.faces, nrm, uv, opt=synth.options(repair_topology=1, **opt))
            assert a == synth.encode_mesh(pos, c.faces, nrm, uv, opt=synth.options(repair_topology=2, **opt)), (c.name, opt)


def test_two_sided_sheet_with_two_normals_through_the_weld():
    """The repair separates the two sides, so no edge is left where the normals differ: 48 faces over 40 points, the normals per
    vertex through their ids ("ids without interior seam" over a repaired table), no corner decoder."""
    c = next(c for c in weldcases.cases() if c.name == "two-sided-sheet-two-normals")
    with pytest.raises(RuntimeError, match="not implemented"):
        synth.encode_mesh_points(c.pos, c.faces, c.normals, c.uvs, opt=synth.options(repair_topology=1))
    s = synth.encode_mesh_points(c.pos, c.faces, c.normals, c.uvs, opt=synth.options(repair_topology=2))
    assert sd.header_counts(s) == (40, 48)
    d = oracle.decode(s)
    assert d.end_pos == len(s) and [x["element_type"] for x in d.decoders] == [0, 0, 0]
    w = weldcases.pin(c.pos, c.faces, c.normals, c.uvs)
    assert w.normal_corners is not None          # (the weld hands the normals on with ids)
    m = sd.Seamed(c.name, w.pos, w.faces, w.normals, w.normal_corners, w.uvs, w.uv_corners)
    sd.check(oracle, s, m, 40)
