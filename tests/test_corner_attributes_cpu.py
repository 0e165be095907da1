"""Listed attributes given per corner (synth.Extra(corners=): a second UV set, a colour, feature ids with seams of their own)
through the CPU coder and the oracle, against the pin of tests/cornerattrcases.py, which is written from the contract and not from
the coder; the coder's refusals word for word; ids over a repaired table (repair_topology = 2); and the weld with every listed
attribute a key set of its own (weld_attributes).  This is the coder the device encoder is held against
(tests/test_gpu_encode_corner_attributes.py).  No GPU needed."""
import numpy as np
import pytest

import cornerattrcases as K
import defects
import meshutil
import oracle
import seamdefects as sd
import weldcases
import draco_sharp_amd.synth as synth

DIALECTS = [dict(), dict(predictive_connectivity=2)]                                     # standard, valence
PREDICTIONS = [dict(pos_prediction=0), dict(pos_prediction=1), dict(pos_prediction=4)]   # Difference, Parallelogram, multi_parallelogram = 4
TRAVERSALS = [dict(traversal_method=0), dict(traversal_method=2)]


def seamed_kinds(b):
    """Per attribute of the stream (positions first): has it an edge both of whose faces exist and across which its ids differ?"""
    f = np.asarray(b.faces, np.int64)
    n = int(f.max()) + 1
    half = {}
    for i, t in enumerate(f.tolist()):
        for k in range(3):
            half[t[k] * n + t[(k + 1) % 3]] = (i, k)

    def seamed(ids):
        if ids is None:
            return False
        ids = np.asarray(ids, np.int64).reshape(-1, 3)
        for i, t in enumerate(f.tolist()):
            for k in range(3):
                o = half.get(t[(k + 1) % 3] * n + t[k])
                if o is None:
                    continue
                j, kj = o
                # the edge t[k] -> t[k + 1] of face i is t[k + 1] -> t[k] of face j: corner kj of j lies on t[k + 1], kj + 1 on t[k]
                if ids[i, k] != ids[j, (kj + 1) % 3] or ids[i, (k + 1) % 3] != ids[j, kj]:
                    return True
        return False
    out = [False]
    if b.nrm is not None:
        out.append(seamed(b.nid))
    if b.uv is not None:
        out.append(seamed(b.uid))
    return out + [seamed(e.corners) for e in b.extras]


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.name)
def test_every_case_decodes_to_the_pin(case):
    b = K.build(case)
    want = K.pin(b)
    corner = [int(s) for s in seamed_kinds(b)]
    for dialect in DIALECTS:
        for prediction in PREDICTIONS:
            for traversal in TRAVERSALS:
                opt = dict(dialect, **prediction, **traversal)
                s = K.encode(b, **opt)
                ref = oracle.decode(s)
                assert ref.end_pos == len(s), opt
                assert ref.num_faces == len(b.faces) and ref.traversal_type == opt.get("predictive_connectivity", 0)
                assert K.same(K.oracle_multiset(ref), want), (case.name, opt)
                # an attribute with an interior seam has a corner-attribute decoder, every other the positions' connectivity
                assert [d["element_type"] for d in ref.decoders] == corner, (case.name, opt)
                first = len(ref.attributes) - len(b.extras)
                for e, a in zip(b.extras, ref.attributes[first:]):
                    # the prediction of the generic attribute: the positions' family, never TexCoordsPortable
                    assert (a.att_type, a.num_components, a.pred_method) == (e.attribute_type, e.num_components, 4 if opt["pos_prediction"] == 4 else 1)
                    if e.values.dtype == np.float32:
                        mn, rng, _ = meshutil.source_quantization(e.values, K.extra_bits(e))
                        assert np.array_equal(np.asarray(a.q_min[:e.num_components], np.float32), mn) and np.float32(a.q_range) == rng      # over ALL rows


def test_the_cases_hold_what_the_issue_asks_for():
    names = {c.name for c in K.CASES}
    assert len(names) == len(K.CASES)
    cuts = {cut for c in K.CASES for _, cut in c.attrs}
    assert cuts >= {None, "none", "corner", "one-row", "stripes", "checker", "island", "random", "single"}
    assert {kind for c in K.CASES for kind, _ in c.attrs} == set(K.KINDS)
    points = [len(K.build(c).pos) for c in K.GRIDS]
    assert min(points) == 9 and max(points) == 561
    # the charts of a listed attribute differ from those of the first UV set wherever both are cut
    for c in K.CASES:
        b = K.build(c)
        for e in b.extras:
            if e.corners is not None and b.uid is not None and e.corners.max() > 0:
                assert not np.array_equal(e.corners, b.uid), c.name
    # a seam along every edge: one row per corner; ids that name one row; ids without an interior seam
    assert any(seamed_kinds(K.build(c))[-1] is False and K.build(c).extras[-1].corners is not None for c in K.CASES)
    every = K.build(next(c for c in K.CASES if c.name == "grid33x17/uv1-corner"))
    assert len(every.extras[0].values) == 3 * len(every.faces)


# ---------------------------------------------------------------------------------------------------------- refusals
def _small():
    return K.build(next(c for c in K.CASES if c.name == "grid7x7/uv1-checker+colour-random"))


def test_single_connectivity_with_ids_is_refused_as_ever():
    b = K.build(next(c for c in K.CASES if c.name == "grid3x3/uv1-single"))
    assert b.nid is None and b.uid is None and b.extras[0].corners is not None      # the listed attribute alone carries ids
    with pytest.raises(RuntimeError) as e:
        K.encode(b, single_connectivity=1)
    assert str(e.value) == "attributes given per corner need a connectivity of their own (single_connectivity = 0)"


def test_an_id_past_the_rows_is_refused():
    b = _small()
    bad = synth.Extra(b.extras[1].values, attribute_type=2, normalized=True, corners=b.extras[1].corners, rows=int(b.extras[1].corners.max()))
    with pytest.raises(RuntimeError) as e:
        synth.encode_mesh_corners(b.pos, b.faces, b.nrm, b.nid, b.uv, b.uid, extra=[b.extras[0], bad])
    assert str(e.value) == "attribute 1 id out of range"


def test_ids_past_stream_index_seven_are_refused():
    b = _small()
    plain = [synth.Extra(np.zeros(len(b.pos), np.uint8)) for _ in range(5)]      # normals + uvs + 5: the next attribute is at index 8
    e7 = synth.Extra(b.extras[1].values, corners=b.extras[1].corners)
    ref = oracle.decode(synth.encode_mesh_corners(b.pos, b.faces, b.nrm, b.nid, b.uv, b.uid, extra=plain[:4] + [e7]))      # index 7: coded
    assert ref.decoders[7]["element_type"] == 1
    with pytest.raises(RuntimeError) as e:
        synth.encode_mesh_corners(b.pos, b.faces, b.nrm, b.nid, b.uv, b.uid, extra=plain + [e7])
    assert str(e.value) == "attribute 5: corner ids on attribute 8 of the stream: corner attributes are decoded for attributes 1 to 7"


def test_a_sequential_stream_takes_no_ids():
    b = _small()
    with pytest.raises(RuntimeError) as e:
        synth.encode_sequential(b.pos, b.faces, extra=b.extras)
    assert str(e.value) == "a sequential stream has one value per point"


def test_per_point_input_takes_no_ids():
    b = _small()
    with pytest.raises(ValueError, match="per-point input takes no corner ids"):
        synth.encode_mesh_points(b.pos, b.faces, extra=b.extras, weld_attributes=True)


# ------------------------------------------------------------------------------------------------- over a repaired table
REPAIRED = [("grid", synth.GRID, 6, 5, (None, "stripes"), "double", [("uv1", "checker"), ("fid16", "island")]),
            ("torus", synth.TORUS, 9, 8, ("checker", "island"), "pinch", [("colour", "stripes"), ("fid32", None)])]


@pytest.mark.parametrize("spec", REPAIRED, ids=lambda s: "%s-%s" % (s[0], s[5]))
def test_ids_over_a_table_that_needs_repair(spec):
    name, kind, nx, ny, charts, defect, attrs = spec
    clean = sd.seamed_source(synth, name, kind, nx, ny, charts, 6)
    for count in (1, 5):
        b = K.with_listed(sd.inject(clean, defect, count, np.random.default_rng(31 + count)), attrs)
        keep = ~defects.is_degenerate(b.faces)
        with pytest.raises(RuntimeError):
            K.encode(b)                                                       # (the strict coder refuses the mesh)
        with pytest.raises(RuntimeError) as e:
            K.encode(b, repair_topology=1)
        assert str(e.value) == "attributes given per corner over a mesh whose topology needs repair are not implemented"
        for opt in sd.OPTIONS:
            s = K.encode(b, repair_topology=2, **opt)
            ref = oracle.decode(s)
            assert ref.end_pos == len(s) and ref.num_faces == int(keep.sum())
            assert K.same(K.oracle_multiset(ref), K.pin(b, keep=keep)), (b.name, opt)
    # a clean mesh: the bytes of every value of repair_topology
    b = K.with_listed(clean, attrs)
    assert K.encode(b) == K.encode(b, repair_topology=1) == K.encode(b, repair_topology=2)


# ---------------------------------------------------------------------------------------------------------------- weld
def distinct_positions(pos, faces):
    used = np.unique(np.asarray(faces, np.int64))
    return len(np.unique(np.ascontiguousarray(pos, np.float32)[used].view(np.uint32).reshape(len(used), -1), axis=0))


@pytest.mark.parametrize("case", [c for c in K.CASES if any(cut is not None for _, cut in c.attrs)][::2], ids=lambda c: c.name)
def test_weld_attributes_keeps_the_positions_together(case):
    b = K.build(case)
    pos, faces, nrm, uv, arrays = K.unweld(b, np.random.default_rng(3))
    extras = K.point_extras(b, arrays)
    w1 = synth.weld_points(pos, faces, nrm, uv, extra=extras, weld_attributes=True)
    assert w1.num_vertices == distinct_positions(pos, faces) == distinct_positions(b.pos, b.faces)
    w0 = synth.weld_points(pos, faces, nrm, uv, extra=extras)
    assert w0.num_vertices >= w1.num_vertices
    # per attribute: ids exactly when some vertex has two of its rows; the rows are then the attribute's distinct rows
    for k, a in enumerate(arrays):
        rows_at = {}
        for p in np.unique(faces):
            rows_at.setdefault(int(w1.vertex_of_point[p]), set()).add(a[p].tobytes())
        two = any(len(r) > 1 for r in rows_at.values())
        assert (w1.extra_corners[k] is not None) == two, (case.name, k)
        if two:
            assert len(w1.extra[k]) == len(np.unique(a[np.unique(faces)], axis=0))
            assert np.array_equal(w1.extra[k][w1.extra_corners[k]], a[faces])
        else:
            assert np.array_equal(w1.extra[k][w1.faces], a[faces])
    s = synth.encode_mesh_points(pos, faces, nrm, uv, extra=extras, weld_attributes=True)
    ref = oracle.decode(s)
    assert ref.num_vertices >= w1.num_vertices and sd.header_counts(s)[0] == w1.num_vertices
    assert K.same(K.oracle_multiset(ref), K.pin(b)), case.name
    # with the attributes in the vertex key their seams cut the positions' connectivity: a table that may need the repair
    in_key = synth.encode_mesh_points(pos, faces, nrm, uv, extra=extras, opt=synth.options(repair_topology=2))
    assert K.same(K.oracle_multiset(oracle.decode(in_key)), K.pin(b)), case.name


def test_weld_attributes_changes_no_byte_where_no_vertex_has_two_rows():
    ran = 0
    for c in weldcases.small_cases():
        if c.refused or c.weld_only or len(c.pos) < 3:
            continue
        P = len(c.pos)
        key = np.ascontiguousarray(c.pos, np.float32).view(np.uint32).reshape(P, -1).astype(np.uint64).sum(axis=1)
        extras = [synth.Extra((key % np.uint64(251)).astype(np.uint8), attribute_type=2, normalized=True),            # functions of the position: one row per vertex
                  synth.Extra(np.stack([key % np.uint64(1000), key % np.uint64(77)], axis=1).astype(np.float32) / np.float32(16), attribute_type=3)]
        a = synth.encode_mesh_points(c.pos, c.faces, c.normals, c.uvs, c.generic, extras)
        assert a == synth.encode_mesh_points(c.pos, c.faces, c.normals, c.uvs, c.generic, extras, weld_attributes=True), c.name
        ran += 1
    assert ran >= 40, ran


def test_an_attribute_past_index_seven_stays_in_the_vertex_key():
    b = K.build(next(c for c in K.CASES if c.name == "grid9x8/colour-island+fid16-random"))
    pos, faces, nrm, uv, arrays = K.unweld(b, np.random.default_rng(5))
    filler = [synth.Extra(np.zeros(len(pos), np.uint8)) for _ in range(5)]            # normals + uvs + 5: indices 3 .. 7
    extras = filler + K.point_extras(b, arrays)                                       # the two cut attributes at indices 8 and 9
    w = synth.weld_points(pos, faces, nrm, uv, extra=extras, weld_attributes=True)
    assert all(c is None for c in w.extra_corners)
    assert w.num_vertices == synth.weld_points(pos, faces, nrm, uv, extra=extras).num_vertices > distinct_positions(pos, faces)
    repair = synth.options(repair_topology=2)                                         # (the cut positions: a table that may need the repair)
    assert synth.encode_mesh_points(pos, faces, nrm, uv, extra=extras, opt=repair, weld_attributes=True) == synth.encode_mesh_points(pos, faces, nrm, uv, extra=extras, opt=repair)
    moved = K.point_extras(b, arrays) + filler                                        # the cut ones first: welded alone
    w = synth.weld_points(pos, faces, nrm, uv, extra=moved, weld_attributes=True)
    assert w.num_vertices == distinct_positions(pos, faces) and w.extra_corners[0] is not None and w.extra_corners[1] is not None
