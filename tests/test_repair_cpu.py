"""The CPU coder with repair_topology = 1 (dsa_encode_host.h: CornerTable::build_repaired -- the reference's corner table,
CornerTable.cs:28-43 -- in place of the refusal of degenerate faces, non-manifold edges and vertices and isolated vertices),
decoded through the oracle: the header counts, and the decoded face multiset against the pin of tests/defects.py, which is
written from the contract and not from the coder.  This is the coder the device encoder is held against
(tests/test_gpu_encode_repair.py).  No GPU needed."""
import itertools

import numpy as np
import pytest

import defects
import irregular
import oracle
import draco_sharp_amd.synth as synth

# {standard, valence} x {parallelogram, difference, ConstrainedMultiParallelogram} x {depth first, prediction degree}
#   x single_connectivity x {normals by difference, GeometricNormal} x {UV parallelogram, TexCoordsPortable}
PRODUCT = [dict(predictive_connectivity=e, pos_prediction=p, traversal_method=t, single_connectivity=s, normal_prediction=n, uv_prediction=u)
           for e, p, t, s, n, u in itertools.product((0, 2), (1, 0, 4), (0, 1), (0, 1), (0, 6), (1, 5))]
SMALL = defects.named() + defects.placed()


def encode(c, seed=0, full=True, **opt):
    pos, nrm, uv, generic, extra = defects.attributes(c.nv, seed)
    if not full:
        return synth.encode_mesh(pos, c.faces, opt=synth.options(**opt)), defects.pin(c.faces, pos)
    if opt.get("pos_prediction") == 4 and opt.get("uv_prediction", 1) == 1:
        opt["uv_prediction"] = 4                 # (what multi_parallelogram = 4 means for the first UV set)
    s = synth.encode_mesh(pos, c.faces, nrm, uv, generic=generic, opt=synth.options(generic_components=2, **opt), extra=[synth.Extra(extra)])
    return s, defects.pin(c.faces, pos, nrm, uv, [generic, extra])


def check(stream, want, params, c=None):
    m = oracle.decode(stream)
    if c is not None and c.points is not None:
        assert (m.num_points, m.num_faces) == (c.points, c.num_faces), c.name
    assert m.num_faces == len(want)
    got = defects.decoded(m.faces, [(a.portable, a.point_map) for a in m.attributes])
    assert got.shape == want.shape and np.array_equal(got, want), c.name if c else None
    pmin, prange, umin, urange = params
    ap = m.attributes[0]                         # the bounds over all rows the caller passed, isolated ones included
    assert np.array_equal(np.asarray(ap.q_min[:3], np.float32), pmin) and np.float32(ap.q_range) == prange
    if umin is not None:
        au = m.attributes[2]
        assert np.array_equal(np.asarray(au.q_min[:2], np.float32), umin) and np.float32(au.q_range) == urange
    return m


@pytest.mark.parametrize("c", SMALL, ids=lambda c: c.name)
def test_header_counts_and_pin_over_the_option_product(c):
    for k, opt in enumerate(PRODUCT):
        stream, (want, params) = encode(c, k % 3, repair_topology=1, **opt)
        m = check(stream, want, params, c)
        assert m.traversal_type == opt["predictive_connectivity"] and len(m.attributes) == 5


def test_isolated_rows_shape_the_quantisation_bounds():
    """An isolated vertex far outside the others: the stream's range is the one over all rows (AttributeQuantizationTransform.cs:66-100)."""
    c = defects.placed()[2]                      # isolated vertices last
    pos = defects.attributes(c.nv)[0]
    pos[-1] = [50.0, -7.0, 3.0]
    m = oracle.decode(synth.encode_mesh(pos, c.faces, opt=synth.options(repair_topology=1)))
    want, (pmin, prange, _, _) = defects.pin(c.faces, pos)
    assert np.float32(m.attributes[0].q_range) == prange and prange > 49      # (50 less the least x of the others, which lie in 0 .. 1)
    assert np.array_equal(defects.decoded(m.faces, [(m.attributes[0].portable, m.attributes[0].point_map)]), want)


def test_injected_defects_in_irregular_meshes():
    for k, c in enumerate(defects.injected_small()):
        for opt in (PRODUCT[0], PRODUCT[-1], PRODUCT[37]):
            stream, (want, params) = encode(c, k, repair_topology=1, **opt)
            check(stream, want, params, c)


def test_every_soup_encodes_and_round_trips():
    """None is left out: every soup with a face that is not degenerate encodes, and decodes to its pin."""
    coded = refused = broke = 0
    for k, c in enumerate(defects.soups(4000)):
        if defects.is_degenerate(c.faces).all():
            with pytest.raises(RuntimeError, match="all triangles are degenerate"):
                encode(c, full=False, repair_topology=1)
            refused += 1
            continue
        opt = PRODUCT[k % len(PRODUCT)] if k % 4 == 0 else {}
        stream, (want, params) = encode(c, k, full=k % 4 == 0, repair_topology=1, **opt)
        m = check(stream, want, params, c)
        coded += 1
        broke += m.num_points > len(np.unique(c.faces[~defects.is_degenerate(c.faces)]))
    assert coded + refused == 4000 and coded > refused and broke > 0      # (broke: the repair made new points)


def test_all_faces_degenerate_and_no_faces():
    with pytest.raises(RuntimeError, match="all triangles are degenerate"):
        encode(defects.ALL_DEGENERATE, full=False, repair_topology=1)


def test_clean_meshes_give_the_same_bytes_with_and_without_the_option():
    for k, c in enumerate(irregular.SMALL):
        pos, nrm, uv, faces = irregular.mesh(c)
        for opt in (PRODUCT[0], PRODUCT[-1], PRODUCT[50], PRODUCT[21]):
            opt = dict(opt)
            if opt["pos_prediction"] == 4 and opt["uv_prediction"] == 1:
                opt["uv_prediction"] = 4
            a = synth.encode_mesh(pos, faces, nrm, uv, opt=synth.options(**opt))
            assert a == synth.encode_mesh(pos, faces, nrm, uv, opt=synth.options(repair_topology=1, **opt)), (c.name, opt)
    from meshutil import seamed_mesh             # attributes given per corner over a clean table: coded as ever
    pos, faces, nrm, nid, uv, uid = seamed_mesh(synth, synth.TORUS, 9, 8, 4)
    a = synth.encode_mesh_corners(pos, faces, nrm, nid, uv, uid)
    assert a == synth.encode_mesh_corners(pos, faces, nrm, nid, uv, uid, opt=synth.options(repair_topology=1))


def test_per_corner_attributes_over_a_table_that_needs_repair_are_refused():
    from meshutil import seamed_mesh
    pos, faces, nrm, nid, uv, uid = seamed_mesh(synth, synth.GRID, 6, 5, 4)
    faces2, uid2 = np.concatenate([faces, faces[2:3]]), np.concatenate([uid.reshape(-1, 3), uid.reshape(-1, 3)[2:3]])
    nid2 = None if nid is None else np.concatenate([nid.reshape(-1, 3), nid.reshape(-1, 3)[2:3]])
    with pytest.raises(RuntimeError, match="not implemented"):
        synth.encode_mesh_corners(pos, faces2, nrm, nid2, uv, uid2, opt=synth.options(repair_topology=1))


@pytest.mark.parametrize("name,message", [("two-tetrahedra-one-vertex", "non-manifold vertex in input mesh"), ("fin", "non-manifold edge (duplicate half-edge)"),
                                          ("face-twice", "non-manifold edge (duplicate half-edge)"), ("isolated-and-degenerate", "degenerate face in input mesh"),
                                          ("isolated-last", "isolated vertex in input mesh")])
def test_without_the_option_the_old_refusals_stand(name, message):
    c = next(c for c in SMALL if c.name == name)
    with pytest.raises(RuntimeError) as e:
        encode(c, full=False)
    assert str(e.value) == message
    with pytest.raises(RuntimeError) as e:
        encode(c, full=False, repair_topology=0)
    assert str(e.value) == message
