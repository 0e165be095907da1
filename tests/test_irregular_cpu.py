"""Irregular connectivity on the CPU (tests/irregular.py): the conditions the shared list CASES has to keep, so that a later
edit cannot quietly make it regular again, and the reference side of tests/test_gpu_irregular.py -- for every case and
dialect the oracle's decode of the CPU coder's stream equals the numpy pin of the INPUT (meshutil.source_corner_faces*),
as tests/test_independent_pin.py shows it for grids.  That is what entitles the GPU tests to hold the kernels against the
oracle on this input.  No case may be refused by either coder."""
import numpy as np
import pytest

import irregular
import oracle
import draco_sharp_amd.synth as synth
from meshutil import source_corner_faces, source_corner_faces_seamed
from test_independent_pin import check_params, decoded_faces

NAMES = [c.name for c in irregular.CASES]
SMALL = [c.name for c in irregular.SMALL]
CHARTS = irregular.CHARTS
SEAM_DIALECTS = [dict(), dict(predictive_connectivity=2, uv_prediction=5, normal_prediction=6), dict(uv_prediction=5), dict(pos_prediction=4, uv_prediction=4)]


def case(name):
    return next(c for c in irregular.CASES if c.name == name)


def test_the_list_has_every_kind_at_both_sizes():
    assert len(set(NAMES)) == len(NAMES)
    for c in irregular.SMALL:
        assert 200 <= len(irregular.mesh(c)[3]) <= 5000, c.name
    assert len(irregular.BENCH_SIZE) == 3
    for c in irregular.BENCH_SIZE:
        assert 60000 <= len(irregular.mesh(c)[3]) <= 70000, c.name
    for word in ("grid", "torus", "sphere", "holes", "two-parts", "thickened", "subdivided", "shuffled", "fan-closed", "fan-open", "strip", "components"):
        assert any(word in n for n in SMALL), word


@pytest.mark.parametrize("name", NAMES)
def test_cases_are_oriented_manifolds(name):
    pos, nrm, uv, faces = irregular.mesh(name)
    assert len(nrm) == len(pos) and len(uv) == len(pos)
    assert irregular.is_oriented_manifold(len(pos), faces)      # no isolated vertex, no degenerate face, one fan per vertex
    assert np.isfinite(pos).all() and np.isfinite(nrm).all() and np.isfinite(uv).all()


@pytest.mark.parametrize("name", [c.name for c in irregular.CASES if c.spread])
def test_flipped_and_subdivided_cases_are_irregular(name):
    pos, _, _, faces = irregular.mesh(name)
    hist = irregular.valence_histogram(faces)
    print(name, hist)
    assert len(hist) >= 8, hist
    assert hist.get(6, 0) <= 0.35 * len(pos), hist


@pytest.mark.parametrize("name", [c.name for c in irregular.CASES if c.genus is not None])
def test_thickened_cases_have_one_handle_per_hole(name):
    c = case(name)
    assert c.genus > 0 and irregular.genus(irregular.mesh(c)[3]) == c.genus


def test_the_checks_themselves_notice_a_damaged_mesh():
    pos, _, _, faces = irregular.mesh("torus-flipped")
    assert irregular.is_oriented_manifold(len(pos), faces)
    bad = faces.copy()
    bad[5] = bad[5][::-1]
    assert not irregular.is_oriented_manifold(len(pos), bad)                 # a face turned over
    assert not irregular.is_oriented_manifold(len(pos) + 1, faces)           # an isolated vertex
    bad = faces.copy()
    bad[7, 1] = bad[7, 0]
    assert not irregular.is_oriented_manifold(len(pos), bad)                 # a degenerate face
    # two fans that meet in one vertex
    bow = np.array([[0, 1, 2], [0, 3, 4]], np.uint32)
    assert not irregular.is_oriented_manifold(5, bow)
    assert irregular.valence_histogram(synth.make_mesh(synth.TORUS, 24, 40, 1)[3]) == {6: 960}


def test_flips_and_shuffles_keep_the_surface():
    pos, nrm, uv, faces = synth.make_mesh(synth.HOLES, 20, 16, 3)
    flipped = irregular.flip_edges(faces, 300, np.random.default_rng(1))
    assert len(flipped) == len(faces) and not np.array_equal(flipped, faces)
    assert np.array_equal(np.sort(irregular.boundary_edges(flipped), axis=0), np.sort(irregular.boundary_edges(faces), axis=0))
    assert irregular.euler_characteristic(flipped) == irregular.euler_characteristic(faces)
    assert np.array_equal(irregular.flip_edges(faces, 300, np.random.default_rng(1)), flipped)          # deterministic
    a = source_corner_faces(pos, nrm, uv, flipped)[0]
    b = source_corner_faces(*irregular.shuffle(pos, nrm, uv, flipped, np.random.default_rng(2)))[0]
    assert np.array_equal(a, b)                                               # a shuffle changes nothing a decoder can see


def pin_check(m, expected, params):
    ap, an, au = m.attributes
    assert (ap.q_bits, an.oct_bits, au.q_bits) == (11, 8, 10)
    check_params((ap.q_min, ap.q_range), (au.q_min, au.q_range), params)
    ident = np.arange(m.num_points, dtype=np.uint32)
    got = decoded_faces(m.faces, [(a.portable, a.point_map if len(a.point_map) else ident) for a in m.attributes])
    assert got.shape == expected.shape and np.array_equal(got, expected)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_the_quantised_input(name):
    pos, nrm, uv, faces = irregular.mesh(name)
    expected, params = source_corner_faces(pos, nrm, uv, faces)
    splits = set()
    for dialect, opt in irregular.DIALECTS.items():
        data = synth.encode_mesh(pos, faces, nrm, uv, opt=synth.options(**opt))        # (a refusal raises)
        m = oracle.decode(data)
        assert m.end_pos == len(data), dialect
        assert m.traversal_type == opt.get("predictive_connectivity", 0), dialect
        pin_check(m, expected, params)
        splits.add(m.num_vertices - m.num_points)
    print(name, "split events", splits)
    if case(name).spread and case(name).splits:
        assert min(splits) >= 30              # handles, holes and components under flips: the split-corner paths are in use


@pytest.mark.parametrize("name", SMALL)
def test_oracle_reproduces_the_quantised_input_with_seams(name):
    mesh = irregular.mesh(name)
    for k, charts in enumerate(CHARTS):
        args = irregular.with_seams(*mesh, *charts, seed=5 + k)
        expected, params = source_corner_faces_seamed(*args)
        for opt in SEAM_DIALECTS:
            data = synth.encode_mesh_corners(*args, opt=synth.options(**opt))
            m = oracle.decode(data)
            assert m.end_pos == len(data), (charts, opt)
            pin_check(m, expected, params)


def test_seamed_mesh_is_with_seams_of_a_generated_mesh():
    """meshutil.seamed_mesh keeps its results: the mesh make_mesh returns, cut by the same charts."""
    import meshutil
    pos, nrm, uv, faces = synth.make_mesh(synth.HOLES, 20, 16, 11)
    got = meshutil.seamed_mesh(synth, synth.HOLES, 20, 16, 11, "checker", "island")
    nid, rows_n = meshutil.split_by_chart(faces, nrm, meshutil.chart_of_faces(pos, faces, "checker", 12), [0.3, -0.2, 0.1])
    uid, rows_u = meshutil.split_by_chart(faces, uv, meshutil.chart_of_faces(pos, faces, "island", 13), [1.25, 0.5])
    for a, b in zip(got, (pos, faces, rows_n, nid, rows_u, uid)):
        assert np.array_equal(a, b)
    assert meshutil.seamed_mesh(synth, synth.GRID, 6, 5, 1, None, None)[3] is None


def test_the_encoder_inputs_are_coded_by_the_cpu_coder():
    """What tests/test_gpu_irregular.py gives the device encoder (shuffled cases, per vertex and with seams): the CPU coder,
    the reference of that comparison, refuses none of them and the oracle decodes its streams to the quantised input."""
    for name, (pos, nrm, uv, faces) in irregular.shuffled_small():
        assert irregular.is_oriented_manifold(len(pos), faces), name
        expected, params = source_corner_faces(pos, nrm, uv, faces)
        assert np.array_equal(expected, source_corner_faces(*irregular.mesh(name))[0]), name
        for opt in (dict(), irregular.DIALECTS["stock-default"]):
            pin_check(oracle.decode(synth.encode_mesh(pos, faces, nrm, uv, opt=synth.options(**opt))), expected, params)
    seamed = irregular.seamed_small(shuffled=True)
    assert len(seamed) == 2 * len(SMALL) and {c for _, c, _ in seamed} == set(CHARTS)
    for name, charts, args in seamed:
        expected, params = source_corner_faces_seamed(*args)
        for opt in (dict(), irregular.DIALECTS["stock-default"]):
            pin_check(oracle.decode(synth.encode_mesh_corners(*args, opt=synth.options(**opt))), expected, params)
