"""The HIP prediction kernels on designed geometry (tests/predictcases.py): k_texcoords_prepare and k_texcoords, k_predict_geometric with
geometric_normal_finish, k_predict_wrap, k_multipara and their serial twins in k_general, on triangles as long as the box at 17 - 20
bits, collinear, flat, coincident and collapsed vertices, axis-aligned normals, vertices on opposite walls and strips around the
texture-coordinate chain's groups of 12.

Reference: the oracle on the same bytes (test_gpu_parity.assert_same: integers, point maps, floats bit for bit, the debug tables) and
the numpy pin of the quantised input.  tests/test_predict_designs_cpu.py shows, without a GPU, that the oracle's symbols on these
streams are those of a Python-integer restatement of the arithmetic and that the designs reach the branches they are made for; the
meshes have 3 to 169 vertices, so every test here is a matter of a second or two."""
import numpy as np
import pytest

import oracle
import predictcases as P
import draco_sharp_amd as dsa
import draco_sharp_amd.synth as synth
from meshutil import source_corner_faces
from test_gpu_irregular import decode_profiled, pin_equal
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

DEBUG_CLOCKS, TRAVERSE_CLOCK = 4, 6          # batch.debug_array: the clock k_traverse leaves where the fast kernels took the mesh


@pytest.fixture(scope="module")
def ctx():
    c = dsa.Context(0)
    yield c
    c.close()


_pins = {}


def item(d, o):
    """(name, options name, stream, oracle result, pin)"""
    if d.name not in _pins:
        _pins[d.name] = P.pin(d)
    return ("%s %s" % (d.name, o), o, P.stream(d, o), P.decoded(d, o), _pins[d.name])


def ordinary():
    """Two synth.make_mesh streams: the smooth neighbours the designs share their waves with."""
    out = []
    for (kind, nx, ny), opt in (((synth.GRID, 40, 33), P.OPTION_SETS["stock"]), ((synth.TORUS, 24, 40), P.MULTI)):
        pos, nrm, uv, faces = synth.make_mesh(kind, nx, ny, 71)
        s = synth.encode_mesh(pos, faces, nrm, uv, opt=synth.options(**opt))
        out.append(("make_mesh %d" % kind, "stock" if opt is not P.MULTI else "multi", s, oracle.decode(s), source_corner_faces(pos, nrm, uv, faces)[0]))
    return out


def everything():
    items = [item(d, o) for d in P.PLAIN for o in P.OPTION_SETS] + [item(d, "multi") for d in P.MULTI_DESIGNS] + ordinary()
    order = np.random.default_rng(5).permutation(len(items))          # neighbours in a wave: other designs, other options
    return [items[k] for k in order]


def fast_path_expected(o, ref):
    """A valence stream of under 1000 faces may carry tagged context lists, which take the second chance (decode_path 2); everything
    else here belongs to the wave-per-mesh kernels."""
    return not (ref.traversal_type == 2 and ref.num_faces < 1000)


def check_all(b, items, general=False, chained=False):
    """chained: the batch took k_chain, which leaves no k_traverse clock; decode_path says it all then."""
    fast = 0
    for i, (name, o, stream, ref, pin) in enumerate(items):
        info = b.mesh_info(i)
        assert info.status == 0, (i, name, info.status, info.detail)
        got = b.result(i)
        assert_same(got, ref, b, i)
        pin_equal(got.ConnectedData, pin)
        clock = int(b.debug_array(i, DEBUG_CLOCKS, np.uint32, 12)[TRAVERSE_CLOCK])
        if general:
            assert info.decode_path != 0 and clock == 0, (i, name, info.decode_path, clock)
        elif fast_path_expected(o, ref):
            assert info.decode_path == 0 and (clock != 0 or chained), (i, name, info.decode_path, clock)
        else:
            assert info.decode_path in (0, 2), (i, name, info.decode_path)
        fast += info.decode_path == 0
    return fast


def test_every_design_and_option_set_in_one_batch(ctx):
    items = everything()
    assert len(items) == len(P.PLAIN) * 4 + len(P.MULTI_DESIGNS) + 2
    b, kernels = decode_profiled(ctx, [it[2] for it in items])
    try:
        assert kernels.get("k_texcoords", 0) > 0 and (kernels.get("k_traverse", 0) > 0 or kernels.get("k_chain", 0) > 0), kernels
        fast = check_all(b, items, chained=kernels.get("k_chain", 0) > 0)
        assert fast >= len(P.PLAIN) * 3 + len(P.MULTI_DESIGNS) + 2
    finally:
        b.close()


def test_the_same_batch_on_the_general_path(ctx, monkeypatch):
    monkeypatch.setenv("DSA_FORCE_GENERAL", "1")
    items = everything()
    b = dsa.Batch(ctx, [it[2] for it in items])
    try:
        b.decode()
        check_all(b, items, general=True)
    finally:
        b.close()


@pytest.mark.parametrize("name", ["strip-%d-18b" % n for n in P.STRIP_ENTRIES] + ["needle-20b"])
def test_a_strip_alone_in_its_batch(ctx, name):
    """One mesh, one lane pair of k_texcoords' wave alive: 3 to 80 entries, around the groups of 12 the chain requests ahead in."""
    it = item(P.design(name), "stock")
    b = dsa.Batch(ctx, [it[2]])
    try:
        b.decode()
        assert check_all(b, [it]) == 1
    finally:
        b.close()


def test_seamed_designs_on_the_seam_kernels(ctx):
    items = [item(d, o) for d in P.SEAMED for o in P.OPTION_SETS]
    assert len(items) == 16
    b, kernels = decode_profiled(ctx, [it[2] for it in items])
    try:
        assert all(kernels.get(k, 0) > 0 for k in ("k_connectivity", "k_traverse", "k_seam_tables", "k_traverse_att", "k_texcoords")), kernels
        assert check_all(b, items) >= 12
    finally:
        b.close()


@pytest.mark.parametrize("general", [False, True])
def test_constrained_multi_parallelogram_on_the_designs(ctx, monkeypatch, general):
    """Positions and texture coordinates by ConstrainedMultiParallelogram on rough, wall-hugger and lattice at 8, 14 and 20 bits: sums of
    up to four parallelograms that leave the box on both sides, negative ones with a remainder by 2, 3 and 4 among them
    (tests/test_predict_designs_cpu.py counts them) -- k_multipara, and k_general's loop."""
    if general:
        monkeypatch.setenv("DSA_FORCE_GENERAL", "1")
    items = [item(d, "multi") for d in P.MULTI_DESIGNS]
    assert len(items) >= 14 and all(it[3].attributes[0].pred_method == 4 and it[3].attributes[2].pred_method == 4 for it in items)
    b = dsa.Batch(ctx, [it[2] for it in items])
    try:
        b.decode()
        assert check_all(b, items, general=general) == (0 if general else len(items))
    finally:
        b.close()
