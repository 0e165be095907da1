"""Every encode entry point is one request in the library (EncRequest over dsa_mesh_attr_input, one option check): each wider
call with its added fields at their defaults must give, byte for byte and message for message, what the narrower call gives, and
the CPU coder's stream where the mesh is legal.  The batch runs in chunks of two (DSA_ENC_CHUNK), so that chunks start inside the
array an entry widened, on both connectivity paths.  And the option check names the outermost illegal field of the layered
options, in the texts the entries had when each checked its own layer."""
import ctypes as C
import itertools

import numpy as np
import pytest

import defects
import draco_sharp_amd as dsa
import draco_sharp_amd.synth as synth
import encodecall
import meshutil
from draco_sharp_amd import native

pytestmark = pytest.mark.gpu

BOTH_PATHS = pytest.mark.parametrize("host", ["0", "1"])
SHAPES = ((synth.GRID, 6, 5), (synth.HOLES, 12, 9))      # those of the layout host check
# by input form, narrowest first: an entry takes the meshes its form can express
EDGEBREAKER = (("dsa_encode_batch", "base"), ("dsa_encode_batch_corners", "base"), ("dsa_encode_batch_ex", "ex"), ("dsa_encode_attributes_batch", "ex"),
               ("dsa_encode_level_batch", "level"), ("dsa_encode_repair_batch", "repair"), ("dsa_encode_grid_batch", "grid"), ("dsa_encode_seam_repair_batch", "seam"))
SEQUENTIAL = ("dsa_encode_sequential_batch", "dsa_encode_attributes_sequential_batch", "dsa_encode_grid_sequential_batch")


@pytest.fixture(scope="module")
def ctx():
    c = dsa.Context(0)
    yield c
    c.close()


def force(monkeypatch, host):
    monkeypatch.setenv("DSA_ENC_HOST_CONN", host)
    monkeypatch.setenv("DSA_ENC_HOST_PLAN", host)
    monkeypatch.setenv("DSA_ENC_CHUNK", "2")


def batch():
    """(per vertex, seamed, with an attribute list): the two shapes per vertex with normals and UVs, one more with a uint8 generic
    and the doubled-face defect; the two shapes seamed; one with a uint16 x 4 extra"""
    vertex, seamed = [], []
    for k, (kind, nx, ny) in enumerate(SHAPES):
        pos, nrm, uv, faces = synth.make_mesh(kind, nx, ny, 1 + k)
        vertex.append(dsa.MeshData(pos, faces, nrm, uv))
        pos, faces, nrm, nid, uv, uid = meshutil.seamed_mesh(synth, kind, nx, ny, 20 + k, normal_charts="island", uv_charts="stripes")
        seamed.append(dsa.MeshData(pos, faces, nrm, uv, normal_corners=nid, texcoord_corners=uid))
    rng = np.random.default_rng(4)
    pos, nrm, uv, faces = synth.make_mesh(synth.GRID, 6, 5, 7)
    vertex.append(dsa.MeshData(pos, faces, nrm, uv, generic=rng.integers(0, 256, (len(pos), 3)).astype(np.uint8)))
    doubled = [c for c in defects.named() if c.name == "grid-face-doubled"][0]
    vertex.insert(1, dsa.MeshData(defects.attributes(doubled.nv, 3)[0], doubled.faces))
    pos, nrm, uv, faces = synth.make_mesh(synth.HOLES, 12, 9, 8)
    listed = [dsa.MeshData(pos, faces, nrm, uv, attributes=[dsa.Attribute(rng.integers(0, 900, (len(pos), 4)).astype(np.uint16))])]
    return vertex, seamed, listed


def cpu(m, sequential=False, repair=0):
    """The CPU coder's stream of MeshData m at the default options, or the text of its refusal."""
    opt = synth.options(generic_components=m.generic.shape[1] if m.generic is not None else 1, repair_topology=repair)
    extra = [synth.Extra(a.values, a.attribute_type, a.normalized, a.unique_id, a.quantization_bits) for a in m.attributes] or None
    try:
        if sequential:
            return synth.encode_sequential(m.positions, m.faces, m.normals, m.texcoords, m.generic, compressed=False, opt=opt, extra=extra)
        return synth.encode_mesh_corners(m.positions, m.faces, m.normals, m.normal_corners, m.texcoords, m.texcoord_corners, opt=opt, generic=m.generic, extra=extra)
    except RuntimeError as e:
        return str(e)


def options(layer, topology=0):
    """the option struct of `layer` made from a default Config: every field the layers above the base add at its default"""
    cfg = dsa.Config(repair_topology=bool(topology))
    if layer in ("base", "ex", "level", "repair"):
        return {"base": cfg._native, "ex": cfg._native_ex, "level": cfg._native_level, "repair": cfg._native_repair}[layer]()
    so = native.EncodeSeamRepairOptions()
    native.lib().dsa_encode_default_seam_repair_options(C.byref(so))
    so.grid.repair = cfg._native_repair()
    return so if layer == "seam" else so.grid


def through(ctx, calls, meshes):
    """the answers of every (entry, options) of `calls` to the meshes, which must be one answer"""
    got = None
    for name, opt in calls:
        st, out = encodecall.call(ctx, name, meshes, opt, grids=None)
        assert st == 0, (name, ctx.error())
        assert got is None or out == got, name
        got = out
    return got


@BOTH_PATHS
def test_edgebreaker_entries_give_one_answer(ctx, monkeypatch, host):
    force(monkeypatch, host)
    vertex, seamed, listed = batch()
    # per vertex: all eight; with ids: all but dsa_encode_batch; with a list: the entries over dsa_mesh_attr_input
    for meshes, entries in ((vertex, EDGEBREAKER), (vertex[:2] + seamed + vertex[2:], EDGEBREAKER[1:]), (vertex[:2] + seamed + listed + vertex[2:], EDGEBREAKER[3:])):
        got = through(ctx, [(name, options(layer)) for name, layer in entries], meshes)
        for m, (st, g) in zip(meshes, got):
            want = cpu(m)
            if isinstance(want, bytes):
                assert (st, g) == (0, want)
            else:                                                  # the doubled face: refused, in the CPU coder's words
                assert m is vertex[1] and st == native.DSA_ERR_INVALID_DATA and want in g, g
    # topology 1: the entries that have the switch code the defect, and the clean meshes as ever
    meshes = vertex[:2] + seamed + listed + vertex[2:]
    got = through(ctx, [(name, options(layer, topology=1)) for name, layer in EDGEBREAKER[5:]], meshes)
    assert got == [(0, cpu(m, repair=1)) for m in meshes]
    assert got[1][1] != cpu(vertex[1]) and all(g == cpu(m) for m, (_, g) in zip(meshes, got) if m is not vertex[1])


@BOTH_PATHS
def test_sequential_entries_give_one_answer(ctx, monkeypatch, host):
    force(monkeypatch, host)
    vertex, _, listed = batch()
    opt = dsa.Config(encoding_method=0)._native_sequential(1)
    for meshes, entries in ((vertex, SEQUENTIAL), (vertex[:3] + listed + vertex[3:], SEQUENTIAL[1:])):
        got = through(ctx, [(name, opt) for name in entries], meshes)
        assert got == [(0, cpu(m, sequential=True)) for m in meshes]            # (any list of triangles is legal)


def seam_options():
    o = native.EncodeSeamRepairOptions()
    native.lib().dsa_encode_default_seam_repair_options(C.byref(o))
    return o


def _set(path, value):
    def apply(o):
        *head, last = path.split(".")
        for name in head:
            o = getattr(o, name)
        if "[" in last:
            getattr(o, last[:last.index("[")])[int(last[last.index("[") + 1:-1])] = value
        else:
            setattr(o, last, value)
    return apply


LEVEL, EX = "grid.repair.level.", "grid.repair.level.ex."
# (layer, field of dsa_encode_seam_repair_options, an illegal value, dsa_last_error), the outermost check first
FAULTS = [
    ("seam", "corner_repair", 2, "corner_repair 2: 0 (refused as ever) or 1 (coded over the repaired table)"),
    ("seam", "reserved[3]", 1, "dsa_encode_seam_repair_options.reserved[3] is not zero"),
    ("seam", "corner_repair", 1, "corner_repair 1 needs topology 1 (the reference's corner table), topology is 0"),
    ("grid", "grid.weld_points", 2, "weld_points 2: 0 (rows per vertex) or 1 (rows per point)"),
    ("grid", "grid.reserved[0]", 9, "dsa_encode_grid_options.reserved[0] is not zero"),
    ("repair", "grid.repair.topology", 3, "topology 3: 0 (strict) or 1 (the reference's corner table)"),
    ("repair", "grid.repair.reserved[6]", 1, "dsa_encode_repair_options.reserved[6] is not zero"),
    ("base", EX + "base.position_prediction", 2, "position_prediction 2: the encoder writes 0 (difference) or 1 (parallelogram)"),
    ("base", EX + "base.texcoord_prediction", 4, "texcoord_prediction 4: the encoder writes 0 (difference), 1 (parallelogram) or 5 (TexCoordsPortable)"),
    ("ex", EX + "edgebreaker_method", 1, "edgebreaker_method 1: 0 (standard), 2 (valence) or -1 (by speed and face count)"),
    ("ex", EX + "normal_prediction", 5, "normal_prediction 5: 0 (difference) or 6 (GeometricNormal)"),
    ("ex", EX + "reserved[5]", 1, "dsa_encode_options_ex.reserved[5] is not zero"),
    ("level", LEVEL + "multi_parallelogram", 3, "multi_parallelogram 3: 0 (off), 2 (MultiParallelogram), 4 (ConstrainedMultiParallelogram) or -1 (by speed and vertex count)"),
    ("level", LEVEL + "traversal_method", 3, "traversal_method 3: 0 (depth first), 1 (prediction degree for the positions' decoder) or 2 (for every decoder without interior seams)"),
    ("level", LEVEL + "reserved[2]", 1, "dsa_encode_level_options.reserved[2] is not zero"),
]


def test_the_option_check_names_the_outermost_field(ctx):
    """a real context and no meshes: nothing but the check runs"""
    for _, field, value, text in FAULTS:
        o = seam_options()
        _set(field, value)(o)
        assert encodecall.call(ctx, "dsa_encode_seam_repair_batch", [], o)[0] == native.DSA_ERR_INVALID_ARGUMENT
        assert ctx.error() == text
    pairs = 0
    for (la, fa, va, text), (lb, fb, vb, _) in itertools.combinations(FAULTS, 2):
        if la == lb:
            continue
        o = seam_options()
        _set(fb, vb)(o)
        _set(fa, va)(o)                                            # (the outer one last: topology 3 under corner_repair 1 is the outer's to name)
        assert encodecall.call(ctx, "dsa_encode_seam_repair_batch", [], o)[0] == native.DSA_ERR_INVALID_ARGUMENT
        assert ctx.error() == (text if (fa, va, fb) != ("corner_repair", 1, "grid.repair.topology") else "corner_repair 1 needs topology 1 (the reference's corner table), topology is 3"), (fa, fb)
        pairs += 1
    assert pairs > 80
    # and the null argument sits between the repair layer and the schemes
    o = seam_options()
    o.grid.repair.level.traversal_method = 3
    h = C.c_void_p()
    assert native.lib().dsa_encode_seam_repair_batch(ctx._h, 1, None, None, C.byref(o), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT
    assert ctx.error() == "null argument"
    o.grid.repair.topology = 3
    assert native.lib().dsa_encode_seam_repair_batch(ctx._h, 1, None, None, C.byref(o), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT
    assert ctx.error() == FAULTS[5][3]
