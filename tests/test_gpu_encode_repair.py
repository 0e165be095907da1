"""Encode direction, meshes that are not clean (dsa_encode_repair_batch, topology = 1): the same face twice, fins, fans that meet at
a vertex, faces turned over, degenerate faces, isolated vertices.  The device coder must write, byte for byte, the stream of the
CPU coder with repair_topology = 1 on both connectivity paths (DSA_ENC_HOST_CONN: the repair kernels of dsa_encode_repair.h on the
device path, the host coder's table on the other), clean meshes must get the bytes of dsa_encode_level_batch, the refusals that
remain must fail their mesh alone, and every repaired stream must decode on the device to the pin of tests/defects.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

import encodecall
import defects
import draco_sharp_amd as dsa
import draco_sharp_amd.synth as synth
from draco_sharp_amd import native

pytestmark = pytest.mark.gpu

BOTH_PATHS = pytest.mark.parametrize("host", ["0", "1"])
ALL_DEGENERATE, NOT_IMPLEMENTED = "all triangles are degenerate", "not implemented"


@pytest.fixture(scope="module")
def ctx():
    c = dsa.Context(0)
    yield c
    c.close()


def force_path(monkeypatch, host):
    monkeypatch.setenv("DSA_ENC_HOST_CONN", host)
    monkeypatch.setenv("DSA_ENC_HOST_PLAN", host)


def mesh_of(case, seed=0, full=True):
    """MeshData of a tests/defects.py case: every attribute kind (normals, UVs, a generic attribute, one int16 extra), or positions alone."""
    pos, nrm, uv, generic, extra = defects.attributes(case.nv, seed)
    if not full:
        return dsa.MeshData(pos, case.faces)
    return dsa.MeshData(pos, case.faces, nrm, uv, generic=generic, attributes=[dsa.Attribute(extra)])


def pin_of(m):
    ints = ([m.generic] if m.generic is not None else []) + [a.values for a in m.attributes]
    return defects.pin(m.faces, m.positions, m.normals, m.texcoords, ints)[0]


def opt_of(cfg, m, repair=1):
    mp = cfg.multi_parallelogram
    return synth.options(pos_bits=cfg.position_bits, uv_bits=cfg.texcoord_bits, normal_bits=cfg.normal_bits,
                         single_connectivity=1 if cfg.single_connectivity else 0, force_scheme=cfg.symbol_scheme,
                         compression_level=10 - cfg.speed,
                         pos_prediction=mp if mp and cfg.position_prediction == 1 else cfg.position_prediction,
                         uv_prediction=mp if mp and cfg.texcoord_prediction == 1 else cfg.texcoord_prediction,
                         normal_prediction=cfg.normal_prediction, traversal_method=cfg.traversal_method,
                         predictive_connectivity=2 if cfg.edgebreaker_method == 2 else 0,
                         generic_components=m.generic.shape[1] if m.generic is not None else 1, repair_topology=repair)


def cpu(m, cfg, repair=1):
    """The CPU coder's stream of MeshData m, or the text of its refusal."""
    extra = [synth.Extra(a.values, a.attribute_type, a.normalized, a.unique_id, a.quantization_bits) for a in m.attributes] or None
    try:
        if m.per_corner:
            return synth.encode_mesh_corners(m.positions, m.faces, m.normals, m.normal_corners, m.texcoords, m.texcoord_corners,
                                             opt=opt_of(cfg, m, repair), generic=m.generic, extra=extra)
        return synth.encode_mesh(m.positions, m.faces, m.normals, m.texcoords, generic=m.generic, opt=opt_of(cfg, m, repair), extra=extra)
    except RuntimeError as e:
        return str(e)


def raw(ctx, meshes, opt, entry="dsa_encode_repair_batch"):
    """(call status, [(status, bytes or the refusal's text) per mesh])"""
    return encodecall.call(ctx, entry, meshes, opt)


def repair(ctx, meshes, cfg, topology=1):
    o = cfg._native_repair()
    o.topology = topology
    st, out = raw(ctx, meshes, o)
    assert st == 0, ctx.error()
    return out


def level(ctx, meshes, cfg):
    st, out = raw(ctx, meshes, cfg._native_level(), "dsa_encode_level_batch")
    assert st == 0, ctx.error()
    return out


def check_decodes_to_the_pin(ctx, streams, meshes):
    b = dsa.Batch(ctx, streams)
    b.decode()
    for i, m in enumerate(meshes):
        assert b.status(i) == 0, (i, b.status(i))
        d = b.result(i).ConnectedData
        got = defects.decoded(d.Faces, [(a.PortableValues, a.PointMap) for a in d.Attributes])
        want = pin_of(m)
        assert got.shape == want.shape and np.array_equal(got, want), i
    b.close()


SMALL_CASES = defects.named() + defects.placed()[:5]
# {standard, valence} x {parallelogram, difference, ConstrainedMultiParallelogram}: a test each; inside it the product of
# {depth first, prediction degree} x single_connectivity x {normals by difference, GeometricNormal} x {UV parallelogram, TexCoordsPortable}
OUTER = [dict(edgebreaker_method=e, **p) for e in (0, 2) for p in (dict(), dict(position_prediction=0), dict(multi_parallelogram=4))]
INNER = [dict(traversal_method=t, single_connectivity=bool(s), normal_prediction=n, texcoord_prediction=u)
         for t, s, n, u in itertools.product((0, 1), (0, 1), (0, 6), (1, 5))]


@BOTH_PATHS
@pytest.mark.parametrize("outer", OUTER, ids=lambda o: "-".join("%s%s" % (k[:4], v) for k, v in o.items()))
def test_named_cases_match_the_cpu_coder(ctx, monkeypatch, host, outer):
    force_path(monkeypatch, host)
    meshes = [mesh_of(c, k) for k, c in enumerate(SMALL_CASES)]
    for inner in INNER:
        cfg = dsa.Config(repair_topology=True, **outer, **inner)
        got = repair(ctx, meshes, cfg)
        for c, m, (st, g) in zip(SMALL_CASES, meshes, got):
            assert st == 0, (c.name, g, inner)
            assert g == cpu(m, cfg), (c.name, inner)
    check_decodes_to_the_pin(ctx, [g for _, g in got], meshes)            # (the last option set's streams)


def crowded():
    """About 300 meshes, one in four defective (every named and placed case, injected defects of every kind, soups) among clean grids
    of 4 x 4 ... 12 x 12; one mesh with every face degenerate and one given per corner that needs the repair."""
    bad = [mesh_of(c, k, full=k % 2 == 0) for k, c in enumerate(defects.named() + defects.placed())]
    rng = np.random.default_rng(21)
    for k, kind in enumerate(defects.KINDS * 3):
        pos, _, _, faces = synth.make_mesh(synth.GRID, 5 + k % 4, 4 + k % 5, 60 + k)
        nv, f = defects.inject(len(pos), faces, kind, 1 + k % 8, rng)
        bad.append(mesh_of(defects.Defect("injected", nv, f, None, None), k, full=k % 3 == 0))
    soups = [s for s in defects.soups(60, seed=5) if not defects.is_degenerate(s.faces).all()]
    bad += [mesh_of(s, k, full=False) for k, s in enumerate(soups[:36])]
    bad.append(mesh_of(defects.ALL_DEGENERATE, full=False))
    pos, nrm, uv, faces = synth.make_mesh(synth.GRID, 4, 4, 2)              # per corner and a face doubled
    faces = np.concatenate([faces, faces[3:4]])
    bad.append(dsa.MeshData(pos, faces, nrm, uv, texcoord_corners=faces))
    meshes, is_bad = [], []
    for k in range(4 * len(bad)):
        if k % 4 == 1:
            meshes.append(bad[k // 4]); is_bad.append(True)
        else:
            n = 3 + k % 9
            pos, nrm, uv, faces = synth.make_mesh(synth.GRID, n, 3 + (k // 9) % 9, k)
            meshes.append(dsa.MeshData(pos, faces, nrm, uv)); is_bad.append(False)
    return meshes, is_bad


@pytest.fixture(scope="module")
def crowd():
    meshes, is_bad = crowded()
    cfg = dsa.Config(repair_topology=True, edgebreaker_method=2, texcoord_prediction=5, normal_prediction=6, traversal_method=1)
    return meshes, is_bad, cfg, [cpu(m, cfg) for m in meshes]


@pytest.mark.parametrize("host,chunk", [(None, None), (None, "37"), ("0", "64"), ("1", None)])
def test_crowded_batch(ctx, monkeypatch, crowd, host, chunk):
    """host None: the library's own choice (device connectivity from 256 meshes on)."""
    meshes, is_bad, cfg, want = crowd
    assert 280 <= len(meshes) <= 340
    for name in ("DSA_ENC_HOST_CONN", "DSA_ENC_HOST_PLAN", "DSA_ENC_CHUNK"):
        monkeypatch.delenv(name, raising=False)
    if host is not None:
        force_path(monkeypatch, host)
    if chunk is not None:
        monkeypatch.setenv("DSA_ENC_CHUNK", chunk)
    got = repair(ctx, meshes, cfg)
    strict = level(ctx, meshes, cfg)
    failed = 0
    for i, (m, (st, g), w) in enumerate(zip(meshes, got, want)):
        if not is_bad[i]:
            assert st == 0 and g == w and strict[i] == (0, g), i
            continue
        old = cpu(m, cfg, repair=0)                                       # the level call's answer: a refusal, but for the one defect the strict
        if isinstance(old, bytes):                                        # table takes (two faces turned against each other over the same vertices)
            assert strict[i] == (0, old), i
        else:
            assert strict[i][0] != 0 and old in strict[i][1], i
        if m.per_corner:
            assert st == native.DSA_ERR_NOT_IMPLEMENTED and NOT_IMPLEMENTED in g and NOT_IMPLEMENTED in w, (i, g)
            failed += 1
        elif defects.is_degenerate(m.faces).all():
            assert st == native.DSA_ERR_INVALID_DATA and ALL_DEGENERATE in g and ALL_DEGENERATE in w, (i, g)
            failed += 1
        else:
            assert st == 0, (i, g)
            assert g == w, i
    assert failed == 2
    ok = [i for i in range(len(meshes)) if is_bad[i] and got[i][0] == 0]
    check_decodes_to_the_pin(ctx, [got[i][1] for i in ok], [meshes[i] for i in ok])


@BOTH_PATHS
def test_a_grid_with_50_defects_and_the_fan(ctx, monkeypatch, host):
    force_path(monkeypatch, host)
    rng = np.random.default_rng(3)
    pos, _, _, faces = synth.make_mesh(synth.GRID, 32, 32, 8)
    nv, f = len(pos), faces
    for k in range(50):
        nv, f = defects.inject(nv, f, defects.KINDS[k % len(defects.KINDS)], 1, rng)
    meshes = [mesh_of(defects.Defect("grid-50", nv, f, None, None)), mesh_of(defects.placed()[5])]
    for cfg in (dsa.Config(repair_topology=True), dsa.Config(repair_topology=True, multi_parallelogram=4, traversal_method=2, edgebreaker_method=2, normal_prediction=6, texcoord_prediction=5)):
        got = repair(ctx, meshes, cfg)
        for m, (st, g) in zip(meshes, got):
            assert st == 0, g
            assert g == cpu(m, cfg)
        check_decodes_to_the_pin(ctx, [g for _, g in got], meshes)


@BOTH_PATHS
def test_every_soup_encodes_and_round_trips(ctx, monkeypatch, host):
    force_path(monkeypatch, host)
    soups = defects.soups(600, seed=9)
    meshes = [mesh_of(s, k, full=k % 5 == 0) for k, s in enumerate(soups)]
    cfg = dsa.Config(repair_topology=True)
    got = repair(ctx, meshes, cfg)
    ok, refused = [], 0
    for i, (s, m, (st, g)) in enumerate(zip(soups, meshes, got)):
        if defects.is_degenerate(s.faces).all():
            assert st == native.DSA_ERR_INVALID_DATA and ALL_DEGENERATE in g
            refused += 1
            continue
        assert st == 0, (i, s.faces.tolist(), g)
        assert g == cpu(m, cfg), (i, s.faces.tolist())
        ok.append(i)
    assert len(ok) + refused == 600 and len(ok) > refused                # none is left out
    check_decodes_to_the_pin(ctx, [got[i][1] for i in ok], [meshes[i] for i in ok])


@BOTH_PATHS
def test_topology_0_is_the_level_call(ctx, monkeypatch, host):
    force_path(monkeypatch, host)
    cases = defects.named()[:6] + defects.placed()[:2]
    meshes = [mesh_of(c, k) for k, c in enumerate(cases)]
    for k in range(4):
        pos, nrm, uv, faces = synth.make_mesh(synth.GRID, 5 + k, 6, k)
        meshes.append(dsa.MeshData(pos, faces, nrm, uv))
    cfg = dsa.Config(multi_parallelogram=4, traversal_method=1)
    a, b = repair(ctx, meshes, cfg, topology=0), level(ctx, meshes, cfg)
    assert a == b
    # the strict table refuses every defective case but the mirrored pair (every half-edge once, every vertex one closed fan of two),
    # which it codes as it always did; the answers are the CPU coder's without the option
    refused = 0
    for c, m, (st, g) in zip(cases + [None] * 4, meshes, a):
        old = cpu(m, cfg, repair=0)
        if isinstance(old, bytes):
            assert c is None or c.name == "mirrored-pair"
            assert (st, g) == (0, old)
        else:
            assert st == native.DSA_ERR_INVALID_DATA and old in g            # the old refusal, word for word
            refused += 1
    assert refused == len(cases) - 1


def test_invalid_options_fail_the_call(ctx):
    L = native.lib()
    m = [mesh_of(defects.named()[1])]
    for value in (2, -1, 7):
        o = native.EncodeRepairOptions()
        L.dsa_encode_default_repair_options(C.byref(o))
        o.topology = value
        assert raw(ctx, m, o)[0] == native.DSA_ERR_INVALID_ARGUMENT
        assert "topology" in ctx.error()
    for k in (0, 6):
        o = native.EncodeRepairOptions()
        L.dsa_encode_default_repair_options(C.byref(o))
        o.reserved[k] = 1
        assert raw(ctx, m, o)[0] == native.DSA_ERR_INVALID_ARGUMENT
        assert "dsa_encode_repair_options.reserved" in ctx.error()
    o = native.EncodeRepairOptions()
    L.dsa_encode_default_repair_options(C.byref(o))
    o.topology, o.level.traversal_method = 1, 3                            # the options underneath keep their checks
    assert raw(ctx, m, o)[0] == native.DSA_ERR_INVALID_ARGUMENT
    assert "traversal_method" in ctx.error()


def test_encode_batch_routes_the_option(ctx):
    m = mesh_of(defects.named()[1])
    with pytest.raises(Exception, match="non-manifold"):
        dsa.DracoEncoder(ctx).EncodeBatch([m], dsa.Config())
    got = dsa.DracoEncoder(ctx).EncodeBatch([m], dsa.Config(repair_topology=True))
    assert got[0] == cpu(m, dsa.Config(repair_topology=True))
