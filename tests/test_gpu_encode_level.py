"""Encode direction, the levels above the default of the reference's speed ladder (dsa_encode_level_batch): MultiParallelogram /
ConstrainedMultiParallelogram in place of Parallelogram and the prediction-degree attribute order.  The device coder must write,
byte for byte, the stream of the CPU coder (synth.encode_mesh / encode_mesh_corners with pos_prediction / uv_prediction /
traversal_method set the same way) on both connectivity paths, for per-vertex meshes, meshes with attribute seams, a generic
attribute and an attribute list, and the streams must round-trip through the GPU decoder."""
import ctypes as C

import numpy as np
import pytest

import encodecall
import irregular
import oracle
import draco_sharp_amd as dsa
import draco_sharp_amd.synth as synth
from draco_sharp_amd import native
from meshutil import face_multiset_fast, seamed_mesh, source_corner_faces, source_corner_faces_seamed

pytestmark = pytest.mark.gpu

KINDS = (synth.GRID, synth.TORUS, synth.SPHERE, synth.HOLES, synth.TWO_PARTS)
STOCK = dict(edgebreaker_method=2, texcoord_prediction=5, normal_prediction=6)
# each option alone, 4 + 1, 4 + 2, 2 + 1
LEVELS = [dict(multi_parallelogram=4), dict(multi_parallelogram=2), dict(traversal_method=1), dict(traversal_method=2),
          dict(multi_parallelogram=4, traversal_method=1), dict(multi_parallelogram=4, traversal_method=2),
          dict(multi_parallelogram=2, traversal_method=1)]
# ... combined with the stock schemes, both symbol schemes, difference positions, coarse and fine quantisation
VARIANTS = [dict(), dict(STOCK), dict(symbol_scheme=0, **STOCK), dict(symbol_scheme=1, position_prediction=0, **STOCK),
            dict(position_bits=4, texcoord_bits=4, normal_bits=4, speed=1, **STOCK), dict(position_bits=18, texcoord_bits=16, normal_bits=12)]
BOTH_PATHS = pytest.mark.parametrize("host", ["0", "1"])


@pytest.fixture(scope="module")
def ctx():
    c = dsa.Context(0)
    yield c
    c.close()


def multi_for(cfg, m):
    mp = cfg.multi_parallelogram
    return (4 if cfg.speed < 2 and len(m.positions) >= 40 else 0) if mp == -1 else mp


def opt_of(cfg, m):
    mp = multi_for(cfg, m)
    valence = cfg.edgebreaker_method == 2 or (cfg.edgebreaker_method == -1 and cfg.speed < 5 and len(m.faces) >= 1000)
    return synth.options(pos_bits=cfg.position_bits, uv_bits=cfg.texcoord_bits, normal_bits=cfg.normal_bits,
                         single_connectivity=1 if cfg.single_connectivity else 0, force_scheme=cfg.symbol_scheme,
                         compression_level=10 - cfg.speed,
                         pos_prediction=mp if mp and cfg.position_prediction == 1 else cfg.position_prediction,
                         uv_prediction=mp if mp and cfg.texcoord_prediction == 1 else cfg.texcoord_prediction,
                         normal_prediction=cfg.normal_prediction, traversal_method=cfg.traversal_method,
                         predictive_connectivity=2 if valence else 0,
                         generic_components=m.generic.shape[1] if m.generic is not None else 1)


def cpu(m, cfg):
    """The CPU coder's stream of MeshData m under cfg."""
    extra = [synth.Extra(a.values, a.attribute_type, a.normalized, a.unique_id, a.quantization_bits) for a in m.attributes] or None
    if m.per_corner:
        return synth.encode_mesh_corners(m.positions, m.faces, m.normals, m.normal_corners, m.texcoords, m.texcoord_corners,
                                         opt=opt_of(cfg, m), generic=m.generic, extra=extra)
    return synth.encode_mesh(m.positions, m.faces, m.normals, m.texcoords, generic=m.generic, opt=opt_of(cfg, m), extra=extra)


def raw(ctx, meshes, opt, entry="dsa_encode_level_batch"):
    """(call status, [(status, bytes) per mesh]) from dsa_encode_level_batch (opt: an EncodeLevelOptions) or another entry point
    that takes dsa_mesh_attr_input."""
    return encodecall.call(ctx, entry, meshes, opt, messages=False)


def encode(ctx, meshes, cfg):
    st, out = raw(ctx, meshes, cfg._native_level())
    assert st == 0, ctx.error()
    return out


def check_equal(ctx, meshes, cfg):
    got = encode(ctx, meshes, cfg)
    for i, (m, (st, g)) in enumerate(zip(meshes, got)):
        assert st == 0, (i, vars(cfg))
        assert g == cpu(m, cfg), (i, vars(cfg))
    return [g for _, g in got]


def per_vertex_meshes(k0=0):
    out = []
    for k, kind in enumerate(KINDS):
        nx, ny = (16, 14) if kind == synth.HOLES else (9 + k + k0, 7 + 2 * k)
        pos, nrm, uv, faces = synth.make_mesh(kind, nx, ny, 30 + k + k0)
        out.append(dsa.MeshData(pos, faces, nrm, uv))
    return out


def seamed_tuples():
    out = []
    for k, kind in enumerate(KINDS):
        nx, ny = (16, 14) if kind == synth.HOLES else (10 + k, 8 + k)
        for j, (nc, uc) in enumerate(((None, "stripes"), (None, "checker"), ("island", "stripes"), ("checker", "random"), (None, "none"))):
            out.append(seamed_mesh(synth, kind, nx, ny, 10 * k + j, normal_charts=nc, uv_charts=uc))
    return out


def corner_data(t):
    pos, faces, nrm, nid, uv, uid = t
    return dsa.MeshData(pos, faces, nrm, uv, normal_corners=nid, texcoord_corners=uid)


def generic_meshes():
    rng = np.random.default_rng(11)
    out = []
    for k, kind in enumerate(KINDS):
        pos, nrm, uv, faces = synth.make_mesh(kind, 11 + k, 9 + k, 60 + k)
        nc = 1 + k % 4
        g = (np.round(np.concatenate([pos, uv], axis=1)[:, :nc] * 40) + rng.integers(0, 3, (len(pos), nc))).astype(np.int64) % 256
        out.append(dsa.MeshData(pos, faces, nrm if k % 2 else None, uv, generic=g))
    return out


def listed_meshes():
    rng = np.random.default_rng(12)
    out = []
    for k, kind in enumerate(KINDS):
        pos, nrm, uv, faces = synth.make_mesh(kind, 12 + k, 8 + k, 70 + k)
        joints = (np.round(pos * 300) + rng.integers(-2, 3, pos.shape)).astype(np.int16)
        uv2 = (uv * 0.5 + 0.25).astype(np.float32)
        atts = [dsa.Attribute(joints, attribute_type=4), dsa.Attribute(uv2, attribute_type=3, quantization_bits=9)]
        if k % 2:
            atts.append(dsa.Attribute((np.round(pos[:, :2] * 90000)).astype(np.int32), attribute_type=4, unique_id=40 + k))
        out.append(dsa.MeshData(pos, faces, nrm, uv, generic=(np.arange(len(pos)) % 7).astype(np.uint8) if k == 2 else None, attributes=atts))
    return out


def fan(n, closed):
    """A fan of n triangles around vertex 0 (closed: the rim returns to its start), the apex off the rim's plane."""
    ang = np.linspace(0, 2 * np.pi, n, endpoint=False) if closed else np.linspace(0, 1.7 * np.pi, n + 1)
    rim = np.stack([np.cos(ang) * (1 + 0.1 * np.sin(5 * ang)), np.sin(ang), 0.2 * np.cos(3 * ang)], axis=1)
    pos = np.concatenate([[[0, 0, 0.5]], rim]).astype(np.float32)
    r = len(rim)
    faces = np.array([[0, 1 + i, 1 + (i + 1) % r] for i in range(n)], np.uint32)
    uv = (pos[:, :2] * 0.4 + 0.5).astype(np.float32)
    return dsa.MeshData(pos, faces, None, uv)


def force_path(monkeypatch, host):
    monkeypatch.setenv("DSA_ENC_HOST_CONN", host)
    monkeypatch.setenv("DSA_ENC_HOST_PLAN", host)


def configs():
    """Every level with every variant."""
    return [dsa.Config(**lv, **var) for lv in LEVELS for var in VARIANTS]


@pytest.fixture(scope="module")
def groups():
    return dict(vertex=per_vertex_meshes(), seamed=[corner_data(t) for t in seamed_tuples()], generic=generic_meshes(), listed=listed_meshes())


@BOTH_PATHS
def test_per_vertex_matches_cpu_coder(ctx, monkeypatch, host, groups):
    force_path(monkeypatch, host)
    for cfg in configs():
        check_equal(ctx, groups["vertex"], cfg)
    for lv in LEVELS:
        for var in (dict(single_connectivity=True, **STOCK), dict(single_connectivity=True, symbol_scheme=1)):
            check_equal(ctx, groups["vertex"], dsa.Config(**lv, **var))


@BOTH_PATHS
def test_seamed_matches_cpu_coder(ctx, monkeypatch, host, groups):
    force_path(monkeypatch, host)
    for cfg in configs():
        check_equal(ctx, groups["seamed"], cfg)


@BOTH_PATHS
def test_generic_and_attribute_list_match_cpu_coder(ctx, monkeypatch, host, groups):
    force_path(monkeypatch, host)
    for cfg in configs():
        check_equal(ctx, groups["generic"] + groups["listed"], cfg)
    for lv in LEVELS:
        check_equal(ctx, groups["generic"] + groups["listed"], dsa.Config(single_connectivity=True, **lv))


@BOTH_PATHS
def test_tiny_meshes_and_fans(ctx, monkeypatch, host):
    force_path(monkeypatch, host)
    tri = dsa.MeshData(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], np.float32), np.array([[0, 1, 2]], np.uint32), None,
                       np.array([[0, 0], [1, 0], [0, 1]], np.float32))
    tp = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.3, 0.3, 1]], np.float32)
    tet = dsa.MeshData(tp, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.uint32), None, tp[:, :2].copy())
    meshes = [tri, tet, fan(200, True), fan(200, False)]
    for lv in LEVELS:
        streams = check_equal(ctx, meshes, dsa.Config(**lv))
        if lv.get("multi_parallelogram") == 4 and not lv.get("traversal_method"):
            # one triangle: no entry finds a parallelogram, the four crease lists are four zero counts in front of the wrap bounds;
            # the CPU coder's stream (equal above) carries them, the decoder reads them
            assert oracle.decode(streams[0]).faces.shape[0] == 1
            assert oracle.decode(streams[1]).faces.shape[0] == 4


def test_rule_by_speed_and_vertex_count(ctx):
    meshes = []
    for nx, ny in ((5, 6), (5, 5)):                       # cells: 6 x 7 = 42 and 6 x 6 = 36 points, either side of the rule's 40
        pos, nrm, uv, faces = synth.make_mesh(synth.GRID, nx, ny, 9)
        meshes.append(dsa.MeshData(pos, faces, nrm, uv))
    counts = [len(m.positions) for m in meshes]
    assert counts == [42, 36]
    for speed in (1, 2):
        cfg = dsa.Config(speed=speed, multi_parallelogram=-1)
        got = encode(ctx, meshes, cfg)
        for m, (st, g) in zip(meshes, got):
            assert st == 0 and g == cpu(m, cfg)
            want = 4 if speed < 2 and len(m.positions) >= 40 else 1
            four = cpu(m, dsa.Config(speed=speed, multi_parallelogram=4))
            one = cpu(m, dsa.Config(speed=speed))
            assert four != one
            assert g == (four if want == 4 else one)          # the method byte and everything behind it


@BOTH_PATHS
def test_irregular_meshes(ctx, monkeypatch, host):
    force_path(monkeypatch, host)
    meshes = []
    for c in irregular.SMALL:
        pos, nrm, uv, faces = irregular.mesh(c)
        meshes.append(dsa.MeshData(pos, faces, nrm, uv))
    check_equal(ctx, meshes, dsa.Config(multi_parallelogram=4, traversal_method=1))
    check_equal(ctx, meshes, dsa.Config(multi_parallelogram=4, traversal_method=2, **STOCK))


def test_default_device_path_at_scale(ctx, monkeypatch, groups):
    monkeypatch.delenv("DSA_ENC_HOST_CONN", raising=False)
    monkeypatch.delenv("DSA_ENC_HOST_PLAN", raising=False)
    base = groups["vertex"] + groups["seamed"][:8] + groups["generic"][:2] + groups["listed"][:3]
    meshes = [base[i % len(base)] for i in range(320)]
    for cfg in (dsa.Config(multi_parallelogram=4, traversal_method=2, **STOCK), dsa.Config(multi_parallelogram=2, traversal_method=1)):
        got = encode(ctx, meshes, cfg)
        for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 160, 319):
            assert got[i] == (0, cpu(meshes[i], cfg)), i


def test_bench_shape_on_the_device_path(ctx, monkeypatch):
    monkeypatch.setenv("DSA_ENC_HOST_CONN", "0")
    monkeypatch.delenv("DSA_ENC_HOST_PLAN", raising=False)
    meshes = []
    for seed in (1000, 1001):
        pos, nrm, uv, faces = synth.make_mesh(synth.GRID, 128, 256, seed)
        meshes.append(dsa.MeshData(pos, faces, nrm, uv))
    assert len(meshes[0].faces) == 65536
    check_equal(ctx, meshes, dsa.Config(multi_parallelogram=4, traversal_method=1))


def decode_paths(ctx, streams):
    b = dsa.Batch(ctx, streams)
    b.decode()
    out = []
    for i in range(len(streams)):
        assert b.status(i) == 0
        out.append(b.mesh_info(i).decode_path)
    return b, out


@BOTH_PATHS
def test_round_trip(ctx, monkeypatch, host):
    force_path(monkeypatch, host)
    pv = per_vertex_meshes(3)
    tuples = seamed_tuples()[::4]
    sm = [corner_data(t) for t in tuples]
    for cfg in (dsa.Config(multi_parallelogram=4, traversal_method=1, **STOCK), dsa.Config(multi_parallelogram=4), dsa.Config(multi_parallelogram=2, traversal_method=2)):
        got = [g for _, g in encode(ctx, pv + sm, cfg)]
        b, paths = decode_paths(ctx, got)
        _, cpu_paths = decode_paths(ctx, [cpu(m, cfg) for m in pv + sm])
        assert paths == cpu_paths
        for i, m in enumerate(pv):
            d = b.result(i).ConnectedData
            want, _ = source_corner_faces(m.positions, m.normals, m.texcoords, m.faces)
            keys = np.concatenate([np.asarray(a.PortableValues, np.int64)[np.asarray(a.PointMap, np.int64)] for a in d.Attributes], axis=1)
            assert np.array_equal(face_multiset_fast(d.Faces, keys), want)
        for j, t in enumerate(tuples):
            d = b.result(len(pv) + j).ConnectedData
            want, _ = source_corner_faces_seamed(*t)
            keys = np.concatenate([np.asarray(a.PortableValues, np.int64)[np.asarray(a.PointMap, np.int64)] for a in d.Attributes], axis=1)
            got_faces = face_multiset_fast(d.Faces, keys)
            assert got_faces.shape == want.shape and np.array_equal(got_faces, want)
        b.close()
        for i in (0, 3, len(pv) + 1):
            ref = oracle.decode(got[i])
            assert ref.faces.shape[0] == len((pv + sm)[i].faces)


def test_invalid_options_fail_the_call(ctx):
    L = native.lib()
    m = per_vertex_meshes()[:1]
    for field, value in (("multi_parallelogram", 1), ("multi_parallelogram", 3), ("multi_parallelogram", -2), ("multi_parallelogram", 5),
                         ("traversal_method", 3), ("traversal_method", -1)):
        o = native.EncodeLevelOptions()
        L.dsa_encode_default_level_options(C.byref(o))
        setattr(o, field, value)
        assert raw(ctx, m, o)[0] == native.DSA_ERR_INVALID_ARGUMENT
        assert field in ctx.error()
    for k in (0, 5):
        o = native.EncodeLevelOptions()
        L.dsa_encode_default_level_options(C.byref(o))
        o.reserved[k] = 1
        assert raw(ctx, m, o)[0] == native.DSA_ERR_INVALID_ARGUMENT
        assert "dsa_encode_level_options.reserved" in ctx.error()
    o = native.EncodeLevelOptions()
    L.dsa_encode_default_level_options(C.byref(o))
    o.ex.reserved[2] = 1
    assert raw(ctx, m, o)[0] == native.DSA_ERR_INVALID_ARGUMENT
    assert "dsa_encode_options_ex.reserved" in ctx.error()
    o = native.EncodeLevelOptions()
    L.dsa_encode_default_level_options(C.byref(o))
    o.ex.base.position_prediction = 4                        # the method ids of the options underneath stay what they were
    assert raw(ctx, m, o)[0] == native.DSA_ERR_INVALID_ARGUMENT
    assert "position_prediction" in ctx.error()


@BOTH_PATHS
def test_non_manifold_mesh_fails_alone(ctx, monkeypatch, host):
    force_path(monkeypatch, host)
    good = per_vertex_meshes()
    pos, nrm, uv, faces = synth.make_mesh(synth.GRID, 10, 8, 3)
    bad = dsa.MeshData(pos, np.concatenate([faces, faces[:1]]), nrm, uv)      # a duplicated face: non-manifold edges
    cfg = dsa.Config(multi_parallelogram=4, traversal_method=1, **STOCK)
    got = encode(ctx, good[:2] + [bad] + good[2:], cfg)
    assert got[2][0] == native.DSA_ERR_INVALID_DATA
    for m, (st, g) in zip(good, got[:2] + got[3:]):
        assert st == 0 and g == cpu(m, cfg)


@pytest.fixture(scope="module")
def mixed():
    """Meshes whose differences meet inside one chunk: either side of the valence rule (1000 faces) and of the multi-parallelogram
    rule (40 points), attribute seams, an attribute list, a closed fan."""
    pos, nrm, uv, faces = synth.make_mesh(synth.GRID, 23, 22, 5)
    big = dsa.MeshData(pos, faces, nrm, uv)
    small = []
    for nx, ny in ((5, 6), (5, 5)):
        pos, nrm, uv, faces = synth.make_mesh(synth.GRID, nx, ny, 9)
        small.append(dsa.MeshData(pos, faces, nrm, uv))
    meshes = [big, per_vertex_meshes()[1], small[0], small[1], corner_data(seamed_tuples()[2]), listed_meshes()[0], fan(50, True)]
    assert len(big.faces) >= 1000 > len(meshes[1].faces) and len(small[0].positions) >= 40 > len(small[1].positions)
    assert len(meshes[5].attributes) == 2
    return meshes


@BOTH_PATHS
@pytest.mark.parametrize("chunk", [None, "3"])
@pytest.mark.parametrize("traversal", [0, 2])
def test_mixed_meshes_in_one_chunk(ctx, monkeypatch, host, chunk, traversal, mixed):
    """The per-mesh conditions of the arena layout interleaved in one batch, in one chunk and in chunks of three, with a mesh that
    fails its checks in the middle: every other stream is the CPU coder's."""
    force_path(monkeypatch, host)
    if chunk is None:
        monkeypatch.delenv("DSA_ENC_CHUNK", raising=False)
    else:
        monkeypatch.setenv("DSA_ENC_CHUNK", chunk)
    bad_faces = mixed[1].faces.copy()
    bad_faces[3, 1] = len(mixed[1].positions) + 4
    bad = dsa.MeshData(mixed[1].positions, bad_faces, mixed[1].normals, mixed[1].texcoords)
    meshes = mixed[:4] + [bad] + mixed[4:]
    cfg = dsa.Config(speed=1, edgebreaker_method=-1, multi_parallelogram=-1, traversal_method=traversal)
    assert [multi_for(cfg, m) for m in mixed[:4]] == [4, 4, 4, 0]
    got = encode(ctx, meshes, cfg)
    assert got[4] == (native.DSA_ERR_INVALID_DATA, None)
    for i, (m, (st, g)) in enumerate(zip(meshes, got)):
        if i != 4:
            assert st == 0 and g == cpu(m, cfg), i


@BOTH_PATHS
def test_both_options_off_is_the_attributes_entry_point(ctx, monkeypatch, host, groups):
    force_path(monkeypatch, host)
    meshes = groups["vertex"] + groups["seamed"][:4] + groups["listed"]
    for cfg in (dsa.Config(), dsa.Config(**STOCK)):
        assert not cfg.leveled
        st, level = raw(ctx, meshes, cfg._native_level())
        st2, plain = raw(ctx, meshes, cfg._native_ex(), entry="dsa_encode_attributes_batch")
        assert st == 0 and st2 == 0
        assert level == plain
        assert all(s == 0 for s, _ in level)


def test_encode_batch_routes_leveled_configs(ctx, groups):
    cfg = dsa.Config(multi_parallelogram=4, traversal_method=1)
    assert cfg.leveled
    meshes = groups["vertex"][:2] + groups["seamed"][:1] + groups["listed"][:1]
    got = dsa.DracoEncoder(ctx).EncodeBatch(meshes, cfg)
    for m, g in zip(meshes, got):
        assert g == cpu(m, cfg)
    with pytest.raises(ValueError):
        dsa.DracoEncoder(ctx).EncodeBatch([dsa.PointCloudData(meshes[0].positions)], cfg)
