"""Encode direction, the schemes stock encoders write at their default level (dsa_encode_batch_ex): valence Edgebreaker symbols,
TexCoordsPortable texture coordinates, GeometricNormal normals.  The device coder must write, byte for byte, the stream of the CPU
coder (synth.encode_mesh / encode_mesh_corners with the same schemes) on both connectivity paths, for per-vertex meshes and for
meshes with attribute seams, and the streams must round-trip through the GPU decoder."""
import ctypes as C

import numpy as np
import pytest

import encodecall
import oracle
import draco_sharp_amd as dsa
import draco_sharp_amd.synth as synth
from draco_sharp_amd import native
from meshutil import face_multiset_fast, seamed_mesh, source_corner_faces, source_corner_faces_seamed

pytestmark = pytest.mark.gpu

KINDS = (synth.GRID, synth.TORUS, synth.SPHERE, synth.HOLES, synth.TWO_PARTS)
STOCK = dict(edgebreaker_method=2, texcoord_prediction=5, normal_prediction=6)
# each scheme alone, all three together, with the option variants of the per-vertex tests
CONFIGS = [
    dsa.Config(edgebreaker_method=2),
    dsa.Config(texcoord_prediction=5),
    dsa.Config(normal_prediction=6),
    dsa.Config(**STOCK),
    dsa.Config(symbol_scheme=0, **STOCK),
    dsa.Config(symbol_scheme=1, position_prediction=0, **STOCK),
    dsa.Config(position_bits=4, texcoord_bits=4, normal_bits=4, speed=1, **STOCK),
    dsa.Config(position_bits=18, texcoord_bits=16, normal_bits=12, **STOCK),
]
SINGLE = [dsa.Config(single_connectivity=True, **STOCK), dsa.Config(single_connectivity=True, symbol_scheme=1, **STOCK)]
BOTH_PATHS = pytest.mark.parametrize("host", ["0", "1"])


@pytest.fixture(scope="module")
def ctx():
    c = dsa.Context(0)
    yield c
    c.close()


def valence_for(cfg, faces):
    m = cfg.edgebreaker_method
    return m == 2 or (m == -1 and cfg.speed < 5 and len(faces) >= 1000)


def opt_of(cfg, faces):
    return synth.options(pos_bits=cfg.position_bits, uv_bits=cfg.texcoord_bits, normal_bits=cfg.normal_bits,
                         single_connectivity=1 if cfg.single_connectivity else 0, force_scheme=cfg.symbol_scheme,
                         compression_level=10 - cfg.speed, pos_prediction=cfg.position_prediction,
                         uv_prediction=cfg.texcoord_prediction, normal_prediction=cfg.normal_prediction,
                         predictive_connectivity=2 if valence_for(cfg, faces) else 0)


def cpu(m, cfg):
    """The CPU coder's stream of MeshData m under cfg."""
    if m.per_corner:
        return synth.encode_mesh_corners(m.positions, m.faces, m.normals, m.normal_corners, m.texcoords, m.texcoord_corners,
                                         opt=opt_of(cfg, m.faces))
    return synth.encode_mesh(m.positions, m.faces, m.normals, m.texcoords, opt=opt_of(cfg, m.faces))


def raw_ex(ctx, meshes, opt):
    """(status, bytes) per mesh from dsa_encode_batch_ex; opt: an EncodeOptionsEx.  Returns (call status, list)."""
    return encodecall.call(ctx, "dsa_encode_batch_ex", meshes, opt, messages=False)


def encode(ctx, meshes, cfg):
    st, out = raw_ex(ctx, meshes, cfg._native_ex())
    assert st == 0, ctx.error()
    return out


def per_vertex_meshes(k0=0):
    out = []
    for k, kind in enumerate(KINDS):
        nx, ny = (16, 14) if kind == synth.HOLES else (9 + k + k0, 7 + 2 * k)
        pos, nrm, uv, faces = synth.make_mesh(kind, nx, ny, 30 + k + k0)
        out.append(dsa.MeshData(pos, faces, nrm, uv))
    return out


def seamed_meshes():
    out = []
    for k, kind in enumerate(KINDS):
        nx, ny = (16, 14) if kind == synth.HOLES else (10 + k, 8 + k)
        for j, (nc, uc) in enumerate(((None, "stripes"), (None, "checker"), ("island", "stripes"), ("checker", "random"))):
            out.append(seamed_mesh(synth, kind, nx, ny, 10 * k + j, normal_charts=nc, uv_charts=uc))
    return out


def corner_data(t):
    pos, faces, nrm, nid, uv, uid = t
    return dsa.MeshData(pos, faces, nrm, uv, normal_corners=nid, texcoord_corners=uid)


def force_path(monkeypatch, host):
    monkeypatch.setenv("DSA_ENC_HOST_CONN", host)
    monkeypatch.setenv("DSA_ENC_HOST_PLAN", host)


def traversal_byte(stream):
    return stream[11]       # 'DRACO', major, minor, type, method, flags (2): then the Edgebreaker traversal decoder type


@BOTH_PATHS
def test_per_vertex_matches_cpu_coder(ctx, monkeypatch, host):
    force_path(monkeypatch, host)
    meshes = per_vertex_meshes()
    for cfg in CONFIGS + SINGLE:
        got = encode(ctx, meshes, cfg)
        for m, (st, g) in zip(meshes, got):
            assert st == 0
            exp = cpu(m, cfg)
            assert g == exp
            assert traversal_byte(g) == (2 if cfg.edgebreaker_method == 2 else 0)


@BOTH_PATHS
def test_seamed_matches_cpu_coder(ctx, monkeypatch, host):
    force_path(monkeypatch, host)
    tuples = seamed_meshes()
    meshes = [corner_data(t) for t in tuples]
    for ci, cfg in enumerate(CONFIGS):
        group = meshes if ci in (2, 3) else meshes[ci % 4::4]
        got = encode(ctx, group, cfg)
        for m, (st, g) in zip(group, got):
            assert st == 0
            assert g == cpu(m, cfg)


def test_texcoords_portable_through_the_standard_entry_points(ctx):
    meshes = per_vertex_meshes()
    cfg = dsa.Config(texcoord_prediction=5)
    assert not cfg.extended
    got = dsa.DracoEncoder(ctx).EncodeBatch(meshes, cfg)
    for m, g in zip(meshes, got):
        assert g == cpu(m, cfg)
    t = seamed_meshes()[0]
    assert dsa.DracoEncoder(ctx).Encode(corner_data(t), cfg) == cpu(corner_data(t), cfg)


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
    cfg = dsa.Config(**STOCK)
    pv = per_vertex_meshes(3)
    tuples = seamed_meshes()[::3]
    sm = [corner_data(t) for t in tuples]
    got = [g for _, g in encode(ctx, pv + sm, cfg)]
    b, paths = decode_paths(ctx, got)
    _, cpu_paths = decode_paths(ctx, [cpu(m, cfg) for m in pv + sm])
    assert paths == cpu_paths
    for i, m in enumerate(pv):
        assert paths[i] == 0
        d = b.result(i).ConnectedData
        want, _ = source_corner_faces(m.positions, m.normals, m.texcoords, m.faces)
        keys = np.concatenate([np.asarray(a.PortableValues, np.int64)[np.asarray(a.PointMap, np.int64)] for a in d.Attributes], axis=1)
        assert np.array_equal(face_multiset_fast(d.Faces, keys), want)
    for j, t in enumerate(tuples):
        i = len(pv) + j
        if t[3] is None:
            assert paths[i] == 0                          # UV seams only: the wave-per-mesh kernels
        d = b.result(i).ConnectedData
        want, _ = source_corner_faces_seamed(*t)
        keys = np.concatenate([np.asarray(a.PortableValues, np.int64)[np.asarray(a.PointMap, np.int64)] for a in d.Attributes], axis=1)
        got_faces = face_multiset_fast(d.Faces, keys)
        assert got_faces.shape == want.shape and np.array_equal(got_faces, want)
    b.close()
    for i in (0, 3, len(pv) + 1):
        ref = oracle.decode(got[i])
        assert ref.faces.shape[0] == len((pv + sm)[i].faces)


def test_rule_by_speed_and_face_count(ctx):
    small_pos, small_nrm, small_uv, small_faces = synth.make_mesh(synth.GRID, 12, 10, 5)
    big_pos, big_nrm, big_uv, big_faces = synth.make_mesh(synth.TORUS, 30, 24, 6)
    assert len(small_faces) < 1000 <= len(big_faces)
    meshes = [dsa.MeshData(small_pos, small_faces, small_nrm, small_uv), dsa.MeshData(big_pos, big_faces, big_nrm, big_uv)]
    for speed, bytes_ in ((3, (0, 2)), (5, (0, 0))):
        cfg = dsa.Config(speed=speed, edgebreaker_method=-1, texcoord_prediction=5, normal_prediction=6)
        got = encode(ctx, meshes, cfg)
        for m, (st, g), tb in zip(meshes, got, bytes_):
            assert st == 0 and traversal_byte(g) == tb
            assert g == cpu(m, cfg)


def test_invalid_options_fail_the_call(ctx):
    L = native.lib()
    m = per_vertex_meshes()[:1]
    for field, value in (("edgebreaker_method", 1), ("edgebreaker_method", 3), ("normal_prediction", 5), ("normal_prediction", 1)):
        o = native.EncodeOptionsEx()
        L.dsa_encode_default_options_ex(C.byref(o))
        setattr(o, field, value)
        assert raw_ex(ctx, m, o)[0] == native.DSA_ERR_INVALID_ARGUMENT
        assert field in ctx.error()
    for field, value in (("position_prediction", 4), ("position_prediction", 2), ("texcoord_prediction", 3), ("texcoord_prediction", 6)):
        o = native.EncodeOptionsEx()
        L.dsa_encode_default_options_ex(C.byref(o))
        setattr(o.base, field, value)
        assert raw_ex(ctx, m, o)[0] == native.DSA_ERR_INVALID_ARGUMENT
        # the standard entry points refuse what they cannot write as well (instead of a method byte that does not match the data)
        arr = (native.MeshInput * 1)()
        arr[0].num_vertices, arr[0].num_faces = len(m[0].positions), len(m[0].faces)
        arr[0].positions, arr[0].faces = m[0].positions.ctypes.data, m[0].faces.ctypes.data
        h = C.c_void_p()
        assert L.dsa_encode_batch(ctx._h, 1, arr, C.byref(o.base), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT
        assert field in ctx.error()
    o = native.EncodeOptionsEx()
    L.dsa_encode_default_options_ex(C.byref(o))
    o.reserved[3] = 1
    assert raw_ex(ctx, m, o)[0] == native.DSA_ERR_INVALID_ARGUMENT


@BOTH_PATHS
def test_non_manifold_mesh_fails_alone(ctx, monkeypatch, host):
    force_path(monkeypatch, host)
    good = per_vertex_meshes()
    pos, nrm, uv, faces = synth.make_mesh(synth.GRID, 10, 8, 3)
    bad_faces = np.concatenate([faces, faces[:1]])                       # a duplicated face: non-manifold edges
    bad = dsa.MeshData(pos, bad_faces, nrm, uv)
    cfg = dsa.Config(**STOCK)
    got = encode(ctx, good[:2] + [bad] + good[2:], cfg)
    assert got[2][0] == native.DSA_ERR_INVALID_DATA
    for m, (st, g) in zip(good, got[:2] + got[3:]):
        assert st == 0 and g == cpu(m, cfg)


def test_default_device_path_at_scale(ctx, monkeypatch):
    monkeypatch.delenv("DSA_ENC_HOST_CONN", raising=False)
    monkeypatch.delenv("DSA_ENC_HOST_PLAN", raising=False)
    base = per_vertex_meshes() + [corner_data(t) for t in seamed_meshes()[:6]]
    meshes = [base[i % len(base)] for i in range(320)]
    cfg = dsa.Config(**STOCK)
    got = encode(ctx, meshes, cfg)
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 160, 319):
        assert got[i] == (0, cpu(meshes[i], cfg))


def test_bench_batch_in_the_stock_default(ctx, monkeypatch):
    monkeypatch.delenv("DSA_ENC_HOST_CONN", raising=False)
    monkeypatch.delenv("DSA_ENC_HOST_PLAN", raising=False)
    a = dsa.MeshData(*[x for x in (lambda p, n, u, f: (p, f, n, u))(*synth.make_mesh(synth.GRID, 128, 256, 1000))])
    b = dsa.MeshData(*[x for x in (lambda p, n, u, f: (p, f, n, u))(*synth.make_mesh(synth.GRID, 128, 256, 1001))])
    assert len(a.faces) == 65536
    meshes = [a if i % 2 == 0 else b for i in range(4096)]
    cfg = dsa.Config(**STOCK)
    got = dsa.DracoEncoder(ctx).EncodeBatch(meshes, cfg)
    assert got[0] == cpu(a, cfg) and got[4095] == cpu(b, cfg)
    got.close()
