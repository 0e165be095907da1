"""Encode direction, attributes given per corner (dsa_encode_batch_corners): normals and texture coordinates with their own row
ids per face corner become attribute seams (seam bits, the attribute's own corner table and order, corner attributes).  The
device coder must write, byte for byte, the stream of the CPU coder (synth.encode_mesh_corners) on both connectivity paths,
round-trip through the GPU decoder's wave-per-mesh kernels, and fail mesh by mesh where the CPU coder refuses."""
import os

import numpy as np
import pytest

import encodecall
import oracle
import draco_sharp_amd as dsa
import draco_sharp_amd.synth as synth
from draco_sharp_amd import native
from draco_sharp_amd.decoder import InvalidDataException
from meshutil import chart_of_faces, face_multiset_fast, seamed_mesh, source_corner_faces_seamed, split_by_chart

pytestmark = pytest.mark.gpu

PATTERNS = ("stripes", "island", "checker", "random", "single", "none")
KINDS = (synth.GRID, synth.TORUS, synth.SPHERE, synth.HOLES, synth.TWO_PARTS)
# the option variants of test_gpu_encode.CASES that corner ids allow (single_connectivity = 1 is refused with ids)
CONFIGS = [
    dsa.Config(),
    dsa.Config(symbol_scheme=0),
    dsa.Config(symbol_scheme=1, position_prediction=0, texcoord_prediction=0),
    dsa.Config(position_bits=16, texcoord_bits=14, normal_bits=10),
    dsa.Config(position_bits=4, texcoord_bits=4, normal_bits=4, speed=1),
    dsa.Config(speed=9),
]


@pytest.fixture(scope="module")
def ctx():
    c = dsa.Context(0)
    yield c
    c.close()


def opt_of(cfg, **kw):
    return synth.options(pos_bits=cfg.position_bits, uv_bits=cfg.texcoord_bits, normal_bits=cfg.normal_bits,
                         single_connectivity=1 if cfg.single_connectivity else 0, force_scheme=cfg.symbol_scheme,
                         compression_level=10 - cfg.speed, pos_prediction=cfg.position_prediction, uv_prediction=cfg.texcoord_prediction, **kw)


def cpu(mesh, cfg):
    pos, faces, nrm, nid, uv, uid = mesh
    return synth.encode_mesh_corners(pos, faces, nrm, nid, uv, uid, opt=opt_of(cfg))


def data(mesh):
    pos, faces, nrm, nid, uv, uid = mesh
    return dsa.MeshData(pos, faces, nrm, uv, normal_corners=nid, texcoord_corners=uid)


def raw_encode(ctx, meshes, cfg=None, corners=True):
    """(status, bytes) per mesh straight from the C-ABI: a failure stays with its mesh."""
    def edit(arr, keep):
        for i, m in enumerate(meshes):
            if hasattr(m, "generic_components_override"):
                (arr[i].mesh if corners else arr[i]).generic_components = m.generic_components_override
    st, out = encodecall.call(ctx, "dsa_encode_batch_corners" if corners else "dsa_encode_batch", meshes, (cfg or dsa.Config())._native(), edit=edit, messages=False)
    assert st == 0, ctx.error()
    return out


def check_round_trip(ctx, streams, meshes, cfg):
    b = dsa.Batch(ctx, streams)
    b.decode()
    for i, (pos, faces, nrm, nid, uv, uid) in enumerate(meshes):
        assert b.status(i) == 0
        assert b.mesh_info(i).decode_path == 0
        m = b.result(i).ConnectedData
        want, _ = source_corner_faces_seamed(pos, faces, nrm, nid, uv, uid, cfg.position_bits, cfg.normal_bits, cfg.texcoord_bits)
        keys = np.concatenate([np.asarray(a.PortableValues, np.int64)[np.asarray(a.PointMap, np.int64)] for a in m.Attributes], axis=1)
        got = face_multiset_fast(m.Faces, keys)
        assert got.shape == want.shape and np.array_equal(got, want)
    b.close()


def matrix():
    out = []
    for k, kind in enumerate(KINDS):
        nx, ny = (16, 14) if kind == synth.HOLES else (10 + k, 8 + k)
        for j, pat in enumerate(PATTERNS):
            out.append(seamed_mesh(synth, kind, nx, ny, 10 * k + j, normal_charts=None, uv_charts=pat))
            out.append(seamed_mesh(synth, kind, nx, ny, 10 * k + j, normal_charts=pat, uv_charts=None))
            out.append(seamed_mesh(synth, kind, nx, ny, 10 * k + j, normal_charts=pat, uv_charts=PATTERNS[(j + 2) % len(PATTERNS)]))
    return out


@pytest.mark.parametrize("host_conn", ["0", "1"])
def test_matrix_matches_cpu_coder_and_round_trips(ctx, monkeypatch, host_conn):
    monkeypatch.setenv("DSA_ENC_HOST_CONN", host_conn)
    meshes = matrix()
    for ci, cfg in enumerate(CONFIGS):
        group = meshes if ci == 0 else meshes[ci::7]
        ok, refused = [], []
        for m in group:
            try:
                ok.append((m, cpu(m, cfg)))
            except RuntimeError as e:
                refused.append((m, str(e)))
        got = raw_encode(ctx, [data(m) for m, _ in ok] + [data(m) for m, _ in refused], cfg)
        for (m, exp), (st, g) in zip(ok, got):
            assert st == 0 and g == exp
        for (m, why), (st, g) in zip(refused, got[len(ok):]):
            assert st == 1, why
        if ci in (0, 2, 4):
            check_round_trip(ctx, [g for _, g in got[:len(ok)]], [m for m, _ in ok], cfg)


def test_bench_size_batch_on_the_default_path(ctx, monkeypatch):
    monkeypatch.delenv("DSA_ENC_HOST_CONN", raising=False)
    base = [seamed_mesh(synth, synth.GRID, 128, 256, s, normal_charts=None if s % 2 else "checker", uv_charts="stripes") for s in range(4)]
    meshes = [base[i % 4] for i in range(256)]
    got = dsa.DracoEncoder(ctx).EncodeBatch([data(m) for m in meshes])
    for i in (0, 1, 2, 3, 129, 255):
        assert got[i] == cpu(meshes[i], dsa.Config())
    check_round_trip(ctx, [got[i] for i in range(4)], base, dsa.Config())


@pytest.mark.parametrize("host_conn", ["0", "1"])
def test_mixed_batch(ctx, monkeypatch, host_conn):
    monkeypatch.setenv("DSA_ENC_HOST_CONN", host_conn)
    meshes, plain = [], []
    for s in range(12):
        kind = KINDS[s % len(KINDS)]
        if s % 3 == 0:
            pos, nrm, uv, faces = synth.make_mesh(kind, 12, 10, s)
            meshes.append(dsa.MeshData(pos, faces, nrm, uv))
            plain.append(len(meshes) - 1)
        else:
            meshes.append(data(seamed_mesh(synth, kind, 12, 10, s, normal_charts="island" if s % 2 else None, uv_charts="stripes")))
    got = raw_encode(ctx, meshes)
    per_vertex = raw_encode(ctx, [meshes[i] for i in plain], corners=False)
    for k, i in enumerate(plain):
        assert got[i][0] == 0 and got[i][1] == per_vertex[k][1]
    for i, m in enumerate(meshes):
        if i in plain:
            continue
        exp = synth.encode_mesh_corners(m.positions, m.faces, m.normals, m.normal_corners, m.texcoords, m.texcoord_corners)
        assert got[i] == (0, exp)


def house04_corners():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "house_04.obj.drc"), "rb") as f:
        m = oracle.decode(f.read())
    P, U, G = m.attributes
    assert np.array_equal(P.point_map, G.point_map)            # the generic attribute is per position vertex
    faces = P.point_map[m.faces].astype(np.uint32)
    uid = U.point_map[m.faces].astype(np.uint32)
    return m, P.values, faces, U.values, uid, G.values


@pytest.mark.parametrize("host_conn", ["0", "1"])
def test_house_04_in_corner_form(ctx, monkeypatch, host_conn):
    monkeypatch.setenv("DSA_ENC_HOST_CONN", host_conn)
    m, pos, faces, uv, uid, gen = house04_corners()
    opt = synth.options(generic_components=1)
    exp = synth.encode_mesh_corners(pos, faces, uvs=uv, uv_corners=uid, generic=gen, opt=opt)
    got = dsa.DracoEncoder(ctx).Encode(dsa.MeshData(pos, faces, texcoords=uv, generic=gen, texcoord_corners=uid))
    assert got == exp
    per_point = synth.encode_mesh(pos[m.attributes[0].point_map], m.faces, None, uv[m.attributes[1].point_map],
                                  generic=gen[m.attributes[2].point_map], opt=opt)
    assert len(got) < len(per_point)
    b = dsa.Batch(ctx, [got])
    b.decode()
    assert b.status(0) == 0 and b.mesh_info(0).decode_path == 0
    d = b.result(0).ConnectedData
    want, _ = source_corner_faces_seamed(pos, faces, None, None, uv, uid)
    keys = np.concatenate([np.asarray(a.PortableValues, np.int64)[np.asarray(a.PointMap, np.int64)] for a in d.Attributes[:2]], axis=1)
    assert np.array_equal(face_multiset_fast(d.Faces, keys), want)
    b.close()


@pytest.mark.parametrize("host_conn", ["0", "1"])
def test_checker_grid_is_refused_per_point_and_coded_per_corner(ctx, monkeypatch, host_conn):
    monkeypatch.setenv("DSA_ENC_HOST_CONN", host_conn)
    pos, nrm, uv, faces = synth.make_mesh(synth.GRID, 128, 256, 7)
    uid, rows = split_by_chart(faces, uv, chart_of_faces(pos, faces, "checker"), [1.25, 0.5])
    # per point: one point per (vertex, uv row) in use -- the charts touch at single vertices, which become non-manifold
    key = faces.astype(np.int64) * len(rows) + uid
    uniq, inv = np.unique(key.ravel(), return_inverse=True)
    pfaces = inv.reshape(faces.shape).astype(np.uint32)
    st = raw_encode(ctx, [dsa.MeshData(pos[uniq // len(rows)], pfaces, None, rows[uniq % len(rows)])], corners=False)
    assert st[0][0] == 1
    mesh = (pos, faces, None, None, rows, uid)
    got = dsa.DracoEncoder(ctx).Encode(data(mesh))
    assert got == cpu(mesh, dsa.Config())
    check_round_trip(ctx, [got], [mesh], dsa.Config())


@pytest.mark.parametrize("host_conn", ["0", "1"])
def test_failures_stay_with_their_mesh(ctx, monkeypatch, host_conn):
    monkeypatch.setenv("DSA_ENC_HOST_CONN", host_conn)
    good = [data(seamed_mesh(synth, synth.TORUS, 10, 8, s, normal_charts="checker", uv_charts="stripes")) for s in range(3)]
    bad_id = data(seamed_mesh(synth, synth.GRID, 10, 8, 5, uv_charts="stripes"))
    bad_id.texcoord_corners = bad_id.texcoord_corners.copy()
    bad_id.texcoord_corners[4, 1] = len(bad_id.texcoords)                 # a row id == its row count (past MeshData's check)
    bad_gen = data(seamed_mesh(synth, synth.GRID, 10, 8, 6, uv_charts="stripes"))
    bad_gen.generic = np.zeros((len(bad_gen.positions), 1), np.uint8)
    bad_gen.generic_components_override = 5
    got = raw_encode(ctx, [good[0], bad_id, good[1], bad_gen, good[2]])
    assert got[1][0] == 1 and got[3][0] == 3
    for i, g in ((0, good[0]), (2, good[1]), (4, good[2])):
        assert got[i][0] == 0
        assert got[i][1] == synth.encode_mesh_corners(g.positions, g.faces, g.normals, g.normal_corners, g.texcoords, g.texcoord_corners)
    single = raw_encode(ctx, good[:2], dsa.Config(single_connectivity=True))
    assert [s for s, _ in single] == [1, 1]
    with pytest.raises(InvalidDataException, match="single_connectivity"):
        dsa.DracoEncoder(ctx).Encode(good[0], dsa.Config(single_connectivity=True))
