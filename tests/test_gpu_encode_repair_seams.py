"""Encode direction, attributes given per corner over meshes whose topology needs the repair (dsa_encode_seam_repair_batch with
corner_repair = 1; Config(repair_topology=True, repair_seams=True)): the streams byte for byte against the CPU coder with
repair_topology = 2 and its refusals word for word, on both connectivity paths (DSA_ENC_HOST_CONN) and, for meshes given as one
row per point, both weld paths (DSA_ENC_HOST_WELD); narrow and wide ids; a crowded batch over several chunks in which every mesh
gives its own bytes or its own refusal; many defects in one mesh; and the decode of what was written against the pin of
tests/seamdefects.py and the oracle."""
import ctypes as C

import numpy as np
import pytest

import encodecall
import defects
import draco_sharp_amd as dsa
import draco_sharp_amd.synth as synth
import meshutil
import oracle
import seamdefects as sd
import weldcases
from draco_sharp_amd import native
from test_gpu_encode_points import LEVELS as POINT_LEVELS, opt_of

pytestmark = pytest.mark.gpu

LEVELS = [dict()] + [kw for kw in POINT_LEVELS if not kw.get("single_connectivity")]      # (single_connectivity with ids stays refused)
CONN = pytest.mark.parametrize("conn_host", ["0", "1"])


@pytest.fixture(scope="module")
def ctx():
    c = dsa.Context(0)
    yield c
    c.close()


def force_paths(monkeypatch, weld_host, conn_host, chunk=None):
    for name, value in (("DSA_ENC_HOST_WELD", weld_host), ("DSA_ENC_HOST_CONN", conn_host), ("DSA_ENC_HOST_PLAN", conn_host), ("DSA_ENC_CHUNK", chunk)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


def mesh_of(m):
    """dsa.MeshData of a seamdefects.Seamed (ids past their rows go in behind MeshData's own check: the library is asked)"""
    out = dsa.MeshData(m.pos, m.faces, m.nrm, m.uv)
    out.normal_corners = None if m.nid is None else np.ascontiguousarray(m.nid, np.uint32).reshape(-1, 3)
    out.texcoord_corners = None if m.uid is None else np.ascontiguousarray(m.uid, np.uint32).reshape(-1, 3)
    return out


def cfg_of(weld=False, **kw):
    return dsa.Config(repair_topology=True, repair_seams=True, weld_points=weld, **kw)


def cpu(m, cfg, value=2):
    """The CPU coder's stream of MeshData m (corner form, or per point under cfg.weld_points), or the text of its refusal."""
    o = opt_of(cfg, m)
    o.repair_topology = value
    try:
        if cfg.weld_points:
            return synth.encode_mesh_points(m.positions, m.faces, m.normals, m.texcoords, opt=o)
        return synth.encode_mesh_corners(m.positions, m.faces, m.normals, m.normal_corners, m.texcoords, m.texcoord_corners, opt=o)
    except RuntimeError as e:
        return str(e)


def encode(ctx, meshes, cfg, corner_repair=1, entry="dsa_encode_seam_repair_batch"):
    """[(status, bytes or the refusal's text) per mesh] through the new call (or dsa_encode_grid_batch with the same grid options)"""
    so = native.EncodeSeamRepairOptions()
    native.lib().dsa_encode_default_seam_repair_options(C.byref(so))
    so.grid.repair = cfg._native_repair()
    so.grid.weld_points = 1 if cfg.weld_points else 0
    so.corner_repair = corner_repair
    st, out = encodecall.call(ctx, entry, meshes, so if entry == "dsa_encode_seam_repair_batch" else so.grid, grids=None)
    assert st == 0, ctx.error()
    return out


def same(names, got, want):
    for name, (st, g), w in zip(names, got, want):
        if isinstance(w, str):
            assert st != 0 and w in g, (name, g, w)
        else:
            assert st == 0, (name, g)
            assert g == w, (name, "bytes differ")


def point_pin(m):
    """the pin of a MeshData given as one row per point: its faces that are not degenerate over its quantised rows"""
    return meshutil.source_corner_faces(m.positions, m.normals, m.texcoords, m.faces[~defects.is_degenerate(m.faces)])[0]


def round_trip(ctx, streams, sources):
    """The GPU decoder on what was written: the face multiset of quantised corner values against the pin (of a seamdefects.Seamed,
    or of a MeshData given per point) and against the oracle."""
    b = dsa.Batch(ctx, streams)
    b.decode()
    for i, (s, m) in enumerate(zip(streams, sources)):
        name = getattr(m, "name", i)
        assert b.status(i) == 0, name
        d = b.result(i).ConnectedData
        keys = np.concatenate([x.PortableValues[x.PointMap] if len(x.PointMap) else x.PortableValues for x in d.Attributes], axis=1)
        have = meshutil.face_multiset_fast(d.Faces, keys)
        want = sd.pin(m)[0] if isinstance(m, sd.Seamed) else point_pin(m)
        assert have.shape == want.shape and (have == want).all(), name
        o = oracle.decode(s)
        ref = defects.decoded(o.faces, [(a.portable, a.point_map) for a in o.attributes])
        assert np.array_equal(have, ref), name
    b.close()


SMALL = [sd.with_ids(c, kind, j) for c in defects.named() + defects.placed() for j, kind in enumerate(sd.ID_KINDS)]      # 2 - 18 faces, and fan-300-face-doubled


@CONN
def test_small_shapes_over_the_levels(ctx, monkeypatch, conn_host):
    force_paths(monkeypatch, None, conn_host)
    meshes = [mesh_of(m) for m in SMALL]
    for kw in LEVELS:
        cfg = cfg_of(**kw)
        got = encode(ctx, meshes, cfg)
        want = [cpu(m, cfg) for m in meshes]
        assert not any(isinstance(w, str) for w in want), kw
        same([m.name for m in SMALL], got, want)
        round_trip(ctx, [g for _, g in got], SMALL)


def twenty_faces(rows):
    """grid-face-doubled behind a degenerate face: 20 faces, the UV ids one row per corner at the top of `rows` rows"""
    c = next(c for c in defects.named() if c.name == "grid-face-doubled")
    faces = np.concatenate([[[3, 3, 4]], c.faces]).astype(np.uint32)
    assert len(faces) == 20
    m = sd.with_ids(c._replace(faces=faces), "stripes")
    uv = np.random.default_rng(rows).random((rows, 2)).astype(np.float32)
    uid = (rows - 1 - np.arange(60, dtype=np.uint32)).reshape(20, 3)
    return m._replace(name="20-faces-%d-uv-rows" % rows, uv=uv, uid=uid)


@CONN
def test_wide_and_narrow_ids(ctx, monkeypatch, conn_host):
    """70 000 UV rows: the smallest shape on the u32 path of k_enc_repair_ids and the layout; 60 000 (and 65 536): u16."""
    force_paths(monkeypatch, None, conn_host)
    sources = [twenty_faces(70000), twenty_faces(60000), twenty_faces(65536), twenty_faces(65537)]
    meshes = [mesh_of(m) for m in sources]
    cfg = cfg_of()
    got = encode(ctx, meshes, cfg)
    same([m.name for m in sources], got, [cpu(m, cfg) for m in meshes])
    round_trip(ctx, [g for _, g in got], sources)


def crowded():
    """About 300 meshes: clean seamed, defective seamed, defective per vertex, all-degenerate, and one with an id out of range."""
    srcs = (("grid", synth.GRID, 6, 5), ("torus", synth.TORUS, 9, 8), ("holes", synth.HOLES, 14, 12))
    clean = [sd.seamed_source(synth, name, kind, nx, ny, sd.CHARTS[j], 4 + j) for j in range(len(sd.CHARTS)) for name, kind, nx, ny in srcs]
    broken = [sd.inject(m, defects.KINDS[k % 6], 1 + 4 * (k % 2), np.random.default_rng(50 + k)) for k, m in enumerate(clean + clean)]
    per_vertex = []
    for k, c in enumerate(defects.named() + defects.placed()[:5]):
        pos, nrm, uv, _, _ = defects.attributes(c.nv, k)
        per_vertex.append(sd.Seamed(c.name, pos, c.faces, nrm, None, uv, None))
    all_deg = sd.with_ids(defects.ALL_DEGENERATE, "corner")._replace(name="all-degenerate")
    bad = broken[3]._replace(name="id-out-of-range", uid=np.where(np.arange(broken[3].uid.size).reshape(-1, 3) == 11, len(broken[3].uv), broken[3].uid).astype(np.uint32))
    pool = [clean, broken, SMALL, per_vertex]
    out = []
    for k in range(300):
        if k == 150:
            out.append(("bad", bad))
        elif k % 23 == 7:
            out.append(("degenerate", all_deg))
        else:
            p = pool[k % 4]
            out.append((("clean", "broken", "small", "vertex")[k % 4], p[(k // 4) % len(p)]))
    return out


@pytest.fixture(scope="module")
def crowd():
    tagged = crowded()
    cfg = cfg_of()
    meshes, memo = {}, {}
    for _, m in tagged:
        if id(m) not in meshes:
            meshes[id(m)] = mesh_of(m)
            memo[id(m)] = cpu(meshes[id(m)], cfg)
    return tagged, [meshes[id(m)] for _, m in tagged], [memo[id(m)] for _, m in tagged], cfg


@pytest.mark.parametrize("conn_host", [None, "1"])
def test_crowded_batch_over_several_chunks(ctx, monkeypatch, crowd, conn_host):
    """None: the library's own choice (device connectivity from 256 meshes on).  Every mesh its own bytes or its own refusal; the
    clean ones byte for byte those of dsa_encode_grid_batch."""
    tagged, meshes, want, cfg = crowd
    force_paths(monkeypatch, None, conn_host, "37")
    got = encode(ctx, meshes, cfg)
    same(["%d:%s:%s" % (i, t, m.name) for i, (t, m) in enumerate(tagged)], got, want)
    old = encode(ctx, meshes, cfg, entry="dsa_encode_grid_batch")
    off = encode(ctx, meshes, cfg, corner_repair=0)
    assert old == off                                # corner_repair = 0 is dsa_encode_grid_batch: the same bytes and the same messages
    seen, refused_before = set(), 0
    for (tag, m), (st, g), w, (st0, g0) in zip(tagged, got, want, old):
        seen.add(tag)
        if tag in ("clean", "vertex"):
            assert st == st0 == 0 and g == g0, m.name
        elif tag == "degenerate":
            assert st == native.DSA_ERR_INVALID_DATA and "all triangles are degenerate" in g, (m.name, g)
            assert st0 == native.DSA_ERR_NOT_IMPLEMENTED and "not implemented" in g0, (m.name, g0)      # (the old call refuses the ids before it looks at the faces)
        elif tag == "bad":
            assert st == st0 == native.DSA_ERR_INVALID_DATA and "texture coordinate id out of range" in g and g == g0, (m.name, g)
        elif tag in ("broken", "small"):             # (a pinch of a vertex onto itself leaves a mesh clean: then the old call codes it too)
            assert st == 0 and ((st0 == 0 and g0 == g) or (st0 == native.DSA_ERR_NOT_IMPLEMENTED and "not implemented" in g0)), (m.name, g0)
            refused_before += st0 != 0
    assert seen == {"clean", "broken", "small", "vertex", "degenerate", "bad"} and refused_before > 100
    assert sum(1 for w in want if isinstance(w, str)) == sum(1 for t, _ in tagged if t in ("degenerate", "bad"))
    coded = [k for k, (st, _) in enumerate(got) if st == 0]
    round_trip(ctx, [got[k][1] for k in coded], [tagged[k][1] for k in coded])


@CONN
def test_many_defects_in_one_mesh(ctx, monkeypatch, conn_host):
    force_paths(monkeypatch, None, conn_host)
    m = sd.seamed_source(synth, "grid-32x32", synth.GRID, 32, 32, ("checker", "stripes"), 9)
    rng = np.random.default_rng(32)
    for kind, count in zip(defects.KINDS, (9, 9, 8, 8, 8, 8)):      # 50 in all
        m = sd.inject(m, kind, count, rng)
    mesh = mesh_of(m)
    for kw in (dict(), LEVELS[3]):
        cfg = cfg_of(**kw)
        (st, g), = encode(ctx, [mesh], cfg)
        assert st == 0, g
        assert g == cpu(mesh, cfg), kw
        round_trip(ctx, [g], [m])


@pytest.mark.parametrize("weld_host,conn_host", [("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")])
def test_one_row_per_point(ctx, monkeypatch, weld_host, conn_host):
    force_paths(monkeypatch, weld_host, conn_host)
    c = next(c for c in weldcases.cases() if c.name == "two-sided-sheet-two-normals")
    sheet = dsa.MeshData(c.pos, c.faces, c.normals, c.uvs)
    cfg = cfg_of(weld=True)
    want = synth.encode_mesh_points(c.pos, c.faces, c.normals, c.uvs, opt=synth.options(repair_topology=2))
    assert sd.header_counts(want) == (40, 48)
    (st, g), = encode(ctx, [sheet], cfg)
    assert st == 0, g
    assert g == want
    round_trip(ctx, [g], [sheet])
    # without the switch: today's refusal, through the new call and through the old one
    for kw in (dict(corner_repair=0), dict(entry="dsa_encode_grid_batch")):
        (st, g), = encode(ctx, [sheet], cfg, **kw)
        assert st == native.DSA_ERR_NOT_IMPLEMENTED and "not implemented" in g, g
    # defective seamed meshes unwelded into one row per point, over the levels
    sources, points = [], []
    for k, (name, kind, nx, ny) in enumerate((("grid", synth.GRID, 6, 5), ("torus", synth.TORUS, 9, 8), ("holes", synth.HOLES, 14, 12))):
        for j in (k, k + 2):
            m = sd.inject(sd.seamed_source(synth, name, kind, nx, ny, sd.CHARTS[j], 4 + j), defects.KINDS[(k + j) % 4], 3, np.random.default_rng(70 + k + j))
            p, f, n, u = weldcases.unweld(m.pos, m.faces, m.nrm, m.nid, m.uv, m.uid, np.random.default_rng(80 + k + j))
            sources.append(m)
            points.append(dsa.MeshData(p, f, n, u))
    for kw in LEVELS:
        cfg = cfg_of(weld=True, **kw)
        got = encode(ctx, points, cfg)
        same([m.name for m in sources], got, [cpu(p, cfg) for p in points])
        round_trip(ctx, [g for _, g in got], points)


def test_encode_batch_routes_and_raises(ctx, monkeypatch):
    force_paths(monkeypatch, None, None)
    m = SMALL[31]
    mesh = mesh_of(m)
    enc = dsa.DracoEncoder(ctx)
    assert enc.EncodeBatch([mesh], cfg_of())[0] == cpu(mesh, cfg_of())
    with pytest.raises(Exception, match="not implemented"):
        enc.EncodeBatch([mesh], dsa.Config(repair_topology=True))
    got = enc.TryEncodeBatch([mesh, mesh_of(sd.with_ids(defects.ALL_DEGENERATE, "corner"))], cfg_of())
    assert isinstance(got[0], bytes) and "all triangles are degenerate" in str(got[1])
