"""Encode direction, meshes given as one row per point (dsa_weld_batch, dsa_encode_points_batch): the weld kernels of
dsa_encode_weld.h against the numpy pin of tests/weldcases.py, the streams byte for byte against the CPU coder
(synth.encode_mesh_points) with its refusals word for word, on both weld paths (DSA_ENC_HOST_WELD) and both connectivity paths
(DSA_ENC_HOST_CONN); a crowded batch in which every fifth mesh is bad and fails alone; a bench-size seamed mesh; several chunks;
the level options and the topology repair on the welded table; and the decode of what was written."""
import ctypes as C

import numpy as np
import pytest

import encodecall
import draco_sharp_amd as dsa
import draco_sharp_amd.synth as synth
import irregular
import meshutil
import weldcases
from draco_sharp_amd import native

pytestmark = pytest.mark.gpu

CASES = weldcases.cases()
CODED = [c for c in CASES if not c.weld_only]
PATHS = pytest.mark.parametrize("weld_host,conn_host", [("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")])
CORNER_IDS = "per-point input takes no corner ids"


@pytest.fixture(scope="module")
def ctx():
    c = dsa.Context(0)
    yield c
    c.close()


def force_paths(monkeypatch, weld_host, conn_host):
    for name, value in (("DSA_ENC_HOST_WELD", weld_host), ("DSA_ENC_HOST_CONN", conn_host), ("DSA_ENC_HOST_PLAN", conn_host)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    monkeypatch.delenv("DSA_ENC_CHUNK", raising=False)


def mesh_of(c):
    return dsa.MeshData(c.pos, c.faces, c.normals, c.uvs, generic=c.generic,
                        attributes=[dsa.Attribute(e, attribute_type=2, normalized=True) for e in c.extra])


def opt_of(cfg, m):
    mp = cfg.multi_parallelogram
    return synth.options(pos_bits=cfg.position_bits, uv_bits=cfg.texcoord_bits, normal_bits=cfg.normal_bits,
                         single_connectivity=1 if cfg.single_connectivity else 0, force_scheme=cfg.symbol_scheme,
                         compression_level=10 - cfg.speed,
                         pos_prediction=mp if mp and cfg.position_prediction == 1 else cfg.position_prediction,
                         uv_prediction=mp if mp and cfg.texcoord_prediction == 1 else cfg.texcoord_prediction,
                         normal_prediction=cfg.normal_prediction, traversal_method=cfg.traversal_method,
                         predictive_connectivity=2 if cfg.edgebreaker_method == 2 else 0,
                         generic_components=m.generic.shape[1] if m.generic is not None else 1, repair_topology=1 if cfg.repair_topology else 0)


def cpu(m, cfg):
    """The CPU coder's stream of per-point MeshData m, or the text of its refusal."""
    if m.per_corner:
        return CORNER_IDS
    extra = [synth.Extra(a.values, a.attribute_type, a.normalized, a.unique_id, a.quantization_bits) for a in m.attributes] or None
    try:
        return synth.encode_mesh_points(m.positions, m.faces, m.normals, m.texcoords, m.generic, extra, opt_of(cfg, m))
    except RuntimeError as e:
        return str(e)


def encode(ctx, meshes, cfg, entry="dsa_encode_points_batch"):
    """[(status, bytes or the refusal's text) per mesh]"""
    st, out = encodecall.call(ctx, entry, meshes, cfg._native_repair())
    assert st == 0, ctx.error()
    return out


def weld(ctx, meshes):
    """[(status, WeldedMaps or the refusal's text) per mesh]"""
    L = native.lib()
    n = len(meshes)
    arr, _, keep = encodecall.arrays(meshes)
    h = C.c_void_p()
    assert L.dsa_weld_batch(ctx._h, n, arr, C.byref(h)) == 0, ctx.error()
    assert L.dsa_welded_size(h) == n
    out = []
    info = native.WeldedInfo()
    for i in range(n):
        s = L.dsa_welded_mesh(h, i, C.byref(info))
        assert s == info.status and info.reserved == 0
        out.append((s, dsa.WeldedMaps(info) if s == 0 else ctx.error()))
    L.dsa_welded_free(h)
    return out


def check_maps(c, got):
    want = weldcases.pin(c.pos, c.faces, c.normals, c.uvs, c.generic, c.extra)
    assert (got.num_points, got.num_vertices) == (len(c.pos), len(want.vertex_point)), c.name
    assert (got.normals_per_vertex, got.texcoords_per_vertex) == (want.normals_per_vertex, want.texcoords_per_vertex), c.name
    for f in ("vertex_of_point", "vertex_point", "normal_of_point", "normal_point", "texcoord_of_point", "texcoord_point"):
        a, b = getattr(got, f), getattr(want, f)
        if b is None or (len(c.pos) == 0):
            continue
        assert a is not None and a.shape == b.shape and np.array_equal(a, b), (c.name, f)
    assert got.num_normals == (0 if want.normal_point is None else len(want.normal_point)), c.name
    assert got.num_texcoords == (0 if want.texcoord_point is None else len(want.texcoord_point)), c.name


@pytest.mark.parametrize("weld_host", ["0", "1"])
def test_the_weld_equals_the_pin(ctx, monkeypatch, weld_host):
    force_paths(monkeypatch, weld_host, None)
    got = weld(ctx, [mesh_of(c) for c in CASES])
    for c, (st, g) in zip(CASES, got):
        if c.refused == "face index out of range":
            assert st == native.DSA_ERR_INVALID_DATA and c.refused in g, c.name
            continue
        assert st == 0, (c.name, g)
        check_maps(c, g)


@pytest.fixture(scope="module")
def cpu_streams():
    cfg = dsa.Config()
    return [cpu(mesh_of(c), cfg) for c in CODED]


@PATHS
def test_streams_equal_the_cpu_coder(ctx, monkeypatch, cpu_streams, weld_host, conn_host):
    force_paths(monkeypatch, weld_host, conn_host)
    got = encode(ctx, [mesh_of(c) for c in CODED], dsa.Config(weld_points=True))
    for c, (st, g), want in zip(CODED, got, cpu_streams):
        assert (want if isinstance(want, str) else None) == c.refused, (c.name, want)
        if c.refused:
            assert st == native.DSA_ERR_INVALID_DATA and want in g, (c.name, g)
        else:
            assert st == 0, (c.name, g)
            assert g == want, c.name


def crowded():
    """300 small cases; every fifth one bad, each kind of refusal in turn."""
    small = [c for c in weldcases.small_cases() if not c.refused and not c.weld_only]
    by = {c.name: c for c in CASES}
    sheet = by["two-sided-sheet"]
    bad = [mesh_of(by["index-out-of-range"]), mesh_of(by["all-equal"]), mesh_of(by["degenerate-after-weld"]), mesh_of(sheet), mesh_of(by["no-faces"]),
           dsa.MeshData(sheet.pos, sheet.faces, sheet.normals, sheet.uvs, texcoord_corners=sheet.faces)]
    meshes, is_bad = [], []
    for k in range(300):
        if k % 5 == 2:
            meshes.append(bad[(k // 5) % len(bad)]); is_bad.append(True)
        else:
            meshes.append(mesh_of(small[k % len(small)])); is_bad.append(False)
    return meshes, is_bad


@pytest.fixture(scope="module")
def crowd():
    meshes, is_bad = crowded()
    cfg = dsa.Config(weld_points=True)
    memo = {}
    want = [memo.setdefault(id(m), cpu(m, cfg)) for m in meshes]
    return meshes, is_bad, cfg, want


@pytest.mark.parametrize("weld_host,conn_host,chunk", [(None, None, None), (None, None, "37"), ("0", "1", "64"), ("1", "0", None)])
def test_crowded_batch_every_fifth_one_bad(ctx, monkeypatch, crowd, weld_host, conn_host, chunk):
    """None: the library's own choice (device weld and device connectivity from 256 meshes on); a chunk size: several chunks."""
    meshes, is_bad, cfg, want = crowd
    force_paths(monkeypatch, weld_host, conn_host)
    if chunk is not None:
        monkeypatch.setenv("DSA_ENC_CHUNK", chunk)
    got = encode(ctx, meshes, cfg)
    for i, (m, (st, g), w) in enumerate(zip(meshes, got, want)):
        if not is_bad[i]:
            assert st == 0 and g == w, (i, g if st else "bytes differ")
            continue
        assert isinstance(w, str) and w in g, (i, g, w)
        assert st == (native.DSA_ERR_INVALID_ARGUMENT if m.per_corner else native.DSA_ERR_INVALID_DATA), (i, g)
    welded = weld(ctx, meshes)
    for i, (m, (st, g)) in enumerate(zip(meshes, welded)):
        if m.per_corner:
            assert st == native.DSA_ERR_INVALID_ARGUMENT and CORNER_IDS in g, i
        elif len(m.faces) and int(m.faces.max()) >= len(m.positions):
            assert st == native.DSA_ERR_INVALID_DATA and "face index out of range" in g, i
        else:
            assert st == 0, (i, g)


@pytest.mark.parametrize("weld_host", ["0", "1"])
def test_a_bench_size_seamed_mesh(ctx, monkeypatch, weld_host):
    force_paths(monkeypatch, weld_host, "0")
    m = synth.make_mesh(synth.GRID, 128, 256, 11)
    p, f, n, u = weldcases.unweld(*irregular.with_seams(*m, None, "stripes", seed=2), np.random.default_rng(12))
    assert 33000 < len(p) < 40000
    mesh = dsa.MeshData(p, f, n, u)
    cfg = dsa.Config(weld_points=True)
    (st, g), = encode(ctx, [mesh], cfg)
    assert st == 0, g
    assert g == cpu(mesh, cfg)
    (st, maps), = weld(ctx, [mesh])
    assert st == 0 and maps.num_vertices == 129 * 257 and not maps.texcoords_per_vertex and maps.normals_per_vertex


LEVELS = [dict(multi_parallelogram=4, traversal_method=1), dict(multi_parallelogram=2, traversal_method=2, edgebreaker_method=2),
          dict(edgebreaker_method=2, normal_prediction=6, texcoord_prediction=5), dict(position_prediction=0, texcoord_prediction=0, speed=0, multi_parallelogram=-1),
          dict(single_connectivity=True, position_bits=14, normal_bits=10, texcoord_bits=12)]


@PATHS
def test_level_options_and_repair_on_the_welded_table(ctx, monkeypatch, weld_host, conn_host):
    force_paths(monkeypatch, weld_host, conn_host)
    by = {c.name: c for c in CASES}
    some = [CASES[k] for k in (0, 8, 15, 22, 29, 33, 34)] + [by[n] for n in ("unused-points", "colours-split", "generic-splits", "differ-in-sign-of-zero")]
    meshes = [mesh_of(c) for c in some]
    for kw in LEVELS:
        cfg = dsa.Config(weld_points=True, **kw)
        for c, m, (st, g) in zip(some, meshes, encode(ctx, meshes, cfg)):
            w = cpu(m, cfg)
            if isinstance(w, str):                       # (ids with single_connectivity: refused, word for word)
                assert st == native.DSA_ERR_INVALID_DATA and w in g, (c.name, kw, g)
            else:
                assert st == 0 and g == w, (c.name, kw, g if st else "bytes differ")
    # the two-sided sheet: refused strict, coded on the repaired table; with two normals per vertex the seams are not implemented there
    sheets = [mesh_of(by["two-sided-sheet"]), mesh_of(by["two-sided-sheet-two-normals"]), meshes[0], mesh_of(by["no-faces"])]
    strict = encode(ctx, sheets, dsa.Config(weld_points=True))
    assert [s for s, _ in strict] == [native.DSA_ERR_INVALID_DATA, native.DSA_ERR_INVALID_DATA, 0, native.DSA_ERR_INVALID_DATA]
    assert "non-manifold edge" in strict[0][1] and "non-manifold edge" in strict[1][1]
    cfg = dsa.Config(weld_points=True, repair_topology=True)
    fixed = encode(ctx, sheets, cfg)
    assert fixed[0][0] == 0 and fixed[0][1] == cpu(sheets[0], cfg)
    assert fixed[1][0] == native.DSA_ERR_NOT_IMPLEMENTED and "not implemented" in fixed[1][1] and "not implemented" in cpu(sheets[1], cfg)
    assert fixed[2] == strict[2]
    assert fixed[3][0] == native.DSA_ERR_INVALID_DATA and fixed[3][1].endswith(cpu(sheets[3], cfg))


def test_streams_decode_like_the_same_mesh_given_with_ids(ctx, monkeypatch):
    """The welded mesh given with ids through dsa_encode_repair_batch (strict) is the same stream; both decode on the wave-per-mesh path
    wherever either does, to the face multiset of quantised corner values of the per-point source."""
    force_paths(monkeypatch, "0", "0")
    some = [c for c in CODED if not c.refused and c.generic is None and not c.extra and len(c.pos) < 2000][::3]
    cfg = dsa.Config(weld_points=True)
    got = encode(ctx, [mesh_of(c) for c in some], cfg)
    with_ids = []
    for c in some:
        w = synth.weld_points(c.pos, c.faces, c.normals, c.uvs)
        with_ids.append(dsa.MeshData(w.pos, w.faces, w.normals, w.uvs, normal_corners=w.normal_corners, texcoord_corners=w.uv_corners))
    ids = encode(ctx, with_ids, dsa.Config(), "dsa_encode_repair_batch")      # (topology 0: the level call)
    assert [g for _, g in got] == [g for _, g in ids]
    a, b = dsa.Batch(ctx, [g for _, g in got]), dsa.Batch(ctx, [g for _, g in ids])
    a.decode(); b.decode()
    on_fast = 0
    for i, c in enumerate(some):
        assert a.status(i) == 0, c.name
        if b.mesh_info(i).decode_path == 0:
            assert a.mesh_info(i).decode_path == 0, c.name
            on_fast += 1
        d = a.result(i).ConnectedData
        keys = np.concatenate([x.PortableValues[x.PointMap] if len(x.PointMap) else x.PortableValues for x in d.Attributes], axis=1)
        want, _ = meshutil.source_corner_faces(c.pos, c.normals, c.uvs, c.faces)
        have = meshutil.face_multiset_fast(d.Faces, keys)
        assert have.shape == want.shape and (have == want).all(), c.name
    assert on_fast > 0
    a.close(); b.close()


def test_encode_batch_and_weld_batch_route(ctx, monkeypatch):
    force_paths(monkeypatch, None, None)
    c = CASES[3]
    m = mesh_of(c)
    enc = dsa.DracoEncoder(ctx)
    assert enc.EncodeBatch([m], dsa.Config(weld_points=True))[0] == cpu(m, dsa.Config(weld_points=True))
    maps, = enc.WeldBatch([m])
    check_maps(c, maps)
    with pytest.raises(Exception, match="face index out of range"):
        enc.WeldBatch([mesh_of(next(x for x in CASES if x.name == "index-out-of-range"))])
