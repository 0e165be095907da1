"""Encode direction, listed attributes given per corner (dsa_encode_corner_attributes_batch): explicit ids on attributes of the list
and the weld with every listed attribute a key set of its own (dsa_encode_weld.h over 3 + L key sets), byte for byte against the
CPU coder (synth.Extra(corners=), synth.encode_mesh_points(weld_attributes=True)) on both connectivity paths (DSA_ENC_HOST_CONN /
DSA_ENC_HOST_PLAN) and both weld paths (DSA_ENC_HOST_WELD), with its refusals word for word; the same streams decoded on the device
against the oracle and the pin of tests/cornerattrcases.py; the call without ids against dsa_encode_seam_repair_batch; crowded
batches over three chunks in which every fifth mesh is bad and fails alone; a bench-size mesh with one row per corner (wide ids);
ids over a repaired table (corner_repair = 1); a shared grid over the rows the ids index."""
import ctypes as C

import numpy as np
import pytest

import cornerattrcases as K
import defects
import encodecall
import oracle
import seamdefects as sd
import draco_sharp_amd as dsa
import draco_sharp_amd.synth as synth
from draco_sharp_amd import native
from draco_sharp_amd.encoder import _fill_attribute_corners

pytestmark = pytest.mark.gpu

CONN = pytest.mark.parametrize("conn_host", ["0", "1"])
PATHS = pytest.mark.parametrize("weld_host,conn_host", [("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")])
SINGLE = "attributes given per corner need a connectivity of their own (single_connectivity = 0)"


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


def attribute_of(e, values=None, ids=True):
    a = dsa.Attribute(e.values if values is None else values, attribute_type=e.attribute_type, normalized=bool(e.normalized), quantization_bits=e.quantization_bits)
    a.corners = e.corners if ids else None          # (behind MeshData's own check: the library is asked)
    return a


def mesh_of(b):
    """dsa.MeshData of a cornerattrcases.Built"""
    m = dsa.MeshData(b.pos, b.faces, b.nrm, b.uv)
    m.normal_corners = None if b.nid is None else np.ascontiguousarray(b.nid, np.uint32).reshape(-1, 3)
    m.texcoord_corners = None if b.uid is None else np.ascontiguousarray(b.uid, np.uint32).reshape(-1, 3)
    m.attributes = [attribute_of(e) for e in b.extras]
    return m


def points_of(b, seed=3):
    """dsa.MeshData of a Built given as one row per point"""
    pos, faces, nrm, uv, arrays = K.unweld(b, np.random.default_rng(seed))
    return dsa.MeshData(pos, faces, nrm, uv, attributes=[attribute_of(e, a, ids=False) for e, a in zip(b.extras, arrays)])


def opt_of(cfg, repair=0):
    mp = cfg.multi_parallelogram
    return synth.options(pos_bits=cfg.position_bits, uv_bits=cfg.texcoord_bits, normal_bits=cfg.normal_bits,
                         single_connectivity=1 if cfg.single_connectivity else 0, force_scheme=cfg.symbol_scheme, compression_level=10 - cfg.speed,
                         pos_prediction=mp if mp and cfg.position_prediction == 1 else cfg.position_prediction,
                         uv_prediction=mp if mp and cfg.texcoord_prediction == 1 else cfg.texcoord_prediction,
                         normal_prediction=cfg.normal_prediction, traversal_method=cfg.traversal_method,
                         predictive_connectivity=2 if cfg.edgebreaker_method == 2 else 0, repair_topology=repair)


def extras_of(m, rows=None):
    return [synth.Extra(a.values, a.attribute_type, a.normalized, a.unique_id, a.quantization_bits, corners=getattr(a, "corners", None),
                        rows=None if rows is None else rows.get(k)) for k, a in enumerate(m.attributes)] or None


def cpu(m, cfg, weld_attributes=False, rows=None):
    """The CPU coder's stream of MeshData m (corner form, or per point under cfg.weld_points), or the text of its refusal."""
    o = opt_of(cfg, (2 if cfg.repair_seams else 1) if cfg.repair_topology else 0)
    try:
        if cfg.weld_points:
            if m.per_corner:
                return "per-point input takes no corner ids"
            return synth.encode_mesh_points(m.positions, m.faces, m.normals, m.texcoords, extra=extras_of(m), opt=o, weld_attributes=weld_attributes)
        return synth.encode_mesh_corners(m.positions, m.faces, m.normals, m.normal_corners, m.texcoords, m.texcoord_corners, opt=o, extra=extras_of(m, rows))
    except RuntimeError as e:
        return str(e)


def encode(ctx, meshes, cfg, weld_attributes=False, corners=True, rows=None, grids=False):
    """[(status, bytes or the refusal's text) per mesh] through dsa_encode_corner_attributes_batch.  corners False: the array is
    NULL; rows: {mesh: {attribute: num_rows}} in place of the arrays' own row counts."""
    L = native.lib()
    n = len(meshes)
    arr, own_grids, keep = encodecall.arrays(meshes)
    co = native.EncodeCornerAttributesOptions()
    L.dsa_encode_default_corner_attributes_options(C.byref(co))
    co.seam_repair.grid.repair = cfg._native_repair()
    co.seam_repair.grid.weld_points = 1 if cfg.weld_points else 0
    co.seam_repair.corner_repair = 1 if cfg.repair_seams else 0
    co.weld_attributes = 1 if weld_attributes else 0
    ca = None
    if corners:
        ca = (native.MeshAttributeCorners * max(1, n))()
        for i, m in enumerate(meshes):
            _fill_attribute_corners(ca[i], m, keep)
            for k, r in (rows or {}).get(i, {}).items():
                ca[i].attributes[k].num_rows = r
    h = C.c_void_p()
    st = L.dsa_encode_corner_attributes_batch(ctx._h, n, arr, own_grids if grids else None, ca, C.byref(co), C.byref(h))
    assert st == 0, ctx.error()
    return encodecall.streams(ctx, h, n)


def same(names, got, want):
    for name, (st, g), w in zip(names, got, want):
        if isinstance(w, str):
            assert st != 0 and w in g, (name, g, w)
        else:
            assert st == 0, (name, g)
            assert g == w, (name, "bytes differ")


def round_trip(ctx, streams, pins, names):
    """The GPU decoder on what was written: equal to the oracle attribute by attribute, and its face multiset equal to the pin."""
    b = dsa.Batch(ctx, streams)
    b.decode()
    for i, (s, want, name) in enumerate(zip(streams, pins, names)):
        assert b.status(i) == 0, name
        d = b.result(i).ConnectedData
        ref = oracle.decode(s)
        assert np.array_equal(d.Faces, ref.faces), name
        cols = []
        for a, r in zip(d.Attributes, ref.attributes):
            assert np.array_equal(a.PortableValues, r.portable) and np.array_equal(a.PointMap, r.point_map), name
            assert a.Values.tobytes() == r.values.tobytes(), name
            cols.append((a.Values if r.seq_type == 1 else a.PortableValues, a.PointMap))
        assert K.same(K.decoded_multiset(d.Faces, cols), want), name
        assert K.same(K.oracle_multiset(ref), want), name
    b.close()


LEVELS = [dict(), dict(edgebreaker_method=2, multi_parallelogram=4, traversal_method=2), dict(position_prediction=0, texcoord_prediction=5, normal_prediction=6),
          dict(multi_parallelogram=2, traversal_method=1, speed=3)]
BUILT = [K.build(c) for c in K.CASES]


@pytest.fixture(scope="module")
def cpu_ids():
    meshes = [mesh_of(b) for b in BUILT]
    return meshes, {k: [cpu(m, dsa.Config(**kw)) for m in meshes] for k, kw in enumerate(LEVELS)}


@CONN
def test_explicit_ids_equal_the_cpu_coder(ctx, monkeypatch, cpu_ids, conn_host):
    force_paths(monkeypatch, None, conn_host)
    meshes, want = cpu_ids
    for k, kw in enumerate(LEVELS):
        assert not any(isinstance(w, str) for w in want[k]), kw
        same([b.name for b in BUILT], encode(ctx, meshes, dsa.Config(**kw)), want[k])


def test_explicit_ids_decode_to_the_pin(ctx, monkeypatch, cpu_ids):
    force_paths(monkeypatch, None, "0")
    meshes, want = cpu_ids
    for k in (0, 1):
        got = encode(ctx, meshes, dsa.Config(**LEVELS[k]))
        same([b.name for b in BUILT], got, want[k])
        round_trip(ctx, [g for _, g in got], [K.pin(b) for b in BUILT], [b.name for b in BUILT])


WELDED = [b for b in BUILT if any(e.corners is not None for e in b.extras)]


@pytest.fixture(scope="module")
def cpu_welds():
    meshes = [points_of(b, 3 + k) for k, b in enumerate(WELDED)]
    cfgs = [dsa.Config(weld_points=True), dsa.Config(weld_points=True, edgebreaker_method=2, multi_parallelogram=4, traversal_method=2)]
    return meshes, cfgs, [[cpu(m, cfg, weld_attributes=True) for m in meshes] for cfg in cfgs]


@PATHS
def test_weld_attributes_equals_the_cpu_coder(ctx, monkeypatch, cpu_welds, weld_host, conn_host):
    force_paths(monkeypatch, weld_host, conn_host)
    meshes, cfgs, want = cpu_welds
    for cfg, w in zip(cfgs, want):
        assert not any(isinstance(x, str) for x in w)
        same([b.name for b in WELDED], encode(ctx, meshes, cfg, weld_attributes=True), w)


def test_weld_attributes_keeps_the_surface_and_decodes_to_the_pin(ctx, monkeypatch, cpu_welds):
    force_paths(monkeypatch, "0", "0")
    meshes, cfgs, want = cpu_welds
    got = encode(ctx, meshes, cfgs[0], weld_attributes=True)
    same([b.name for b in WELDED], got, want[0])
    for b, m, (_, g) in zip(WELDED, meshes, got):
        used = np.unique(m.faces)
        assert sd.header_counts(g)[0] == len(np.unique(m.positions[used].view(np.uint32), axis=0)), b.name      # the stream's vertices: the distinct positions
    round_trip(ctx, [g for _, g in got], [K.pin(b) for b in WELDED], [b.name for b in WELDED])


def test_no_listed_attribute_welds_like_the_points_call(ctx, monkeypatch):
    """The device weld of both calls is one set of kernels: per-point meshes without a listed attribute give the same bytes through
    dsa_encode_points_batch (three key sets) and through this call with weld_attributes = 1 (3 + L key sets, L = 0), the CPU
    coder's; and still do beside a mesh with two listed attributes in the middle of the batch, which sizes the grid for five."""
    import weldcases
    force_paths(monkeypatch, "0", None)
    small = [c for c in weldcases.small_cases() if not c.refused and not c.weld_only]
    plain = [c for c in small if not c.extra]
    assert len(plain) == len(small) - 1 > 40 and any(c.generic is not None for c in plain)      # (all but "colours-split")
    cfg = dsa.Config(weld_points=True)

    def data(c, listed=()):
        return dsa.MeshData(c.pos, c.faces, c.normals, c.uvs, generic=c.generic, attributes=[dsa.Attribute(a, attribute_type=4) for a in listed])

    def want_of(c, listed=()):
        o = opt_of(cfg)
        o.generic_components = c.generic.shape[1] if c.generic is not None else 1
        return synth.encode_mesh_points(c.pos, c.faces, c.normals, c.uvs, c.generic, [synth.Extra(a, attribute_type=4) for a in listed] or None, o, weld_attributes=bool(listed))
    names = [c.name for c in plain]
    want = [want_of(c) for c in plain]
    st, points = encodecall.call(ctx, "dsa_encode_points_batch", [data(c) for c in plain], cfg._native_repair())
    assert st == 0, ctx.error()
    alone = encode(ctx, [data(c) for c in plain], cfg, weld_attributes=True)
    assert len(points) == len(alone) == len(want) == len(plain)
    same(names, points, want)
    same(names, alone, want)
    assert points == alone
    # one mesh with two listed attributes in the middle: the first the same for all points of a vertex, the second not
    c = next(c for c in small if c.name == "colours-split")
    key = np.ascontiguousarray(c.pos, np.float32).view(np.uint32).astype(np.uint64).sum(axis=1)
    listed = [np.ascontiguousarray((key % 251).astype(np.uint8)[:, None]), np.ascontiguousarray(c.extra[0])]
    w = want_of(c, listed)
    assert sd.header_counts(w)[0] == len(np.unique(c.pos[np.unique(c.faces)].view(np.uint32), axis=0))      # (the colour cuts no vertex)
    h = len(plain) // 2
    mixed = encode(ctx, [data(c) for c in plain[:h]] + [data(c, listed)] + [data(c) for c in plain[h:]], cfg, weld_attributes=True)
    assert len(mixed) == len(plain) + 1
    same(names[:h] + [c.name] + names[h:], mixed, want[:h] + [w] + want[h:])
    assert mixed[:h] + mixed[h + 1:] == points


def test_without_ids_it_is_the_seam_repair_call(ctx, monkeypatch):
    """corners == NULL, weld_attributes = 0 over a mixed batch: the streams and the messages of dsa_encode_seam_repair_batch."""
    force_paths(monkeypatch, None, None)
    plain = [mesh_of(b._replace(extras=[e for e in b.extras if e.corners is None])) for b in BUILT[:12]]
    bad = dsa.MeshData(BUILT[0].pos, BUILT[0].faces)
    bad.faces = bad.faces.copy()
    bad.faces[0, 0] = 10 ** 6
    plain.insert(5, bad)
    for cfg in (dsa.Config(), dsa.Config(repair_topology=True, repair_seams=True, multi_parallelogram=4)):
        so = native.EncodeSeamRepairOptions()
        native.lib().dsa_encode_default_seam_repair_options(C.byref(so))
        so.grid.repair = cfg._native_repair()
        so.corner_repair = 1 if cfg.repair_seams else 0
        st, want = encodecall.call(ctx, "dsa_encode_seam_repair_batch", plain, so, grids=None)
        assert st == 0
        assert encode(ctx, plain, cfg, corners=False) == want
        assert encode(ctx, plain, cfg, corners=True) == want               # (an array whose meshes all have attributes == NULL)
        assert want[5][0] == native.DSA_ERR_INVALID_DATA and "face index out of range" in want[5][1]
    per_point = [points_of(b) for b in BUILT[4:9]]
    cfg = dsa.Config(weld_points=True)
    so = native.EncodeSeamRepairOptions()
    native.lib().dsa_encode_default_seam_repair_options(C.byref(so))
    so.grid.repair = cfg._native_repair()
    so.grid.weld_points = 1
    st, want = encodecall.call(ctx, "dsa_encode_seam_repair_batch", per_point, so, grids=None)
    assert st == 0 and encode(ctx, per_point, cfg, corners=False) == want


# ------------------------------------------------------------------------------------------------------ crowded batches
def crowded_ids(single):
    """300 small meshes; every fifth one bad, each kind of refusal in turn: (meshes, per mesh None or (status, text), row-count
    overrides, per good mesh a key under which its CPU stream is shared).  single: the batch is coded under single_connectivity,
    which takes per-vertex lists and refuses every mesh with ids."""
    small = [b for b in BUILT if len(b.pos) < 700]
    with_ids = [b for b in small if b.extras[0].corners is not None]
    meshes, bad, rows, keys = [], [], {}, []
    for k in range(300):
        b = small[k % len(small)]
        keys.append(k % len(small))
        if k % 5 != 2:
            if single:                                        # no ids anywhere: what single_connectivity takes
                b = b._replace(nrm=None, nid=None, uv=None if b.uid is not None else b.uv, uid=None, extras=[e for e in b.extras if e.corners is None])
            meshes.append(mesh_of(b)); bad.append(None)
            continue
        m = mesh_of(with_ids[(k // 5) % len(with_ids)])
        kind = (k // 5) % 4
        if single:
            bad.append((native.DSA_ERR_INVALID_DATA, SINGLE))
        elif kind == 0:                                       # an id at the row count
            m.attributes[0].corners = m.attributes[0].corners.copy()
            m.attributes[0].corners[-1, 1] = len(m.attributes[0].values)
            bad.append((native.DSA_ERR_INVALID_DATA, "attribute 0 id out of range"))
        elif kind == 1:                                       # a row count below the ids
            rows[k] = {0: int(m.attributes[0].corners.max())}
            bad.append((native.DSA_ERR_INVALID_DATA, "attribute 0 id out of range"))
        elif kind == 2:                                       # ids on the attribute at index 8 of the stream
            builtins = 1 + (m.normals is not None) + (m.texcoords is not None)
            fill = [dsa.Attribute(np.zeros(len(m.positions), np.uint8)) for _ in range(8 - builtins)]
            m.attributes = fill + m.attributes[:1]
            bad.append((native.DSA_ERR_INVALID_ARGUMENT, "attribute %d: corner ids on attribute 8 of the stream: corner attributes are decoded for attributes 1 to 7" % len(fill)))
        else:                                                 # a face index out of range beside good ids
            m.faces = m.faces.copy()
            m.faces[-1, 2] = len(m.positions)
            bad.append((native.DSA_ERR_INVALID_DATA, "face index out of range"))
        meshes.append(m)
    return meshes, bad, rows, keys


@pytest.mark.parametrize("single,conn_host", [(False, None), (False, "1"), (True, None)])
def test_crowded_batch_with_ids_every_fifth_one_bad(ctx, monkeypatch, single, conn_host):
    meshes, bad, rows, keys = crowded_ids(single)
    assert sum(b is not None for b in bad) == 60
    cfg = dsa.Config(single_connectivity=single)
    force_paths(monkeypatch, None, conn_host)
    monkeypatch.setenv("DSA_ENC_CHUNK", "100")                # three chunks
    got = encode(ctx, meshes, cfg, rows=rows)
    memo = {}
    for i, (m, (st, g)) in enumerate(zip(meshes, got)):
        if bad[i] is not None:
            assert st == bad[i][0] and bad[i][1] in g, (i, st, g, bad[i])
            w = cpu(m, cfg, rows=rows.get(i))
            assert isinstance(w, str) and w in g, (i, w, g)  # the CPU coder refuses it in the same words
            continue
        if keys[i] not in memo:
            memo[keys[i]] = cpu(m, cfg)
        assert st == 0 and g == memo[keys[i]], (i, g if st else "bytes differ")


@pytest.mark.parametrize("weld_host", [None, "1"])
def test_crowded_weld_batch_every_fifth_one_bad(ctx, monkeypatch, weld_host):
    small = [b for b in WELDED if len(b.pos) < 700]
    per_point = [points_of(b, 20 + k) for k, b in enumerate(small)]
    cfg = dsa.Config(weld_points=True)
    want = [cpu(m, cfg, weld_attributes=True) for m in per_point]
    meshes, expect = [], []
    for k in range(300):
        j = k % len(small)
        if k % 5 != 2:
            meshes.append(per_point[j]); expect.append(want[j])
        elif (k // 5) % 2:
            m = mesh_of(small[j])                             # explicit ids together with weld_points
            meshes.append(m); expect.append((native.DSA_ERR_INVALID_ARGUMENT, "per-point input takes no corner ids"))
        else:
            p = per_point[j]
            m = dsa.MeshData(p.positions, p.faces, p.normals, p.texcoords, attributes=p.attributes)
            m.faces = m.faces.copy()
            m.faces[0, 1] = len(m.positions)
            meshes.append(m); expect.append((native.DSA_ERR_INVALID_DATA, "face index out of range"))
    force_paths(monkeypatch, weld_host, None)
    monkeypatch.setenv("DSA_ENC_CHUNK", "100")
    got = encode(ctx, meshes, cfg, weld_attributes=True)
    for i, ((st, g), w) in enumerate(zip(got, expect)):
        if isinstance(w, tuple):
            assert st == w[0] and w[1] in g, (i, st, g)
        else:
            assert st == 0 and g == w, (i, g if st else "bytes differ")


# ------------------------------------------------------------------------------------------------------------ bench size
@pytest.fixture(scope="module")
def bench_mesh():
    pos, nrm, uv, faces = synth.make_mesh(synth.GRID, 128, 256, 7)
    rng = np.random.default_rng(4)
    rows = (uv[faces.ravel()] * np.float32(0.5) + rng.uniform(0, 0.002, (3 * len(faces), 2))).astype(np.float32)      # one row per corner
    assert len(rows) == 196608
    b = K.Built("grid128x256/uv1-corner", pos, np.ascontiguousarray(faces, np.uint32), None, None, uv, None,
                [synth.Extra(rows, attribute_type=3, corners=np.arange(len(rows), dtype=np.uint32).reshape(-1, 3))])
    return b, K.encode(b)


@CONN
def test_a_bench_size_mesh_with_one_row_per_corner(ctx, monkeypatch, bench_mesh, conn_host):
    """196 608 rows: the wide-id form beside the narrow one of every small case."""
    force_paths(monkeypatch, None, conn_host)
    b, want = bench_mesh
    (st, g), = encode(ctx, [mesh_of(b)], dsa.Config())
    assert st == 0, g
    assert g == want
    if conn_host == "0":
        round_trip(ctx, [g], [K.pin(b)], [b.name])


# ----------------------------------------------------------------------------------------------------- over a repaired table
@CONN
def test_corner_repair_codes_listed_ids_over_the_repaired_table(ctx, monkeypatch, conn_host):
    force_paths(monkeypatch, None, conn_host)
    specs = [("grid", synth.GRID, 6, 5, (None, "stripes"), "double", [("uv1", "checker"), ("fid16", "island")]),
             ("torus", synth.TORUS, 9, 8, ("checker", "island"), "pinch", [("colour", "stripes"), ("fid32", None)])]
    built = []
    for name, kind, nx, ny, charts, defect, attrs in specs:
        clean = sd.seamed_source(synth, name, kind, nx, ny, charts, 6)
        built += [K.with_listed(sd.inject(clean, defect, count, np.random.default_rng(31 + count)), attrs) for count in (1, 5)]
        built.append(K.with_listed(clean, attrs))
    meshes = [mesh_of(b) for b in built]
    for kw in (dict(), dict(edgebreaker_method=2, multi_parallelogram=4, traversal_method=2)):
        cfg = dsa.Config(repair_topology=True, repair_seams=True, **kw)
        want = [cpu(m, cfg) for m in meshes]
        assert not any(isinstance(w, str) for w in want)
        got = encode(ctx, meshes, cfg)
        same([b.name for b in built], got, want)
        round_trip(ctx, [g for _, g in got], [K.pin(b, keep=~defects.is_degenerate(b.faces)) for b in built], [b.name for b in built])
    # corner_repair 0: refused as the built-in ids are, in the CPU coder's words
    cfg = dsa.Config(repair_topology=True)
    got = encode(ctx, meshes, cfg)
    for b, m, (st, g) in zip(built, meshes, got):
        w = cpu(m, cfg)
        if isinstance(w, str):
            assert st == native.DSA_ERR_NOT_IMPLEMENTED and "over a mesh whose topology needs repair are not implemented" in g and "not implemented" in w, b.name
        else:
            assert st == 0 and g == w, b.name
    assert sum(st != 0 for st, _ in got) == 4


# --------------------------------------------------------------------------------------------------------------- grids
@CONN
def test_a_shared_grid_is_taken_over_the_rows_the_ids_index(ctx, monkeypatch, conn_host):
    force_paths(monkeypatch, None, conn_host)
    some = [K.build(next(c for c in K.CASES if c.name == n)) for n in ("grid7x7/uv1-checker+colour-random", "grid17x16/uv1-random", "grid33x17/uv1-corner")]
    meshes = []
    for b in some:
        m = mesh_of(b)
        m.attributes[0].grid = dsa.Grid.shared()
        m.group = 5
        meshes.append(m)
    shared = synth.shared_grid([b.extras[0].values for b in some])                  # over ALL rows of every member, not its vertex count
    want = []
    for b in some:
        e = b.extras[0]
        ex = [synth.Extra(e.values, e.attribute_type, corners=e.corners, grid=shared)] + b.extras[1:]
        want.append(synth.encode_grid(b.pos, b.faces, b.nrm, b.uv, extra=ex, form=1, normal_corners=b.nid, uv_corners=b.uid))
    got = encode(ctx, meshes, dsa.Config(), grids=True)
    same([b.name for b in some], got, want)
    own = encode(ctx, [mesh_of(b) for b in some], dsa.Config())
    assert all(a[1] != o[1] for a, o in zip(got, own))                                # (the grid is not any member's own)


# ----------------------------------------------------------------------------------------------------------- refusals
def test_call_level_refusals_name_the_field(ctx):
    L = native.lib()
    arr, _, keep = encodecall.arrays([mesh_of(BUILT[0])])

    def refused(field, **kw):
        co = native.EncodeCornerAttributesOptions()
        L.dsa_encode_default_corner_attributes_options(C.byref(co))
        for k, v in kw.items():
            if k == "weld_points":
                co.seam_repair.grid.weld_points = v
            elif k == "reserved":
                co.reserved[v] = 1
            else:
                setattr(co, k, v)
        h = C.c_void_p()
        assert L.dsa_encode_corner_attributes_batch(ctx._h, 1, arr, None, None, C.byref(co), C.byref(h)) == native.DSA_ERR_INVALID_ARGUMENT, field
        assert field in ctx.error(), (field, ctx.error())
        return ctx.error()
    for value in (2, -1):
        assert "weld_attributes %d" % value in refused("weld_attributes", weld_attributes=value)
    assert "needs weld_points 1" in refused("weld_attributes", weld_attributes=1)
    refused("weld_attributes", weld_attributes=1, weld_points=0)
    for k in (0, 6):
        assert "dsa_encode_corner_attributes_options.reserved[%d] is not zero" % k in refused("reserved", reserved=k)


@CONN
def test_reserved_words_of_the_id_structs_fail_the_mesh_alone(ctx, monkeypatch, conn_host):
    force_paths(monkeypatch, "1", conn_host)
    L = native.lib()
    some = [b for b in BUILT if b.extras[0].corners is not None][:4]
    meshes = [mesh_of(b) for b in some]
    want = [cpu(m, dsa.Config()) for m in meshes]

    def call(cfg, meshes, edit, weld_attributes=False):
        n = len(meshes)
        arr, _, keep = encodecall.arrays(meshes)
        co = native.EncodeCornerAttributesOptions()
        L.dsa_encode_default_corner_attributes_options(C.byref(co))
        co.seam_repair.grid.repair = cfg._native_repair()
        co.seam_repair.grid.weld_points = 1 if cfg.weld_points else 0
        co.weld_attributes = 1 if weld_attributes else 0
        ca = (native.MeshAttributeCorners * n)()
        for i, m in enumerate(meshes):
            _fill_attribute_corners(ca[i], m, keep)
        edit(ca)
        h = C.c_void_p()
        assert L.dsa_encode_corner_attributes_batch(ctx._h, n, arr, None, ca, C.byref(co), C.byref(h)) == 0, ctx.error()
        return encodecall.streams(ctx, h, n)

    def set_words(ca):
        ca[1].reserved[1] = 7
        ca[2].attributes[0].reserved = 1
    got = call(dsa.Config(), meshes, set_words)
    assert got[1][0] == native.DSA_ERR_INVALID_ARGUMENT and "dsa_mesh_attribute_corners.reserved is not zero" in got[1][1], got[1]
    assert got[2][0] == native.DSA_ERR_INVALID_ARGUMENT and "attribute 0: dsa_attribute_corners.reserved is not zero" in got[2][1], got[2]
    for k in (0, 3):
        assert got[k] == (0, want[k]), some[k].name
    # per-point input: the word of the mesh's struct is read before the weld
    per_point = [points_of(b) for b in some[:3]]
    cfg = dsa.Config(weld_points=True)

    def set_word(ca):
        ca[1].reserved[0] = 1
    got = call(cfg, per_point, set_word, weld_attributes=True)
    assert got[1][0] == native.DSA_ERR_INVALID_ARGUMENT and "dsa_mesh_attribute_corners.reserved is not zero" in got[1][1], got[1]
    for k in (0, 2):
        assert got[k] == (0, cpu(per_point[k], cfg, weld_attributes=True)), some[k].name
