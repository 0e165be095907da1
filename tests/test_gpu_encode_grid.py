"""Encode direction, quantisation grids given by the caller (mode 1) or shared by the meshes of a group (mode 2):
dsa_encode_grid_batch / dsa_encode_grid_sequential_batch through dsa.Grid, MeshData(position_grid=, texcoord_grid=, group=) and
Attribute(grid=).  The device coder must write, byte for byte, the stream of the CPU coder (synth.encode_grid with the same
explicit grid; for a shared grid with synth.shared_grid over the group's arrays) on both connectivity paths and whatever the
chunks, refuse what the CPU coder refuses in its words, and with every mode 0 give the bytes of the calls it stands beside.  The
tiles of one surface decode without a crack on a shared grid (dsa.Batch), which the numpy pin of tests/gridcases.py states."""
import ctypes as C

import numpy as np
import pytest

import encodecall
import defects
import gridcases as gc
import irregular
import draco_sharp_amd as dsa
import draco_sharp_amd.synth as synth
from draco_sharp_amd import native

pytestmark = pytest.mark.gpu

BOTH_PATHS = pytest.mark.parametrize("host", ["0", "1"])
MODES = pytest.mark.parametrize("mode", [1, 2])


@pytest.fixture(scope="module")
def ctx():
    c = dsa.Context(0)
    yield c
    c.close()


def force_path(monkeypatch, host):
    for name in ("DSA_ENC_HOST_CONN", "DSA_ENC_HOST_PLAN", "DSA_ENC_HOST_WELD"):
        monkeypatch.setenv(name, host)


def opt_of(cfg, m):
    mp = cfg.multi_parallelogram
    return synth.options(pos_bits=cfg.position_bits, uv_bits=cfg.texcoord_bits, normal_bits=cfg.normal_bits,
                         single_connectivity=1 if cfg.single_connectivity else 0, force_scheme=cfg.symbol_scheme, compression_level=10 - cfg.speed,
                         pos_prediction=mp if mp and cfg.position_prediction == 1 else cfg.position_prediction,
                         uv_prediction=mp if mp and cfg.texcoord_prediction == 1 else cfg.texcoord_prediction,
                         normal_prediction=cfg.normal_prediction, traversal_method=cfg.traversal_method,
                         predictive_connectivity=2 if cfg.edgebreaker_method == 2 else 0,
                         generic_components=m.generic.shape[1] if m.generic is not None else 1, repair_topology=1 if cfg.repair_topology else 0)


def slots(m):
    """(name, values, Grid or None) of every attribute of MeshData / PointCloudData m that can take a grid"""
    out = [("position", m.positions, m.position_grid)]
    if m.texcoords is not None:
        out.append(("texcoord", m.texcoords, m.texcoord_grid))
    out += [(k, a.values, a.grid) for k, a in enumerate(m.attributes) if a.values.dtype == np.float32]
    return out


def cpu_grid(meshes, m, name, values, grid):
    """the CPU coder's grid for a slot: the explicit one, or the group's by synth.shared_grid over the members' arrays"""
    if grid is None:
        return None
    if grid.mode == 1:
        return synth.grid(grid.origin, grid.range)
    members = []
    for o in meshes:
        for n2, v2, g2 in slots(o):
            if o.group == m.group and n2 == name and g2 is not None and g2.mode == 2 and v2.shape[1] == values.shape[1]:
                members.append(v2)
    try:
        return synth.shared_grid(members)
    except RuntimeError:                      # no member without a value that is not finite: every member is refused whatever the grid
        return synth.grid(np.zeros(values.shape[1], np.float32), 1.0)


def cpu(meshes, m, cfg):
    """The CPU coder's stream of mesh m of the batch under cfg, or the text of its refusal."""
    by = {name: cpu_grid(meshes, m, name, values, grid) for name, values, grid in slots(m)}
    extra = [synth.Extra(a.values, a.attribute_type, a.normalized, a.unique_id, a.quantization_bits, grid=by.get(k)) for k, a in enumerate(m.attributes)] or None
    kw = dict(generic=m.generic, extra=extra, opt=opt_of(cfg, m), pos_grid=by["position"], uv_grid=by.get("texcoord"))
    try:
        if isinstance(m, dsa.PointCloudData):
            return synth.encode_grid(m.positions, None, m.normals, m.texcoords, form=0, geometry=0, **kw)
        if cfg.sequential:
            return synth.encode_grid(m.positions, m.faces, m.normals, m.texcoords, form=0, geometry=1, compressed=cfg.compress_connectivity, **kw)
        if cfg.weld_points:
            return synth.encode_grid(m.positions, m.faces, m.normals, m.texcoords, form=2, **kw)
        return synth.encode_grid(m.positions, m.faces, m.normals, m.texcoords, form=1, normal_corners=m.normal_corners, uv_corners=m.texcoord_corners, **kw)
    except RuntimeError as e:
        return str(e)


def check_equal(ctx, meshes, cfg):
    got = dsa.DracoEncoder(ctx).TryEncodeBatch(meshes, cfg)
    for i, (m, g) in enumerate(zip(meshes, got)):
        want = cpu(meshes, m, cfg)
        if isinstance(want, bytes):
            assert g == want, (i, g if isinstance(g, Exception) else "bytes differ")
        else:
            assert isinstance(g, Exception) and str(g).endswith(want), (i, g if isinstance(g, Exception) else "coded", want)
    return got


def grid_for(mode, arrays):
    """mode 1: an explicit grid a little wider than the arrays' union; mode 2: the shared one"""
    if mode == 2:
        return dsa.Grid.shared()
    o, r = gc.shared_bounds(arrays)
    return dsa.Grid(o - np.float32(0.125), r + np.float32(0.5))


def tile_meshes(mode, what):
    tiles = [c for c, _ in gc.tiles()]
    pg, ug = grid_for(mode, [c.pos for c in tiles]), grid_for(mode, [c.uvs for c in tiles])
    rng = np.random.default_rng(4)
    out = []
    seamed = [irregular.with_seams(c.pos, np.zeros_like(c.pos), c.uvs, c.faces, None, "stripes", seed=k) for k, c in enumerate(tiles)]
    if what == "corners":                              # (a chart moves its texture coordinates: the grid is that of the rows given)
        ug = grid_for(mode, [s[4] for s in seamed])
    for k, c in enumerate(tiles):
        if what == "corners":                          # texture coordinates per corner, with seams
            pos, faces, _, _, uv, uci = seamed[k]
            assert len(uv) > len(pos)
            out.append(dsa.MeshData(pos, faces, texcoords=uv, texcoord_corners=uci, position_grid=pg, texcoord_grid=ug, group=3))
        elif what == "attributes":                     # a float32 extra on a grid beside an integer extra without one
            w = (rng.random((len(c.pos), 2)) * (k + 1)).astype(np.float32)
            ids = rng.integers(0, 4000, (len(c.pos), 1)).astype(np.uint16)
            wg = dsa.Grid.shared() if mode == 2 else dsa.Grid([0, -1], 8.0)
            out.append(dsa.MeshData(c.pos, c.faces, texcoords=c.uvs, position_grid=pg, group=3,
                                    attributes=[dsa.Attribute(ids), dsa.Attribute(w, quantization_bits=12, grid=wg)]))
        elif what == "cloud":
            out.append(dsa.PointCloudData(c.pos, texcoords=c.uvs, position_grid=pg, texcoord_grid=ug, group=3))
        else:
            out.append(dsa.MeshData(c.pos, c.faces, texcoords=c.uvs, position_grid=pg, texcoord_grid=ug, group=3))
    return out


def damaged_tile(mode):
    """a tile-sized mesh with a fin and a doubled face, in the tiles' group: it is coded in the second pass of a repair request"""
    c = gc.tiles()[0][0]
    faces = np.concatenate([c.faces, c.faces[:1], [[0, 1, len(c.pos) - 1]]]).astype(np.uint32)
    pos = (c.pos + np.float32(0.25)).astype(np.float32)
    pg = dsa.Grid.shared() if mode == 2 else grid_for(1, [t.pos for t, _ in gc.tiles()])
    return dsa.MeshData(pos, faces, texcoords=c.uvs, position_grid=pg, group=3)


CASES = {
    "edgebreaker": (lambda mode: tile_meshes(mode, "plain"), dict()),
    "corners": (lambda mode: tile_meshes(mode, "corners"), dict()),
    "attributes": (lambda mode: tile_meshes(mode, "attributes"), dict()),
    "multi": (lambda mode: tile_meshes(mode, "plain"), dict(multi_parallelogram=4, traversal_method=1)),
    "repair": (lambda mode: tile_meshes(mode, "plain")[:2] + [damaged_tile(mode)] + tile_meshes(mode, "plain")[2:], dict(repair_topology=True)),
    "weld": (lambda mode: tile_meshes(mode, "plain"), dict(weld_points=True)),
    "sequential": (lambda mode: tile_meshes(mode, "plain"), dict(encoding_method=0, compress_connectivity=True)),
    "cloud": (lambda mode: tile_meshes(mode, "cloud"), dict()),
}


@BOTH_PATHS
@MODES
@pytest.mark.parametrize("case", list(CASES))
def test_matches_cpu_coder(ctx, monkeypatch, host, mode, case):
    force_path(monkeypatch, host)
    make, cfg = CASES[case]
    got = check_equal(ctx, make(mode), dsa.Config(**cfg))
    assert all(isinstance(g, bytes) for g in got)


@MODES
@pytest.mark.parametrize("case", ["edgebreaker", "repair", "cloud"])
def test_a_group_in_three_chunks_gives_the_bytes_of_one_chunk(ctx, monkeypatch, mode, case):
    """DSA_ENC_CHUNK = 2: the four tiles of the group lie in three chunks, between two meshes of another group."""
    force_path(monkeypatch, "0")
    make, cfg = CASES[case]
    tiles = make(mode)
    c = gc.texel()
    other = [dsa.PointCloudData(c.pos + k, position_grid=dsa.Grid.shared(), group=8) if case == "cloud" else
             dsa.MeshData(c.pos + k, c.faces, texcoords=c.uvs, position_grid=dsa.Grid.shared(), group=8) for k in (0, 5)]
    meshes = other[:1] + tiles + other[1:]
    assert len(tiles) >= 4 and len(meshes) >= 6
    one = check_equal(ctx, meshes, dsa.Config(**cfg))
    monkeypatch.setenv("DSA_ENC_CHUNK", "2")
    assert dsa.DracoEncoder(ctx).TryEncodeBatch(meshes, dsa.Config(**cfg)) == one


def test_tiles_on_a_shared_grid_decode_without_a_crack(ctx):
    tiles = gc.tiles()
    # the precondition, from the pin alone: on their own grids some border vertex dequantises differently in two tiles
    own = {}
    for c, index in tiles:
        o, r = gc.own_bounds(c.pos)
        deq = gc.dequantize(gc.pin(c.pos, o, r, gc.POS_BITS), o, r, gc.POS_BITS)
        for row, rc in enumerate(index):
            own.setdefault(tuple(int(x) for x in rc), set()).add(deq[row].tobytes())
    assert any(len(v) > 1 for v in own.values())
    meshes = [dsa.MeshData(c.pos, c.faces, position_grid=dsa.Grid.shared(), group=1) for c, _ in tiles]
    streams = list(dsa.DracoEncoder(ctx).EncodeBatch(meshes))
    origin, rng = gc.shared_bounds([c.pos for c, _ in tiles])
    b = dsa.Batch(ctx, streams)
    b.decode(wait=False)
    b.vertex_arrays("values")
    seen = {}
    for i, (c, index) in enumerate(tiles):
        assert b.status(i) == 0 and b.mesh_info(i).decode_path == 0
        v = b.vertex_views(i)
        pos = [a for a in v["attributes"] if a["info"].attribute_type == 0][0]
        assert np.array_equal(np.float32(pos["info"].min_values[:3]), origin) and np.float32(pos["info"].range) == rng
        want = gc.dequantize(gc.pin(c.pos, origin, rng, gc.POS_BITS), origin, rng, gc.POS_BITS)
        got = {r.tobytes() for r in np.ascontiguousarray(pos["values"], np.float32)}
        assert got == {r.tobytes() for r in want}                     # every position is origin + q * (range / max_q) of the pin
        for row, rc in enumerate(index):
            assert want[row].tobytes() in got
            seen.setdefault(tuple(int(x) for x in rc), set()).add(want[row].tobytes())
    b.close()
    assert sum(1 for v in seen.values() if len(v) > 1) == 0            # one decoded position per vertex of the field, in every tile that holds it


@BOTH_PATHS
def test_refusals_in_a_batch_of_eight(ctx, monkeypatch, host):
    force_path(monkeypatch, host)
    tiles = [c for c, _ in gc.tiles()]
    off, (origin, rng), off_row = gc.damaged("off")
    nan, _, nan_row = gc.damaged("nan")
    explicit = dsa.Grid(origin, rng)
    meshes = [dsa.MeshData(c.pos, c.faces, texcoords=c.uvs, position_grid=dsa.Grid.shared(), group=2) for c in tiles[:3]]
    meshes.append(dsa.MeshData(nan.pos + np.float32(100.0), nan.faces, position_grid=dsa.Grid.shared(), group=2))      # would move the group's grid
    meshes.append(dsa.MeshData(off.pos, off.faces, position_grid=explicit))
    meshes += [dsa.MeshData(c.pos, c.faces, position_grid=explicit) for c in (gc.damaged("edge")[0], gc.texel(seed=7))]
    meshes.append(dsa.MeshData(tiles[3].pos, tiles[3].faces, texcoords=tiles[3].uvs, position_grid=dsa.Grid.shared(), group=2))
    assert len(meshes) == 8
    got = check_equal(ctx, meshes, dsa.Config())
    failed = [i for i, g in enumerate(got) if isinstance(g, Exception)]
    assert failed == [3, 4]
    assert isinstance(got[3], ValueError) and str(got[3]).endswith(gc.refusal("positions", nan_row, False))
    assert isinstance(got[4], ValueError) and str(got[4]).endswith(gc.refusal("positions", off_row, True))
    # the group's grid is that of its four clean members
    import oracle
    o4, r4 = gc.shared_bounds([c.pos for c in tiles])
    a = oracle.decode(got[0]).attributes[0]
    assert np.array_equal(np.float32(a.q_min[:3]), o4) and np.float32(a.q_range) == r4


def raw(ctx, entry, meshes, opt, *grids):
    st, out = encodecall.call(ctx, entry, meshes, opt, *grids)
    assert st == 0, ctx.error()
    return out


@BOTH_PATHS
def test_mode_0_through_the_new_calls_is_the_call_it_stands_beside(ctx, monkeypatch, host):
    force_path(monkeypatch, host)
    L = native.lib()
    tiles = [c for c, _ in gc.tiles()]
    meshes = [dsa.MeshData(c.pos, c.faces, texcoords=c.uvs) for c in tiles] + [damaged_tile(1)]
    n = len(meshes)
    zero = (native.MeshGrids * n)()
    for weld in (0, 1):
        ro = dsa.Config(repair_topology=True, multi_parallelogram=4)._native_repair()
        go = native.EncodeGridOptions()
        L.dsa_encode_default_grid_options(C.byref(go))
        go.repair, go.weld_points = ro, weld
        want = raw(ctx, "dsa_encode_points_batch" if weld else "dsa_encode_repair_batch", meshes, ro)
        assert all(s == 0 for s, _ in want)
        assert raw(ctx, "dsa_encode_grid_batch", meshes, go, None) == want
        assert raw(ctx, "dsa_encode_grid_batch", meshes, go, zero) == want
    clouds = [dsa.PointCloudData(p) for p in gc.cloud_chunks()]
    for geometry, ms in ((1, meshes[:4]), (0, clouds)):
        so = dsa.Config(encoding_method=0)._native_sequential(geometry)
        want = raw(ctx, "dsa_encode_attributes_sequential_batch", ms, so)
        assert all(s == 0 for s, _ in want)
        assert raw(ctx, "dsa_encode_grid_sequential_batch", ms, so, None) == want
        assert raw(ctx, "dsa_encode_grid_sequential_batch", ms, so, zero) == want


def test_a_point_cloud_in_four_chunks_shares_one_grid(ctx):
    chunks = gc.cloud_chunks()
    clouds = [dsa.PointCloudData(p, position_grid=dsa.Grid.shared(), group=5) for p in chunks]
    got = check_equal(ctx, clouds, dsa.Config())
    import oracle
    origin, rng = gc.shared_bounds(chunks)
    for p, s in zip(chunks, got):
        a = oracle.decode(s).attributes[0]
        assert np.array_equal(np.float32(a.q_min[:3]), origin) and np.float32(a.q_range) == rng
        assert np.array_equal(a.portable, gc.pin(p, origin, rng, gc.POS_BITS))


def test_argument_failures_per_mesh(ctx):
    """what the structs say against themselves fails the mesh alone, with the field in the message"""
    L = native.lib()
    c = gc.voxel()
    m = dsa.MeshData(c.pos, c.faces)
    n = 6
    grids = (native.MeshGrids * n)()
    grids[0].position.mode = 7
    grids[1].position.mode, grids[1].position.range = 1, 0.0
    grids[2].position.mode, grids[2].position.range, grids[2].position.origin[2] = 1, 1.0, float("nan")
    grids[3].texcoord.mode = 2
    grids[4].reserved = 1
    grids[5].position.reserved[0] = 1
    go = native.EncodeGridOptions()
    L.dsa_encode_default_grid_options(C.byref(go))
    got = raw(ctx, "dsa_encode_grid_batch", [m] * n, go, grids)
    assert [s for s, _ in got] == [native.DSA_ERR_INVALID_ARGUMENT] * n
    for (_, text), field in zip(got, ("positions: grid.mode 7", "positions: grid.range 0", "positions: grid.origin[2] is not finite",
                                      "texcoords: grid.mode 2 for an attribute the mesh does not have", "dsa_mesh_grids.reserved is not zero",
                                      "positions: grid.reserved is not zero")):
        assert field in text
