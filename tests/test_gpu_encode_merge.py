"""Encode direction, one point per occupied quantisation cell of a point cloud on the device (dsa_encode_merged_sequential_batch,
merge_points = 1; Config(merge_points=dsa.MERGE_CELLS); k_enc_merge_* of draco-sharp_amd/csrc/dsa_encode_order.h).  Every stream
must be, byte for byte, the CPU coder's (synth.encode_merged) and the device's own plain stream of the kept rows with every
quantised attribute on an explicit grid equal to the bounds of all rows (dsa_encode_grid_sequential_batch in the same process);
the handle's entry rows must be the twin's kept rows for every attribute and its row entries the twin's.  The shapes sit on the
kernels' edges: the 64 entries of a step, the tile, runs of equal keys across both, tiles without a head; the cells of those are
exact by construction (mergecases.along_z)."""
import ctypes as C

import numpy as np
import pytest

import encodecall
import mergecases as mc
import ordercases as oc
import draco_sharp_amd as dsa
import draco_sharp_amd.synth as synth
from draco_sharp_amd import native

pytestmark = pytest.mark.gpu

T = dsa.ENCODE_ORDER_TILE


@pytest.fixture(scope="module")
def ctx():
    c = dsa.Context(0)
    yield c
    c.close()


def synth_grid(g):
    return None if g is None else synth.grid(g.origin, g.range)


def config(merge=dsa.MERGE_CELLS, order=dsa.POINT_ORDER_MORTON, **kw):
    return dsa.Config(encoding_method=0, point_order=order, merge_points=merge, **kw)


def cloud(c, **kw):
    return dsa.PointCloudData(c.pos, position_grid=None if c.grid is None else dsa.Grid(c.grid[0], float(c.grid[1])), **kw)


def cpu_args(m, cfg):
    """the arguments of synth.encode_merged for PointCloudData m (explicit grids only)"""
    extra = [synth.Extra(a.values, a.attribute_type, a.normalized, a.unique_id, a.quantization_bits, grid=synth_grid(a.grid)) for a in m.attributes] or None
    opt = synth.options(pos_bits=cfg.position_bits, uv_bits=cfg.texcoord_bits, normal_bits=cfg.normal_bits, force_scheme=cfg.symbol_scheme,
                        compression_level=10 - cfg.speed, generic_components=m.generic.shape[1] if m.generic is not None else 1)
    return dict(pos=m.positions, normals=m.normals, uvs=m.texcoords, generic=m.generic, extra=extra, opt=opt,
                pos_grid=synth_grid(m.position_grid), uv_grid=synth_grid(m.texcoord_grid))


def bounds(values):
    """the explicit grid equal to the own bounds of float32 values (N, nc): minima, largest extent in float32, 1 where that is 0"""
    v = np.asarray(values, np.float32).reshape(len(values), -1)
    mn = v.min(axis=0)
    rng = np.float32((v.max(axis=0) - mn).astype(np.float32).max())
    return dsa.Grid(mn, float(rng) if rng != 0 else 1.0)


def kept_rows(m, kept):
    """the cloud the plain call is given: every array at [kept], every quantised attribute on the bounds of ALL its rows (or the
    grid it came with)"""
    atts = [dsa.Attribute(a.values[kept], a.attribute_type, a.normalized, a.unique_id, a.quantization_bits,
                          grid=a.grid if a.grid is not None or a.values.dtype != np.float32 else bounds(a.values)) for a in m.attributes] or None
    take = lambda a: None if a is None else a[kept]          # noqa: E731
    return dsa.PointCloudData(m.positions[kept], normals=take(m.normals), texcoords=take(m.texcoords), generic=take(m.generic), attributes=atts,
                              position_grid=m.position_grid if m.position_grid is not None else bounds(m.positions),
                              texcoord_grid=m.texcoord_grid if m.texcoord_grid is not None else (None if m.texcoords is None else bounds(m.texcoords)))


def check(ctx, clouds, plain_too=True, **kw):
    """The merged streams of the batch against the CPU coder's, their entry rows and row entries against synth.merge_points, and
    (plain_too) against the device's plain streams of the kept rows.  Returns [(kept, row_entries)]."""
    cfg = config(**kw)
    got = dsa.DracoEncoder(ctx).EncodeBatch(clouds, cfg)
    out = []
    for i, m in enumerate(clouds):
        want, kept, cells = synth.encode_merged(**cpu_args(m, cfg))
        rows = got.entry_rows(i)
        assert len(rows) == 1 + (m.normals is not None) + (m.texcoords is not None) + (m.generic is not None) + len(m.attributes), i
        for k, r in enumerate(rows):
            assert r.dtype == np.uint32 and np.array_equal(r, kept), (i, len(m.positions), len(kept), k, len(r))
        re = got.row_entries(i)
        assert re.dtype == np.uint32 and np.array_equal(re, cells), (i, len(m.positions), np.flatnonzero(np.asarray(re) != cells)[:4])
        assert got[i] == want, (i, len(m.positions), len(kept), len(got[i]), len(want))
        out.append((kept, cells))
    if plain_too:
        plain = dsa.DracoEncoder(ctx).EncodeBatch([kept_rows(m, k) for m, (k, _) in zip(clouds, out)], dsa.Config(encoding_method=0, **kw))
        for i in range(len(clouds)):
            assert plain[i] == got[i], i
        plain.close()
    got.close()
    return out


def test_sizes_around_the_tile_in_one_batch(ctx):
    cases = mc.sized()
    assert sorted({len(c.pos) for c in cases}) == [1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1] and len(cases) == 30 and mc.TILE == T
    out = check(ctx, [cloud(c) for c in cases], position_bits=cases[0].bits)
    for c, (kept, cells) in zip(cases, out):
        n = len(c.pos)
        assert len(kept) == {"distinct": n, "identical": 1, "twice": (n + 1) // 2}[c.name.split("-")[0]], c.name
        assert np.array_equal(cells, c.pos[:, 2].astype(np.int64))


@pytest.mark.parametrize("together", [False, True])
def test_runs_across_the_kernels_boundaries(ctx, together):
    """runs of equal keys over sorted entries 63|64 and 1023|1024, a run of 1 500, a run that is two whole tiles, a head exactly
    at the first entry of a tile, a tile with no head: a cloud each, and one cloud with all of them"""
    cases = mc.boundary_runs()
    assert [c.name for c in cases] == ["run-over-63|64", "run-over-1023|1024", "run-of-1500", "two-whole-tiles", "head-at-a-tile-start", "tile-with-no-head",
                                       "heads-at-every-64", "all-of-it"]
    assert all(mc.spans(cases[-1]).values()), mc.spans(cases[-1])
    group = cases[-1:] if together else cases[:-1]
    out = check(ctx, [cloud(c) for c in group], position_bits=group[0].bits)
    for c, (kept, cells) in zip(group, out):
        z = c.pos[:, 2].astype(np.int64)
        assert len(kept) == len(mc.runs_of(c)) and np.array_equal(cells, z) and np.array_equal(kept, [np.flatnonzero(z == j)[0] for j in range(len(kept))])


def attributes_of(n, seed):
    rng = np.random.default_rng(seed)
    return dict(normals=rng.normal(size=(n, 3)).astype(np.float32), texcoords=rng.random((n, 2)).astype(np.float32),
                generic=rng.integers(0, 256, (n, 3)).astype(np.uint8),
                attributes=[dsa.Attribute(rng.integers(-3000, 3000, (n, 3)).astype(np.int16)),           # rows of 6 bytes: not 4-byte aligned
                            dsa.Attribute(rng.integers(0, 100000, (n, 1)).astype(np.uint32)),
                            dsa.Attribute(rng.random((n, 2)).astype(np.float32), quantization_bits=12)])


def test_every_stream_kind_goes_through_the_kept_map(ctx):
    cases = [mc.half_duplicated(n, 70 + n) for n in (1, 777, T + 5)]
    out = check(ctx, [cloud(c, **attributes_of(len(c.pos), len(c.pos))) for c in cases])
    for c, (kept, _) in zip(cases[1:], out[1:]):
        assert 0.4 * len(c.pos) < len(kept) < 0.75 * len(c.pos)


def test_grids(ctx):
    # own bounds whose minimum and maximum of every component are held by rows the merge drops
    c = mc.dropped_extremes()
    (kept, cells), = check(ctx, [cloud(c, texcoords=np.ascontiguousarray(c.pos[:, :2]))], position_bits=c.bits)
    assert 4 not in kept and 5 not in kept and 2 in kept and 3 in kept and cells[4] == cells[2] and cells[5] == cells[3]
    assert not np.array_equal(c.pos[kept].min(axis=0), c.pos.min(axis=0)) and not np.array_equal(c.pos[kept].max(axis=0), c.pos.max(axis=0))
    # an explicit grid
    e = mc.explicit()
    (kept, _), = check(ctx, [cloud(e)], position_bits=e.bits)
    assert len(kept) < len(e.pos)
    # two clouds of one group on a shared grid: the cells are those of the group's grid, not of each cloud's own bounds
    a, b = mc.half_duplicated(900, 71).pos, mc.half_duplicated(1100, 72).pos * np.float32(0.5) + np.float32(2.0)
    cfg = config(position_bits=4)
    got = dsa.DracoEncoder(ctx).EncodeBatch([dsa.PointCloudData(p, position_grid=dsa.Grid.shared(), group=5) for p in (a, b)], cfg)
    sg = synth.shared_grid([a, b])
    own = 0
    for i, p in enumerate((a, b)):
        want, kept, cells = synth.encode_merged(p, opt=synth.options(pos_bits=4), pos_grid=sg)
        assert got[i] == want and np.array_equal(got.entry_rows(i)[0], kept) and np.array_equal(got.row_entries(i), cells)
        own += len(kept) != len(synth.merge_points(p, 4)[0])
    assert own > 0
    plain = dsa.DracoEncoder(ctx).EncodeBatch([dsa.PointCloudData(p[synth.merge_points(p, 4, sg)[0]], position_grid=dsa.Grid(sg.origin[:3], float(sg.range))) for p in (a, b)],
                                              dsa.Config(encoding_method=0, position_bits=4))
    assert plain[0] == got[0] and plain[1] == got[1]
    plain.close()
    got.close()


@pytest.mark.parametrize("host_plan", ["0", "1"])
@pytest.mark.parametrize("count", [8, 1500])
def test_chunks_and_plans(ctx, monkeypatch, count, host_plan):
    """1 500 clouds of 40 points with duplicates cross a chunk boundary; 8 are one small chunk; the symbol plans by the host and by
    the device"""
    monkeypatch.setenv("DSA_ENC_HOST_PLAN", host_plan)
    rng = np.random.default_rng(90)
    clouds = []
    for _ in range(count):
        p = rng.random((25, 3)).astype(np.float32)
        clouds.append(dsa.PointCloudData(np.ascontiguousarray(np.concatenate([p, p[rng.integers(0, 25, 15)]])[rng.permutation(40)])))
    out = check(ctx, clouds, plain_too=count == 8)
    assert all(len(k) == 25 for k, _ in out)


def test_round_trip(ctx):
    cases = [mc.large(), mc.half_duplicated(2 * T + 77, 95), mc.dropped_extremes()]
    assert 60000 < len(cases[0].pos) < 80000
    for c in cases:
        m = cloud(c, **attributes_of(len(c.pos), 96))
        enc = dsa.DracoEncoder(ctx)
        merged = enc.EncodeBatch([m], config(position_bits=c.bits))
        kept, cells, want_q = mc.pin(c.pos, c.bits, c.grid)
        assert np.array_equal(merged.entry_rows(0)[0], kept) and np.array_equal(merged.row_entries(0), cells)
        plain = enc.EncodeBatch([kept_rows(m, kept)], dsa.Config(encoding_method=0, position_bits=c.bits))
        b = dsa.Batch(ctx, [merged[0], plain[0]])
        b.decode()
        rows = b.source_rows(merged, encoded_mesh=[0, 0])
        assert b.status(0) == 0 and b.status(1) == 0
        o, p = b.result(0).ConnectedData, b.result(1).ConnectedData
        assert o.PointsCount == len(kept) == len(want_q) and len(o.Attributes) == len(p.Attributes) == len(rows[0]) == 7
        assert np.array_equal(np.asarray(o.Attributes[0].PortableValues).reshape(-1, 3), want_q)          # the unique cells, in Morton order
        for a, (x, y) in enumerate(zip(o.Attributes, p.Attributes)):
            assert np.array_equal(np.asarray(rows[0][a]), kept), a
            assert np.array_equal(np.ascontiguousarray(x.Values).view(np.uint8), np.ascontiguousarray(y.Values).view(np.uint8)), a
        b.close()
        merged.close()
        plain.close()


def merge_options(merge, order, geometry=0):
    o = native.EncodeMergeOptions()
    native.lib().dsa_encode_default_merge_options(C.byref(o))
    o.merge_points, o.order.point_order, o.order.sequential.geometry = merge, order, geometry
    return o


def call(ctx, meshes, o, edit=None):
    arr, grids, keep = encodecall.arrays(meshes)
    if edit:
        edit(arr, keep)
    h = C.c_void_p()
    st = native.lib().dsa_encode_merged_sequential_batch(ctx._h, len(meshes), arr, grids, C.byref(o), C.byref(h))
    return st, h


def test_merge_0_through_the_new_entry_is_the_ordered_call(ctx):
    L = native.lib()
    meshes = [cloud(mc.half_duplicated(n, 120 + n), **attributes_of(n, n)) for n in (5, 1500)]
    count = C.c_uint32()
    for order in (0, 1):
        st, h = call(ctx, meshes, merge_options(0, order))
        assert st == 0
        rows = []
        for i, m in enumerate(meshes):
            assert L.dsa_encoded_attributes(h, i, C.byref(count)) == 0 and count.value == 7
            r = np.zeros(len(m.positions), np.uint32)
            assert L.dsa_encoded_entry_rows(h, i, 6, r.ctypes.data, len(r), C.byref(count)) == 0 and count.value == len(r)
            rows.append(r)
            # such a handle keeps no row entries, and says which option would
            assert L.dsa_encoded_row_entries(h, i, None, 0, C.byref(count)) == native.DSA_ERR_INVALID_ARGUMENT and "merge_points" in ctx.error()
        new = encodecall.streams(ctx, h, len(meshes))
        oo = merge_options(0, order).order
        arr, grids, keep = encodecall.arrays(meshes)
        h2 = C.c_void_p()
        assert L.dsa_encode_ordered_sequential_batch(ctx._h, len(meshes), arr, grids, C.byref(oo), C.byref(h2)) == 0
        for i, m in enumerate(meshes):
            r = np.zeros(len(m.positions), np.uint32)
            assert L.dsa_encoded_entry_rows(h2, i, 0, r.ctypes.data, len(r), C.byref(count)) == 0 and np.array_equal(r, rows[i])
            assert np.array_equal(r, synth.point_order(m.positions, 11) if order else np.arange(len(r)))
        old = encodecall.streams(ctx, h2, len(meshes))
        assert new == old and all(s == 0 for s, _ in new)
    # ... and the option check answers before any mesh is looked at, naming the field
    for o, text in ((merge_options(2, 1), "merge_points 2"), (merge_options(-1, 1), "merge_points -1"),
                    (merge_options(1, 0), "merge_points 1 needs point_order 1"), (merge_options(1, 1, geometry=1), "merge_points 1 needs geometry 0")):
        st, _ = call(ctx, meshes, o)
        assert st == native.DSA_ERR_INVALID_ARGUMENT and text in ctx.error(), (text, ctx.error())
    o = merge_options(1, 1)
    o.reserved[3] = 1
    assert call(ctx, meshes, o)[0] == native.DSA_ERR_INVALID_ARGUMENT and "dsa_encode_merge_options.reserved[3]" in ctx.error()
    o = merge_options(0, 2)                     # what the nested structs refuse, in their words
    assert call(ctx, meshes, o)[0] == native.DSA_ERR_INVALID_ARGUMENT and "point_order 2" in ctx.error()
    o = merge_options(1, 1)
    o.order.reserved[1] = 1
    assert call(ctx, meshes, o)[0] == native.DSA_ERR_INVALID_ARGUMENT and "dsa_encode_order_options.reserved[1]" in ctx.error()
    o = merge_options(1, 1)
    o.order.sequential.reserved[0] = 1
    assert call(ctx, meshes, o)[0] == native.DSA_ERR_INVALID_ARGUMENT and "dsa_encode_sequential_options.reserved[0]" in ctx.error()


def test_a_refused_cloud_fails_alone_with_the_text_it_has(ctx):
    """a cloud with a NaN on a grid, and a cloud whose generic attribute claims 9 components, fail alone with the plain call's
    status and text; their neighbours code"""
    g = dsa.Grid([0, 0, 0], 2.0)
    good = [mc.half_duplicated(500, 81).pos, mc.half_duplicated(1300, 82).pos]
    bad = oc.random_cloud(800, 83)
    bad[417, 2] = np.nan
    meshes = [dsa.PointCloudData(good[0], position_grid=g), dsa.PointCloudData(bad, position_grid=g),
              dsa.PointCloudData(good[0], generic=np.zeros((500, 2), np.uint8), position_grid=g), dsa.PointCloudData(good[1], position_grid=g)]

    def bad_generic(arr, keep):
        arr[2].mesh.mesh.generic_components = 9
    st, h = call(ctx, meshes, merge_options(1, 1), edit=bad_generic)
    assert st == 0
    count = C.c_uint32()
    assert native.lib().dsa_encoded_row_entries(h, 1, None, 0, C.byref(count)) == native.DSA_ERR_INVALID_ARGUMENT and "row 417" in ctx.error()
    assert native.lib().dsa_encoded_row_entries(h, 3, None, 0, C.byref(count)) == 0 and count.value == 1300
    merged = encodecall.streams(ctx, h, 4)
    st, plain = encodecall.call(ctx, "dsa_encode_grid_sequential_batch", meshes, merge_options(0, 0).order.sequential, edit=bad_generic)
    assert st == 0
    assert merged[1] == plain[1] and merged[1][0] == native.DSA_ERR_INVALID_ARGUMENT and "row 417" in merged[1][1]
    assert merged[2] == plain[2] and merged[2][0] == native.DSA_ERR_INVALID_ARGUMENT and "generic attribute needs 1 - 4 components" in merged[2][1]
    for i in (0, 3):
        want, kept, _ = synth.encode_merged(meshes[i].positions, opt=synth.options(pos_bits=11), pos_grid=synth.grid([0, 0, 0], 2.0))
        assert merged[i] == (0, want) and len(kept) < len(meshes[i].positions)
