"""Encode direction, the Morton order of a point cloud in parts of bounded size on the device (dsa_encode_split_sequential_batch,
part_points >= 1; Config(part_points=N); k_enc_part_bounds of draco-sharp_amd/csrc/dsa_encode_order.h and the per-part stream
records of dsa_encode_layout.h).  Every part's stream must be, byte for byte, the CPU coder's (synth.encode_split) and the device's
own plain stream of the slice with every quantised attribute on an explicit grid equal to the bounds of all the cloud's rows
(dsa_encode_grid_sequential_batch in the same process); the handle's slots, entry rows and part records must be the twin's.  The
shapes sit on the kernels' edges: the 64 entries of a wave step and the 1024-entry tile (splitcases)."""
import ctypes as C

import numpy as np
import pytest

import encodecall
import mergecases as mc
import ordercases as oc
import splitcases as sc
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


def config(N, **kw):
    return dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, part_points=N, **kw)


def cloud(c, **kw):
    return dsa.PointCloudData(c.pos, position_grid=None if c.grid is None else dsa.Grid(c.grid[0], float(c.grid[1])), **kw)


def cpu_args(m, cfg):
    """the arguments of synth.encode_split for PointCloudData m (explicit grids only)"""
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


def slice_of(m, rows):
    """the cloud the plain call is given for a part: every array at [rows], every quantised attribute on the bounds of ALL the
    cloud's rows (or the grid it came with)"""
    atts = [dsa.Attribute(a.values[rows], a.attribute_type, a.normalized, a.unique_id, a.quantization_bits,
                          grid=a.grid if a.grid is not None or a.values.dtype != np.float32 else bounds(a.values)) for a in m.attributes] or None
    take = lambda a: None if a is None else a[rows]          # noqa: E731
    return dsa.PointCloudData(m.positions[rows], normals=take(m.normals), texcoords=take(m.texcoords), generic=take(m.generic), attributes=atts,
                              position_grid=m.position_grid if m.position_grid is not None else bounds(m.positions),
                              texcoord_grid=m.texcoord_grid if m.texcoord_grid is not None else (None if m.texcoords is None else bounds(m.texcoords)))


def check_handle(got, i, first, twin, attributes, bits):
    """slots first .. of `got` against the twin's parts of input i: streams, entry rows, part records; returns the slot behind"""
    r = got.parts(i)
    assert r == range(first, first + len(twin)), (i, r, len(twin))
    lo = 0
    for p, (s, (want, rows, qmin, qmax)) in enumerate(zip(r, twin)):
        assert got[s] == want, (i, p, len(got[s]), len(want))
        er = got.entry_rows(s)
        assert len(er) == attributes
        for k, e in enumerate(er):
            assert e.dtype == np.uint32 and np.array_equal(e, rows), (i, p, k)
        info = got.part_info(s)
        assert (info.input, info.part, info.parts, info.first_entry, info.num_points, info.position_bits) == (i, p, len(twin), lo, len(rows), bits), (i, p)
        assert np.array_equal(list(info.qmin), qmin) and np.array_equal(list(info.qmax), qmax) and list(info.reserved) == [0, 0], (i, p, list(info.qmin), qmin)
        lo += len(rows)
    return first + len(twin)


def check(ctx, clouds, N, plain_too=True, **kw):
    """The parts of every cloud of the batch against the CPU coder's (streams, slots, rows, part records) and (plain_too) against
    the device's plain streams of the slices.  Returns the twin's [(stream, rows, qmin, qmax)] per cloud."""
    cfg = config(N, **kw)
    got = dsa.DracoEncoder(ctx).EncodeBatch(clouds, cfg)
    out, first = [], 0
    for i, m in enumerate(clouds):
        twin = synth.encode_split(part_points=N, **cpu_args(m, cfg))
        assert len(twin) == len(sc.parts(len(m.positions), N))
        attributes = 1 + (m.normals is not None) + (m.texcoords is not None) + (m.generic is not None) + len(m.attributes)
        first = check_handle(got, i, first, twin, attributes, cfg.position_bits)
        out.append(twin)
    assert len(got) == first
    if plain_too:
        plain = dsa.DracoEncoder(ctx).EncodeBatch([slice_of(m, rows) for m, twin in zip(clouds, out) for _, rows, _, _ in twin], dsa.Config(encoding_method=0, **kw))
        assert len(plain) == len(got)
        for s in range(len(got)):
            assert plain[s] == got[s], s
        plain.close()
    got.close()
    return out


def test_sizes_and_part_sizes(ctx):
    """every size around the wave step and the tile at every part size around them: the clouds cut at one part_points are a batch"""
    cases = sc.sized()
    assert sorted({len(c.pos) for c in cases}) == [1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 2 * T, 2 * T + 1] and sc.TILE == T
    every = sorted({c.part_points for c in cases})
    assert {1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T, 2 * T + 1, 2 * T + 2, 2**31 - 1} <= set(every)
    for N in every:
        group = [c for c in cases if c.part_points == N]
        assert N != 1 or max(len(c.pos) for c in group) == 65
        check(ctx, [cloud(c) for c in group], N, position_bits=group[0].bits)


def test_cuts_at_a_wave_step_a_tile_edge_and_inside_a_run(ctx):
    cases = sc.cuts()
    assert [(len(c.pos), c.part_points) for c in cases[:3]] == [(2 * T, T), (2 * T + 1, T + 1), (130, 65)]
    for c in cases:
        (twin,), = [check(ctx, [cloud(c)], c.part_points, position_bits=c.bits)]
        assert len(twin) == len(sc.parts(len(c.pos), c.part_points)) >= 2
    # the run of equal keys over the cut: its points land in two parts and nothing is merged
    c = sc.run_over_a_cut()
    z = c.pos[:, 2].astype(np.int64)
    (a, b), = [[rows for _, rows, _, _ in twin] for twin in check(ctx, [cloud(c)], c.part_points, plain_too=False, position_bits=c.bits)]
    assert len(a) == len(b) == 150 and (z[a] == 2).sum() == 10 and (z[b] == 2).sum() == 10 and z[a[-1]] == z[b[0]] == 2
    assert mc.runs_of(c).tolist() == [100, 40, 20, 140]


def attributes_of(n, seed):
    rng = np.random.default_rng(seed)
    return dict(normals=rng.normal(size=(n, 3)).astype(np.float32), texcoords=rng.random((n, 2)).astype(np.float32),
                generic=rng.integers(0, 256, (n, 3)).astype(np.uint8),
                attributes=[dsa.Attribute(rng.random((n, 2)).astype(np.float32), quantization_bits=12),
                            dsa.Attribute(rng.integers(-3000, 3000, (n, 3)).astype(np.int16))])          # rows of 6 bytes: not 4-byte aligned


def test_one_cloud_carrying_everything(ctx):
    n = 2 * T + 77
    twin, = check(ctx, [dsa.PointCloudData(oc.random_cloud(n, 701), **attributes_of(n, 702))], 700)
    assert len(twin) == 4 and sorted(len(rows) for _, rows, _, _ in twin) == [531, 531, 531, 532]


def test_grids(ctx):
    # an explicit grid
    e = [c for c in sc.cuts() if c.name == "explicit-grid"][0]
    check(ctx, [cloud(e)], e.part_points, position_bits=e.bits)
    # two clouds of one group on a shared grid: the parts of both carry the group's grid in their headers
    a, b = oc.random_cloud(900, 711), oc.random_cloud(1100, 712) * np.float32(0.5) + np.float32(2.0)
    cfg = config(256, position_bits=9)
    got = dsa.DracoEncoder(ctx).EncodeBatch([dsa.PointCloudData(p, position_grid=dsa.Grid.shared(), group=5) for p in (a, b)], cfg)
    sg = synth.shared_grid([a, b])
    first, slices = 0, []
    for i, p in enumerate((a, b)):
        twin = synth.encode_split(p, opt=synth.options(pos_bits=9), pos_grid=sg, part_points=256)
        own = synth.encode_split(p, opt=synth.options(pos_bits=9), part_points=256)
        assert len(twin) == len(own) and all(x[0] != y[0] for x, y in zip(twin, own))
        first = check_handle(got, i, first, twin, 1, 9)
        slices += [dsa.PointCloudData(p[rows], position_grid=dsa.Grid(sg.origin[:3], float(sg.range))) for _, rows, _, _ in twin]
    assert len(got) == first == 4 + 5
    plain = dsa.DracoEncoder(ctx).EncodeBatch(slices, dsa.Config(encoding_method=0, position_bits=9))
    assert list(plain) == list(got)
    plain.close()
    got.close()


@pytest.mark.parametrize("host_plan", ["0", "1"])
@pytest.mark.parametrize("count", [8, 1500])
def test_chunks_and_plans(ctx, monkeypatch, count, host_plan):
    """1 500 clouds of 40 points in parts of at most 16 (3 each) cross a chunk boundary of inputs; 8 are one small chunk; the symbol
    plans by the host and by the device"""
    monkeypatch.setenv("DSA_ENC_HOST_PLAN", host_plan)
    rng = np.random.default_rng(720)
    out = check(ctx, [dsa.PointCloudData(rng.random((40, 3)).astype(np.float32)) for _ in range(count)], 16, plain_too=count == 8)
    assert all([len(rows) for _, rows, _, _ in twin] == [13, 13, 14] for twin in out)


def test_more_streams_than_the_y_of_a_grid(ctx):
    """one cloud in DSA_ENCODE_MAX_PARTS parts of one point, two attributes each: 131 072 stream records in one chunk, which the
    kernels launched over (blocks, streams) take in three slices of at most 65 535 -- the parts on both sides of either edge,
    and a sample of the rest, against the CPU coder"""
    n, bits = native.ENCODE_MAX_PARTS, 4
    pos, nrm = oc.random_cloud(n, 771), np.random.default_rng(772).normal(size=(n, 3)).astype(np.float32)
    got = dsa.DracoEncoder(ctx).EncodeBatch([dsa.PointCloudData(pos, normals=nrm)], config(1, position_bits=bits))
    assert len(got) == n and got.parts(0) == range(0, n)
    perm, q = synth.point_order(pos, bits), mc.quantised(pos, bits)
    opt, grid = synth.options(pos_bits=bits), synth.bounds_grid(pos)
    # stream record 2 p + k is attribute k of part p: records 65 535 and 131 070 open the second and the third slice
    for p in sorted({0, 1, 32766, 32767, 32768, 65534, 65535} | set(range(5, n, 4099))):
        rows = perm[p:p + 1]
        assert got[p] == synth.encode_grid(pos[rows], None, normals=nrm[rows], opt=opt, form=0, geometry=0, pos_grid=grid), p
        info = got.part_info(p)
        assert (info.part, info.parts, info.first_entry, info.num_points) == (p, n, p, 1) and list(info.qmin) == list(info.qmax) == q[rows[0]].tolist(), p
        assert all(np.array_equal(e, rows) for e in got.entry_rows(p)), p
    got.close()


def test_decode(ctx):
    """all parts of two clouds in one Batch: the box of every part is, bit for bit, the box of its decoded positions; the source
    rows are its slice of the order; every attribute is the plain stream's at those rows"""
    n = 2 * T + 77
    clouds = [dsa.PointCloudData(oc.random_cloud(n, 731), **attributes_of(n, 732)), dsa.PointCloudData(oc.height_field(30, 31, 733), **attributes_of(930, 734))]
    enc = dsa.DracoEncoder(ctx)
    split, plain = enc.EncodeBatch(clouds, config(500)), enc.EncodeBatch(clouds, dsa.Config(encoding_method=0))
    k = len(split)
    assert k == 5 + 2 and [split.parts(i) for i in range(2)] == [range(0, 5), range(5, 7)]
    b = dsa.Batch(ctx, list(split) + list(plain))
    b.decode()
    rows = b.source_rows(split, encoded_mesh=list(range(k)) + [0, 0])
    whole = [b.result(k + i).ConnectedData for i in range(2)]
    for s in range(k):
        info = split.part_info(s)
        m = clouds[info.input]
        perm = synth.point_order(m.positions, 11)[info.first_entry:info.first_entry + info.num_points]
        assert b.status(s) == 0
        o = b.result(s).ConnectedData
        assert o.PointsCount == info.num_points and len(o.Attributes) == len(rows[s]) == 6
        pos = np.ascontiguousarray(o.Attributes[0].Values, np.float32).reshape(-1, 3)
        assert np.array_equal(pos.min(axis=0).view(np.uint32), np.float32(list(info.box_min)).view(np.uint32)), (s, pos.min(axis=0), list(info.box_min))
        assert np.array_equal(pos.max(axis=0).view(np.uint32), np.float32(list(info.box_max)).view(np.uint32)), (s, pos.max(axis=0), list(info.box_max))
        q = np.asarray(o.Attributes[0].PortableValues).reshape(-1, 3)
        assert np.array_equal(q.min(axis=0), list(info.qmin)) and np.array_equal(q.max(axis=0), list(info.qmax))
        for a, (x, y) in enumerate(zip(o.Attributes, whole[info.input].Attributes)):
            r = np.asarray(rows[s][a]).astype(np.int64)
            assert np.array_equal(r, perm), (s, a)
            xv, yv = np.ascontiguousarray(x.Values), np.ascontiguousarray(y.Values)
            assert np.array_equal(xv.view(np.uint8), np.ascontiguousarray(yv[r]).view(np.uint8)), (s, a)
    b.close()
    split.close()
    plain.close()


def split_options(N, order=1, geometry=0, merge=0):
    o = native.EncodeSplitOptions()
    native.lib().dsa_encode_default_split_options(C.byref(o))
    o.part_points, o.merge.merge_points, o.merge.order.point_order, o.merge.order.sequential.geometry = N, merge, order, geometry
    return o


def call(ctx, meshes, o, edit=None):
    arr, grids, keep = encodecall.arrays(meshes)
    if edit:
        edit(arr, keep)
    h = C.c_void_p()
    st = native.lib().dsa_encode_split_sequential_batch(ctx._h, len(meshes), arr, grids, C.byref(o), C.byref(h))
    return st, h


def test_a_refused_cloud_fails_alone_in_its_one_slot(ctx):
    """a cloud with a NaN on a grid, between two good clouds: one slot with the plain call's status and text; the neighbours' parts
    are what they are without it"""
    L = native.lib()
    g = dsa.Grid([0, 0, 0], 2.0)
    good = [oc.random_cloud(500, 741), oc.random_cloud(1300, 742)]
    bad = oc.random_cloud(800, 743)
    bad[417, 2] = np.nan
    meshes = [dsa.PointCloudData(good[0], position_grid=g), dsa.PointCloudData(bad, position_grid=g), dsa.PointCloudData(good[1], position_grid=g)]
    st, h = call(ctx, meshes, split_options(300))
    assert st == 0 and L.dsa_encoded_size(h) == 2 + 1 + 5
    first, count, info = C.c_uint32(), C.c_uint32(), native.PartInfo()
    slots = []
    for i in range(3):
        assert L.dsa_encoded_parts(h, i, C.byref(first), C.byref(count)) == 0
        slots.append((first.value, count.value))
    assert slots == [(0, 2), (2, 1), (3, 5)] and L.dsa_encoded_parts(h, 3, C.byref(first), C.byref(count)) == native.DSA_ERR_INVALID_ARGUMENT
    assert L.dsa_encoded_part_info(h, 2, C.byref(info)) == native.DSA_ERR_INVALID_ARGUMENT and "row 417" in ctx.error()
    assert L.dsa_encoded_part_info(h, 7, C.byref(info)) == 0 and (info.input, info.part, info.parts, info.first_entry, info.num_points) == (2, 4, 5, 1040, 260)
    assert L.dsa_encoded_row_entries(h, 0, None, 0, C.byref(count)) == native.DSA_ERR_INVALID_ARGUMENT and "merge_points" in ctx.error()
    got = encodecall.streams(ctx, h, 8)
    st, plain = encodecall.call(ctx, "dsa_encode_grid_sequential_batch", meshes, split_options(0).merge.order.sequential)
    # (the accessors name the slot they were asked for: "mesh 2: ..." here, "mesh 1: ..." there)
    assert st == 0 and got[2][0] == plain[1][0] == native.DSA_ERR_INVALID_ARGUMENT and got[2][1].split(": ", 1)[1] == plain[1][1].split(": ", 1)[1]
    assert "row 417" in got[2][1]
    want = []
    for p in good:
        want += [(0, t[0]) for t in synth.encode_split(p, opt=synth.options(pos_bits=11), pos_grid=synth.grid([0, 0, 0], 2.0), part_points=300)]
    assert got[:2] + got[3:] == want


def test_the_cap_and_the_refusals_of_the_call(ctx):
    L = native.lib()
    small = dsa.PointCloudData(oc.random_cloud(5, 751))
    over = dsa.PointCloudData(oc.random_cloud(native.ENCODE_MAX_PARTS + 1, 752))
    st, h = call(ctx, [small, over, small], split_options(1))
    assert st == 0 and L.dsa_encoded_size(h) == 5 + 1 + 5
    got = encodecall.streams(ctx, h, 11)
    assert got[5][0] == native.DSA_ERR_INVALID_ARGUMENT and all(w in got[5][1] for w in ("part_points 1", "n = 65537", "65536"))
    one = synth.encode_split(small.positions, opt=synth.options(pos_bits=11), part_points=1)
    assert got[:5] == got[6:] == [(0, t[0]) for t in one]
    # the option check answers before any mesh is looked at, naming the field
    for o, text in ((split_options(-1), "part_points -1"), (split_options(7, order=0), "part_points 7 needs point_order 1"),
                    (split_options(7, geometry=1), "part_points 7 needs geometry 0"), (split_options(7, merge=1), "part_points 7 with merge_points 1")):
        st, _ = call(ctx, [small], o)
        assert st == native.DSA_ERR_INVALID_ARGUMENT and text in ctx.error(), (text, ctx.error())
    o = split_options(7)
    o.reserved[3] = 1
    assert call(ctx, [small], o)[0] == native.DSA_ERR_INVALID_ARGUMENT and "dsa_encode_split_options.reserved[3]" in ctx.error()
    o = split_options(7)                        # what the nested structs refuse, in their words
    o.merge.reserved[1] = 1
    assert call(ctx, [small], o)[0] == native.DSA_ERR_INVALID_ARGUMENT and "dsa_encode_merge_options.reserved[1]" in ctx.error()
    assert call(ctx, [small], split_options(0, merge=2))[0] == native.DSA_ERR_INVALID_ARGUMENT and "merge_points 2" in ctx.error()


def test_part_points_0_through_the_new_entry_is_the_merged_call(ctx):
    L = native.lib()
    meshes = [cloud(mc.half_duplicated(n, 760 + n), **attributes_of(n, n)) for n in (5, 1500)]
    bad = oc.random_cloud(300, 761)
    bad[17, 0] = np.inf
    meshes.insert(1, dsa.PointCloudData(bad, position_grid=dsa.Grid([0, 0, 0], 2.0)))
    count, first, info = C.c_uint32(), C.c_uint32(), native.PartInfo()
    for merge in (0, 1):
        st, h = call(ctx, meshes, split_options(0, merge=merge))
        assert st == 0 and L.dsa_encoded_size(h) == 3
        arr, grids, keep = encodecall.arrays(meshes)
        h2 = C.c_void_p()
        assert L.dsa_encode_merged_sequential_batch(ctx._h, 3, arr, grids, C.byref(split_options(0, merge=merge).merge), C.byref(h2)) == 0
        for i, m in enumerate(meshes):
            # a handle without parts: every input is its own slot, and part_info says which option would give parts
            assert L.dsa_encoded_parts(h, i, C.byref(first), C.byref(count)) == 0 and (first.value, count.value) == (i, 1)
            assert L.dsa_encoded_parts(h2, i, C.byref(first), C.byref(count)) == 0 and (first.value, count.value) == (i, 1)
            assert L.dsa_encoded_part_info(h, i, C.byref(info)) == native.DSA_ERR_INVALID_ARGUMENT and "part_points" in ctx.error()
            if i == 1:
                continue
            rows = []
            for hh in (h, h2):
                assert L.dsa_encoded_entry_rows(hh, i, 4, None, 0, C.byref(count)) == 0
                r = np.zeros(count.value, np.uint32)
                assert L.dsa_encoded_entry_rows(hh, i, 4, r.ctypes.data, len(r), C.byref(count)) == 0
                cells = np.zeros(len(m.positions), np.uint32)
                assert (L.dsa_encoded_row_entries(hh, i, cells.ctypes.data, len(cells), C.byref(count)) == 0) == (merge == 1)
                rows.append((r, cells))
            assert np.array_equal(rows[0][0], rows[1][0]) and np.array_equal(rows[0][1], rows[1][1])
            assert len(rows[0][0]) < len(m.positions) if merge and i == 2 else len(rows[0][0]) <= len(m.positions)
        new, old = encodecall.streams(ctx, h, 3), encodecall.streams(ctx, h2, 3)
        assert new == old and new[0][0] == 0 and new[2][0] == 0 and new[1][0] == native.DSA_ERR_INVALID_ARGUMENT and "row 17" in new[1][1]
