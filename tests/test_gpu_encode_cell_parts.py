"""Encode direction, one point per quantisation cell AND parts of bounded size, sized on the device
(dsa_encode_cell_parts_sequential_batch, part_cells >= 1; Config(merge_points=MERGE_CELLS, part_cells=N); k_enc_part_cells of
draco-sharp_amd/csrc/dsa_encode_order.h and the part slots of dsa_encode_layout.h).  Every part's stream must be, byte for byte, the
CPU coder's (synth.encode_cell_parts); the handle's slots, slices of kept, row entries and part records must be the twin's; all
parts decode side by side to the merged single stream's points.  The shapes sit on the kernels' edges: the 64 entries of a wave
step and the 1024-entry tile, in numbers of kept points and in part sizes (cellpartcases), with clouds that leave every slot but
the first empty."""
import ctypes as C

import numpy as np
import pytest

import cellpartcases as cc
import encodecall
import mergecases as mc
import oracle
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


def config(N, **kw):
    return dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, merge_points=dsa.MERGE_CELLS, part_cells=N, **kw)


def cloud(c, **kw):
    return dsa.PointCloudData(c.pos, position_grid=None if c.grid is None else dsa.Grid(c.grid[0], float(c.grid[1])), **kw)


def cpu_args(m, cfg):
    """the arguments of synth.encode_cell_parts for PointCloudData m (explicit grids only)"""
    extra = [synth.Extra(a.values, a.attribute_type, a.normalized, a.unique_id, a.quantization_bits, grid=synth_grid(a.grid)) for a in m.attributes] or None
    opt = synth.options(pos_bits=cfg.position_bits, uv_bits=cfg.texcoord_bits, normal_bits=cfg.normal_bits, force_scheme=cfg.symbol_scheme,
                        compression_level=10 - cfg.speed, generic_components=m.generic.shape[1] if m.generic is not None else 1)
    return dict(pos=m.positions, normals=m.normals, uvs=m.texcoords, generic=m.generic, extra=extra, opt=opt,
                pos_grid=synth_grid(m.position_grid), uv_grid=synth_grid(m.texcoord_grid))


def dequantized(q, origin, rng, bits):
    """the decoder's float of integer q: every step rounded to float32"""
    delta = np.float32(rng) / np.float32((1 << bits) - 1)
    return (np.asarray(q, np.float32) * delta).astype(np.float32) + np.asarray(origin, np.float32)


def check_handle(ctx, got, i, first, m, twin, attributes, bits):
    """slots first .. of `got` against the twin's parts of input i (PointCloudData m): streams, slices of kept, row entries, part
    records with their boxes, row_parts; returns the slot behind"""
    r = got.parts(i)
    assert r == range(first, first + len(twin.streams)), (i, r, len(twin.streams))
    grid = synth_grid(m.position_grid) or synth.bounds_grid(m.positions)
    for p, (s, want, (lo, hi)) in enumerate(zip(r, twin.streams, twin.ranges)):
        assert got[s] == want, (i, p, len(got[s]), len(want))
        er = got.entry_rows(s)
        assert len(er) == attributes
        for k, e in enumerate(er):
            assert e.dtype == np.uint32 and np.array_equal(e, twin.kept[lo:hi]), (i, p, k)
        info = got.part_info(s)
        assert (info.input, info.part, info.parts, info.first_entry, info.num_points, info.position_bits) == (i, p, len(twin.streams), lo, hi - lo, bits), (i, p)
        assert np.array_equal(list(info.qmin), twin.qmin[p]) and np.array_equal(list(info.qmax), twin.qmax[p]) and list(info.reserved) == [0, 0], (i, p, list(info.qmin), twin.qmin[p])
        for box, q in ((info.box_min, twin.qmin[p]), (info.box_max, twin.qmax[p])):
            assert np.array_equal(np.float32(list(box)).view(np.uint32), dequantized(q, grid.origin[:3], grid.range, bits).view(np.uint32)), (i, p)
        if p:               # row_entries are the cloud's, kept once: a later slot names the first
            with pytest.raises(Exception, match=r"ask its first stream, %d\b" % first):
                got.row_entries(s)
    cells = got.row_entries(first)
    assert cells.dtype == np.uint32 and np.array_equal(cells, twin.row_entries), i
    part, entry = got.row_parts(i)
    want_part = np.searchsorted(twin.ranges[:, 0], twin.row_entries, side="right") - 1
    assert np.array_equal(part, want_part) and np.array_equal(entry, twin.row_entries - twin.ranges[want_part, 0]), i
    assert np.array_equal(twin.kept[twin.ranges[part, 0] + entry], twin.kept[twin.row_entries])
    return first + len(twin.streams)


def check(ctx, clouds, N, **kw):
    """The parts of every cloud of the batch against the CPU coder's.  Returns the twin's CellParts per cloud."""
    cfg = config(N, **kw)
    got = dsa.DracoEncoder(ctx).EncodeBatch(clouds, cfg)
    out, first = [], 0
    for i, m in enumerate(clouds):
        twin = synth.encode_cell_parts(part_cells=N, **cpu_args(m, cfg))
        attributes = 1 + (m.normals is not None) + (m.texcoords is not None) + (m.generic is not None) + len(m.attributes)
        first = check_handle(ctx, got, i, first, m, twin, attributes, cfg.position_bits)
        out.append(twin)
    assert len(got) == first
    got.close()
    return out


def test_kept_points_and_part_sizes(ctx):
    """every number of kept points around the wave step and the tile -- all distinct, every cell twice, all identical -- at every part
    size around them: the clouds cut at one part_cells are a batch"""
    cases = cc.sized() + cc.full_slots()
    assert cc.TILE == T and {c.part_cells for c in cases} >= {1, 2, 63, 64, 65, T - 1, T, T + 1, 2**31 - 1}
    empty = 0
    for N in sorted({c.part_cells for c in cases}):
        group = [c for c in cases if c.part_cells == N]
        assert N > 2 or max(len(c.pos) for c in group) <= 130
        twins = check(ctx, [cloud(c) for c in group], N, position_bits=group[0].bits)
        for c, twin in zip(group, twins):
            assert len(twin.streams) == len(cc.pin(c)[2]) <= cc.slots(c)
            empty += cc.slots(c) - len(twin.streams)
    assert empty > 500          # slots the device left empty


def test_cuts_runs_and_grids(ctx):
    """cuts inside a tile of the sorted order and on its edge, runs of equal keys over a wave step and a tile edge just in front of a
    cut, own bounds and an explicit grid"""
    cases = cc.cuts()
    assert any(c.grid is None for c in cases)
    for c in cases:
        twin, = check(ctx, [cloud(c)], c.part_cells, position_bits=c.bits)
        kept, cells, ranges, qmin, qmax = cc.pin(c)
        assert np.array_equal(twin.kept, kept) and np.array_equal(twin.ranges, ranges) and (len(ranges) >= 2 or c.name == "own-bounds-N440")


def test_the_18_part_cloud(ctx):
    c = cc.large()
    twin, = check(ctx, [cloud(c)], c.part_cells, position_bits=c.bits)
    assert len(c.pos) == 70001 and len(twin.kept) == 2049 and len(twin.streams) == 18 and cc.slots(c) == 584


def attributes_of(n, seed):
    rng = np.random.default_rng(seed)
    return dict(normals=rng.normal(size=(n, 3)).astype(np.float32), texcoords=rng.random((n, 2)).astype(np.float32),
                generic=rng.integers(0, 256, (n, 3)).astype(np.uint8),
                attributes=[dsa.Attribute(rng.random((n, 2)).astype(np.float32), quantization_bits=12),
                            dsa.Attribute(rng.integers(-3000, 3000, (n, 3)).astype(np.int16))])          # rows of 6 bytes: not 4-byte aligned


def test_one_cloud_carrying_everything(ctx):
    c = mc.half_duplicated(2 * T + 77, 801)
    twin, = check(ctx, [cloud(c, **attributes_of(len(c.pos), 802))], 300, position_bits=c.bits)
    m = len(twin.kept)
    assert T < m < len(c.pos) and len(twin.streams) == -(-m // 300) >= 4


def test_a_batch_of_different_clouds_and_a_refused_one(ctx):
    """clouds with different m / n in one call, one of them all identical (one part, every other slot empty), and one with a NaN on
    an explicit grid, which fails alone in its one slot with the plain call's status and text"""
    L = native.lib()
    g = dsa.Grid([0, 0, 0], 2.0)
    good = [mc.half_duplicated(500, 811).pos, np.repeat(oc.random_cloud(1, 812), 700, axis=0), oc.random_cloud(1300, 813), mc.half_duplicated(T + 5, 814).pos]
    bad = oc.random_cloud(800, 815)
    bad[417, 2] = np.nan
    meshes = [dsa.PointCloudData(p, position_grid=g) for p in good[:2]] + [dsa.PointCloudData(bad, position_grid=g)] + [dsa.PointCloudData(p, position_grid=g) for p in good[2:]]
    cfg = config(100, position_bits=4)
    ctx_, h, n = dsa.DracoEncoder(ctx).EncodeBatch(meshes, cfg, handle=True)
    twins = [synth.encode_cell_parts(p, opt=synth.options(pos_bits=4), pos_grid=synth.grid([0, 0, 0], 2.0), part_cells=100) for p in good]
    counts = [len(t.streams) for t in twins]
    assert counts[1] == 1 and len(twins[1].kept) == 1 and all(len(t.kept) < len(p) for t, p in zip(twins, good)) and counts[0] >= 2 and counts[2] >= 3
    assert n == L.dsa_encoded_size(h) == sum(counts) + 1
    first, count, info = C.c_uint32(), C.c_uint32(), native.PartInfo()
    slots = []
    for i in range(5):
        assert L.dsa_encoded_parts(h, i, C.byref(first), C.byref(count)) == 0
        slots.append((first.value, count.value))
    at = np.concatenate([[0], np.cumsum(counts[:2] + [1] + counts[2:])])
    assert slots == [(int(a), int(b - a)) for a, b in zip(at[:-1], at[1:])]
    bad_slot = int(at[2])
    assert L.dsa_encoded_part_info(h, bad_slot, C.byref(info)) == native.DSA_ERR_INVALID_ARGUMENT and "row 417" in ctx.error()
    assert L.dsa_encoded_row_entries(h, bad_slot, None, 0, C.byref(count)) == native.DSA_ERR_INVALID_ARGUMENT and "row 417" in ctx.error()
    got = encodecall.streams(ctx, h, n)
    st, plain = encodecall.call(ctx, "dsa_encode_grid_sequential_batch", meshes, cfg._native_sequential(0))
    assert st == 0 and got[bad_slot][0] == plain[2][0] == native.DSA_ERR_INVALID_ARGUMENT and got[bad_slot][1].split(": ", 1)[1] == plain[2][1].split(": ", 1)[1]
    want = []
    for t in twins:
        want += [(0, s) for s in t.streams]
    assert got[:bad_slot] + got[bad_slot + 1:] == want
    # ... and the handle through the package, for the clouds around the refused one
    ok = [m for k, m in enumerate(meshes) if k != 2]
    got = dsa.DracoEncoder(ctx).EncodeBatch(ok, cfg)
    first = 0
    for i, (m, t) in enumerate(zip(ok, twins)):
        first = check_handle(ctx, got, i, first, m, t, 1, 4)
    got.close()


@pytest.mark.parametrize("host_plan", ["0", "1"])
@pytest.mark.parametrize("count", [8, 1500])
def test_chunks_and_plans(ctx, monkeypatch, count, host_plan):
    """1 500 clouds of 40 points in 3-bit cells, in parts of at most 16 kept points, cross a chunk boundary of inputs; 8 are one small
    chunk; the symbol plans by the host and by the device.  Every cloud has 3 slots, and some fill only 2."""
    monkeypatch.setenv("DSA_ENC_HOST_PLAN", host_plan)
    rng = np.random.default_rng(820)
    clouds = [dsa.PointCloudData((rng.random((40, 3)) * [1.0, 1.0, 0.12]).astype(np.float32)) for _ in range(count)]
    out = check(ctx, clouds, 16, position_bits=3)
    parts = [len(t.streams) for t in out]
    assert set(parts) <= {2, 3} and sum(len(t.kept) < 40 for t in out) > count // 2 and (count == 8 or {2, 3} == set(parts))


def test_decode(ctx):
    """all parts of two clouds in one Batch, beside the merged single streams of the same clouds: positions bit-equal to the oracle,
    the parts one behind the other are the merged stream's points, the source rows are the slices of kept, the box of every part is
    the box of its decoded positions, and no position integer occurs in two parts"""
    clouds = [cloud(mc.half_duplicated(2 * T + 77, 831), **attributes_of(2 * T + 77, 832)), cloud(mc.half_duplicated(930, 833), **attributes_of(930, 834))]
    enc = dsa.DracoEncoder(ctx)
    merged_cfg = dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, merge_points=dsa.MERGE_CELLS)
    parts, merged = enc.EncodeBatch(clouds, config(250)), enc.EncodeBatch(clouds, merged_cfg)
    k = len(parts)
    ranges = [parts.parts(i) for i in range(2)]
    assert ranges[0].start == 0 and ranges[0].stop == ranges[1].start and ranges[1].stop == k and len(ranges[0]) >= 5 and len(ranges[1]) >= 2
    b = dsa.Batch(ctx, list(parts) + list(merged))
    b.decode()
    rows = b.source_rows(parts, encoded_mesh=list(range(k)) + [0, 0])
    for i in range(2):
        whole = b.result(k + i).ConnectedData
        kept = merged.entry_rows(i)[0]
        assert np.array_equal(np.concatenate([parts.entry_rows(s)[0] for s in ranges[i]]), kept)
        joined = [[] for _ in whole.Attributes]
        seen = set()
        for s in ranges[i]:
            info = parts.part_info(s)
            assert b.status(s) == 0 and info.input == i
            o = b.result(s).ConnectedData
            ref = oracle.decode(parts[s])
            assert o.PointsCount == info.num_points and len(o.Attributes) == len(rows[s]) == len(ref.attributes) == 6
            pos = np.ascontiguousarray(o.Attributes[0].Values, np.float32).reshape(-1, 3)
            assert pos.tobytes() == np.ascontiguousarray(ref.attributes[0].values, np.float32).tobytes()
            assert np.array_equal(pos.min(axis=0).view(np.uint32), np.float32(list(info.box_min)).view(np.uint32)), (s, pos.min(axis=0), list(info.box_min))
            assert np.array_equal(pos.max(axis=0).view(np.uint32), np.float32(list(info.box_max)).view(np.uint32)), (s, pos.max(axis=0), list(info.box_max))
            q = np.asarray(o.Attributes[0].PortableValues).reshape(-1, 3)
            assert np.array_equal(q, ref.attributes[0].portable) and np.array_equal(q.min(axis=0), list(info.qmin)) and np.array_equal(q.max(axis=0), list(info.qmax))
            cell = {tuple(t) for t in q.tolist()}
            assert len(cell) == len(q) and not (cell & seen), s
            seen |= cell
            for a, x in enumerate(o.Attributes):
                assert np.array_equal(np.asarray(rows[s][a]), kept[info.first_entry:info.first_entry + info.num_points]), (s, a)
                joined[a].append(np.ascontiguousarray(x.Values))
        for a, y in enumerate(whole.Attributes):
            assert np.concatenate(joined[a]).tobytes() == np.ascontiguousarray(y.Values).tobytes(), (i, a)
    b.close()
    parts.close()
    merged.close()


def options(N, order=1, geometry=0, merge=1, part_points=0):
    o = native.EncodeCellPartsOptions()
    native.lib().dsa_encode_default_cell_parts_options(C.byref(o))
    o.part_cells, o.split.part_points, o.split.merge.merge_points, o.split.merge.order.point_order, o.split.merge.order.sequential.geometry = N, part_points, merge, order, geometry
    return o


def call(ctx, meshes, o, name="dsa_encode_cell_parts_sequential_batch"):
    arr, grids, keep = encodecall.arrays(meshes)
    h = C.c_void_p()
    st = getattr(native.lib(), name)(ctx._h, len(meshes), arr, grids, C.byref(o), C.byref(h))
    return st, h


def test_the_cap_and_the_refusals_of_the_call(ctx):
    L = native.lib()
    small = dsa.PointCloudData(np.repeat(oc.random_cloud(3, 841), 2, axis=0))
    over = dsa.PointCloudData(np.repeat(oc.random_cloud(1, 842), native.ENCODE_MAX_PARTS + 1, axis=0))       # one cell: the host can only bound the parts by n
    st, h = call(ctx, [small, over, small], options(1))
    assert st == 0 and L.dsa_encoded_size(h) == 3 + 1 + 3
    got = encodecall.streams(ctx, h, 7)
    assert got[3][0] == native.DSA_ERR_INVALID_ARGUMENT and all(w in got[3][1] for w in ("part_cells 1", "n = 65537", "65536"))
    one = synth.encode_cell_parts(small.positions, opt=synth.options(pos_bits=11), part_cells=1)
    assert len(one.streams) == 3 and got[:3] == got[4:] == [(0, s) for s in one.streams]
    # the option check answers before any mesh is looked at, naming the field
    for o, text in ((options(-1), "part_cells -1"), (options(7, merge=0), "part_cells 7 needs merge_points 1"), (options(7, order=0), "part_cells 7 needs point_order 1"),
                    (options(7, geometry=1), "part_cells 7 needs geometry 0"), (options(7, part_points=5), "part_cells 7 with part_points 5")):
        st, _ = call(ctx, [small], o)
        assert st == native.DSA_ERR_INVALID_ARGUMENT and text in ctx.error(), (text, ctx.error())
    o = options(7)
    o.reserved[3] = 1
    assert call(ctx, [small], o)[0] == native.DSA_ERR_INVALID_ARGUMENT and "dsa_encode_cell_parts_options.reserved[3]" in ctx.error()
    o = options(7)                              # what the nested structs refuse, in their words
    o.split.reserved[1] = 1
    assert call(ctx, [small], o)[0] == native.DSA_ERR_INVALID_ARGUMENT and "dsa_encode_split_options.reserved[1]" in ctx.error()
    assert call(ctx, [small], options(0, part_points=7))[0] == native.DSA_ERR_INVALID_ARGUMENT and "part_points 7 with merge_points 1" in ctx.error()
    assert call(ctx, [small], options(0, merge=2))[0] == native.DSA_ERR_INVALID_ARGUMENT and "merge_points 2" in ctx.error()


def handle_of(ctx, h, meshes, merge):
    """everything a handle says, slot by slot: (parts per input, [(status, stream or text, entry rows, row entries or None, part record or None)])"""
    L = native.lib()
    first, count, info = C.c_uint32(), C.c_uint32(), native.PartInfo()
    n = L.dsa_encoded_size(h)
    ranges = []
    for i in range(len(meshes)):
        assert L.dsa_encoded_parts(h, i, C.byref(first), C.byref(count)) == 0
        ranges.append((first.value, count.value))
    out = []
    p, ln = C.c_void_p(), C.c_size_t()
    for s in range(n):
        st = L.dsa_encoded_stream(h, s, C.byref(p), C.byref(ln))
        if st != 0:
            out.append((st, ctx.error().split(": ", 1)[1], None, None, None))
            continue
        stream = C.string_at(p, ln.value)
        assert L.dsa_encoded_entry_rows(h, s, 0, None, 0, C.byref(count)) == 0
        rows = np.zeros(count.value, np.uint32)
        assert L.dsa_encoded_entry_rows(h, s, 0, rows.ctypes.data, len(rows), C.byref(count)) == 0
        cells = None
        if L.dsa_encoded_row_entries(h, s, None, 0, C.byref(count)) == 0:
            cells = np.zeros(count.value, np.uint32)
            assert L.dsa_encoded_row_entries(h, s, cells.ctypes.data, len(cells), C.byref(count)) == 0
        else:
            cells = ctx.error()
        record = bytes(info) if L.dsa_encoded_part_info(h, s, C.byref(info)) == 0 else ctx.error()
        out.append((st, stream, rows.tobytes(), cells.tobytes() if isinstance(cells, np.ndarray) else cells, record))
    L.dsa_encoded_free(h)
    return ranges, out


def test_part_cells_0_is_the_split_call_and_no_part_cells_the_merged_call(ctx):
    meshes = [cloud(mc.half_duplicated(n, 850 + n), **attributes_of(n, n)) for n in (5, 1500)]
    bad = oc.random_cloud(300, 851)
    bad[17, 0] = np.inf
    meshes.insert(1, dsa.PointCloudData(bad, position_grid=dsa.Grid([0, 0, 0], 2.0)))
    # part_cells = 0 through the new entry: the split call's bytes, messages, rows and handle shape, with parts and without
    for merge, part_points in ((0, 400), (0, 0), (1, 0)):
        o = options(0, merge=merge, part_points=part_points)
        st, h = call(ctx, meshes, o)
        st2, h2 = call(ctx, meshes, o.split, "dsa_encode_split_sequential_batch")
        assert st == st2 == 0
        new, old = handle_of(ctx, h, meshes, merge), handle_of(ctx, h2, meshes, merge)
        assert new == old and len(new[1]) == (1 + 1 + 4 if part_points else 3) and new[1][1][0] == native.DSA_ERR_INVALID_ARGUMENT and "row 17" in new[1][1][1]
    # a merged config without part_cells arrives at the merged call: its bytes and its handle, and they are the new entry's
    good = [meshes[0], meshes[2]]
    cfg = dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, merge_points=dsa.MERGE_CELLS)
    via_config = dsa.DracoEncoder(ctx).EncodeBatch(good, cfg)
    st, h = call(ctx, good, options(0))
    st2, h2 = call(ctx, good, options(0).split.merge, "dsa_encode_merged_sequential_batch")
    assert st == st2 == 0
    new, old = handle_of(ctx, h, good, 1), handle_of(ctx, h2, good, 1)
    assert new == old and new[0] == [(0, 1), (1, 1)]
    for i in range(2):
        assert via_config[i] == new[1][i][1] and via_config.entry_rows(i)[0].tobytes() == new[1][i][2] and via_config.row_entries(i).tobytes() == new[1][i][3]
        assert via_config.parts(i) == range(i, i + 1) and "part_points" in new[1][i][4]
    via_config.close()
