"""Encode direction, additive levels of detail of merged point clouds on the device (dsa_encode_lod_sequential_batch,
lod_base_bits >= 1; Config(merge_points=MERGE_CELLS, part_cells=N, lod_base_bits=D); k_enc_lod_levels / _scan / _scatter / _cells and
k_enc_part_cells of draco-sharp_amd/csrc/dsa_encode_order.h and the slots of dsa_encode_layout.h).  Every slot's stream must be, byte for
byte, the CPU coder's (synth.encode_lod_parts); the handle's slots, slices of lod, row entries, part records and level records must
be the twin's; all slots decode side by side to the merged single stream's points, and every prefix of levels is one point per cell
of its grid.  The shapes sit on the kernels' edges: the 64 entries of a wave step and the 1024-entry tile, in level populations, in
part sizes and in where a level begins (lodcases)."""
import ctypes as C

import numpy as np
import pytest

import encodecall
import lodcases as lc
import mergecases as mc
import oracle
import ordercases as oc
import test_gpu_encode_cell_parts as cpt
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


def config(N, D, **kw):
    return dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, merge_points=dsa.MERGE_CELLS, part_cells=N, lod_base_bits=D, **kw)


def check_levels(got, i, twin, D):
    """lod_info of every slot of input i and levels(i) against the twin's level per stream"""
    r = got.parts(i)
    level = twin.level.astype(np.int64)
    size = twin.ranges[:, 1].astype(np.int64) - twin.ranges[:, 0]
    want = []
    at = r.start
    for l in range(twin.levels):
        k = int((level == l).sum())
        want.append(range(at, at + k))
        at += k
    assert got.levels(i) == want, (i, got.levels(i), want)
    for p, s in enumerate(r):
        info = got.lod_info(s)
        l = int(level[p])
        assert (info.input, info.level, info.levels, info.cell_bits) == (i, l, twin.levels, D + l), (i, p)
        assert (info.level_first_stream, info.level_streams, info.level_points, info.part_in_level) == (want[l].start, len(want[l]), int(size[level == l].sum()), s - want[l].start), (i, p)
        assert list(info.reserved) == [0] * 4


def check(ctx, clouds, N, D, **kw):
    """The slots of every cloud of the batch against the CPU coder's.  Returns the twin's LodParts per cloud."""
    cfg = config(N, D, **kw)
    got = dsa.DracoEncoder(ctx).EncodeBatch(clouds, cfg)
    out, first = [], 0
    for i, m in enumerate(clouds):
        twin = synth.encode_lod_parts(part_cells=N, lod_base_bits=D, **cpt.cpu_args(m, cfg))
        attributes = 1 + (m.normals is not None) + (m.texcoords is not None) + (m.generic is not None) + len(m.attributes)
        check_levels(got, i, twin, D)
        first = cpt.check_handle(ctx, got, i, first, m, twin, attributes, cfg.position_bits)
        out.append(twin)
    assert len(got) == first
    got.close()
    return out


def test_every_case(ctx):
    """level populations, part sizes and level boundaries around the wave step and the tile, empty levels, one level, one cell, own
    bounds, duplicates over a tile edge of the sorted order: the clouds of one (bits, part_cells, lod_base_bits) are a batch"""
    cases = lc.cases()
    assert lc.TILE == T and {c.part_cells for c in cases} >= {1, 2, 63, 64, 65, T - 1, T, T + 1, 2**31 - 1}
    empty = 0
    for key in sorted({(c.bits, c.part_cells, c.lod_base_bits) for c in cases}):
        group = [c for c in cases if (c.bits, c.part_cells, c.lod_base_bits) == key]
        twins = check(ctx, [cpt.cloud(c) for c in group], key[1], key[2], position_bits=key[0])
        for c, twin in zip(group, twins):
            pin = lc.pin(c)
            assert np.array_equal(twin.kept, pin.lod) and np.array_equal(twin.ranges, pin.ranges) and np.array_equal(twin.level, pin.level), c.name
            empty += lc.slots(c) - len(twin.streams)
    assert empty > 80           # slots the device left empty


def test_the_large_cloud(ctx):
    c = lc.large()
    twin, = check(ctx, [cpt.cloud(c)], c.part_cells, c.lod_base_bits, position_bits=c.bits)
    assert len(c.pos) == 70001 and twin.levels == 5 and len(twin.kept) > 50000 and len(twin.streams) > 180 and lc.slots(c) == 238
    assert np.array_equal(twin.kept, lc.pin(c).lod)


def test_one_cloud_carrying_everything(ctx):
    c = mc.half_duplicated(2 * T + 77, 801)
    twin, = check(ctx, [cpt.cloud(c, **cpt.attributes_of(len(c.pos), 802))], 300, 3, position_bits=c.bits)
    assert T < len(twin.kept) < len(c.pos) and twin.levels == 9 and len(set(twin.level.tolist())) >= 3


def test_a_batch_of_different_clouds_and_a_refused_one(ctx):
    """clouds whose levels differ in one call -- random ones of three sizes, one all identical (one point in level 0, every other slot
    empty), one a single point -- and one with a NaN on an explicit grid, which fails alone in its one slot with the plain call's
    status and text"""
    L = native.lib()
    g = dsa.Grid([0, 0, 0], 2.0)
    good = [mc.half_duplicated(500, 811).pos, np.repeat(oc.random_cloud(1, 812), 700, axis=0), oc.random_cloud(1300, 813), mc.half_duplicated(T + 5, 814).pos, oc.random_cloud(1, 816)]
    bad = oc.random_cloud(800, 815)
    bad[417, 2] = np.nan
    meshes = [dsa.PointCloudData(p, position_grid=g) for p in good[:2]] + [dsa.PointCloudData(bad, position_grid=g)] + [dsa.PointCloudData(p, position_grid=g) for p in good[2:]]
    cfg = config(100, 2, position_bits=5)
    ctx_, h, n = dsa.DracoEncoder(ctx).EncodeBatch(meshes, cfg, handle=True)
    twins = [synth.encode_lod_parts(p, opt=synth.options(pos_bits=5), pos_grid=synth.grid([0, 0, 0], 2.0), part_cells=100, lod_base_bits=2) for p in good]
    counts = [len(t.streams) for t in twins]
    assert counts[1] == counts[4] == 1 and len(twins[1].kept) == 1 and counts[0] >= 3 and counts[2] >= 4 and len({tuple(np.bincount(t.level, minlength=4)) for t in twins}) >= 3
    assert n == L.dsa_encoded_size(h) == sum(counts) + 1
    first, count, info, level = C.c_uint32(), C.c_uint32(), native.PartInfo(), native.LodInfo()
    slots = []
    for i in range(6):
        assert L.dsa_encoded_parts(h, i, C.byref(first), C.byref(count)) == 0
        slots.append((first.value, count.value))
    at = np.concatenate([[0], np.cumsum(counts[:2] + [1] + counts[2:])])
    assert slots == [(int(a), int(b - a)) for a, b in zip(at[:-1], at[1:])]
    bad_slot = int(at[2])
    assert L.dsa_encoded_part_info(h, bad_slot, C.byref(info)) == native.DSA_ERR_INVALID_ARGUMENT and "row 417" in ctx.error()
    assert L.dsa_encoded_lod_info(h, bad_slot, C.byref(level)) == native.DSA_ERR_INVALID_ARGUMENT and "row 417" in ctx.error()
    assert L.dsa_encoded_lod_info(h, bad_slot + 1, C.byref(level)) == 0 and (level.input, level.level, level.levels, level.cell_bits) == (3, 0, 4, 2)
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
        check_levels(got, i, t, 2)
        first = cpt.check_handle(ctx, got, i, first, m, t, 1, 5)
    got.close()


@pytest.mark.parametrize("host_plan", ["0", "1"])
def test_chunks_and_plans(ctx, monkeypatch, host_plan):
    """1 500 clouds of 40 points in 3-bit cells, two levels in parts of at most 16 points, cross a chunk boundary of inputs; the symbol
    plans by the host and by the device.  Every cloud has 4 slots and fills 2 or 3."""
    monkeypatch.setenv("DSA_ENC_HOST_PLAN", host_plan)
    rng = np.random.default_rng(820)
    clouds = [dsa.PointCloudData((rng.random((40, 3)) * [1.0, 1.0, 0.12]).astype(np.float32)) for _ in range(1500)]
    out = check(ctx, clouds, 16, 2, position_bits=3)
    parts = [len(t.streams) for t in out]
    assert set(parts) <= {2, 3, 4} and len(set(parts)) >= 2 and all(t.levels == 2 and t.level[-1] == 1 for t in out)


def test_decode(ctx):
    """all slots of two clouds in one Batch, beside the merged single streams of the same clouds: positions bit-equal to the oracle;
    per level prefix 0 .. l the position integers are one per cell at D + l bits; all levels together are the merged stream's points
    as a set; the box of every slot is the box of its decoded positions; no position integer occurs in two slots; the source rows are
    the slices of lod"""
    D, bits = 3, 11
    clouds = [cpt.cloud(mc.half_duplicated(2 * T + 77, 831), **cpt.attributes_of(2 * T + 77, 832)), cpt.cloud(mc.half_duplicated(930, 833), **cpt.attributes_of(930, 834))]
    enc = dsa.DracoEncoder(ctx)
    merged_cfg = dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, merge_points=dsa.MERGE_CELLS)
    parts, merged = enc.EncodeBatch(clouds, config(250, D)), enc.EncodeBatch(clouds, merged_cfg)
    k = len(parts)
    ranges = [parts.parts(i) for i in range(2)]
    assert ranges[0].start == 0 and ranges[0].stop == ranges[1].start and ranges[1].stop == k and len(ranges[0]) >= 5 and len(ranges[1]) >= 3
    b = dsa.Batch(ctx, list(parts) + list(merged))
    b.decode()
    rows = b.source_rows(parts, encoded_mesh=list(range(k)) + [0, 0])
    for i in range(2):
        whole = b.result(k + i).ConnectedData
        kept = merged.entry_rows(i)[0]
        lod = np.concatenate([parts.entry_rows(s)[0] for s in ranges[i]])
        assert np.array_equal(np.sort(lod), np.sort(kept)) and not np.array_equal(lod, kept)
        whole_q = np.asarray(whole.Attributes[0].PortableValues).reshape(-1, 3)
        levels = parts.levels(i)
        assert len(levels) == bits - D + 1 and levels[0].start == ranges[i].start and levels[-1].stop == ranges[i].stop and sum(len(r) > 0 for r in levels) >= 3
        seen = set()
        cells_so_far = []
        for l, level in enumerate(levels):
            for s in level:
                info, li = parts.part_info(s), parts.lod_info(s)
                assert b.status(s) == 0 and info.input == li.input == i and li.level == l and li.cell_bits == D + l
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
                cells_so_far.append(q)
                for a in range(len(o.Attributes)):
                    assert np.array_equal(np.asarray(rows[s][a]), lod[info.first_entry:info.first_entry + info.num_points]), (s, a)
            # levels 0 .. l: exactly one position integer per occupied cell of the grid with D + l bits per axis
            have = np.concatenate(cells_so_far) >> (bits - D - l)
            every = np.unique(whole_q >> (bits - D - l), axis=0)
            assert len(have) == len(every) and np.array_equal(np.unique(have, axis=0), every), (i, l)
        assert seen == {tuple(t) for t in whole_q.tolist()}
    b.close()
    parts.close()
    merged.close()


def options(N, D, order=1, geometry=0, merge=1, bits=None):
    o = native.EncodeLodOptions()
    native.lib().dsa_encode_default_lod_options(C.byref(o))
    m = o.cell_parts.split.merge
    o.lod_base_bits, o.cell_parts.part_cells, m.merge_points, m.order.point_order, m.order.sequential.geometry = D, N, merge, order, geometry
    if bits is not None:
        m.order.sequential.base.position_bits = bits
    return o


def call(ctx, meshes, o):
    return cpt.call(ctx, meshes, o, "dsa_encode_lod_sequential_batch")


def test_the_cap_and_the_refusals_of_the_call(ctx):
    L = native.lib()
    small = dsa.PointCloudData(np.repeat(oc.random_cloud(3, 841), 2, axis=0))
    # ceil(n / N) + L - 1 slots: 65 534 + 4 - 1 is one over the limit, though n is not (one cell: the host can only bound the parts by n)
    over = dsa.PointCloudData(np.repeat(oc.random_cloud(1, 842), native.ENCODE_MAX_PARTS - 2, axis=0))
    st, h = call(ctx, [small, over, small], options(1, 8))
    one = synth.encode_lod_parts(small.positions, opt=synth.options(pos_bits=11), part_cells=1, lod_base_bits=8)
    assert len(one.streams) == 3
    assert st == 0 and L.dsa_encoded_size(h) == 3 + 1 + 3
    got = encodecall.streams(ctx, h, 7)
    assert got[3][0] == native.DSA_ERR_INVALID_ARGUMENT and all(w in got[3][1] for w in ("lod_base_bits 8", "part_cells 1", "n = 65534", "65536")), got[3]
    assert got[:3] == got[4:] == [(0, s) for s in one.streams]
    # the option check answers before any mesh is looked at, naming the field
    for o, text in ((options(7, -1), "lod_base_bits -1"), (options(7, 12), "lod_base_bits 12 is above position_bits 11"), (options(7, 5, bits=4), "lod_base_bits 5 is above position_bits 4"),
                    (options(0, 3), "lod_base_bits 3 needs part_cells >= 1"), (options(7, 3, merge=0), "lod_base_bits 3 needs merge_points 1"),
                    (options(7, 3, order=0), "lod_base_bits 3 needs point_order 1"), (options(7, 3, geometry=1), "lod_base_bits 3 needs geometry 0")):
        st, _ = call(ctx, [small], o)
        assert st == native.DSA_ERR_INVALID_ARGUMENT and text in ctx.error(), (text, ctx.error())
    o = options(7, 3)
    o.reserved[3] = 1
    assert call(ctx, [small], o)[0] == native.DSA_ERR_INVALID_ARGUMENT and "dsa_encode_lod_options.reserved[3]" in ctx.error()
    o = options(7, 3)                           # what the nested structs refuse, in their words
    o.cell_parts.reserved[1] = 1
    assert call(ctx, [small], o)[0] == native.DSA_ERR_INVALID_ARGUMENT and "dsa_encode_cell_parts_options.reserved[1]" in ctx.error()
    assert call(ctx, [small], options(-1, 0))[0] == native.DSA_ERR_INVALID_ARGUMENT and "part_cells -1" in ctx.error()
    assert call(ctx, [small], options(0, 0, merge=2))[0] == native.DSA_ERR_INVALID_ARGUMENT and "merge_points 2" in ctx.error()
    # a handle without levels has no level records, and says what makes them
    st, h = call(ctx, [small], options(2, 0))
    assert st == 0 and L.dsa_encoded_lod_info(h, 0, C.byref(native.LodInfo())) == native.DSA_ERR_INVALID_ARGUMENT and "lod_base_bits" in ctx.error()
    L.dsa_encoded_free(h)


def test_lod_base_bits_0_is_the_cell_parts_call(ctx):
    meshes = [cpt.cloud(mc.half_duplicated(n, 850 + n), **cpt.attributes_of(n, n)) for n in (5, 1500)]
    bad = oc.random_cloud(300, 851)
    bad[17, 0] = np.inf
    meshes.insert(1, dsa.PointCloudData(bad, position_grid=dsa.Grid([0, 0, 0], 2.0)))
    # lod_base_bits = 0 through the new entry: the cell-parts call's bytes, messages, rows and handle shape, with parts and without
    for N, merge in ((400, 1), (0, 1), (0, 0)):
        o = options(N, 0, merge=merge)
        st, h = call(ctx, meshes, o)
        st2, h2 = cpt.call(ctx, meshes, o.cell_parts)
        assert st == st2 == 0
        new, old = cpt.handle_of(ctx, h, meshes, merge), cpt.handle_of(ctx, h2, meshes, merge)
        assert new == old and len(new[1]) >= 3 and new[1][1][0] == native.DSA_ERR_INVALID_ARGUMENT and "row 17" in new[1][1][1]
        assert N == 0 or len(new[1]) > 3
    # a config without lod_base_bits arrives at the cell-parts call: its bytes and its handle, and they are the new entry's
    good = [meshes[0], meshes[2]]
    via_config = dsa.DracoEncoder(ctx).EncodeBatch(good, cpt.config(400))
    st, h = call(ctx, good, options(400, 0))
    assert st == 0
    new = cpt.handle_of(ctx, h, good, 1)
    assert len(via_config) == len(new[1]) and [via_config.parts(i) for i in range(2)] == [range(f, f + k) for f, k in new[0]]
    for s in range(len(via_config)):
        assert via_config[s] == new[1][s][1] and via_config.entry_rows(s)[0].tobytes() == new[1][s][2] and bytes(via_config.part_info(s)) == new[1][s][4]
    with pytest.raises(Exception, match="lod_base_bits"):
        via_config.lod_info(0)
    via_config.close()


def test_all_points_in_level_0_are_the_streams_of_the_cell_parts_call(ctx):
    """D = B: one level, and the streams, rows and part records are those of part_cells alone"""
    meshes = [cpt.cloud(mc.half_duplicated(n, 860 + n), **cpt.attributes_of(n, n)) for n in (700, 2 * T + 9)]
    enc = dsa.DracoEncoder(ctx)
    levels, plain = enc.EncodeBatch(meshes, config(300, 11)), enc.EncodeBatch(meshes, cpt.config(300))
    assert len(levels) == len(plain) >= 6 and [levels.parts(i) for i in range(2)] == [plain.parts(i) for i in range(2)]
    for s in range(len(levels)):
        assert levels[s] == plain[s] and bytes(levels.part_info(s)) == bytes(plain.part_info(s))
        assert all(np.array_equal(a, b) for a, b in zip(levels.entry_rows(s), plain.entry_rows(s)))
        info = levels.lod_info(s)
        assert (info.level, info.levels, info.cell_bits) == (0, 1, 11) and info.level_streams == len(levels.parts(info.input))
    for i in range(2):
        assert np.array_equal(levels.row_entries(levels.parts(i)[0]), plain.row_entries(plain.parts(i)[0])) and levels.levels(i) == [levels.parts(i)]
    levels.close()
    plain.close()
