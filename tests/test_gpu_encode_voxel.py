"""Encode direction, voxels coarser than the position grid on the device (dsa_encode_voxel_sequential_batch; Config(merge_points=
MERGE_CELLS, voxel_bits=C, voxel_point=VOXEL_POINT_*); the shift in the head predicate, the positions as a stream of k_enc_mean_*,
k_enc_voxel_near / k_enc_voxel_pick of draco-sharp_amd/csrc/dsa_encode_order.h and their regions in dsa_encode_layout.h).  Every stream
must be, byte for byte, the CPU coder's (synth.encode_merged / encode_cell_parts / encode_lod_parts with voxel_bits / voxel_point,
which state the rules serially), the kept rows and the coded position integers the rules restated in Python integers (voxelcases.pin),
and the positions the project's decoder makes of the streams bit for bit the dequantised integers of the pin.  The wave paths -- the
head ballots with the shift, the segmented 64-bit sums of the positions, the segmented maximum of k_enc_voxel_near and its two atomic
phases -- are held to the twin here alone: the runs end on the 64 entries of a wave step and the 1024-entry tile, the nearest rows tie
with the smaller row later in Morton order (voxelcases).  The largest cloud has about 6 600 points."""
import ctypes as C
import functools

import numpy as np
import pytest

import encodecall
import ordercases as oc
import test_gpu_encode_cell_parts as cpt
import test_gpu_encode_lod as lodt
import voxelcases as vc
import draco_sharp_amd as dsa
import draco_sharp_amd.synth as synth
from draco_sharp_amd import encoder, native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = dsa.Context(0)
    yield c
    c.close()


def config(bits, C_, point=0, mean=0, vote=0, normals=False, N=0, D=0, **kw):
    return dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, merge_points=dsa.MERGE_CELLS, part_cells=N, lod_base_bits=D, mean_attributes=mean,
                      vote_attributes=vote, mean_normals=normals, position_bits=bits, voxel_bits=C_, voxel_point=point, **kw)


@functools.lru_cache(maxsize=None)
def twin(name, point):
    """the CPU coder's (stream, kept, row_entries) of a case, computed once for the tests that need it"""
    return synth.encode_merged(voxel_bits=vc.named(name).C, voxel_point=point, **vc.cpu_args(vc.named(name)))


def grid_of(case):
    return synth.grid(case.grid[0], case.grid[1]) if case.grid is not None else synth.bounds_grid(case.pos)


def dequantised(case, q):
    g = grid_of(case)
    return cpt.dequantized(q, g.origin[:3], g.range, case.bits)


def decoded_positions(ctx, streams):
    """[float32 (m, 3)] of the streams' positions through the project's decoder"""
    b = dsa.Batch(ctx, streams)
    b.decode()
    out = []
    for i in range(len(streams)):
        assert b.status(i) == 0, (i, b.status(i))
        a = b.result(i).ConnectedData.Attributes[0]
        assert a.AttributeType == 0
        out.append(np.ascontiguousarray(a.Values, np.float32).reshape(-1, 3))
    b.close()
    return out


@pytest.mark.parametrize("host_plan", ["0", "1"])
def test_every_case(ctx, monkeypatch, host_plan):
    """every case of voxelcases, the cases of one (B, C) crowded into one batch, under the three rules: byte-equal to the twin under
    host and device plans, kept rows, row entries and cell counts the pin's, the decoded position of every kept point the pin's
    dequantised integers bit for bit"""
    monkeypatch.setenv("DSA_ENC_HOST_PLAN", host_plan)
    assert {k for k, _ in vc.groups()} >= set(vc.BC)
    enc = dsa.DracoEncoder(ctx)
    for (bits, C_), group in vc.groups():
        clouds = [vc.cloud(c) for c in group]
        for point in vc.POINTS:
            got = enc.EncodeBatch(clouds, config(bits, C_, point))
            assert len(got) == len(group)
            dec = decoded_positions(ctx, [got[i] for i in range(len(group))])
            for i, c in enumerate(group):
                stream, kept, cells = twin(c.name, point)
                pk, pe, pc = vc.pin(c, point)
                assert np.array_equal(kept, pk) and np.array_equal(cells, pe), (c.name, point)
                assert got[i] == stream, (c.name, point, len(got[i]), len(stream))
                rows = got.entry_rows(i)
                assert len(rows) == 1 and np.array_equal(rows[0], pk), (c.name, point)
                assert np.array_equal(got.row_entries(i), pe), (c.name, point)
                assert np.array_equal(got.cell_counts(i), np.bincount(pe, minlength=len(pk))), (c.name, point)
                assert dec[i].tobytes() == dequantised(c, pc).tobytes(), (c.name, point)
            got.close()


def test_the_designed_values(ctx):
    """centroid ties round up, a centroid lands in a cell no row occupies, the nearest row of equal distances is the smaller row
    though it sorts later: the values written down with the cases"""
    enc = dsa.DracoEncoder(ctx)
    for name, (point, make) in vc.DESIGNED.items():
        case, want = make()
        got = enc.EncodeBatch([vc.cloud(case)], config(case.bits, case.C, point))
        if point == vc.CENTROID:
            assert decoded_positions(ctx, [got[0]])[0].tobytes() == dequantised(case, want).tobytes(), name
        else:
            assert np.array_equal(got.entry_rows(0)[0], want), name
        got.close()


def test_a_shared_grid(ctx):
    """two tiles of one surface on the grid they share: the voxels of both are cells of that one grid, under every rule"""
    rng = np.random.default_rng(3050)
    tiles = [((rng.random((1500, 3)) * [1.0, 1.0, 0.25]) + [k, 0.0, 0.0]).astype(np.float32) for k in range(2)]
    g = synth.shared_grid(tiles)
    clouds = [dsa.PointCloudData(t, position_grid=dsa.Grid.shared()) for t in tiles]
    for point in vc.POINTS:
        got = dsa.DracoEncoder(ctx).EncodeBatch(clouds, config(11, 4, point))
        assert len(got) == 2
        for i, t in enumerate(tiles):
            stream, kept, cells = synth.encode_merged(t, opt=synth.options(pos_bits=11), pos_grid=g, voxel_bits=4, voxel_point=point)
            assert got[i] == stream and np.array_equal(got.entry_rows(i)[0], kept) and np.array_equal(got.row_entries(i), cells), (i, point)
            q = [[int(x) for x in r] for r in synth.quantized(t, 11, g)]
            pk, pe, _ = vc.rule(q, 11, 4, point)
            assert np.array_equal(kept, pk) and np.array_equal(cells, pe) and len(kept) < len(t) // 3, (i, point)
        got.close()


def test_three_hundred_small_clouds_in_one_call(ctx):
    """300 clouds of 1 .. 40 points at 5 bits in 2-bit voxels: one launch sequence for all of them, under every rule"""
    rng = np.random.default_rng(3100)
    clouds, args = [], []
    for k in range(300):
        pos = (rng.random((1 + k % 40, 3)) * [1.0, 1.0, 0.3]).astype(np.float32)
        clouds.append(dsa.PointCloudData(pos))
        args.append(dict(pos=pos, opt=synth.options(pos_bits=5)))
    for point in vc.POINTS:
        got = dsa.DracoEncoder(ctx).EncodeBatch(clouds, config(5, 2, point))
        assert len(got) == 300
        merged = 0
        for i, a in enumerate(args):
            stream, kept, cells = synth.encode_merged(voxel_bits=2, voxel_point=point, **a)
            assert got[i] == stream, (i, point)
            assert np.array_equal(got.entry_rows(i)[0], kept) and np.array_equal(got.cell_counts(i), np.bincount(cells, minlength=len(kept)))
            merged += len(kept) < len(a["pos"])
        assert merged > 200
        got.close()


def beside(n, seed=78):
    """normals to average (attribute 1), a colour to average (attribute 2) and a label to vote on (attribute 3)"""
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, 3)).astype(np.float32), rng.integers(0, 256, (n, 3)).astype(np.uint8), rng.integers(0, 4, (n, 1)).astype(np.uint8)


@pytest.mark.parametrize("point", [vc.CENTROID, vc.NEAREST])
@pytest.mark.parametrize("levels", [False, True])
def test_composition_with_means_votes_normals_parts_and_levels(ctx, point, levels):
    """a colour averaged, a label voted and the normals averaged over the VOXELS, in parts of 64 with and without levels: every stream
    the twin's, the part records, boxes and levels the twin's, L = C - D + 1, levels 0 .. l one point per cell of the grid with D + l
    bits, the boxes those of the decoded positions, the parts joined back in stream order"""
    for name, D in (("mixed-14-13", 10), ("ends-11-10", 7), ("explicit-grid-11-2", 1)):
        c = vc.named(name)
        D = D if levels else 0
        nrm, colour, label = beside(len(c.pos))
        cfg = config(c.bits, c.C, point, mean=0b100, vote=0b1000, normals=True, N=64, D=D)
        cloud = vc.cloud(c, normals=nrm, attributes=[dsa.Attribute(colour), dsa.Attribute(label)])
        got = dsa.DracoEncoder(ctx).EncodeBatch([cloud], cfg)
        tw = synth.encode_lod_parts(part_cells=64, lod_base_bits=D, mean_attributes=0b100, vote_attributes=0b1000, mean_normals=True, voxel_bits=c.C, voxel_point=point,
                                    **vc.cpu_args(c, normals=nrm, extra=[synth.Extra(colour), synth.Extra(label)]))
        if D:
            assert tw.levels == c.C - D + 1 and got.lod_info(got.parts(0)[0]).levels == c.C - D + 1
            lodt.check_levels(got, 0, tw, D)
        assert cpt.check_handle(ctx, got, 0, 0, cloud, tw, 4, c.bits) == len(got)
        pk, pe, pc = vc.pin(c, point)
        assert sorted(tw.kept.tolist()) == sorted(pk.tolist())
        at = np.zeros(len(c.pos), np.int64)
        at[pk] = np.arange(len(pk))
        want = dequantised(c, pc[at[tw.kept]])                    # the decoded position of every entry, in the order of the parts
        streams, groups, _ = encoder.join_plan(got)
        dec = decoded_positions(ctx, streams)
        assert np.concatenate(dec).tobytes() == want.tobytes(), (name, point)
        for s, d in zip(got.parts(0), dec):                      # the box of a part is the box of its decoded positions
            info = got.part_info(s)
            assert np.float32(list(info.box_min)).tobytes() == d.min(axis=0).tobytes() and np.float32(list(info.box_max)).tobytes() == d.max(axis=0).tobytes(), (name, s)
        if D:                                                    # levels 0 .. l: one point per occupied cell of the grid with D + l bits
            q = np.asarray(vc.integers(c), np.int64)
            for l in range(tw.levels):
                rows = np.concatenate([tw.kept[lo:hi] for (lo, hi), lv in zip(tw.ranges, tw.level) if lv <= l])
                cells = pc[at[rows]] >> (c.bits - D - l)
                assert len(np.unique(cells, axis=0)) == len(rows) == len(np.unique(q >> (c.bits - D - l), axis=0)), (name, l)
        b = dsa.Batch(ctx, streams)
        b.decode()
        joined, = b.joined_arrays(groups, "values")
        assert joined["num_rows"] == len(pk) and np.ascontiguousarray(joined["attributes"][0]["values"], np.float32).tobytes() == want.tobytes(), (name, point)
        b.close()
        assert np.array_equal(got.cell_counts(0), np.bincount(tw.row_entries, minlength=len(pk)))
        got.close()


def options(C_=0, point=0, N=0, D=0, merge=1, order=1, geometry=0, bits=None, mean=0, vote=0, normals=0):
    o = native.EncodeVoxelOptions()
    native.lib().dsa_encode_default_voxel_options(C.byref(o))
    nm = o.normal_mean
    m = nm.vote.mean.lod.cell_parts.split.merge
    o.voxel_bits, o.voxel_point, nm.mean_normals, nm.vote.vote_attributes, nm.vote.mean.mean_attributes, nm.vote.mean.lod.lod_base_bits, nm.vote.mean.lod.cell_parts.part_cells = C_, point, normals, vote, mean, D, N
    m.merge_points, m.order.point_order, m.order.sequential.geometry = merge, order, geometry
    if bits is not None:
        m.order.sequential.base.position_bits = bits
    return o


def call(ctx, meshes, o):
    return cpt.call(ctx, meshes, o, "dsa_encode_voxel_sequential_batch")


def test_voxel_bits_0_and_B_are_the_normal_mean_call(ctx):
    """voxel_bits = 0: handle for handle the call without the struct, a refused cloud in between; voxel_bits = B with any rule: the
    same streams and rows"""
    def cloud_of(n, seed):
        kw = cpt.attributes_of(n, seed)
        kw["attributes"] = kw["attributes"] + [dsa.Attribute(np.random.default_rng(seed).integers(0, 4, (n, 1)).astype(np.uint8))]
        return kw
    import mergecases as mc
    meshes = [cpt.cloud(mc.half_duplicated(n, 3200 + n), **cloud_of(n, n)) for n in (5, 1500)]
    bad = oc.random_cloud(300, 3201)
    bad[17, 0] = np.inf
    meshes.insert(1, dsa.PointCloudData(bad, position_grid=dsa.Grid([0, 0, 0], 2.0), **cloud_of(300, 3202)))
    for N, D, mean, vote, normals in ((400, 3, 0b1000, 0b1000000, 1), (0, 0, 0b1000, 0, 0), (0, 0, 0, 0, 0)):
        o = options(0, 0, N, D, mean=mean, vote=vote, normals=normals)
        st, h = call(ctx, meshes, o)
        st2, h2 = cpt.call(ctx, meshes, o.normal_mean, "dsa_encode_normal_mean_sequential_batch")
        assert st == st2 == 0
        old = cpt.handle_of(ctx, h2, meshes, 1)
        assert cpt.handle_of(ctx, h, meshes, 1) == old and len(old[1]) >= 3 and old[1][1][0] == native.DSA_ERR_INVALID_ARGUMENT and "row 17" in old[1][1][1]
        for point in vc.POINTS:                                  # (the default position_bits are 11)
            st, h = call(ctx, meshes, options(11, point, N, D, mean=mean, vote=vote, normals=normals))
            assert st == 0 and cpt.handle_of(ctx, h, meshes, 1) == old, (N, point)
    # coarser voxels differ, and a refused cloud still fails alone
    st, h = call(ctx, meshes, options(4, 1))
    assert st == 0
    new = cpt.handle_of(ctx, h, meshes, 1)
    assert new[1][1][0] == native.DSA_ERR_INVALID_ARGUMENT and "row 17" in new[1][1][1] and new[1][0][0] == 0 and new[1][2][0] == 0 and new[1][2][1] != old[1][2][1]
    # a config with voxel_bits = 0 arrives at the call it always took
    good = [meshes[0], meshes[2]]
    a = dsa.DracoEncoder(ctx).EncodeBatch(good, config(11, 0))
    b = dsa.DracoEncoder(ctx).EncodeBatch(good, config(11, 11, vc.NEAREST))
    assert len(a) == len(b) == 2 and all(a[i] == b[i] for i in range(2)) and all(np.array_equal(a.entry_rows(i)[0], b.entry_rows(i)[0]) for i in range(2))
    a.close()
    b.close()


def test_refusals(ctx):
    """the call-level refusals and the field each names; a mask bit on the positions stays refused per cloud, in the words it always had"""
    pos = np.repeat(oc.random_cloud(40, 3301), 3, axis=0)
    label = dsa.Attribute(np.random.default_rng(3300).integers(0, 4, (len(pos), 1)).astype(np.uint8))
    cloud = dsa.PointCloudData(pos, attributes=[label])
    for o, text in ((options(-1), "voxel_bits -1: 0"), (options(12), "voxel_bits 12 is above position_bits 11"), (options(15, bits=14), "voxel_bits 15 is above position_bits 14"),
                    (options(5, merge=0), "voxel_bits 5 needs merge_points 1"), (options(5, 3), "voxel_point 3: 0 (DSA_VOXEL_POINT_FIRST)"), (options(5, -1), "voxel_point -1"),
                    (options(0, 1), "voxel_point 1 needs voxel_bits >= 1"), (options(0, 2), "voxel_point 2 needs voxel_bits >= 1"),
                    (options(5, 1, N=7, D=6), "lod_base_bits 6 is above voxel_bits 5"), (options(5, 1, D=3), "lod_base_bits 3 needs part_cells >= 1"),
                    (options(5, order=0), "merge_points 1 needs point_order 1"), (options(5, geometry=1), "merge_points 1 needs geometry 0"), (options(5, normals=2), "mean_normals 2: 0")):
        st, _ = call(ctx, [cloud], o)
        assert st == native.DSA_ERR_INVALID_ARGUMENT and text in ctx.error(), (text, ctx.error())
    for k in (0, 3, 5):
        o = options(5, 1)
        o.reserved[k] = 1
        assert call(ctx, [cloud], o)[0] == native.DSA_ERR_INVALID_ARGUMENT and "dsa_encode_voxel_options.reserved[%d]" % k in ctx.error()
    o = options(5, 1)
    o.normal_mean.reserved[4] = 1
    assert call(ctx, [cloud], o)[0] == native.DSA_ERR_INVALID_ARGUMENT and "dsa_encode_normal_mean_options.reserved[4]" in ctx.error()
    # a bit of either mask on the positions: the cloud fails alone, with the centroid as without
    for point in vc.POINTS:
        st, h = call(ctx, [cloud], options(5, point, mean=1))
        assert st == 0
        got = encodecall.streams(ctx, h, 1)
        assert got[0][0] == native.DSA_ERR_INVALID_ARGUMENT and "mean_attributes 0x1: bit 0 names attribute 0, the positions" in got[0][1], got[0]
        st, h = call(ctx, [cloud], options(5, point, vote=1))
        assert st == 0
        got = encodecall.streams(ctx, h, 1)
        assert got[0][0] == native.DSA_ERR_INVALID_ARGUMENT and "vote_attributes 0x1: bit 0 names attribute 0, the positions" in got[0][1], got[0]
    # the label voted over the voxels, the centroid beside it: what the refusals leave to ask for
    st, h = call(ctx, [cloud], options(5, 1, vote=0b10))
    assert st == 0
    got = encodecall.streams(ctx, h, 1)
    assert got[0] == (0, synth.encode_merged(pos, extra=[synth.Extra(label.values)], opt=synth.options(pos_bits=11), vote_attributes=0b10, voxel_bits=5, voxel_point=1)[0])


def test_a_second_run_gives_the_same_bytes(ctx):
    """one batch twice in one process (the lane's arena is used again: sums, counts, best distances and rows start from the memset, not
    from what the first run left): byte-equal streams"""
    group = [c for c in vc.cases() if (c.bits, c.C) == (11, 2)]
    clouds = [vc.cloud(c) for c in group]
    enc = dsa.DracoEncoder(ctx)
    for point in (vc.CENTROID, vc.NEAREST):
        a = enc.EncodeBatch(clouds, config(11, 2, point))
        b = enc.EncodeBatch(clouds, config(11, 2, point))
        assert len(a) == len(b) == len(group) >= 3 and all(a[i] == b[i] == twin(c.name, point)[0] for i, c in enumerate(group))
        a.close()
        b.close()
