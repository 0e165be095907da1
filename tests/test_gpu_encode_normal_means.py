"""Encode direction, the mean normal of every cell of merged point clouds on the device (dsa_encode_normal_mean_sequential_batch,
mean_normals = 1; Config(merge_points=MERGE_CELLS, mean_normals=True); k_enc_normal_sum / k_enc_normal_store of
draco-sharp_amd/csrc/dsa_encode_order.h and their regions in dsa_encode_layout.h).  Every stream must be, byte for byte, the CPU
coder's (synth.encode_merged / encode_cell_parts / encode_lod_parts with mean_normals=True, which states the rule serially with a
bitwise square root), its codes the rule restated in Python integers (normalmeancases.pin), and the normals the project's decoder
makes of it bit for bit the dequantised codes of the pin; the handle is the one of the call without the option.  The wave path of
k_enc_normal_sum -- head ballots, the segmented 64-bit sums, one atomic per (run, step), the double seed of the square root and its
integer correction, the unsigned 64-bit divisions -- is held to the twin here alone: the shapes sit on the 64 entries of a wave step
and the 1024-entry tile, cells cancel, tie and cross the fold (normalmeancases).  The largest cloud has about 11 500 points."""
import ctypes as C
import functools

import numpy as np
import pytest

import encodecall
import mergecases as mc
import normalmeancases as nc
import ordercases as oc
import test_gpu_encode_cell_parts as cpt
import test_gpu_encode_lod as lodt
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


def config(bits=nc.BITS, nbits=8, on=True, mean=0, vote=0, N=0, D=0, **kw):
    return dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, merge_points=dsa.MERGE_CELLS, part_cells=N, lod_base_bits=D, mean_attributes=mean,
                      vote_attributes=vote, mean_normals=on, position_bits=bits, normal_bits=nbits, **kw)


@functools.lru_cache(maxsize=None)
def twin(name):
    """the CPU coder's (stream, kept, row_entries) of a case, computed once for the tests that need it"""
    return synth.encode_merged(mean_normals=True, **nc.cpu_args(nc.named(name)))


def decoded_normals(ctx, streams):
    """[(codes (m, 2), float32 values (m, 3))] of the streams' normals through the project's decoder"""
    b = dsa.Batch(ctx, streams)
    b.decode()
    out = []
    for i in range(len(streams)):
        assert b.status(i) == 0, (i, b.status(i))
        a = b.result(i).ConnectedData.Attributes[1]
        assert a.AttributeType == 1
        out.append((np.asarray(a.PortableValues, np.int64).reshape(-1, 2), np.ascontiguousarray(a.Values, np.float32).reshape(-1, 3)))
    b.close()
    return out


@pytest.mark.parametrize("host_plan", ["0", "1"])
def test_every_case(ctx, monkeypatch, host_plan):
    """every case of normalmeancases, the cases of one (position bits, normal bits) crowded into one batch: byte-equal to the twin
    under host and device plans, the codes the pin's, the decoded normals of every kept point the pin's dequantised codes bit for
    bit, the handle the one of the call without the option"""
    monkeypatch.setenv("DSA_ENC_HOST_PLAN", host_plan)
    assert nc.TILE == T and max(len(c.pos) for c in nc.cases()) < 12000 and len(nc.groups()) >= 9
    for (bits, nbits), group in nc.groups():
        clouds = [nc.cloud(c) for c in group]
        enc = dsa.DracoEncoder(ctx)
        got, plain = enc.EncodeBatch(clouds, config(bits, nbits)), enc.EncodeBatch(clouds, config(bits, nbits, on=False))
        assert len(got) == len(plain) == len(group)
        dec = decoded_normals(ctx, [got[i] for i in range(len(group))])
        for i, c in enumerate(group):
            stream, kept, cells = twin(c.name)
            assert got[i] == stream, (c.name, len(got[i]), len(stream))
            want = nc.pin(c)[2]
            assert np.array_equal(nc.decoded([got[i]]), want), c.name
            assert np.array_equal(dec[i][0], want) and dec[i][1].tobytes() == nc.dequantised(c).tobytes(), c.name
            rows = got.entry_rows(i)
            assert len(rows) == 2 and all(np.array_equal(r, kept) for r in rows) and all(np.array_equal(x, y) for x, y in zip(rows, plain.entry_rows(i)))
            assert np.array_equal(got.row_entries(i), cells) and np.array_equal(plain.row_entries(i), cells)
            assert np.array_equal(got.cell_counts(i), np.bincount(cells, minlength=len(kept))) and np.array_equal(got.cell_counts(i), plain.cell_counts(i))
        got.close()
        plain.close()


def test_three_hundred_small_clouds_in_one_call(ctx):
    """300 clouds of 1 .. 40 points in 3-bit cells, every third without normals: one launch sequence for all of them"""
    rng = np.random.default_rng(2100)
    clouds, args = [], []
    for k in range(300):
        n = 1 + k % 40
        pos = (rng.random((n, 3)) * [1.0, 1.0, 0.12]).astype(np.float32)
        nrm = None if k % 3 == 2 else nc.cone(rng, n, rng.normal(size=3), 0.6)
        clouds.append(dsa.PointCloudData(pos, normals=nrm))
        args.append(dict(pos=pos, normals=nrm, opt=synth.options(pos_bits=3, normal_bits=10)))
    got = dsa.DracoEncoder(ctx).EncodeBatch(clouds, config(3, 10))
    assert len(got) == 300
    merged = 0
    for i, a in enumerate(args):
        stream, kept, cells = synth.encode_merged(mean_normals=True, **a)
        assert got[i] == stream, i
        assert np.array_equal(got.cell_counts(i), np.bincount(cells, minlength=len(kept)))
        merged += len(kept) < len(a["pos"])
    assert merged > 150         # (more than half of the clouds have a cell of several rows; those of one or a few points have none)
    got.close()


def beside(case, seed=77):
    """a colour to average (attribute 2) and a label to vote on (attribute 3) beside the normals of a case"""
    rng = np.random.default_rng(seed)
    n = len(case.pos)
    return rng.integers(0, 256, (n, 3)).astype(np.uint8), rng.integers(0, 4, (n, 1)).astype(np.uint8)


@pytest.mark.parametrize("N,levels", [(0, False), (64, False), (64, True)])
def test_composition_with_means_votes_parts_and_levels(ctx, N, levels):
    """the normals averaged beside an averaged colour and a voted label, neither, one or both, merged, in parts and in levels: every
    stream the twin's, the part records and levels the twin's, the cell counts the rows of every cell -- counted once, whether the
    means count them too or not"""
    cases = [nc.named("runs-1-2-5-3000-8"), nc.named("cloud-2100"), nc.named("tile-with-no-head-8")]
    for mean, vote in ((0, 0), (0b100, 0), (0, 0b1000), (0b100, 0b1000)):
        for c in cases:
            colour, label = beside(c)
            D = c.bits - 4 if levels else 0             # five levels
            cfg = config(c.bits, c.nbits, mean=mean, vote=vote, N=N, D=D)
            cloud = nc.cloud(c, attributes=[dsa.Attribute(colour), dsa.Attribute(label)])
            got = dsa.DracoEncoder(ctx).EncodeBatch([cloud], cfg)
            args = nc.cpu_args(c)
            args["extra"] = [synth.Extra(colour), synth.Extra(label)]
            kept, cells, want = nc.pin(c)
            if N == 0:
                stream, k, ce = synth.encode_merged(mean_normals=True, mean_attributes=mean, vote_attributes=vote, **args)
                assert len(got) == 1 and got[0] == stream, (c.name, mean, vote)
                assert np.array_equal(got.cell_counts(0), np.bincount(cells, minlength=len(kept)))
                assert np.array_equal(nc.decoded([got[0]]), want)
            else:
                tw = synth.encode_lod_parts(part_cells=N, lod_base_bits=D, mean_normals=True, mean_attributes=mean, vote_attributes=vote, **args)
                if D:
                    lodt.check_levels(got, 0, tw, D)
                assert cpt.check_handle(ctx, got, 0, 0, cloud, tw, 4, c.bits) == len(got)
                at = np.zeros(len(cells), np.int64)
                at[kept] = np.arange(len(kept))
                assert np.array_equal(nc.decoded([got[s] for s in got.parts(0)]), want[at[tw.kept]]), (c.name, mean, vote)
                assert np.array_equal(got.cell_counts(0), np.bincount(tw.row_entries, minlength=len(kept)))
                assert sorted(got.cell_counts(0).tolist()) == sorted(np.bincount(cells).tolist())
            got.close()


def test_a_cloud_without_normals_in_the_same_call(ctx):
    """normals, none, normals in one call: the bare cloud is the plain merged stream; and a call none of whose clouds has normals is
    the call without the option, stream for stream"""
    a, b = nc.named("runs-1-2-5-3000-8"), nc.named("tile-with-no-head-8")
    bare = dsa.PointCloudData(a.pos, position_grid=dsa.Grid(a.grid[0], float(a.grid[1])))
    enc = dsa.DracoEncoder(ctx)
    got = enc.EncodeBatch([nc.cloud(a), bare, nc.cloud(b)], config(a.bits, 8))
    assert got[0] == twin(a.name)[0] and got[2] == twin(b.name)[0]
    assert got[1] == synth.encode_merged(a.pos, opt=synth.options(pos_bits=a.bits, normal_bits=8), pos_grid=synth.grid(a.grid[0], a.grid[1]))[0]
    assert np.array_equal(got.cell_counts(1), got.cell_counts(0))
    got.close()
    on, off = enc.EncodeBatch([bare, bare], config(a.bits, 8)), enc.EncodeBatch([bare, bare], config(a.bits, 8, on=False))
    assert len(on) == len(off) == 2 and all(on[i] == off[i] for i in range(2))
    on.close()
    off.close()


def test_the_order_of_the_rows_does_not_matter(ctx):
    """two row orders of a cloud: byte-equal streams, normals included, which without the option differ"""
    for name in ("runs-1-2-5-3000-8", "fold-and-diamond-edge-11", "ties-20", "cloud-2100"):
        case = nc.named(name)
        n = len(case.pos)
        orders = [np.random.default_rng(seed).permutation(n) for seed in (31, 32)]
        enc = dsa.DracoEncoder(ctx)
        a, b = [enc.EncodeBatch([nc.cloud(case, rows)], config(case.bits, case.nbits)) for rows in orders]
        assert a[0] == b[0] == twin(name)[0], name
        a.close()
        b.close()
        p, q = [enc.EncodeBatch([nc.cloud(case, rows)], config(case.bits, case.nbits, on=False)) for rows in orders]
        assert p[0] != q[0], name
        p.close()
        q.close()


def test_a_second_run_gives_the_same_bytes(ctx):
    """one batch twice in one process (the lane's arena is used again: sums and counts start from the memset, not from what the first
    run left): byte-equal streams"""
    group = [nc.named(name) for name in ("runs-1-2-5-3000-8", "tile-with-no-head-8", "axes-corners-zero-opposite-8", "ties-8")]
    clouds = [nc.cloud(c) for c in group]
    enc = dsa.DracoEncoder(ctx)
    a = enc.EncodeBatch(clouds, config(nc.BITS, 8))
    b = enc.EncodeBatch(clouds, config(nc.BITS, 8))
    assert len(a) == len(b) == len(group) and all(a[i] == b[i] == twin(c.name)[0] for i, c in enumerate(group))
    a.close()
    b.close()


def options(on=1, mean=0, vote=0, N=0, D=0, merge=1, order=1, geometry=0, bits=None, nbits=None):
    o = native.EncodeNormalMeanOptions()
    native.lib().dsa_encode_default_normal_mean_options(C.byref(o))
    m = o.vote.mean.lod.cell_parts.split.merge
    o.mean_normals, o.vote.vote_attributes, o.vote.mean.mean_attributes, o.vote.mean.lod.lod_base_bits, o.vote.mean.lod.cell_parts.part_cells = on, vote, mean, D, N
    m.merge_points, m.order.point_order, m.order.sequential.geometry = merge, order, geometry
    if bits is not None:
        m.order.sequential.base.position_bits = bits
    if nbits is not None:
        m.order.sequential.base.normal_bits = nbits
    return o


def call(ctx, meshes, o):
    return cpt.call(ctx, meshes, o, "dsa_encode_normal_mean_sequential_batch")


def test_mean_normals_0_is_the_vote_call(ctx):
    """with a mean mask (the generic attribute, stream attribute 3), a vote mask (a listed label) and a refused cloud in between: handle
    for handle"""
    def cloud_of(n, seed):
        kw = cpt.attributes_of(n, seed)
        kw["attributes"] = kw["attributes"] + [dsa.Attribute(np.random.default_rng(seed).integers(0, 4, (n, 1)).astype(np.uint8))]
        return kw
    meshes = [cpt.cloud(mc.half_duplicated(n, 2200 + n), **cloud_of(n, n)) for n in (5, 1500)]
    bad = oc.random_cloud(300, 2201)
    bad[17, 0] = np.inf
    meshes.insert(1, dsa.PointCloudData(bad, position_grid=dsa.Grid([0, 0, 0], 2.0), **cloud_of(300, 2202)))
    for N, D, merge, mean, vote in ((400, 3, 1, 0b1000, 0b1000000), (400, 0, 1, 0b1000, 0), (0, 0, 1, 0, 0b1000000), (0, 0, 1, 0, 0), (0, 0, 0, 0, 0)):
        o = options(0, mean, vote, N, D, merge=merge)
        st, h = call(ctx, meshes, o)
        st2, h2 = cpt.call(ctx, meshes, o.vote, "dsa_encode_vote_sequential_batch")
        assert st == st2 == 0
        new, old = cpt.handle_of(ctx, h, meshes, merge), cpt.handle_of(ctx, h2, meshes, merge)
        assert new == old and len(new[1]) >= 3 and new[1][1][0] == native.DSA_ERR_INVALID_ARGUMENT and "row 17" in new[1][1][1]
    # with the option the same clouds differ in their normals alone, and the handle's rows do not move
    good = [meshes[0], meshes[2]]
    st, h = call(ctx, good, options(1, 0b1000, 0b1000000, 400))
    st2, h2 = call(ctx, good, options(0, 0b1000, 0b1000000, 400))
    assert st == st2 == 0
    new, old = cpt.handle_of(ctx, h, good, 1), cpt.handle_of(ctx, h2, good, 1)
    assert new[0] == old[0] and len(new[1]) == len(old[1]) and any(x[1] != y[1] for x, y in zip(new[1], old[1])) and all(x[2:] == y[2:] for x, y in zip(new[1], old[1]))
    # a config without mean_normals arrives at the call it always took, and its bytes are the new entry's
    via_config = dsa.DracoEncoder(ctx).EncodeBatch(good, cpt.config(400, mean_attributes=0b1000, vote_attributes=0b1000000))
    assert len(via_config) == len(old[1]) and all(via_config[s] == old[1][s][1] for s in range(len(via_config)))
    via_config.close()


def test_refusals(ctx):
    """the call-level refusals and their words; a mask bit on the normals stays refused per cloud with the words it always had, with
    the option as without"""
    rng = np.random.default_rng(2300)
    pos = np.repeat(oc.random_cloud(40, 2301), 3, axis=0)
    n = len(pos)
    label = dsa.Attribute(rng.integers(0, 4, (n, 1)).astype(np.uint8))
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    with_normals = dsa.PointCloudData(pos, normals=nrm, attributes=[label])        # stream: positions, normals, label
    plain = dsa.PointCloudData(pos, attributes=[label])                            # positions, label
    for o, text in ((options(1, merge=0), "mean_normals 1 needs merge_points 1"), (options(2), "mean_normals 2: 0"), (options(0xFFFFFFFF), "mean_normals 4294967295"),
                    (options(2, merge=0), "mean_normals 2"), (options(1, order=0), "merge_points 1 needs point_order 1"), (options(1, geometry=1), "merge_points 1 needs geometry 0"),
                    (options(1, D=3), "lod_base_bits 3 needs part_cells >= 1"), (options(1, N=-1), "part_cells -1"), (options(1, mean=1 << 16), "mean_attributes 0x10000: a bit at or above 16"),
                    (options(1, vote=1 << 16), "vote_attributes 0x10000: a bit at or above 16"), (options(1, mean=0b100, vote=0b110), "vote_attributes 0x6 and mean_attributes 0x4 share a bit")):
        st, _ = call(ctx, [with_normals], o)
        assert st == native.DSA_ERR_INVALID_ARGUMENT and text in ctx.error(), (text, ctx.error())
    for k in (0, 4, 6):
        o = options(1)
        o.reserved[k] = 1
        assert call(ctx, [with_normals], o)[0] == native.DSA_ERR_INVALID_ARGUMENT and "dsa_encode_normal_mean_options.reserved[%d]" % k in ctx.error()
    o = options(0)
    o.reserved[2] = -1
    assert call(ctx, [with_normals], o)[0] == native.DSA_ERR_INVALID_ARGUMENT and "dsa_encode_normal_mean_options.reserved[2]" in ctx.error()
    o = options(1)
    o.vote.reserved[4] = 1
    assert call(ctx, [with_normals], o)[0] == native.DSA_ERR_INVALID_ARGUMENT and "dsa_encode_vote_options.reserved[4]" in ctx.error()
    o = options(1)
    o.vote.mean.reserved[0] = 1
    assert call(ctx, [with_normals], o)[0] == native.DSA_ERR_INVALID_ARGUMENT and "dsa_encode_mean_options.reserved[0]" in ctx.error()
    # a bit of either mask on the normals: the cloud fails alone, in today's words; its neighbour without normals takes the bit as its label
    want = synth.encode_merged(pos, extra=[synth.Extra(label.values)], opt=synth.options(pos_bits=11), mean_attributes=2)[0]
    st, h = call(ctx, [plain, with_normals, plain], options(1, mean=2))
    assert st == 0
    got = encodecall.streams(ctx, h, 3)
    assert got[0] == got[2] == (0, want)
    assert got[1][0] == native.DSA_ERR_INVALID_ARGUMENT and "mean_attributes 0x2" in got[1][1] and "mean normals are not built (octahedral integers do not average across the fold)" in got[1][1], got[1]
    st, h = call(ctx, [with_normals, plain], options(1, vote=2))
    assert st == 0
    got = encodecall.streams(ctx, h, 2)
    assert got[0][0] == native.DSA_ERR_INVALID_ARGUMENT and all(w in got[0][1] for w in ("vote_attributes 0x2", "attribute 1", "normals", "a vote over octahedral integers is not built")), got[0]
    assert got[1] == (0, synth.encode_merged(pos, extra=[synth.Extra(label.values)], opt=synth.options(pos_bits=11), vote_attributes=2)[0])
    # the label beside the normals voted on, the normals averaged: what the refusals leave to ask for
    st, h = call(ctx, [with_normals], options(1, vote=0b100))
    assert st == 0
    got = encodecall.streams(ctx, h, 1)
    assert got[0] == (0, synth.encode_merged(pos, normals=nrm, extra=[synth.Extra(label.values)], opt=synth.options(pos_bits=11), vote_attributes=0b100, mean_normals=True)[0])
    # the package answers earlier
    with pytest.raises(ValueError, match="mean_normals.*merge_points=MERGE_CELLS"):
        dsa.Config(mean_normals=True, encoding_method=0, point_order=dsa.POINT_ORDER_MORTON)
    with pytest.raises(ValueError, match="takes point clouds"):
        dsa.DracoEncoder(ctx).EncodeBatch([dsa.MeshData(pos, np.array([[0, 1, 2]], np.uint32))], config(11, 8))
