"""Encode direction, the most frequent value of every cell in chosen attributes of merged point clouds on the device
(dsa_encode_vote_sequential_batch, vote_attributes != 0; Config(merge_points=MERGE_CELLS, vote_attributes=...); k_enc_vote_count /
k_enc_vote_best / k_enc_vote_store of draco-sharp_amd/csrc/dsa_encode_order.h and the tables of dsa_encode_layout.h).  Every stream
must be, byte for byte, the CPU coder's (synth.encode_merged / encode_cell_parts / encode_lod_parts with vote_attributes=), which sorts
where the kernels hash, and its decode the contract restated in Python (votecases.pin: Counter per cell, the highest count, then min
of the tuples); the handle is the one of the call without the mask.  The wave path of k_enc_vote_count -- head ballots, the shuffle of
the run's first tuple, one insert per agreeing group, the atomicCAS claims -- is held to the twin here alone: the shapes sit on the 64
entries of a wave step and the 1024-entry tile, a table is at load 1/2, winners come late and spread (votecases).  The largest cloud
has about 7 000 points."""
import ctypes as C

import numpy as np
import pytest

import encodecall
import mergecases as mc
import ordercases as oc
import test_gpu_encode_cell_parts as cpt
import test_gpu_encode_lod as lodt
import test_gpu_encode_means as mnt
import votecases as vc
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


def config(vote, mean=0, N=0, D=0, **kw):
    return dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, merge_points=dsa.MERGE_CELLS, part_cells=N, lod_base_bits=D, mean_attributes=mean,
                      vote_attributes=vote, position_bits=kw.pop("position_bits", vc.BITS), **kw)


def check_pin(case, streams, order=None):
    kept, cells, want = vc.pin(case)
    got = vc.decoded(streams)
    for a in want:
        assert np.array_equal(got[a], want[a] if order is None else want[a][order]), (case.name, a)


def test_every_case(ctx):
    """every case of votecases, the cases of one pair of masks crowded into one batch: byte-equal to the twin, the decode equal to the
    pin, the handle the one of the call with vote mask 0"""
    assert vc.TILE == T and max(len(g) for _, g in vc.groups()) >= 12 and max(len(c.pos) for c in vc.cases()) < 8000
    for (vote, mean), group in vc.groups():
        clouds = [vc.cloud(c) for c in group]
        enc = dsa.DracoEncoder(ctx)
        got, plain = enc.EncodeBatch(clouds, config(vote, mean)), enc.EncodeBatch(clouds, config(0, mean))
        assert len(got) == len(plain) == len(group)
        for i, c in enumerate(group):
            stream, kept, cells = synth.encode_merged(vote_attributes=vote, mean_attributes=mean, **vc.cpu_args(c))
            assert got[i] == stream, (c.name, len(got[i]), len(stream))
            check_pin(c, [got[i]])
            rows = got.entry_rows(i)
            assert len(rows) == 1 + len(vc.attributes(c)) and all(np.array_equal(r, kept) for r in rows)
            assert all(np.array_equal(x, y) for x, y in zip(rows, plain.entry_rows(i)))
            assert np.array_equal(got.row_entries(i), cells) and np.array_equal(plain.row_entries(i), cells)
            assert np.array_equal(got.cell_counts(i), np.bincount(cells, minlength=len(kept))) and np.array_equal(got.cell_counts(i), plain.cell_counts(i))
        got.close()
        plain.close()


@pytest.mark.parametrize("D", [0, 10])
def test_parts_and_levels(ctx, D):
    """the same through part_cells = 64 and through lod_base_bits: every part stream byte-equal to the twin, the joined entries equal to
    the pin (in kept or in lod order), the part records, boxes and rows unchanged against vote mask 0"""
    N, most = 64, 0
    for (vote, mean), group in vc.groups():
        clouds = [vc.cloud(c) for c in group]
        enc = dsa.DracoEncoder(ctx)
        got, plain = enc.EncodeBatch(clouds, config(vote, mean, N, D)), enc.EncodeBatch(clouds, config(0, mean, N, D))
        assert len(got) == len(plain)
        first = 0
        for i, (c, m) in enumerate(zip(group, clouds)):
            twin = synth.encode_lod_parts(part_cells=N, lod_base_bits=D, vote_attributes=vote, mean_attributes=mean, **vc.cpu_args(c))
            if D:
                lodt.check_levels(got, i, twin, D)
            r = got.parts(i)
            most = max(most, len(r))
            first = cpt.check_handle(ctx, got, i, first, m, twin, 1 + len(vc.attributes(c)), vc.BITS)
            kept, cells, want = vc.pin(c)
            at = np.zeros(len(cells), np.int64)
            at[kept] = np.arange(len(kept))
            check_pin(c, [got[s] for s in r], at[twin.kept])
            assert plain.parts(i) == r
            for s in r:
                assert bytes(got.part_info(s)) == bytes(plain.part_info(s)) and all(np.array_equal(x, y) for x, y in zip(got.entry_rows(s), plain.entry_rows(s)))
            assert np.array_equal(got.row_entries(r[0]), plain.row_entries(r[0]))
        assert first == len(got)
        got.close()
        plain.close()
    assert most >= 5            # a cloud cut into several parts


def test_the_order_of_the_rows_does_not_matter(ctx):
    """two row orders of ties, pairs and the crowded tables: byte-equal streams, which without the mask differ"""
    for name in ("ties", "pairs", "all-distinct-3000", "three-way-tie-3000", "same-two-values"):
        case = vc.named(name)
        n = len(case.pos)
        orders = [np.random.default_rng(seed).permutation(n) for seed in (21, 22)]      # (whose first rows carry different values, also in the clouds of one cell)
        enc = dsa.DracoEncoder(ctx)
        a, b = [enc.EncodeBatch([vc.cloud(case, rows)], config(case.vote)) for rows in orders]
        assert a[0] == b[0] and a[0] == synth.encode_merged(vote_attributes=case.vote, **vc.cpu_args(case, orders[0]))[0], name
        check_pin(case, [a[0]])
        assert len(a.entry_rows(0)[0]) == 1 or not np.array_equal(a.entry_rows(0)[0], b.entry_rows(0)[0])      # (the kept row of a cloud of one cell is row 0)
        a.close()
        b.close()
        p, q = [enc.EncodeBatch([vc.cloud(case, rows)], config(0)) for rows in orders]
        assert p[0] != q[0], name
        p.close()
        q.close()


def options(vote, mean=0, N=0, D=0, merge=1, order=1, geometry=0, bits=None):
    o = native.EncodeVoteOptions()
    native.lib().dsa_encode_default_vote_options(C.byref(o))
    m = o.mean.lod.cell_parts.split.merge
    o.vote_attributes, o.mean.mean_attributes, o.mean.lod.lod_base_bits, o.mean.lod.cell_parts.part_cells = vote, mean, D, N
    m.merge_points, m.order.point_order, m.order.sequential.geometry = merge, order, geometry
    if bits is not None:
        m.order.sequential.base.position_bits = bits
    return o


def call(ctx, meshes, o):
    return cpt.call(ctx, meshes, o, "dsa_encode_vote_sequential_batch")


def test_mask_0_is_the_mean_call(ctx):
    """with a mean mask (the generic attribute, stream attribute 3) and a refused cloud in between: handle for handle"""
    meshes = [cpt.cloud(mc.half_duplicated(n, 950 + n), **cpt.attributes_of(n, n)) for n in (5, 1500)]
    bad = oc.random_cloud(300, 951)
    bad[17, 0] = np.inf
    meshes.insert(1, dsa.PointCloudData(bad, position_grid=dsa.Grid([0, 0, 0], 2.0), **cpt.attributes_of(300, 952)))
    for N, D, merge, mean in ((400, 3, 1, 0b1000), (400, 0, 1, 0b1000), (0, 0, 1, 0b1000), (0, 0, 1, 0), (0, 0, 0, 0)):
        o = options(0, mean, N, D, merge=merge)
        st, h = call(ctx, meshes, o)
        st2, h2 = cpt.call(ctx, meshes, o.mean, "dsa_encode_mean_sequential_batch")
        assert st == st2 == 0
        new, old = cpt.handle_of(ctx, h, meshes, merge), cpt.handle_of(ctx, h2, meshes, merge)
        assert new == old and len(new[1]) >= 3 and new[1][1][0] == native.DSA_ERR_INVALID_ARGUMENT and "row 17" in new[1][1][1]
    # a config without vote_attributes arrives at the call it always took, and its bytes are the new entry's
    good = [meshes[0], meshes[2]]
    via_config = dsa.DracoEncoder(ctx).EncodeBatch(good, cpt.config(400, mean_attributes=0b1000))
    st, h = call(ctx, good, options(0, 0b1000, 400))
    assert st == 0
    new = cpt.handle_of(ctx, h, good, 1)
    assert len(via_config) == len(new[1]) and all(via_config[s] == new[1][s][1] for s in range(len(via_config)))
    via_config.close()


def test_refusals(ctx):
    """the call-level refusals and their words; a cloud whose mask names positions, normals, a missing attribute or one of three
    components fails alone with its text, and its batch neighbours encode"""
    rng = np.random.default_rng(960)
    pos = np.repeat(oc.random_cloud(40, 961), 3, axis=0)
    n = len(pos)
    label, colour = dsa.Attribute(rng.integers(0, 4, (n, 1)).astype(np.uint8)), dsa.Attribute(rng.integers(0, 256, (n, 3)).astype(np.uint8))
    plain = dsa.PointCloudData(pos, attributes=[label, colour])                                           # stream: positions, label, colour
    with_normals = dsa.PointCloudData(pos, normals=rng.normal(size=(n, 3)).astype(np.float32), attributes=[label])        # positions, normals, label
    coloured = dsa.PointCloudData(pos, attributes=[colour])                                               # positions, colour (three components)
    bare = dsa.PointCloudData(pos)                                                                        # positions
    for o, text in ((options(2, merge=0, order=1), "vote_attributes 0x2 needs merge_points 1"), (options(1 << 16), "vote_attributes 0x10000: a bit at or above 16"),
                    (options(1 << 31), "a bit at or above 16"), (options(0b110, mean=0b100), "vote_attributes 0x6 and mean_attributes 0x4 share a bit"),
                    (options(2, order=0), "merge_points 1 needs point_order 1"), (options(2, geometry=1), "merge_points 1 needs geometry 0"),
                    (options(2, D=3), "lod_base_bits 3 needs part_cells >= 1"), (options(2, N=-1), "part_cells -1"), (options(2, mean=1 << 16), "mean_attributes 0x10000: a bit at or above 16")):
        st, _ = call(ctx, [plain], o)
        assert st == native.DSA_ERR_INVALID_ARGUMENT and text in ctx.error(), (text, ctx.error())
    o = options(2)
    o.reserved[4] = 1
    assert call(ctx, [plain], o)[0] == native.DSA_ERR_INVALID_ARGUMENT and "dsa_encode_vote_options.reserved[4]" in ctx.error()
    o = options(2)
    o.mean.reserved[0] = 1
    assert call(ctx, [plain], o)[0] == native.DSA_ERR_INVALID_ARGUMENT and "dsa_encode_mean_options.reserved[0]" in ctx.error()
    # mask 0b10: the label of `plain`, the normals of `with_normals`, the colour of `coloured`, nothing of `bare`
    st, h = call(ctx, [plain, with_normals, plain, bare, coloured, plain], options(2))
    assert st == 0
    got = encodecall.streams(ctx, h, 6)
    want = synth.encode_merged(pos, extra=[synth.Extra(label.values), synth.Extra(colour.values)], opt=synth.options(pos_bits=11), vote_attributes=2)[0]
    assert got[0] == got[2] == got[5] == (0, want)
    assert got[1][0] == native.DSA_ERR_INVALID_ARGUMENT and all(w in got[1][1] for w in ("vote_attributes 0x2", "attribute 1", "normals", "not built")), got[1]
    assert got[3][0] == native.DSA_ERR_INVALID_ARGUMENT and all(w in got[3][1] for w in ("vote_attributes 0x2", "attribute 1", "has 1 attributes")), got[3]
    assert got[4][0] == native.DSA_ERR_INVALID_ARGUMENT and all(w in got[4][1] for w in ("vote_attributes 0x2", "attribute 1", "3 components", "64 bits")), got[4]
    st, h = call(ctx, [plain, plain], options(3, N=7))               # the positions: every cloud fails alone, each in its one slot
    assert st == 0 and native.lib().dsa_encoded_size(h) == 2
    got = encodecall.streams(ctx, h, 2)
    assert all(g[0] == native.DSA_ERR_INVALID_ARGUMENT and "vote_attributes 0x3" in g[1] and "positions" in g[1] for g in got), got
    # the package answers earlier, in the words of mean_attributes
    base = dict(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON)
    with pytest.raises(ValueError, match="vote_attributes.*merge_points=MERGE_CELLS"):
        dsa.Config(vote_attributes=2, **base)
    with pytest.raises(ValueError, match="positions"):
        dsa.Config(vote_attributes=[0, 1], merge_points=dsa.MERGE_CELLS, **base)
    with pytest.raises(ValueError, match="not both"):
        dsa.Config(vote_attributes=[1], mean_attributes=[1, 2], merge_points=dsa.MERGE_CELLS, **base)
    with pytest.raises(ValueError, match="same attributes"):
        dsa.DracoEncoder(ctx).EncodeBatch([plain, with_normals], config(2, position_bits=11))


def test_clouds_with_different_attribute_lists_in_one_call(ctx):
    """the three clouds of test_gpu_encode_means.mixed_clouds (1, 65 and 1 025 points; one listed attribute, then three) through the
    entry point itself -- the package refuses such a call -- with a mask that names the one-component attribute only the larger
    clouds have.  As with the means, the library refuses the first cloud alone and so does the twin: no cloud that is laid out has
    fewer voted streams than the mask has bits, and the kernels' return on blockIdx.y guards what no accepted call reaches.  Held
    here: the refused cloud in front takes no record, the two behind it read their own and are the twin's, kept rows and row
    entries included"""
    clouds, mask = mnt.mixed_clouds(991), 0b1000
    cfg = config(mask, position_bits=6)
    with pytest.raises(ValueError, match="same attributes"):
        cfg._native_vote(0, clouds)
    st, h = call(ctx, clouds, cfg._native_vote(0, clouds[1:]))
    assert st == 0
    ranges, got = cpt.handle_of(ctx, h, clouds, 1)
    assert ranges == [(0, 1), (1, 1), (2, 1)] and len(got) == 3
    with pytest.raises(ValueError, match="does not have"):
        synth.encode_merged(vote_attributes=mask, **cpt.cpu_args(clouds[0], cfg))
    assert got[0][0] == native.DSA_ERR_INVALID_ARGUMENT and all(w in got[0][1] for w in ("vote_attributes 0x8", "attribute 3", "has 2 attributes")), got[0]
    for i in (1, 2):
        stream, kept, cells = synth.encode_merged(vote_attributes=mask, **cpt.cpu_args(clouds[i], cfg))
        assert got[i][:2] == (0, stream), (i, got[i][0])
        assert len(kept) < len(clouds[i].positions) and got[i][2] == np.asarray(kept, np.uint32).tobytes() and got[i][3] == np.asarray(cells, np.uint32).tobytes()


def test_the_refused_cases(ctx):
    """votecases.refusals: three components, normals, positions and a missing attribute fail their cloud alone, in its one slot,
    between two clouds that encode where the mask lets one; the same bit in both masks fails the call"""
    good = vc.cloud(vc.named("ties"))                       # three attributes of one component beside the positions
    for case, whole, words, _ in vc.refusals():
        o = options(case.vote, case.mean, bits=vc.BITS)
        st, h = call(ctx, [good, vc.cloud(case), good], o)
        if whole:
            assert st == native.DSA_ERR_INVALID_ARGUMENT and all(w in ctx.error() for w in words), (case.name, ctx.error())
            continue
        assert st == 0 and native.lib().dsa_encoded_size(h) == 3, case.name
        got = encodecall.streams(ctx, h, 3)
        assert got[1][0] == native.DSA_ERR_INVALID_ARGUMENT and all(w in got[1][1] for w in words), (case.name, got[1])
        if case.vote & 1:
            assert got[0][0] == got[2][0] == native.DSA_ERR_INVALID_ARGUMENT
        else:
            want = synth.encode_merged(vote_attributes=case.vote, **vc.cpu_args(vc.named("ties")))[0]
            assert got[0] == got[2] == (0, want), case.name


@pytest.mark.parametrize("host_plan", ["0", "1"])
def test_chunks_and_plans(ctx, monkeypatch, host_plan):
    """1 500 clouds of 40 points in 3-bit cells with a voted label and an averaged colour cross a chunk boundary of inputs; the symbol
    plans by the host and by the device"""
    monkeypatch.setenv("DSA_ENC_HOST_PLAN", host_plan)
    rng = np.random.default_rng(980)
    clouds, args = [], []
    for _ in range(1500):
        pos = (rng.random((40, 3)) * [1.0, 1.0, 0.12]).astype(np.float32)
        label, colour = rng.integers(0, 3, (40, 1)).astype(np.uint8), rng.integers(0, 256, (40, 3)).astype(np.uint8)
        clouds.append(dsa.PointCloudData(pos, attributes=[dsa.Attribute(label), dsa.Attribute(colour)]))
        args.append(dict(pos=pos, extra=[synth.Extra(label), synth.Extra(colour)], opt=synth.options(pos_bits=3)))
    got = dsa.DracoEncoder(ctx).EncodeBatch(clouds, config(0b010, 0b100, position_bits=3))
    merged = 0
    for i, a in enumerate(args):
        stream, kept, cells = synth.encode_merged(vote_attributes=0b010, mean_attributes=0b100, **a)
        assert got[i] == stream, i
        merged += len(kept) < 40
    assert merged > 1400
    got.close()


def test_a_second_run_gives_the_same_bytes(ctx):
    """one batch twice in one process (the lane's arena is used again: tables, counts and values start from the memset, not from
    what the first run left): byte-equal streams"""
    group = [vc.named(name) for name in ("late-winner", "spread-majority", "all-distinct-3000", "same-two-values")]
    clouds = [vc.cloud(c) for c in group]
    enc = dsa.DracoEncoder(ctx)
    a = enc.EncodeBatch(clouds, config(0b10))
    b = enc.EncodeBatch(clouds, config(0b10))
    assert len(a) == len(b) == len(group) and all(a[i] == b[i] for i in range(len(group)))
    for i, c in enumerate(group):
        check_pin(c, [b[i]])
    a.close()
    b.close()
