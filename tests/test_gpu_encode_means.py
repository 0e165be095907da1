"""Encode direction, the mean of every cell in chosen attributes of merged point clouds on the device
(dsa_encode_mean_sequential_batch, mean_attributes != 0; Config(merge_points=MERGE_CELLS, mean_attributes=...); k_enc_mean_sum /
k_enc_mean_store of draco-sharp_amd/csrc/dsa_encode_order.h and the sums and counts of dsa_encode_layout.h).  Every stream must be,
byte for byte, the CPU coder's (synth.encode_merged / encode_cell_parts / encode_lod_parts with mean_attributes=), and its decode the
contract restated in Python integers (meancases.pin); the handle is the one of the call without the mask.  The wave path of
k_enc_mean_sum -- ballots, segmented shuffle sums, 64-bit atomics -- is held to the twin here alone: the shapes sit on the 64
entries of a wave step and the 1024-entry tile, the sums leave 32 bits (meancases)."""
import ctypes as C

import numpy as np
import pytest

import encodecall
import meancases as mn
import mergecases as mc
import oracle
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


def config(mask, N=0, D=0, **kw):
    return dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, merge_points=dsa.MERGE_CELLS, part_cells=N, lod_base_bits=D, mean_attributes=mask,
                      position_bits=kw.pop("position_bits", mn.BITS), **kw)


def groups():
    """the cases of one mask are a batch"""
    cases = mn.cases()
    return [(mask, [c for c in cases if c.mask == mask]) for mask in sorted({c.mask for c in cases})]


def check_pin(case, streams):
    kept, cells, want = mn.pin(case)
    got = mn.decoded(streams)
    for a in want:
        assert np.array_equal(got[a], want[a]), (case.name, a)


def test_every_case(ctx):
    """every case of meancases, the cases of one mask crowded into one batch: byte-equal to the twin, the decode equal to the pin, the
    handle the merged call's"""
    assert mn.TILE == T and max(len(g) for _, g in groups()) >= 12
    for mask, group in groups():
        got = dsa.DracoEncoder(ctx).EncodeBatch([mn.cloud(c) for c in group], config(mask))
        assert len(got) == len(group)
        for i, c in enumerate(group):
            stream, kept, cells = synth.encode_merged(mean_attributes=mask, **mn.cpu_args(c))
            assert got[i] == stream, (c.name, len(got[i]), len(stream))
            check_pin(c, [got[i]])
            rows = got.entry_rows(i)
            assert len(rows) == 1 + len(mn.attributes(c)) and all(np.array_equal(r, kept) for r in rows)
            assert np.array_equal(got.row_entries(i), cells) and np.array_equal(got.cell_counts(i), np.bincount(cells, minlength=len(kept)))
            assert got.cell_counts(i).dtype == np.uint32 and got.cell_counts(i).sum() == len(c.pos)
        got.close()


@pytest.mark.parametrize("D", [0, 10])
def test_parts_and_levels(ctx, D):
    """the same through part_cells = 64 and through lod_base_bits: every part stream byte-equal to the twin, the joined entries equal to
    the pin (in kept or in lod order), the part records and boxes unchanged against mask 0"""
    N, most = 64, 0
    for mask, group in groups():
        clouds = [mn.cloud(c) for c in group]
        enc = dsa.DracoEncoder(ctx)
        got, plain = enc.EncodeBatch(clouds, config(mask, N, D)), enc.EncodeBatch(clouds, config(0, N, D))
        assert len(got) == len(plain)
        first = 0
        for i, (c, m) in enumerate(zip(group, clouds)):
            twin = synth.encode_lod_parts(part_cells=N, lod_base_bits=D, mean_attributes=mask, **mn.cpu_args(c))
            if D:
                lodt.check_levels(got, i, twin, D)
            r = got.parts(i)
            most = max(most, len(r))
            first = cpt.check_handle(ctx, got, i, first, m, twin, 1 + len(mn.attributes(c)), mn.BITS)
            kept, cells, want = mn.pin(c)
            at = np.zeros(len(cells), np.int64)
            at[kept] = np.arange(len(kept))
            joined = mn.decoded([got[s] for s in r])
            for a in want:
                assert np.array_equal(joined[a], want[a][at[twin.kept]]), (c.name, a)
            assert plain.parts(i) == r
            for s in r:
                assert bytes(got.part_info(s)) == bytes(plain.part_info(s)) and all(np.array_equal(x, y) for x, y in zip(got.entry_rows(s), plain.entry_rows(s)))
            assert np.array_equal(got.row_entries(r[0]), plain.row_entries(r[0]))
        assert first == len(got)
        got.close()
        plain.close()
    assert most >= 5            # a cloud cut into several parts


def test_the_order_of_the_rows_does_not_matter(ctx):
    """two row orders of a cloud with mean_attributes="all": byte-equal streams, which without the mask differ"""
    for name in ("components", "all-of-it", "wide-sums"):
        case = next(c for c in mn.cases() if c.name == name)
        n = len(case.pos)
        orders = [np.random.default_rng(seed).permutation(n) for seed in (21, 22)]
        enc = dsa.DracoEncoder(ctx)
        cfg = config("all")
        assert cfg._mean_mask([mn.cloud(case)]) == (1 << (1 + len(mn.attributes(case)))) - 2
        a, b = [enc.EncodeBatch([mn.cloud(case, rows)], cfg) for rows in orders]
        assert a[0] == b[0] and a[0] == synth.encode_merged(mean_attributes=cfg._mean_mask([mn.cloud(case)]), **mn.cpu_args(case, orders[0]))[0]
        assert not np.array_equal(a.entry_rows(0)[0], b.entry_rows(0)[0])
        a.close()
        b.close()
        p, q = [enc.EncodeBatch([mn.cloud(case, rows)], config(0)) for rows in orders]
        assert p[0] != q[0]
        p.close()
        q.close()


def options(mask, N=0, D=0, merge=1, order=1, geometry=0):
    o = native.EncodeMeanOptions()
    native.lib().dsa_encode_default_mean_options(C.byref(o))
    m = o.lod.cell_parts.split.merge
    o.mean_attributes, o.lod.lod_base_bits, o.lod.cell_parts.part_cells, m.merge_points, m.order.point_order, m.order.sequential.geometry = mask, D, N, merge, order, geometry
    return o


def call(ctx, meshes, o):
    return cpt.call(ctx, meshes, o, "dsa_encode_mean_sequential_batch")


def test_mask_0_is_the_lod_call(ctx):
    meshes = [cpt.cloud(mc.half_duplicated(n, 950 + n), **cpt.attributes_of(n, n)) for n in (5, 1500)]
    bad = oc.random_cloud(300, 951)
    bad[17, 0] = np.inf
    meshes.insert(1, dsa.PointCloudData(bad, position_grid=dsa.Grid([0, 0, 0], 2.0)))
    for N, D, merge in ((400, 3, 1), (400, 0, 1), (0, 0, 1), (0, 0, 0)):
        o = options(0, N, D, merge=merge)
        st, h = call(ctx, meshes, o)
        st2, h2 = cpt.call(ctx, meshes, o.lod, "dsa_encode_lod_sequential_batch")
        assert st == st2 == 0
        new, old = cpt.handle_of(ctx, h, meshes, merge), cpt.handle_of(ctx, h2, meshes, merge)
        assert new == old and len(new[1]) >= 3 and new[1][1][0] == native.DSA_ERR_INVALID_ARGUMENT and "row 17" in new[1][1][1]
    # a config without mean_attributes arrives at the call it always took, and its bytes are the new entry's
    good = [meshes[0], meshes[2]]
    via_config = dsa.DracoEncoder(ctx).EncodeBatch(good, cpt.config(400))
    st, h = call(ctx, good, options(0, 400))
    assert st == 0
    new = cpt.handle_of(ctx, h, good, 1)
    assert len(via_config) == len(new[1]) and all(via_config[s] == new[1][s][1] for s in range(len(via_config)))
    via_config.close()


def test_refusals(ctx):
    """the call-level refusals and their words; a cloud whose mask names positions, normals or a missing attribute fails alone with
    its text, and its batch neighbours encode"""
    rng = np.random.default_rng(960)
    pos = np.repeat(oc.random_cloud(40, 961), 3, axis=0)
    n = len(pos)
    colour = dsa.Attribute(rng.integers(0, 256, (n, 4)).astype(np.uint8))
    plain = dsa.PointCloudData(pos, attributes=[colour])                                                  # stream: positions, colour
    with_normals = dsa.PointCloudData(pos, normals=rng.normal(size=(n, 3)).astype(np.float32), attributes=[colour])       # positions, normals, colour
    bare = dsa.PointCloudData(pos)                                                                        # positions
    for o, text in ((options(2, merge=0, order=1), "mean_attributes 0x2 needs merge_points 1"), (options(1 << 16), "mean_attributes 0x10000: a bit at or above 16"),
                    (options(1 << 31), "a bit at or above 16"), (options(2, order=0), "merge_points 1 needs point_order 1"), (options(2, geometry=1), "merge_points 1 needs geometry 0"),
                    (options(2, D=3), "lod_base_bits 3 needs part_cells >= 1"), (options(2, N=-1), "part_cells -1")):
        st, _ = call(ctx, [plain], o)
        assert st == native.DSA_ERR_INVALID_ARGUMENT and text in ctx.error(), (text, ctx.error())
    o = options(2)
    o.reserved[4] = 1
    assert call(ctx, [plain], o)[0] == native.DSA_ERR_INVALID_ARGUMENT and "dsa_encode_mean_options.reserved[4]" in ctx.error()
    o = options(2)
    o.lod.reserved[0] = 1
    assert call(ctx, [plain], o)[0] == native.DSA_ERR_INVALID_ARGUMENT and "dsa_encode_lod_options.reserved[0]" in ctx.error()
    # mask 0b10: the colour of `plain`, the normals of `with_normals`, nothing of `bare`
    st, h = call(ctx, [plain, with_normals, plain, bare, plain], options(2))
    assert st == 0
    got = encodecall.streams(ctx, h, 5)
    want = synth.encode_merged(pos, extra=[synth.Extra(colour.values)], opt=synth.options(pos_bits=11), mean_attributes=2)[0]
    assert got[0] == got[2] == got[4] == (0, want)
    assert got[1][0] == native.DSA_ERR_INVALID_ARGUMENT and all(w in got[1][1] for w in ("mean_attributes 0x2", "attribute 1", "normals", "not built")), got[1]
    assert got[3][0] == native.DSA_ERR_INVALID_ARGUMENT and all(w in got[3][1] for w in ("mean_attributes 0x2", "attribute 1", "has 1 attributes")), got[3]
    st, h = call(ctx, [plain, plain], options(3, N=7))               # the positions: every cloud fails alone, each in its one slot
    assert st == 0 and native.lib().dsa_encoded_size(h) == 2
    got = encodecall.streams(ctx, h, 2)
    assert all(g[0] == native.DSA_ERR_INVALID_ARGUMENT and "mean_attributes 0x3" in g[1] and "positions" in g[1] for g in got), got
    # the package answers earlier, in the style of merge_points
    base = dict(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON)
    with pytest.raises(ValueError, match="mean_attributes.*merge_points=MERGE_CELLS"):
        dsa.Config(mean_attributes=2, **base)
    with pytest.raises(ValueError, match="positions"):
        dsa.Config(mean_attributes=[0, 1], merge_points=dsa.MERGE_CELLS, **base)
    with pytest.raises(ValueError, match="same attributes"):
        dsa.DracoEncoder(ctx).EncodeBatch([plain, with_normals], config("all", position_bits=11))


def mixed_clouds(seed):
    """three clouds of 1, 65 and 1 025 points at 6 bits (one entry, a wave step and one, a tile and one), the first with one listed
    attribute, the others with three: a label of one byte, a colour, a float at 10 bits"""
    out = []
    for k, n in enumerate((1, 65, T + 1)):
        c = mc.half_duplicated(n, seed + n, bits=6)
        rng = np.random.default_rng(seed + 7 * n)
        atts = [dsa.Attribute(rng.integers(0, 4, (n, 1)).astype(np.uint8))]
        if k:
            atts += [dsa.Attribute(rng.integers(0, 256, (n, 3)).astype(np.uint8)), dsa.Attribute(rng.random((n, 1)).astype(np.float32), quantization_bits=10)]
        out.append(cpt.cloud(c, attributes=atts))
    return out


def test_clouds_with_different_attribute_lists_in_one_call(ctx):
    """an integer mask over all three listed attributes and the clouds of mixed_clouds in one call.  The mask names two attributes the
    first cloud does not have: the library refuses that cloud alone (test_refusals has the words) and so does the twin, so every cloud
    that is laid out lists as many masked streams as the mask has bits -- a block beyond a cloud's own streams (the kernels' return
    on blockIdx.y) is a guard that no accepted call reaches.  Held here: the refused cloud in front takes no record, the two clouds
    behind it read their own, and their streams, kept rows and row entries are the twin's"""
    clouds, mask = mixed_clouds(990), 0b1110
    cfg = config(mask, position_bits=6)
    got = dsa.DracoEncoder(ctx).TryEncodeBatch(clouds, cfg, keep=True)
    assert len(got) == 3
    with pytest.raises(ValueError, match="does not have"):
        synth.encode_merged(mean_attributes=mask, **cpt.cpu_args(clouds[0], cfg))
    assert isinstance(got[0], Exception) and all(w in str(got[0]) for w in ("mean_attributes 0xe", "attribute 2", "has 2 attributes")), got[0]
    for i in (1, 2):
        stream, kept, cells = synth.encode_merged(mean_attributes=mask, **cpt.cpu_args(clouds[i], cfg))
        assert got[i] == stream, (i, got[i] if isinstance(got[i], Exception) else len(got[i]), len(stream))
        assert len(kept) < len(clouds[i].positions) and all(np.array_equal(r, kept) for r in got.encoded.entry_rows(i))
        assert np.array_equal(got.encoded.row_entries(i), cells)
    got.encoded.close()


def test_an_explicit_grid_on_a_masked_float_attribute(ctx):
    """the means are means of the integers on the caller's grid, and the header carries that grid"""
    rng = np.random.default_rng(970)
    base = mc.along_z("grid", rng.integers(1, 70, 40), mn.BITS, 970)
    n = len(base.pos)
    values = (rng.random((n, 2)) * 3 - 1).astype(np.float32)
    case = mn.make(base, uvs=rng.random((n, 2)).astype(np.float32), extras=[(values, 13, ([-1.25, -1.5], 4.0))], mask=0b110)
    m = dsa.PointCloudData(case.pos, texcoords=case.uvs, attributes=[dsa.Attribute(values, quantization_bits=13, grid=dsa.Grid([-1.25, -1.5], 4.0))],
                           position_grid=dsa.Grid(case.grid[0], float(case.grid[1])), texcoord_grid=dsa.Grid([-0.5, -0.25], 2.0))
    args = mn.cpu_args(case)
    args["uv_grid"] = synth.grid([-0.5, -0.25], 2.0)
    got = dsa.DracoEncoder(ctx).EncodeBatch([m], config(0b110))
    stream, kept, cells = synth.encode_merged(mean_attributes=0b110, **args)
    assert got[0] == stream
    dec = oracle.decode(got[0])
    assert list(dec.attributes[2].q_min[:2]) == [-1.25, -1.5] and dec.attributes[2].q_range == 4.0 and dec.attributes[1].q_range == 2.0
    q = synth.quantized(values, 13, synth.grid([-1.25, -1.5], 4.0)).astype(np.int64)
    want = np.array([[mn.mean(q[cells == j, c]) for c in range(2)] for j in range(len(kept))])
    assert np.array_equal(dec.attributes[2].portable, want) and np.bincount(cells).max() >= 64
    got.close()


@pytest.mark.parametrize("host_plan", ["0", "1"])
def test_chunks_and_plans(ctx, monkeypatch, host_plan):
    """1 500 clouds of 40 points in 3-bit cells with a colour and a float attribute cross a chunk boundary of inputs; the symbol plans
    by the host and by the device"""
    monkeypatch.setenv("DSA_ENC_HOST_PLAN", host_plan)
    rng = np.random.default_rng(980)
    clouds, args = [], []
    for _ in range(1500):
        pos = (rng.random((40, 3)) * [1.0, 1.0, 0.12]).astype(np.float32)
        colour, scalar = rng.integers(0, 256, (40, 3)).astype(np.uint8), rng.normal(size=(40, 1)).astype(np.float32)
        clouds.append(dsa.PointCloudData(pos, attributes=[dsa.Attribute(colour), dsa.Attribute(scalar, quantization_bits=10)]))
        args.append(dict(pos=pos, extra=[synth.Extra(colour), synth.Extra(scalar, quantization_bits=10)], opt=synth.options(pos_bits=3)))
    got = dsa.DracoEncoder(ctx).EncodeBatch(clouds, config(0b110, position_bits=3))
    merged = 0
    for i, a in enumerate(args):
        stream, kept, cells = synth.encode_merged(mean_attributes=0b110, **a)
        assert got[i] == stream, i
        merged += len(kept) < 40
    assert merged > 1400
    got.close()
