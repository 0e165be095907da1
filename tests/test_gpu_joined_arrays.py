"""Joined vertex arrays on the device (dsa_batch_joined_arrays; Batch.joined_arrays; k_joined_arrays of
draco-sharp_amd/csrc/dsa_joined_arrays.h): the part streams of a cloud as one array per attribute.  Everything is compared bit for
bit: the stream order with the concatenation of the same batch's vertex_views (the oracle-pinned path of test_gpu_vertex_arrays),
the input order with the arrays the encoder was given and with the stream order permuted by the handle's entry_rows.  The shapes
sit on the kernel's edges: parts of 1, 2, 63, 64, 65, 255, 256, 257 and TILE + 1 points -- a wave, the 256 points of a chunk, more
than one block -- whose byte rows (uint8 x 3, int16 x 3) start at rows that are not dword aligned, and one cloud of 300 parts."""
import ctypes as C

import numpy as np
import pytest

import draco_sharp_amd as dsa
import draco_sharp_amd.synth as synth
from draco_sharp_amd import encoder, native

pytestmark = pytest.mark.gpu

T = dsa.ENCODE_ORDER_TILE
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, T + 1]
FORMATS = ("values", "quantized")


@pytest.fixture(scope="module")
def ctx():
    c = dsa.Context(0)
    yield c
    c.close()


def cloud(n, seed, extras=True):
    """positions, octahedral normals, a uint8 x 3 colour, an int16 x 3, a uint16 x 1 and a float32 x 4 at 8 bits"""
    rng = np.random.default_rng(seed)
    pos = rng.random((n, 3), np.float32)
    if not extras:
        return dsa.PointCloudData(pos)
    return dsa.PointCloudData(pos, normals=rng.normal(size=(n, 3)).astype(np.float32),
                              attributes=[dsa.Attribute(rng.integers(0, 256, (n, 3)).astype(np.uint8), attribute_type=2),
                                          dsa.Attribute(rng.integers(-30000, 30000, (n, 3)).astype(np.int16)),
                                          dsa.Attribute(rng.integers(0, 65536, (n, 1)).astype(np.uint16)),
                                          dsa.Attribute(rng.random((n, 4)).astype(np.float32), quantization_bits=8)])


def split(ctx, clouds, N, **kw):
    return dsa.DracoEncoder(ctx).EncodeBatch(clouds, dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, part_points=N, **kw))


@pytest.fixture(scope="module")
def sized(ctx):
    """[(cloud, handle)]: per part size s a cloud of 3 s points in 3 parts of s, and 599 points in 300 parts of 1 - 2"""
    out = []
    for k, s in enumerate(SIZES):
        m = cloud(3 * s, 900 + k)
        out.append((m, split(ctx, [m], s)))
        assert [out[-1][1].part_info(p).num_points for p in out[-1][1].parts(0)] == [s, s, s]
    m = cloud(599, 950)
    out.append((m, split(ctx, [m], 2)))
    assert len(out[-1][1].parts(0)) == 300
    yield out
    for _, h in out:
        h.close()


def host(v):
    return None if v is None else np.ascontiguousarray(v)


def concatenated(b, members, fmt, attribute_types=None):
    """per attribute the concatenation of the members' vertex arrays (None: absent), from a request of the same batch"""
    b.vertex_arrays(fmt, attribute_types=attribute_types)
    views = [b.vertex_views(i) for i in members]
    out = []
    for a in range(len(views[0]["attributes"])):
        rows = [host(v["attributes"][a]["values"]) for v in views]
        assert len({r is None for r in rows}) == 1
        out.append(None if rows[0] is None else np.concatenate(rows))
    return out


def same(got, want):
    assert (got is None) == (want is None)
    if want is not None:
        got = host(got)
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def check_group(b, g, views, first, count, fmt, attribute_types=None):
    want = concatenated(b, range(first, first + count), fmt, attribute_types)
    points = [b.mesh_info(i).num_points for i in range(first, first + count)]
    sums = np.cumsum([0] + points)
    assert views["num_rows"] == sums[-1] and views["members"] == [(first + k, int(sums[k]), points[k]) for k in range(count)]
    for k in range(count):
        assert b.joined_member(first + k) == (g, int(sums[k]), points[k])
    assert len(views["attributes"]) == len(want)
    for a, w in enumerate(want):
        same(views["attributes"][a]["values"], w)
    return want


def test_stream_order_is_the_concatenation_of_the_vertex_arrays(ctx, sized):
    streams, groups = [], []
    for m, h in sized:
        s, g, _ = encoder.join_plan(h)
        groups += [(len(streams) + f, c) for f, c in g]
        streams += s
    assert len(groups) == len(SIZES) + 1 and groups[-1][1] == 300
    b = dsa.Batch(ctx, streams)
    b.decode()
    for fmt in FORMATS:
        got = b.joined_arrays(groups, fmt)
        for g, (first, count) in enumerate(groups):
            want = check_group(b, g, got[g], first, count, fmt)
            assert all(w is not None for w in want) and [w.shape[1] for w in want] == ([3, 3, 3, 3, 1, 4] if fmt == "values" else [3, 2, 3, 3, 1, 4])
            assert got[g]["attributes"][0]["quantization"] is None if fmt == "values" else got[g]["attributes"][0]["quantization"][2] == 11
        assert b.joined_arrays_bytes(groups, fmt) > 0
    # an attribute mask: positions and colours alone, nothing reserved for the rest
    got = b.joined_arrays(groups, "values", attribute_types=[0, 2])
    for g, (first, count) in enumerate(groups):
        want = check_group(b, g, got[g], first, count, "values", attribute_types=[0, 2])
        assert [w is None for w in want] == [False, True, False, True, True, True]
    assert b.joined_arrays_bytes(groups, "values", attribute_types=[0, 2]) < b.joined_arrays_bytes(groups, "values")
    b.close()


def test_more_than_16_bits_are_absent_from_the_quantized_join(ctx):
    m = cloud(130, 960)
    h = split(ctx, [m], 65, position_bits=18)
    streams, groups, _ = encoder.join_plan(h)
    b = dsa.Batch(ctx, streams)
    b.decode()
    got, = b.joined_arrays(groups, "quantized")
    want = check_group(b, 0, got, 0, 2, "quantized")
    assert want[0] is None and got["attributes"][0]["values"] is None and want[1] is not None
    got, = b.joined_arrays(groups, "values")
    assert check_group(b, 0, got, 0, 2, "values")[0] is not None
    b.close(); h.close()


def test_groups_beside_an_ungrouped_mesh_into_caller_memory(ctx, sized):
    """two adjacent groups, an ungrouped mesh, a group of one member; the bytes of `dst` outside the reported arrays stay as they were"""
    L = native.lib()
    (_, h63), (_, h257) = sized[2], sized[7]
    streams = h63[:] + h257[:] + h63[:1] + h257[1:2]
    groups = [(0, 3), (3, 3), (7, 1)]                        # mesh 6 is in no group
    b = dsa.Batch(ctx, streams)
    b.decode(wait=False)
    for fmt in FORMATS:
        req, arr, n = b._join_request(groups, fmt, None, "stream", False)
        nbytes = b.joined_arrays_bytes(groups, fmt)
        buf = np.full(nbytes + 64, 0xA5, np.uint8)
        assert L.dsa_batch_joined_arrays(b._h, C.byref(req), n, arr, None, None, buf.ctypes.data, nbytes - 1) == native.DSA_ERR_INVALID_ARGUMENT and "dst_bytes" in ctx.error()
        assert L.dsa_batch_joined_arrays(b._h, C.byref(req), n, arr, None, None, buf.ctypes.data, nbytes) == 0
        b.wait()
        assert L.dsa_batch_host_joined_arrays(b._h) == buf.ctypes.data
        covered = np.zeros(len(buf), bool)
        for g, (first, count) in enumerate(groups):
            views = b.joined_views(g)
            check_group(b, g, views, first, count, fmt)
            lay = native.JoinedArrays()
            assert L.dsa_batch_joined_arrays_layout(b._h, g, C.byref(lay)) == 0 and (lay.first_mesh, lay.num_meshes, lay.order) == (first, count, 0)
            for a in range(6):
                va = lay.attributes[a]
                assert va.offset % 64 == 0 and va.offset + va.stride * lay.num_rows <= nbytes and not covered[va.offset:va.offset + va.stride * lay.num_rows].any()
                covered[va.offset:va.offset + va.stride * lay.num_rows] = True
        assert (buf[~covered] == 0xA5).all()
        with pytest.raises(Exception, match="mesh 6 is in no group"):
            b.joined_member(6)
    b.close()


def entry_rows_of(h, i):
    return np.concatenate([h.entry_rows(s)[0] for s in h.parts(i)]).astype(np.int64)


def check_input_order(b, m, h, i, g, first, count, got_input, got_stream):
    perm = entry_rows_of(h, i)
    n = len(m.positions)
    assert np.array_equal(np.sort(perm), np.arange(n)) and got_input["num_rows"] == n
    for a, (vi, vs) in enumerate(zip(got_input["attributes"], got_stream["attributes"])):
        want = np.empty_like(host(vs["values"]))
        want[perm] = host(vs["values"])
        same(vi["values"], want)
    if len(m.attributes):
        for a, att in zip((2, 3, 4), m.attributes[:3]):             # integer attributes: the caller's own arrays
            same(got_input["attributes"][a]["values"], att.values.reshape(n, -1))


def test_input_order_of_part_handles_and_a_plain_ordered_handle(ctx, sized):
    for m, h in sized:
        streams, groups, em = encoder.join_plan(h)
        b = dsa.Batch(ctx, streams)
        b.decode(wait=False)
        for fmt in FORMATS:
            stream, = b.joined_arrays(groups, fmt)
            stream = {"attributes": [{"values": None if v["values"] is None else host(v["values"]).copy()} for v in stream["attributes"]]}
            got, = b.joined_arrays(groups, fmt, order="input", encoded=h, encoded_mesh=em)
            check_input_order(b, m, h, 0, 0, 0, len(streams), got, stream)
        b.close()
    # a plain point_order = 1 handle (one stream per cloud) and two split clouds in one batch, the groups shuffled: encoded_mesh says which stream a mesh is
    clouds = [cloud(300, 970), cloud(2 * 257 + 5, 971)]
    plain = dsa.DracoEncoder(ctx).EncodeBatch(clouds, dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON))
    b = dsa.Batch(ctx, plain[:])
    b.decode()
    for fmt in FORMATS:
        stream = b.joined_arrays([(0, 1), (1, 1)], fmt)
        stream = [{"attributes": [{"values": host(v["values"]).copy()} for v in s["attributes"]]} for s in stream]
        got = b.joined_arrays([(0, 1), (1, 1)], fmt, order="input", encoded=plain)
        for i in range(2):
            check_input_order(b, clouds[i], plain, i, i, i, 1, got[i], stream[i])
    b.close(); plain.close()
    h = split(ctx, clouds, 257)
    r0, r1 = h.parts(0), h.parts(1)
    assert (len(r0), len(r1)) == (2, 3)
    order = list(r1) + list(r0)                             # input 1's parts first
    b = dsa.Batch(ctx, [h[s] for s in order])
    b.decode()
    groups = [(0, 3), (3, 2)]
    stream = b.joined_arrays(groups, "values")
    stream = [{"attributes": [{"values": host(v["values"]).copy()} for v in s["attributes"]]} for s in stream]
    got = b.joined_arrays(groups, "values", order="input", encoded=h, encoded_mesh=order)
    check_input_order(b, clouds[1], h, 1, 0, 0, 3, got[0], stream[0])
    check_input_order(b, clouds[0], h, 0, 1, 3, 2, got[1], stream[1])
    # members that are not all parts of one input in part order fail alone, with the member named
    bad = b.joined_arrays([(0, 2), (3, 2)], "values", order="input", encoded=h, encoded_mesh=order)
    assert isinstance(bad[0], Exception) and "all parts of one input in part order" in str(bad[0]) and not isinstance(bad[1], Exception)
    swapped = [order[1], order[0]] + order[2:]
    bad = b.joined_arrays(groups, "values", order="input", encoded=h, encoded_mesh=swapped)
    assert isinstance(bad[0], Exception) and "part order" in str(bad[0]) and "compressed length" not in str(bad[1])
    b.close(); h.close()


def test_levels_of_a_lod_handle_are_prefixes(ctx):
    rng = np.random.default_rng(980)
    m = dsa.PointCloudData(rng.random((3000, 3), np.float32), attributes=[dsa.Attribute(rng.integers(0, 256, (3000, 3)).astype(np.uint8), attribute_type=2)])
    h = dsa.DracoEncoder(ctx).EncodeBatch([m], dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, merge_points=dsa.MERGE_CELLS, part_cells=100, lod_base_bits=2,
                                                          position_bits=5))
    streams, groups, _ = encoder.join_plan(h)
    levels = h.levels(0)
    assert len(levels) == 4 and sum(len(r) for r in levels) == len(streams) and sum(len(r) > 0 for r in levels) >= 3
    b = dsa.Batch(ctx, streams)
    b.decode()
    for fmt in FORMATS:
        got, = b.joined_arrays(groups, fmt)
        want = check_group(b, 0, got, 0, len(streams), fmt)
        end = 0
        for level, r in enumerate(levels):
            if len(r) == 0:
                continue
            info = h.lod_info(r.start)
            assert info.level == level and b.joined_member(r.start)[1] == end         # the level starts where the levels before it end
            end += info.level_points
            nxt = b.joined_member(r.stop)[1] if r.stop < len(streams) else got["num_rows"]
            assert nxt == end
            prefix = concatenated(b, range(0, r.stop), fmt)                            # levels 0 .. level alone
            for a, p in enumerate(prefix):
                same(host(got["attributes"][a]["values"])[:end], p)
        assert end == got["num_rows"]
    b.close(); h.close()


def bits_of(t, like):
    """A device tensor's bits as the numpy array the host view is (torch has no uint16 / uint32: those arrive as signed views)."""
    a = t.cpu().numpy()
    assert a.dtype.itemsize == like.dtype.itemsize and a.dtype.kind == ("i" if like.dtype.kind == "u" and like.dtype.itemsize > 1 else like.dtype.kind)
    return a.view(like.dtype)


def test_device_only_views_equal_the_host_views(ctx, sized):
    (m, h) = sized[8]
    streams, groups, em = encoder.join_plan(h)
    b = dsa.Batch(ctx, streams)
    b.decode(wait=False)
    for fmt in FORMATS:
        for order in ("stream", "input"):
            kw = dict(order=order, encoded=h if order == "input" else None, encoded_mesh=em if order == "input" else None)
            want, = b.joined_arrays(groups, fmt, **kw)
            want = [host(v["values"]).copy() for v in want["attributes"]]
            got, = b.joined_arrays(groups, fmt, device_only=True, **kw)
            assert not native.lib().dsa_batch_host_joined_arrays(b._h) and native.lib().dsa_batch_device_joined_arrays(b._h)
            with pytest.raises(RuntimeError):
                b.joined_views(0)
            for v, w in zip(got["attributes"], want):
                same(bits_of(v["values"], w), w)
    b.close()


def test_groups_fail_alone(ctx, sized):
    (_, h64), (_, h65) = sized[3], sized[4]
    # a member with a truncated stream: its group returns the member's status, the neighbour is intact
    cut = h64[1][:len(h64[1]) // 2]
    b = dsa.Batch(ctx, [h64[0], cut, h64[2]] + h65[:])
    b.decode()
    assert b.status(1) != 0
    got = b.joined_arrays([(0, 3), (3, 3)], "values")
    assert isinstance(got[0], Exception) and "group 0, member 1: mesh 1 failed to decode" in str(got[0])
    lay = native.JoinedArrays()
    assert native.lib().dsa_batch_joined_arrays_layout(b._h, 0, C.byref(lay)) == b.status(1)
    check_group(b, 1, got[1], 3, 3, "values")
    b.close()
    # members on different grids: two clouds coded on their own bounds
    two = dsa.DracoEncoder(ctx).EncodeBatch([cloud(70, 990), cloud(90, 991)], dsa.Config(encoding_method=0))
    pos, nrm, uv, faces = synth.make_mesh(synth.GRID, 6, 5, 1)
    mesh = synth.encode_mesh(pos, faces, nrm, uv)
    merged = dsa.DracoEncoder(ctx).EncodeBatch([cloud(200, 992)], dsa.Config(encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, merge_points=dsa.MERGE_CELLS, position_bits=4))
    b = dsa.Batch(ctx, two[:] + [mesh, two[0], two[0]] + dsa.DracoEncoder(ctx).EncodeBatch([cloud(70, 993, extras=False)], dsa.Config(encoding_method=0))[:] + merged[:])
    b.decode()
    got = b.joined_arrays([(0, 2), (2, 2), (4, 2), (6, 1)], "quantized")
    assert isinstance(got[0], Exception) and "another grid" in str(got[0]) and "group 0, member 1" in str(got[0])
    assert isinstance(got[1], Exception) and "group 1, member 0: mesh 2 has faces" in str(got[1])
    assert isinstance(got[2], Exception) and "group 2, member 1: the attribute table of mesh 5 differs" in str(got[2])
    check_group(b, 3, got[3], 6, 1, "quantized")
    got = b.joined_arrays([(0, 2), (6, 1)], "values")                     # floats need no common grid
    check_group(b, 0, got[0], 0, 2, "values")
    got = b.joined_arrays([(6, 1)], "values", order="input", encoded=merged, encoded_mesh=[0] * 7)
    assert isinstance(got[0], Exception) and "merge_points = 1" in str(got[0])
    two.close(); merged.close()
    # what the call itself refuses
    L = native.lib()

    def call(groups, fmt="values", order="stream", encoded=None, edit=None, null_groups=False):
        req, arr, n = b._join_request(groups, fmt, None, order, False)
        if edit:
            edit(req)
        st = L.dsa_batch_joined_arrays(b._h, C.byref(req), n, None if null_groups else arr, encoded, None, None, 0)
        if order == "stream":                       # what the call refuses has no size either
            assert L.dsa_batch_joined_arrays_bytes(b._h, C.byref(req), n, None if null_groups else arr) == 0
        return st, ctx.error()

    for kw, text in ((dict(groups=[(0, 1)], edit=lambda r: setattr(r.arrays, "format", 7)), "arrays.format"),
                     (dict(groups=[(0, 1)], edit=lambda r: setattr(r.arrays, "flags", 4)), "arrays.flags"),
                     (dict(groups=[(0, 1)], edit=lambda r: r.arrays.reserved.__setitem__(1, 1)), "arrays.reserved"),
                     (dict(groups=[(0, 1)], edit=lambda r: setattr(r, "order", 2)), "dsa_join_request.order"),
                     (dict(groups=[(0, 1)], edit=lambda r: r.reserved.__setitem__(6, 1)), "dsa_join_request.reserved"),
                     (dict(groups=[(0, 1)], null_groups=True), "groups is null"),
                     (dict(groups=[(0, 0)]), "groups[0].num_meshes is 0"),
                     (dict(groups=[(0, 1), (5, 3)]), "groups[1] (first_mesh 5, num_meshes 3) reaches beyond the batch of 7"),
                     (dict(groups=[(7, 1)]), "reaches beyond the batch"),
                     (dict(groups=[(0, 2), (1, 1)]), "groups[1]: mesh 1 is in two groups"),
                     (dict(groups=[(0, 1)], order="input"), "needs `encoded`")):
        st, err = call(**kw)
        assert st == native.DSA_ERR_INVALID_ARGUMENT and text in err, (kw, err)
    for cfg, text in ((dsa.Config(), "kept no rows"), (dsa.Config(track_rows=True), "Edgebreaker handle")):
        e = dsa.DracoEncoder(ctx).EncodeBatch([dsa.MeshData(pos, faces, nrm, uv)], cfg)
        st, err = call([(0, 1)], order="input", encoded=e._h)
        assert st == native.DSA_ERR_INVALID_ARGUMENT and text in err, err
        e.close()
    b.close()


def test_request_state(ctx, sized):
    (_, h) = sized[8]
    streams, groups, _ = encoder.join_plan(h)
    b = dsa.Batch(ctx, streams)
    with pytest.raises(Exception, match="dsa_batch_decode was not called"):
        b.joined_arrays(groups)
    b.decode(wait=False)
    assert b.joined_arrays(groups, "values", wait=False) is None          # queued before the wait, beside vertex arrays and a download
    b.vertex_arrays("values", wait=False)
    b.download(wait=False)
    with pytest.raises(Exception, match="joined arrays are still in flight"):
        b.joined_arrays(groups, "values", wait=False)
    b.wait()
    first = b.joined_views(0)
    want = [np.concatenate([host(b.vertex_views(i)["attributes"][a]["values"]) for i in range(3)]) for a in range(6)]
    for a in range(6):
        same(first["attributes"][a]["values"], want[a])
    b.decode()                                                               # a new decode invalidates the block
    with pytest.raises(Exception, match="no joined arrays were requested since the batch was decoded"):
        b.joined_views(0)
    assert not native.lib().dsa_batch_host_joined_arrays(b._h) and not native.lib().dsa_batch_device_joined_arrays(b._h)
    got, = b.joined_arrays(groups, "quantized")
    check_group(b, 0, got, 0, 3, "quantized")
    b.close()
