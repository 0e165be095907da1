"""Vertex arrays (dsa_batch_vertex_arrays, Batch.vertex_arrays): per mesh one index array and per attribute one row per point,
gathered on the device (k_vertex_arrays) and downloaded in one transfer, as decoded values or as the portable integers of the
quantised attributes.  Every comparison is exact (bytes or integers): against the oracle's arrays gathered through its own point
maps, and, where it says so, against the INPUT alone."""
import ctypes as C
import os

import numpy as np
import pytest

import draco_sharp_amd as dsa
import draco_sharp_amd.synth as synth
import meshutil
import oracle
import typedcases
import vacases
from draco_sharp_amd import native
from test_gpu_download import check_views, streams_mixed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = dsa.Context(0)
    yield c
    c.close()


_refs = {}


def reference(stream):
    """The oracle's decode of a stream (None: it refuses the stream), once per distinct stream."""
    if stream not in _refs:
        try:
            _refs[stream] = oracle.decode(stream)
        except oracle.OracleError:
            _refs[stream] = None
    return _refs[stream]


def unsigned(t):
    """A device tensor's bits as the numpy array the host view would be (torch has no uint16 / uint32)."""
    a = t.cpu().numpy()
    return a.view({np.dtype(np.int16): np.uint16, np.dtype(np.int32): np.uint32}.get(a.dtype, a.dtype))


def check_mesh(views, ref, fmt, absent=(), device=False):
    """views: Batch.vertex_views(i) (device: device_vertex_views(i)) against the oracle mesh gathered by its own maps."""
    conv = unsigned if device else np.ascontiguousarray
    if ref.encoder_type == 0:
        assert views["indices"] is None
    else:
        idx = conv(views["indices"])
        assert idx.dtype in (np.uint16, np.uint32) and idx.shape == ref.faces.shape
        assert np.array_equal(idx, ref.faces)
    assert len(views["attributes"]) == len(ref.attributes)
    for a, (got, att) in enumerate(zip(views["attributes"], ref.attributes)):
        rows = vacases.expected_rows(ref, a, fmt)
        if rows is None or a in absent:
            assert got["values"] is None and got["quantization"] is None, (a, fmt)
            continue
        vals = conv(got["values"])
        assert vals.dtype == rows.dtype and vals.shape == rows.shape, (a, fmt, vals.dtype, vals.shape, rows.dtype, rows.shape)
        assert vals.tobytes() == rows.tobytes(), (a, fmt)
        if fmt == "quantized" and att.seq_type in (2, 3):
            qmin, qrange, bits = got["quantization"]
            assert bits == vacases.quantisation_bits(att)
            if att.seq_type == 2:
                assert np.array_equal(np.float32(qmin), np.float32(att.q_min[: att.num_components])) and np.float32(qrange) == np.float32(att.q_range)
        else:
            assert got["quantization"] is None


def check_batch(b, streams, fmt, device=False):
    for i, s in enumerate(streams):
        ref = reference(s)
        if ref is None:
            assert b.status(i) != 0
            with pytest.raises(Exception):
                b.vertex_views(i)
            continue
        assert b.status(i) == 0, (i, b.mesh_info(i).detail)
        check_mesh(b.device_vertex_views(i) if device else b.vertex_views(i), ref, fmt, device=device)


def seamed_grid():
    return synth.encode_mesh_corners(*meshutil.seamed_mesh(synth, synth.GRID, 40, 33, 3, "checker", "stripes"), opt=synth.options(force_scheme=1))


@pytest.fixture(scope="module")
def mixed():
    pos, nrm, uv, faces = synth.make_mesh(synth.TWO_PARTS, 12, 9, 6)
    # (and a sequential mesh: the general path in the first batch, one map per attribute)
    # (and the general path in the first batch -- a sequential mesh, prediction-degree order: one map per attribute -- and a
    # MultiParallelogram stream, which the fast kernels hand back: decoded a second time, block 1)
    return streams_mixed(5) + [seamed_grid(), synth.encode_mesh_sequential(pos, faces, nrm, uv),
                               synth.encode_mesh(pos, faces, nrm, uv, opt=synth.options(traversal_method=1)),
                               synth.encode_mesh(pos, faces, nrm, uv, opt=synth.options(pos_prediction=2))]


def test_every_kind_of_map_in_both_formats_beside_a_compact_download(ctx, mixed):
    """Per-vertex maps, the general path, a second chance (block 1), level 9 with a uint8 x 4 colour, a garbage stream, a point
    cloud and a seamed grid: vertex arrays and a compact download of one batch, one wait."""
    b = dsa.Batch(ctx, mixed)
    b.decode(wait=False)
    b.download(wait=False, compact=True)
    b.vertex_arrays("values", wait=False)
    b.wait()
    paths = {b.mesh_info(i).decode_path for i in range(b.n) if b.status(i) == 0}
    assert paths >= {0, 1, 2}, paths
    assert any(b.status(i) != 0 for i in range(b.n))
    check_batch(b, mixed, "values")
    check_views(b, mixed, compact=True)          # the download's arrays are untouched by the gather
    b.vertex_arrays("quantized")                 # the first request is complete: another one may follow
    check_batch(b, mixed, "quantized")
    check_views(b, mixed, compact=True)
    lay = native.MeshVertexArrays()
    retried = [i for i in range(b.n) if b.status(i) == 0 and b.mesh_info(i).decode_path == 2]
    assert native.lib().dsa_batch_vertex_arrays_layout(b._h, retried[0], C.byref(lay)) == 0 and lay.block == 1
    b.close()


def test_quantised_rows_against_the_input_alone(ctx):
    """Oracle-free: the faces over the concatenated quantised rows are the quantised input mesh, and the dequantisation parameters
    are the ones the input determines."""
    inputs = [synth.make_mesh(synth.GRID, 40, 33, 21), synth.make_mesh(synth.TORUS, 24, 20, 22)]
    b = dsa.Batch(ctx, [synth.encode_mesh(pos, faces, nrm, uv) for pos, nrm, uv, faces in inputs])
    b.decode(wait=False)
    b.vertex_arrays("quantized")
    for i, (pos, nrm, uv, faces) in enumerate(inputs):
        v = b.vertex_views(i)
        by_type = {a["info"].attribute_type: a for a in v["attributes"]}
        keys = np.concatenate([by_type[t]["values"].astype(np.int64) for t in (0, 1, 3)], axis=1)
        assert keys.shape[1] == 3 + 2 + 2
        want, (pmin, prange, umin, urange) = meshutil.source_corner_faces(pos, nrm, uv, faces)
        got = meshutil.face_multiset_fast(v["indices"], keys)
        assert got.shape == want.shape and np.array_equal(got, want)
        qmin, qrange, bits = by_type[0]["quantization"]
        assert bits == 11 and np.array_equal(np.float32(qmin), pmin) and np.float32(qrange) == prange
        qmin, qrange, bits = by_type[3]["quantization"]
        assert bits == 10 and np.array_equal(np.float32(qmin), umin) and np.float32(qrange) == urange
        assert by_type[1]["quantization"][2] == 8
    b.close()


ROW_SHAPES = ((np.uint8, 1, "random"), (np.uint8, 3, "random"), (np.int16, 3, "random"), (np.uint32, 4, "sentinel"))


def test_row_shapes_of_integer_attributes(ctx):
    """uint8 x 1 / x 3 and int16 x 3 (byte-granular rows), uint32 x 4 (dword rows): the rows are the INPUT values bit for bit -- as
    the oracle's map orders them, and as a multiset of face corners from the input alone -- and the quantized format leaves them be."""
    shuffled = [n for n in typedcases.mesh_names() if n.startswith("shuffled-")][0]
    cases, streams = [], []
    for pos, nrm, uv, faces in (synth.make_mesh(synth.GRID, 6, 5, 1), typedcases.mesh(shuffled)):
        for k, (dtype, nc, pattern) in enumerate(ROW_SHAPES):
            gen = typedcases.values(dtype, pattern, len(pos), nc, seed=40 + k)
            cases.append((pos, faces, gen))
            streams.append(synth.encode_mesh(pos, faces, nrm, uv, generic=gen, opt=synth.options(generic_components=nc)))
    b = dsa.Batch(ctx, streams)
    b.decode(wait=False)
    b.vertex_arrays("values")
    check_batch(b, streams, "values")
    rows = [np.array(b.vertex_views(i)["attributes"][-1]["values"]) for i in range(b.n)]
    b.vertex_arrays("quantized")
    check_batch(b, streams, "quantized")
    for i, (pos, faces, gen) in enumerate(cases):
        v = b.vertex_views(i)
        g = v["attributes"][-1]
        assert g["values"].dtype == gen.dtype and g["values"].shape[1] == gen.shape[1] and g["quantization"] is None
        assert np.ascontiguousarray(g["values"]).tobytes() == rows[i].tobytes()
        assert v["attributes"][0]["info"].attribute_type == 0
        got = typedcases.decoded_multiset(v["indices"], v["attributes"][0]["values"], None, g["values"], None)
        assert typedcases.same_multiset(got, typedcases.pin(pos, faces, gen))
    b.close()


def test_index_width_follows_the_point_count(ctx):
    """A grid just under 65 536 points: uint16 indices; one just over: uint32.  All in one batch, so one block holds both widths.
    The width is fixed from the stream header before the decode (encoded vertices + split symbols bound the point count: the rule
    of the compact download), so the grid of exactly 65 536 points, whose header allows 65 791, has uint32 indices too."""
    streams = []
    for nx, ny in ((254, 255), (255, 256), (255, 255)):
        pos, nrm, uv, faces = synth.make_mesh(synth.GRID, nx, ny, 2)
        streams.append(synth.encode_mesh(pos, faces))
    assert [reference(s).num_points for s in streams] == [65280, 65792, 65536]
    b = dsa.Batch(ctx, streams)
    b.decode(wait=False)
    b.vertex_arrays("quantized")
    assert [b.vertex_views(i)["indices"].dtype for i in range(3)] == [np.uint16, np.uint32, np.uint32]
    check_batch(b, streams, "quantized")
    b.close()


def test_more_than_16_bits_are_absent_from_the_quantized_format(ctx):
    inputs = [synth.make_mesh(synth.GRID, 9, 7, 3), synth.make_mesh(synth.TORUS, 8, 6, 4), synth.make_mesh(synth.HOLES, 12, 9, 5)]
    streams = [synth.encode_mesh(pos, faces, nrm, uv, opt=synth.options(pos_bits=18) if k == 1 else None) for k, (pos, nrm, uv, faces) in enumerate(inputs)]
    assert reference(streams[1]).attributes[0].q_bits == 18
    b = dsa.Batch(ctx, streams)
    b.decode(wait=False)
    b.vertex_arrays("quantized")
    v = b.vertex_views(1)
    assert v["attributes"][0]["values"] is None and all(a["values"] is not None for a in v["attributes"][1:])
    lay = native.MeshVertexArrays()
    assert native.lib().dsa_batch_vertex_arrays_layout(b._h, 1, C.byref(lay)) == 0
    assert lay.attributes[0].flags & native.DSA_VA_ABSENT and lay.attributes[0].offset == native.VA_NONE
    check_batch(b, streams, "quantized")          # the other attributes of that mesh and its neighbours are intact
    b.vertex_arrays("values")
    assert all(a["values"] is not None for a in b.vertex_views(1)["attributes"])
    check_batch(b, streams, "values")
    b.close()


def test_the_attribute_mask_leaves_out_and_reserves_nothing(ctx):
    inputs = [synth.make_mesh(synth.GRID, 9, 7, 3), synth.make_mesh(synth.TORUS, 8, 6, 4)]
    streams = [synth.encode_mesh(pos, faces, nrm, uv) for pos, nrm, uv, faces in inputs]
    b = dsa.Batch(ctx, streams)
    b.decode(wait=False)
    normals_rows = sum(12 * reference(s).num_points for s in streams)
    assert b.vertex_arrays_bytes("values", attribute_types=[0, 3]) <= b.vertex_arrays_bytes("values") - normals_rows
    b.vertex_arrays("values", attribute_types=[0, 3])
    for i, s in enumerate(streams):
        ref = reference(s)
        normals = [a for a, att in enumerate(ref.attributes) if att.att_type == 1]
        assert len(normals) == 1
        check_mesh(b.vertex_views(i), ref, "values", absent=normals)
    b.close()


def test_bytes_of_the_three_host_forms(ctx):
    """Per-vertex meshes: no maps on the link, and 16 against 32 bytes per point -- arithmetic of the layout, known before the decode."""
    pos, nrm, uv, faces = synth.make_mesh(synth.GRID, 128, 256, 1)
    s = synth.encode_mesh(pos, faces, nrm, uv)
    b = dsa.Batch(ctx, [s] * 8)
    values, quantized = b.vertex_arrays_bytes("values"), b.vertex_arrays_bytes("quantized")
    assert 0 < quantized < values < b.compact_bytes < b.output_bytes
    assert values >= 8 * (6 * len(faces) + 32 * len(pos)) and quantized >= 8 * (6 * len(faces) + 16 * len(pos))
    b.close()


def test_vertex_arrays_into_caller_memory(ctx):
    L = native.lib()
    pos, nrm, uv, faces = synth.make_mesh(synth.GRID, 64, 48, 2)
    s = synth.encode_mesh(pos, faces, nrm, uv)
    b = dsa.Batch(ctx, [s, s])
    b.decode(wait=False)
    nbytes = b.vertex_arrays_bytes("values")
    canary = 64
    p = L.dsa_host_alloc(nbytes + canary)
    assert p
    try:
        C.memset(p + nbytes, 0xA5, canary)
        req = native.VertexRequest(native.DSA_VA_VALUES, 0, 0)
        assert L.dsa_batch_vertex_arrays(b._h, C.byref(req), p, nbytes - 1) == native.DSA_ERR_INVALID_ARGUMENT     # too small a destination is refused
        assert L.dsa_batch_vertex_arrays(b._h, C.byref(req), p, nbytes) == 0
        b.wait()
        assert bytes((C.c_uint8 * canary).from_address(p + nbytes)) == b"\xA5" * canary
        assert L.dsa_batch_host_vertex_arrays(b._h, 0) == p
        check_batch(b, [s, s], "values")
        bad = native.VertexRequest(native.DSA_VA_VALUES, 0, 0)
        bad.reserved[2] = 1
        assert L.dsa_batch_vertex_arrays(b._h, C.byref(bad), None, 0) == native.DSA_ERR_INVALID_ARGUMENT and "reserved" in ctx.error()
        bad = native.VertexRequest(7, 0, 0)
        assert L.dsa_batch_vertex_arrays(b._h, C.byref(bad), None, 0) == native.DSA_ERR_INVALID_ARGUMENT and "format" in ctx.error()
    finally:
        b.close()
        L.dsa_host_free(p)


def test_three_batches_in_flight_with_download_and_vertex_arrays(ctx):
    """upload(k+1) beside decode(k) beside download(k-1), every batch with a download AND vertex arrays queued before its one wait."""
    sets = [streams_mixed(11 + 7 * k) for k in range(4)]
    live = []

    def finish(b0, s0):
        b0.wait()
        check_batch(b0, s0, "values")
        check_views(b0, s0)
        b0.close()

    for k, streams in enumerate(sets):
        b = dsa.Batch(ctx, streams)
        b.decode(wait=False)
        b.download(wait=False)
        b.vertex_arrays("values", wait=False)
        if k == 0:
            with pytest.raises(ValueError):          # a second request while the first is in flight is refused
                b.vertex_arrays("quantized", wait=False)
        live.append((b, streams))
        if len(live) == 3:
            finish(*live.pop(0))
    b, streams = live.pop()
    for b0, s0 in live:
        finish(b0, s0)
    # decode again, then the other format on the same batch
    b.wait()
    check_batch(b, streams, "values")
    b.decode(wait=False)
    assert not native.lib().dsa_batch_host_vertex_arrays(b._h, 0)        # the new decode invalidated them
    b.vertex_arrays("quantized", wait=False)
    b.wait()
    check_batch(b, streams, "quantized")
    b.close()


def test_crowded_batch_of_small_meshes(ctx):
    """300 small meshes of every kind in mixed order: a block per mesh and chunk, most of them partly filled."""
    pos, nrm, uv, faces = synth.make_mesh(synth.GRID, 6, 5, 1)
    hp, hn, hu, hf = synth.make_mesh(synth.HOLES, 14, 12, 2)
    rng = np.random.default_rng(5)
    distinct = [synth.encode_mesh(pos, faces, nrm, uv),
                synth.encode_mesh_corners(*meshutil.seamed_mesh(synth, synth.HOLES, 12, 9, 4, "checker", "stripes")),
                synth.encode_point_cloud(rng.random((1, 3), np.float32)),
                synth.encode_point_cloud(rng.random((500, 3), np.float32)),
                synth.encode_mesh(hp, hf, hn, hu, opt=synth.options(normal_prediction=6)),
                synth.encode_mesh(hp, hf, hn, hu, opt=synth.options(pos_prediction=2)),                       # second chance
                synth.encode_mesh(hp, hf, hn, hu, opt=synth.options(traversal_method=1)),                     # general path
                synth.encode_mesh(pos, faces, nrm, uv, opt=synth.options(pos_bits=18))]
    for k, (dtype, nc, pattern) in enumerate(ROW_SHAPES):
        gen = typedcases.values(dtype, pattern, len(pos), nc, seed=60 + k)
        distinct.append(synth.encode_mesh(pos, faces, nrm, uv, generic=gen, opt=synth.options(generic_components=nc)))
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "house_04.obj.drc"), "rb") as f:
        distinct.append(f.read())
    streams = [distinct[k] for k in rng.integers(0, len(distinct), 300)]
    b = dsa.Batch(ctx, streams)
    b.decode(wait=False)
    b.vertex_arrays("quantized", wait=False)
    b.wait()
    check_batch(b, streams, "quantized")
    b.vertex_arrays("values")
    check_batch(b, streams, "values")
    b.close()


def test_device_views_without_a_transfer(ctx, mixed):
    b = dsa.Batch(ctx, mixed)
    b.decode(wait=False)
    b.vertex_arrays("values", wait=False, device_only=True)
    b.wait()
    assert not native.lib().dsa_batch_host_vertex_arrays(b._h, 0) and not native.lib().dsa_batch_host_vertex_arrays(b._h, 1)
    assert native.lib().dsa_batch_device_vertex_arrays(b._h, 0)
    with pytest.raises(RuntimeError):
        b.vertex_views(0)
    check_batch(b, mixed, "values", device=True)
    b.vertex_arrays("quantized", device_only=True)
    check_batch(b, mixed, "quantized", device=True)
    b.close()


def dequantise(rows, info, quantization):
    """The header's formulas (dsa_batch_vertex_arrays in include/draco_mi355x.h) in numpy, float32 with separate roundings."""
    qmin, qrange, bits = quantization
    q = rows.astype(np.float32)
    if info.decoder_type == 2:
        delta = np.float32(qrange) / np.float32((1 << bits) - 1)
        return (q * delta).astype(np.float32) + np.float32(qmin)[None, :]
    k = np.float32(2.0) / np.float32((1 << bits) - 2)
    y = (q[:, 0] * k).astype(np.float32) - np.float32(1)
    z = (q[:, 1] * k).astype(np.float32) - np.float32(1)
    x = (np.float32(1) - np.abs(y)).astype(np.float32) - np.abs(z)
    o = np.maximum(-x, np.float32(0))
    y = y + np.where(y < 0, o, -o)
    z = z + np.where(z < 0, o, -o)
    n = ((x * x).astype(np.float32) + (y * y).astype(np.float32)).astype(np.float32) + (z * z).astype(np.float32)
    d = 1.0 / np.sqrt(n.astype(np.float64))
    out = np.stack([x.astype(np.float64) * d, y.astype(np.float64) * d, z.astype(np.float64) * d], axis=1).astype(np.float32)
    out[n.astype(np.float64) < 1e-6] = 0
    return out


def test_gltf_quantized_arrays_dequantise_to_the_float_arrays(ctx, tmp_path):
    """load(quantized=True): the integer arrays, dequantised in float32 by the formulas the header states, are load()'s float
    arrays bit for bit -- positions, texture coordinates AND octahedral normals (the normals' formula has one double step, the
    reciprocal square root, which numpy reproduces)."""
    from draco_sharp_amd import gltf
    from test_gltf import _assets
    _, sources = _assets(tmp_path)
    loader = gltf.GltfDracoLoader(ctx)
    floats, ints = loader.load(sources[:2]), loader.load(sources[:2], quantized=True)
    seen = set()
    for fa, ia in zip(floats, ints):
        assert len(fa) == len(ia) == 3
        for fp, ip in zip(fa, ia):
            assert np.array_equal(fp.indices, ip.indices) and not fp.quantization
            infos = {a.UniqueId: a for a in ip.draco.Attributes}
            for semantic, uid in ip.source.attribute_ids.items():
                rows, want = ip.attributes[semantic], fp.attributes[semantic]
                assert rows.dtype == np.uint16 and want.dtype == np.float32
                a = infos[uid]
                info = type("Info", (), {"decoder_type": a.DecoderType})
                got = dequantise(rows, info, ip.quantization[semantic])
                assert got.shape == want.shape and got.tobytes() == want.tobytes(), semantic
                seen.add(semantic)
    assert seen == {"POSITION", "NORMAL", "TEXCOORD_0"}
