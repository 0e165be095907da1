"""Encode direction, the quantisers at the front of every encode call on the designed floats of tests/quantcases.py: k_enc_bounds
and k_enc_quantize (draco-sharp_amd/csrc/dsa_encode.h) and, on the way back, the dequantisation of k_finalize / k_predict_wrap
(dsa_kernels.h).  The device must write the CPU coder's bytes; header floats (as bit patterns) and integers must be the numpy
reference's; the floats the device decoder returns must be dequantised(...) bit for bit; and what the rules refuse -- a value that
is not finite, a range the bit depth cannot carry -- fails alone with the CPU coder's words.  Integers and bit patterns only: no
tolerance, no case set aside."""
import numpy as np
import pytest

import meshutil
import oracle
import quantcases as qc
import draco_sharp_amd as dsa
import draco_sharp_amd.synth as synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = dsa.Context(0)
    yield c
    c.close()


def attributes_of(c):
    return [dsa.Attribute(e, quantization_bits=c.extra_bits) for e in c.extras] or None


def cloud_of(c):
    return dsa.PointCloudData(c.pos, normals=c.normals, texcoords=c.uvs, attributes=attributes_of(c))


def mesh_of(c, faces):
    return dsa.MeshData(c.pos, faces, normals=c.normals, texcoords=c.uvs, attributes=attributes_of(c))


def config_of(c, **kw):
    return dsa.Config(position_bits=c.pos_bits, texcoord_bits=c.uv_bits, normal_bits=c.normal_bits, **kw)


def opt_of(c):
    return synth.options(pos_bits=c.pos_bits, uv_bits=c.uv_bits, normal_bits=c.normal_bits)


def extras_of(c):
    return [synth.Extra(e, quantization_bits=c.extra_bits) for e in c.extras] or None


def cpu_cloud(c):
    return synth.encode_point_cloud_attributes(c.pos, c.normals, c.uvs, None, opt_of(c), extras_of(c))


def cpu_mesh(c, faces):
    return synth.encode_mesh(c.pos, faces, c.normals, c.uvs, None, opt_of(c), extras_of(c))


def check_device_decode(ctx, cases, streams):
    """dsa.Batch on the device: integers and header as the reference has them, the floats dequantised(...) bit for bit, the normals
    the oracle's"""
    b = dsa.Batch(ctx, list(streams))
    b.decode()
    for i, (c, s) in enumerate(zip(cases, streams)):
        assert b.status(i) == 0, (c.name, b.mesh_info(i).detail)
        d = b.result(i).ConnectedData
        ref = oracle.decode(s)
        assert d.PointsCount == len(c.pos) and len(d.Attributes) == len(ref.attributes)
        slots = qc.quantised_slots(c)
        k = 0
        for a, r in zip(d.Attributes, ref.attributes):
            assert np.array_equal(np.asarray(a.PointMap, np.int64), np.arange(len(c.pos)))
            if a.AttributeType == 1:
                assert np.array_equal(np.asarray(a.PortableValues, np.int64), meshutil.oct_quantize(c.normals, c.normal_bits)), (c.name, "normals")
                assert np.ascontiguousarray(a.Values).tobytes() == r.values.tobytes(), (c.name, "normals", "values")
                continue
            slot, v, bits = slots[k]
            k += 1
            qmin, qrange = qc.own_bounds(v)
            want = qc.quantised(v, bits)
            assert a.QuantizationBits == bits
            assert qc.bits_of(np.float32(a.MinValues)).tolist() == qc.bits_of(qmin).tolist() and qc.bits_of(np.float32(a.Range)).item() == qc.bits_of(qrange).item(), (c.name, slot)
            assert np.array_equal(np.asarray(a.PortableValues, np.int64).reshape(want.shape), want), (c.name, slot, "integers")
            got = np.ascontiguousarray(a.Values, np.float32).reshape(want.shape)
            back = qc.dequantised(want, qmin, qrange, bits)
            differ = np.flatnonzero((qc.bits_of(got) != qc.bits_of(back)).any(axis=1))
            assert len(differ) == 0, (c.name, slot, "values", len(differ), differ[:4].tolist(), got[differ[:2]].tolist(), back[differ[:2]].tolist())
        assert k == len(slots)
    b.close()


@pytest.mark.parametrize("family", list(qc.families()))
def test_sequential_clouds_match_the_cpu_coder_and_the_reference(ctx, family):
    """every coded case as a point cloud (entry = row), a family at a time, one call per set of bit depths"""
    for _, cases in qc.grouped_by_bits(qc.families()[family]):
        got = list(dsa.DracoEncoder(ctx).EncodeBatch([cloud_of(c) for c in cases], config_of(cases[0], encoding_method=0)))
        for c, g in zip(cases, got):
            qc.check_stream(c, g, True)                              # header bits, integers, the oracle's values
            assert g == cpu_cloud(c), (c.name, "bytes differ from the CPU coder's")
        check_device_decode(ctx, cases, got)


@pytest.mark.parametrize("family", ["zeros", "ties", "subnormal"])
def test_edgebreaker_meshes_match_the_cpu_coder_and_the_reference(ctx, family):
    """encode_chunk launches the quantisers on its own path: the case's rows on the vertices of a GRID mesh"""
    for _, cases in qc.grouped_by_bits(qc.families()[family]):
        meshed = [qc.as_mesh(c) for c in cases]
        got = list(dsa.DracoEncoder(ctx).EncodeBatch([mesh_of(c, f) for c, f in meshed], config_of(cases[0])))
        for (c, f), g in zip(meshed, got):
            qc.check_stream(c, g, False)
            assert g == cpu_mesh(c, f), (c.name, "bytes differ from the CPU coder's")


def good_clouds(like):
    """two clouds with the attributes of case `like`, for either side of it"""
    out = []
    for seed in (81, 82):
        rng = np.random.default_rng(seed)
        n = 300 + seed
        out.append(qc.case("good-%d" % seed, "good", rng.random((n, 3)), like.pos_bits, None if like.uvs is None else rng.random((n, 2)), like.uv_bits,
                           extras=[rng.random((n, e.shape[1])) for e in like.extras], extra_bits=like.extra_bits))
    return out


def refusal_of(g):
    """the text of a per-mesh failure without the slot the accessor names in front of it ("mesh 1: ...")"""
    assert isinstance(g, ValueError), g                              # DSA_ERR_INVALID_ARGUMENT
    return str(g).split(": ", 1)[1]


@pytest.mark.parametrize("name", [c.name for c in qc.refused()])
def test_refused_clouds_fail_alone_with_the_cpu_coders_words(ctx, name):
    bad = {c.name: c for c in qc.refused()}[name]
    a, b = good_clouds(bad)
    with pytest.raises(RuntimeError) as e:
        cpu_cloud(bad)
    assert str(e.value) == bad.refusal
    cfg = config_of(bad, encoding_method=0)
    got = dsa.DracoEncoder(ctx).TryEncodeBatch([cloud_of(a), cloud_of(bad), cloud_of(b)], cfg)
    assert refusal_of(got[1]) == bad.refusal
    assert got[0] == cpu_cloud(a) and got[2] == cpu_cloud(b)
    assert list(dsa.DracoEncoder(ctx).EncodeBatch([cloud_of(a), cloud_of(b)], cfg)) == [got[0], got[2]]


def test_refused_meshes_fail_alone_with_the_cpu_coders_words(ctx):
    by = {c.name: c for c in qc.refused()}
    meshes, want = [], []
    for name in ("refused-nan-row-417", "refused-range-too-small", "refused-nan-in-an-extra", "refused-range-infinite"):
        bad = by[name]
        for c in (good_clouds(bad)[0], bad):
            faces = synth.make_mesh(synth.GRID, len(c.pos) // 2 - 1, 1, 1)[3]
            c = c._replace(pos=c.pos[:int(faces.max()) + 1], uvs=None, extras=tuple(e[:int(faces.max()) + 1] for e in c.extras))
            assert len(c.pos) == int(faces.max()) + 1
            meshes.append(mesh_of(c, faces))
            try:
                want.append(cpu_mesh(c, faces))
            except RuntimeError as e:
                want.append(str(e))
    assert [w for w in want if isinstance(w, str)] == [by[n].refusal for n in ("refused-nan-row-417", "refused-range-too-small", "refused-nan-in-an-extra", "refused-range-infinite")]
    got = dsa.DracoEncoder(ctx).TryEncodeBatch(meshes, dsa.Config())
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g == w) if isinstance(w, bytes) else (refusal_of(g) == w), (i, g if isinstance(g, Exception) else "coded", w if isinstance(w, str) else "coded")


def split_config(c, **kw):
    return config_of(c, encoding_method=0, point_order=dsa.POINT_ORDER_MORTON, **kw)


def test_ordered_clouds_keep_the_header_and_the_refusal(ctx):
    """point_order = MORTON: the zeros and a refused cloud between them"""
    zeros = qc.families()["zeros"]
    bad = qc.refused()[0]._replace(uvs=zeros[0].uvs[:1].repeat(len(qc.refused()[0].pos), axis=0),
                                   extras=tuple(e[:1].repeat(len(qc.refused()[0].pos), axis=0) for e in zeros[0].extras), extra_bits=zeros[0].extra_bits)
    cases = zeros[:2] + [bad] + zeros[2:]
    got = dsa.DracoEncoder(ctx).TryEncodeBatch([cloud_of(c) for c in cases], split_config(zeros[0]))
    for c, g in zip(cases, got):
        if c.refusal:
            assert refusal_of(g) == c.refusal == "positions: row 417 is not finite"
            continue
        # The bounds are those of the caller's rows in the caller's order, as in every split or merged call: the stream is the
        # permuted input's on the explicit grid of those bounds (synth.encode_ordered codes the permuted input afresh, and would
        # give a zero minimum the sign of the first zero in Morton order).
        perm = synth.point_order(c.pos, c.pos_bits)
        grid = lambda v: synth.grid(*qc.own_bounds(v))          # noqa: E731
        extra = [synth.Extra(e[perm], quantization_bits=c.extra_bits, grid=grid(e)) for e in c.extras]
        stream = synth.encode_grid(c.pos[perm], None, None, c.uvs[perm], None, extra, opt_of(c), form=0, geometry=0, pos_grid=grid(c.pos), uv_grid=grid(c.uvs))
        assert g == stream, c.name
        for a, (slot, v, bits) in zip(oracle.decode(g).attributes, qc.quantised_slots(c)):
            qmin, qrange = qc.own_bounds(v)
            assert qc.bits_of(np.float32(a.q_min[:v.shape[1]])).tolist() == qc.bits_of(qmin).tolist() and qc.bits_of(np.float32(a.q_range)).item() == qc.bits_of(qrange).item(), (c.name, slot)
            assert np.array_equal(a.portable, qc.quantised(v, bits)[perm]), (c.name, slot)


def test_split_clouds_give_every_part_the_clouds_header_and_a_refused_cloud_one_slot(ctx):
    """part_points = 256: the zeros with 258 and 259 rows fall into two parts each, whose headers are the cloud's; a refused cloud
    fails alone in its one slot, and its neighbours' parts are what they are without it"""
    zeros = qc.families()["zeros"]
    bad = qc.refused()[0]._replace(uvs=zeros[0].uvs[:1].repeat(len(qc.refused()[0].pos), axis=0),
                                   extras=tuple(e[:1].repeat(len(qc.refused()[0].pos), axis=0) for e in zeros[0].extras), extra_bits=zeros[0].extra_bits)
    cases = zeros[:2] + [bad] + zeros[2:]
    cfg = split_config(zeros[0], part_points=256)
    got = dsa.DracoEncoder(ctx).TryEncodeBatch([cloud_of(c) for c in cases], cfg)
    slot, parts_seen = 0, []
    for c in cases:
        if c.refusal:
            assert refusal_of(got[slot]) == c.refusal
            slot += 1
            continue
        twin = synth.encode_split(c.pos, c.normals, c.uvs, None, extras_of(c), opt_of(c), part_points=256)
        parts_seen.append(len(twin))
        for p, (stream, rows, _, _) in enumerate(twin):
            assert got[slot] == stream, (c.name, p)
            for a, (name, v, bits) in zip(oracle.decode(got[slot]).attributes, qc.quantised_slots(c)):
                qmin, qrange = qc.own_bounds(v)
                assert qc.bits_of(np.float32(a.q_min[:v.shape[1]])).tolist() == qc.bits_of(qmin).tolist(), (c.name, p, name)
                assert qc.bits_of(np.float32(a.q_range)).item() == qc.bits_of(qrange).item(), (c.name, p, name)
                assert np.array_equal(a.portable, qc.quantised(v, bits)[rows]), (c.name, p, name)
            slot += 1
    assert slot == len(got) and parts_seen == [1, 2, 2, 1]
    without = dsa.DracoEncoder(ctx).TryEncodeBatch([cloud_of(c) for c in cases if not c.refusal], cfg)
    assert [g for g in got if isinstance(g, bytes)] == list(without)
