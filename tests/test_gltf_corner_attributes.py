"""The glTF writer with the attributes of the list welded each alone (Config(weld_points=True, weld_attributes=True)): an asset of
two primitives whose TEXCOORD_1 is a lightmap set with a chart layout of its own and whose COLOR_0 has a hard edge.  Without a
device: the plan, the switch, and what the CPU coder makes of the planned meshes; on the GPU: compress with and without the
switch, loaded back with GltfDracoLoader against the pin of tests/cornerattrcases.py."""
import numpy as np
import pytest

import cornerattrcases as K
import meshutil
import oracle
import seamdefects as sd
import draco_sharp_amd as dsa
import draco_sharp_amd.synth as synth
from draco_sharp_amd import gltf
from test_gltf_writer import Builder

SPECS = [K.Case("gltf/grid", lambda: synth.make_mesh(synth.GRID, 14, 11, 3), (None, "stripes"), [("uv1", "checker"), ("colour", "island")]),
         K.Case("gltf/torus", lambda: synth.make_mesh(synth.TORUS, 12, 10, 4), (None, "checker"), [("uv1", "island")])]


def lightmap_asset():
    """(glb, [(Built, (pos, faces, normals, uvs, [listed arrays]) per point)]): one mesh of two primitives"""
    b = Builder()
    sources = []
    mesh = None
    for k, case in enumerate(SPECS):
        built = K.build(case)
        pos, faces, nrm, uv, arrays = K.unweld(built, np.random.default_rng(8 + k))
        atts = {"POSITION": b.accessor(pos), "NORMAL": b.accessor(nrm), "TEXCOORD_0": b.accessor(uv), "TEXCOORD_1": b.accessor(arrays[0])}
        if len(arrays) > 1:
            atts["COLOR_0"] = b.accessor(arrays[1], normalized=True)
        mesh = b.primitive(atts, b.accessor(faces.reshape(-1)), mesh=mesh)
        sources.append((built, (pos, faces, nrm, uv, arrays)))
    return b.glb(), sources


def distinct_positions(pos, faces):
    used = np.unique(np.asarray(faces, np.int64))
    return len(np.unique(np.ascontiguousarray(pos, np.float32)[used].view(np.uint32).reshape(len(used), -1), axis=0))


def test_the_plan_and_the_cpu_coder_on_it():
    glb, sources = lightmap_asset()
    planned, skipped = gltf.plan_compression([gltf.read_asset(glb)])
    assert [(p.mesh, p.primitive) for p in planned] == [(0, 0), (0, 1)] and not skipped
    assert planned[0].attribute_ids == {"POSITION": 0, "NORMAL": 1, "TEXCOORD_0": 2, "TEXCOORD_1": 3, "COLOR_0": 4}
    assert planned[1].attribute_ids == {"POSITION": 0, "NORMAL": 1, "TEXCOORD_0": 2, "TEXCOORD_1": 3}
    for p, (built, (pos, faces, nrm, uv, arrays)) in zip(planned, sources):
        d = p.data
        assert [(a.attribute_type, a.values.dtype, a.values.shape[1], a.normalized) for a in d.attributes] == \
            [(3, np.float32, 2, False), (2, np.uint8, 4, True)][:len(arrays)]
        assert all(a.corners is None and a.values.tobytes() == x.tobytes() for a, x in zip(d.attributes, arrays))      # one row per point, no ids
        extra = [synth.Extra(a.values, a.attribute_type, a.normalized) for a in d.attributes]
        # the attributes in the vertex key: their charts cut the positions, and the strict coder may refuse what is left
        key = synth.weld_points(d.positions, d.faces, d.normals, d.texcoords, extra=extra)
        alone = synth.weld_points(d.positions, d.faces, d.normals, d.texcoords, extra=extra, weld_attributes=True)
        assert alone.num_vertices == distinct_positions(pos, faces) == distinct_positions(built.pos, built.faces) < key.num_vertices
        assert alone.extra_corners[0] is not None
        s = synth.encode_mesh_points(d.positions, d.faces, d.normals, d.texcoords, extra=extra, weld_attributes=True)
        assert sd.header_counts(s)[0] == alone.num_vertices
        ref = oracle.decode(s)
        assert K.same(K.oracle_multiset(ref), K.pin(built))
        assert [x["element_type"] for x in ref.decoders][3] == 1                       # TEXCOORD_1: a corner attribute of its own
        cut = synth.encode_mesh_points(d.positions, d.faces, d.normals, d.texcoords, extra=extra, opt=synth.options(repair_topology=2))
        assert sd.header_counts(cut)[0] >= key.num_vertices > alone.num_vertices


def test_the_switch_needs_weld_points():
    with pytest.raises(ValueError, match="weld_attributes welds the listed attributes of per-point input each alone: it needs weld_points=True"):
        dsa.Config(weld_attributes=True)
    cfg = dsa.Config(weld_points=True, weld_attributes=True)
    assert cfg.weld_points and cfg.weld_attributes and not dsa.Config(weld_points=True).weld_attributes
    cfg.weld_points = False                                   # (set behind the constructor: EncodeBatch asks again)
    with pytest.raises(ValueError, match="it needs weld_points=True"):
        dsa.DracoEncoder(object()).EncodeBatch([], cfg)


@pytest.mark.gpu
def test_compress_with_and_without_weld_attributes():
    glb, sources = lightmap_asset()
    ctx = dsa.Context(0)
    try:
        writer = gltf.GltfDracoWriter(ctx)
        # without: today's bytes -- what EncodeBatch gives for the planned meshes under weld_points
        planned, _ = gltf.plan_compression([gltf.read_asset(glb)])
        (plain,) = writer.compress([glb], dsa.Config(repair_topology=True, repair_seams=True))
        today = dsa.DracoEncoder(ctx).TryEncodeBatch([p.data for p in planned], dsa.Config(weld_points=True, repair_topology=True, repair_seams=True))
        assert [(m, p) for m, p, _, _ in plain.compressed] == [(0, 0), (0, 1)] and [s for _, _, s, _ in plain.compressed] == today
        (default,) = writer.compress([glb])
        strict = dsa.DracoEncoder(ctx).TryEncodeBatch([p.data for p in planned], dsa.Config(weld_points=True))
        assert [s for _, _, s, _ in default.compressed] == [s for s in strict if isinstance(s, bytes)]
        # with: the stream's vertices are the distinct positions, and the loader returns the same rows per point
        (welded,) = writer.compress([glb], dsa.Config(weld_points=True, weld_attributes=True))
        assert [(m, p) for m, p, _, _ in welded.compressed] == [(0, 0), (0, 1)] and not welded.skipped
        for (m, p, stream, points), (built, (pos, faces, nrm, uv, arrays)), (_, _, cut, _) in zip(welded.compressed, sources, plain.compressed):
            assert sd.header_counts(stream)[0] == distinct_positions(pos, faces) < sd.header_counts(cut)[0]
            extra = [synth.Extra(a, attribute_type=e.attribute_type, normalized=bool(e.normalized)) for e, a in zip(built.extras, arrays)]
            assert stream == synth.encode_mesh_points(pos, faces, nrm, uv, extra=extra, weld_attributes=True)
        (prims,) = gltf.GltfDracoLoader(ctx).load([welded.glb], quantized=True)
        doc = gltf.read_asset(welded.glb).doc
        for d, (_, _, stream, points), (built, _) in zip(prims, welded.compressed, sources):
            semantics = ["POSITION", "NORMAL", "TEXCOORD_0", "TEXCOORD_1"] + (["COLOR_0"] if len(built.extras) > 1 else [])
            assert d.source.attribute_ids == {s: k for k, s in enumerate(semantics)}
            cols = []
            for s in semantics:
                a = np.asarray(d.attributes[s])
                assert len(a) == points == doc["accessors"][d.source.accessors[s]]["count"]
                if a.dtype.kind == "f":
                    mn, rng, bits = d.quantization[s] if s in d.quantization else (None, None, None)
                    assert mn is not None, s
                    a = meshutil.quantize(a, mn, rng, bits)
                cols.append(a.astype(np.int64).reshape(len(a), -1))
            have = meshutil.face_multiset_fast(d.indices.reshape(-1, 3), np.concatenate(cols, axis=1))
            assert K.same(have, K.pin(built)), built.name
    finally:
        ctx.close()
