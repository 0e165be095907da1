"""The glTF writer on the asset from the wild: a primitive with a UV seam, a doubled face and a sliver with a repeated index.
Today's configs leave it uncompressed (`skipped`: the strict coder refuses the topology, the repair alone refuses the seams);
with Config(repair_topology=True, repair_seams=True) it is written with KHR_draco_mesh_compression and loads back to the pin.
The CPU coder's side needs no device."""
import numpy as np
import pytest

import defects
import draco_sharp_amd as dsa
import draco_sharp_amd.synth as synth
import meshutil
import oracle
from draco_sharp_amd import gltf
from test_gltf_writer import Builder, seamed


def wild_primitive():
    """One row per point (pos, faces, normals, uvs): a grid cut by UV stripes, face 7 listed twice, a sliver (a, b, a) on an edge."""
    p, f, n, u = seamed(synth.GRID, 8, 6, 3)
    f = np.concatenate([f[:20], [[f[4, 0], f[4, 1], f[4, 0]]], f[20:], f[7:8]]).astype(np.uint32)
    return p, f, n, u


def pin(p, f, n, u):
    keep = ~defects.is_degenerate(f)
    assert keep.sum() == len(f) - 1
    return meshutil.source_corner_faces(p, n, u, f[keep])[0]


def asset():
    p, f, n, u = wild_primitive()
    b = Builder()
    b.primitive({"POSITION": b.accessor(p), "NORMAL": b.accessor(n), "TEXCOORD_0": b.accessor(u)}, b.accessor(f.reshape(-1)))
    gp, gn, gu, gf = synth.make_mesh(synth.GRID, 5, 4, 2)              # a clean neighbour: compressed under every config
    b.primitive({"POSITION": b.accessor(gp), "NORMAL": b.accessor(gn)}, b.accessor(gf.reshape(-1)))
    return b.glb(), (p, f, n, u)


def test_the_cpu_coder_on_the_planned_primitive():
    glb, (p, f, n, u) = asset()
    planned, skipped = gltf.plan_compression([gltf.read_asset(glb)])
    assert [(x.mesh, x.primitive) for x in planned] == [(0, 0), (1, 0)] and not skipped
    d = planned[0].data
    assert d.normal_corners is None and d.texcoord_corners is None and np.array_equal(d.faces, f)
    with pytest.raises(RuntimeError, match="degenerate face in input mesh"):
        synth.encode_mesh_points(d.positions, d.faces, d.normals, d.texcoords)
    with pytest.raises(RuntimeError, match="not implemented"):
        synth.encode_mesh_points(d.positions, d.faces, d.normals, d.texcoords, opt=synth.options(repair_topology=1))
    m = oracle.decode(synth.encode_mesh_points(d.positions, d.faces, d.normals, d.texcoords, opt=synth.options(repair_topology=2)))
    assert any(x["element_type"] == 1 for x in m.decoders)               # (the UV seam is a seam of the stream)
    want = pin(p, f, n, u)
    got = defects.decoded(m.faces, [(a.portable, a.point_map) for a in m.attributes])
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.gpu
def test_the_primitive_is_compressed_instead_of_skipped():
    glb, (p, f, n, u) = asset()
    ctx = dsa.Context(0)
    try:
        w = gltf.GltfDracoWriter(ctx)
        for cfg, word in ((None, "degenerate face"), (dsa.Config(repair_topology=True), "not implemented")):
            (r,) = w.compress([glb], cfg)
            assert [(m, k) for m, k, _, _ in r.compressed] == [(1, 0)]
            (s,) = r.skipped
            assert (s.mesh, s.primitive) == (0, 0) and "the encoder refused it" in s.reason and word in s.reason, s.reason
        (r,) = w.compress([glb], dsa.Config(repair_topology=True, repair_seams=True))
        assert [(m, k) for m, k, _, _ in r.compressed] == [(0, 0), (1, 0)] and not r.skipped
        out = gltf.read_asset(r.glb)
        assert out.doc["extensionsRequired"] == [gltf.EXTENSION]
        prim = out.doc["meshes"][0]["primitives"][0]
        assert gltf.EXTENSION in prim["extensions"] and out.doc["accessors"][prim["indices"]]["count"] == 3 * (len(f) - 1)
        stream = r.compressed[0][2]
        planned, _ = gltf.plan_compression([gltf.read_asset(glb)])
        d = planned[0].data
        assert stream == synth.encode_mesh_points(d.positions, d.faces, d.normals, d.texcoords, opt=synth.options(repair_topology=2))
        (loaded,) = gltf.GltfDracoLoader(ctx).load([r.glb], quantized=True)
        got = loaded[0]
        keys = np.concatenate([np.asarray(got.attributes[s], np.int64).reshape(len(got.attributes["POSITION"]), -1) for s in ("POSITION", "NORMAL", "TEXCOORD_0")], axis=1)
        want = pin(p, f, n, u)
        have = meshutil.face_multiset_fast(got.indices.reshape(-1, 3), keys)
        assert have.shape == want.shape and (have == want).all()
    finally:
        ctx.close()
