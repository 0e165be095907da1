"""The glTF writer (draco-sharp_amd/gltf.py GltfDracoWriter): the device-free planning function on hand-built documents -- mixed
primitives, other modes, missing indices, integer colours, interleaved views -- and the structure of the rewritten document from
streams of the CPU coder; on the GPU, several assets compressed in one call and loaded back with GltfDracoLoader."""
import json
import struct

import numpy as np
import pytest

import draco_sharp_amd as dsa
import draco_sharp_amd.synth as synth
import irregular
import meshutil
import oracle
import weldcases
from draco_sharp_amd import gltf

TYPES = {1: "SCALAR", 2: "VEC2", 3: "VEC3", 4: "VEC4"}
CODES = {np.dtype(np.int8): 5120, np.dtype(np.uint8): 5121, np.dtype(np.int16): 5122, np.dtype(np.uint16): 5123, np.dtype(np.uint32): 5125, np.dtype(np.float32): 5126}


class Builder:
    """A GLB of uncompressed primitives from arrays."""

    def __init__(self):
        self.blob, self.views, self.accessors, self.meshes = bytearray(), [], [], []

    def accessor(self, array, normalized=False, target=None):
        a = np.ascontiguousarray(array)
        a = a.reshape(len(a), -1)
        while len(self.blob) % 4:
            self.blob.append(0)
        self.views.append({"buffer": 0, "byteOffset": len(self.blob), "byteLength": a.nbytes})
        self.blob += a.tobytes()
        acc = {"bufferView": len(self.views) - 1, "componentType": CODES[a.dtype], "count": len(a), "type": TYPES[a.shape[1]]}
        if normalized:
            acc["normalized"] = True
        if a.dtype == np.float32 and a.shape[1] == 3:
            acc["min"], acc["max"] = a.min(axis=0).tolist(), a.max(axis=0).tolist()
        self.accessors.append(acc)
        return len(self.accessors) - 1

    def interleaved(self, arrays):
        """float32 arrays of one count in one view with a byteStride; the accessor of each."""
        rows = np.concatenate([np.ascontiguousarray(a, np.float32) for a in arrays], axis=1)
        while len(self.blob) % 4:
            self.blob.append(0)
        self.views.append({"buffer": 0, "byteOffset": len(self.blob), "byteLength": rows.nbytes, "byteStride": rows.shape[1] * 4})
        self.blob += rows.tobytes()
        out, off = [], 0
        for a in arrays:
            self.accessors.append({"bufferView": len(self.views) - 1, "byteOffset": off, "componentType": 5126, "count": len(a), "type": TYPES[a.shape[1]]})
            out.append(len(self.accessors) - 1)
            off += 4 * a.shape[1]
        return out

    def primitive(self, attributes, indices=None, mode=None, mesh=None, **more):
        prim = {"attributes": attributes}
        if indices is not None:
            prim["indices"] = indices
        if mode is not None:
            prim["mode"] = mode
        prim.update(more)
        if mesh is None:
            self.meshes.append({"primitives": []})
            mesh = len(self.meshes) - 1
        self.meshes[mesh]["primitives"].append(prim)
        return mesh

    def glb(self):
        doc = {"asset": {"version": "2.0"}, "buffers": [{"byteLength": len(self.blob)}], "bufferViews": self.views, "accessors": self.accessors,
               "meshes": self.meshes, "nodes": [{"mesh": i} for i in range(len(self.meshes))], "scenes": [{"nodes": list(range(len(self.meshes)))}]}
        js = json.dumps(doc).encode()
        js += b" " * (-len(js) % 4)
        binc = bytes(self.blob) + b"\0" * (-len(self.blob) % 4)
        return struct.pack("<III", 0x46546C67, 2, 28 + len(js) + len(binc)) + struct.pack("<II", len(js), 0x4E4F534A) + js + struct.pack("<II", len(binc), 0x004E4942) + binc


def seamed(kind, nx, ny, seed, charts=(None, "stripes")):
    return weldcases.unweld(*irregular.with_seams(*synth.make_mesh(kind, nx, ny, seed), *charts, seed=seed), np.random.default_rng(seed))


def mixed_asset():
    """mesh 0: a seamed sphere with every kind of attribute (indices uint16, positions and normals interleaved) and, sharing its
    position accessor, a LINES primitive; mesh 1: a grid without indices, a grid with a TANGENT, a grid with int16 positions, a
    plain grid (indices uint32)."""
    b = Builder()
    p, f, n, u = seamed(synth.SPHERE, 12, 9, 3)
    colour = np.ascontiguousarray(np.tile(np.array([[200, 100, 50, 255]], np.uint8), (len(p), 1)))
    joints = np.ascontiguousarray(np.tile(np.array([[3, 2, 1, 0]], np.uint16), (len(p), 1)))
    weights = np.ascontiguousarray(np.tile(np.array([[0.5, 0.25, 0.25, 0.0]], np.float32), (len(p), 1)))
    uv1 = np.ascontiguousarray(p[:, :2] * 0.5)
    pa, na = b.interleaved([p, n])
    source = dict(pos=p, faces=f, normals=n, uvs=u, colour=colour, joints=joints, weights=weights, uv1=uv1)
    full = {"POSITION": pa, "NORMAL": na, "TEXCOORD_0": b.accessor(u), "COLOR_0": b.accessor(colour, normalized=True), "JOINTS_0": b.accessor(joints),
            "WEIGHTS_0": b.accessor(weights), "TEXCOORD_1": b.accessor(uv1)}
    m0 = b.primitive(full, b.accessor(f.astype(np.uint16).reshape(-1)), 4)
    b.primitive({"POSITION": pa}, b.accessor(np.arange(6, dtype=np.uint16)), 1, mesh=m0)
    gp, gn, gu, gf = synth.make_mesh(synth.GRID, 5, 4, 2)
    m1 = b.primitive({"POSITION": b.accessor(gp)})
    b.primitive({"POSITION": b.accessor(gp), "TANGENT": b.accessor(np.concatenate([gn, np.ones((len(gn), 1), np.float32)], axis=1))}, b.accessor(gf.reshape(-1)), mesh=m1)
    b.primitive({"POSITION": b.accessor((gp * 1000).astype(np.int16))}, b.accessor(gf.reshape(-1)), mesh=m1)
    b.primitive({"POSITION": b.accessor(gp), "NORMAL": b.accessor(gn)}, b.accessor(gf.reshape(-1)), mesh=m1)
    return b.glb(), source, dict(pos=gp, normals=gn, faces=gf)


def test_planning_needs_no_device_and_sorts_the_primitives():
    glb, src, grid = mixed_asset()
    asset = gltf.read_asset(glb)
    planned, skipped = gltf.plan_compression([asset])
    assert [(p.mesh, p.primitive) for p in planned] == [(0, 0), (1, 3)]
    reasons = {(s.mesh, s.primitive): s.reason for s in skipped}
    assert sorted(reasons) == [(0, 1), (1, 0), (1, 1), (1, 2)]
    assert "mode 1" in reasons[(0, 1)] and "no indices" in reasons[(1, 0)] and "TANGENT" in reasons[(1, 1)] and "float32 VEC3" in reasons[(1, 2)]
    d = planned[0].data
    assert d.positions.tobytes() == src["pos"].tobytes() and d.normals.tobytes() == src["normals"].tobytes() and d.texcoords.tobytes() == src["uvs"].tobytes()
    assert d.faces.dtype == np.uint32 and np.array_equal(d.faces, src["faces"]) and d.normal_corners is None and d.texcoord_corners is None
    assert planned[0].attribute_ids == {"POSITION": 0, "NORMAL": 1, "TEXCOORD_0": 2, "COLOR_0": 3, "JOINTS_0": 4, "WEIGHTS_0": 5, "TEXCOORD_1": 6}
    kinds = [(a.attribute_type, a.values.dtype, a.values.shape[1], a.normalized) for a in d.attributes]
    assert kinds == [(2, np.uint8, 4, True), (4, np.uint16, 4, False), (4, np.float32, 4, False), (3, np.float32, 2, False)]
    for a, name in zip(d.attributes, ("colour", "joints", "weights", "uv1")):
        assert a.values.tobytes() == src[name].tobytes(), name
    g = planned[1].data
    assert g.positions.tobytes() == grid["pos"].tobytes() and g.texcoords is None and planned[1].attribute_ids == {"POSITION": 0, "NORMAL": 1}


def cpu_coded(planned):
    """What the writer's encode and decode batches give, from the CPU coder and the oracle."""
    coded = {}
    for p in planned:
        d = p.data
        extra = [synth.Extra(a.values, a.attribute_type, a.normalized) for a in d.attributes]
        stream = synth.encode_mesh_points(d.positions, d.faces, d.normals, d.texcoords, None, extra)
        ref = oracle.decode(stream)
        coded[(p.mesh, p.primitive)] = (stream, ref.num_points, len(ref.faces), p.attribute_ids)
    return coded


def test_the_rewritten_document():
    glb, src, grid = mixed_asset()
    asset = gltf.read_asset(glb)
    planned, skipped = gltf.plan_compression([asset])
    coded = cpu_coded(planned)
    out = gltf.rewrite_asset(asset, coded)
    assert len(out) < len(glb)
    new = gltf.read_asset(out)
    doc = new.doc
    assert doc["extensionsUsed"] == [gltf.EXTENSION] and doc["extensionsRequired"] == [gltf.EXTENSION]
    assert len(doc["buffers"]) == 1 and "uri" not in doc["buffers"][0]
    prims = gltf.draco_primitives(new)
    assert [(p.mesh, p.primitive) for p in prims] == sorted(coded)
    for p in prims:
        stream, points, faces, ids = coded[(p.mesh, p.primitive)]
        assert p.stream == stream and p.attribute_ids == ids
        prim = doc["meshes"][p.mesh]["primitives"][p.primitive]
        old = asset.doc["meshes"][p.mesh]["primitives"][p.primitive]
        assert set(prim["attributes"]) == set(old["attributes"]) and prim.get("mode", 4) == 4
        for s, a in prim["attributes"].items():
            acc, was = doc["accessors"][a], asset.doc["accessors"][old["attributes"][s]]
            assert "bufferView" not in acc and "byteOffset" not in acc and acc["count"] == points
            assert (acc["componentType"], acc["type"], acc.get("normalized"), acc.get("min")) == (was["componentType"], was["type"], was.get("normalized"), was.get("min"))
        acc = doc["accessors"][prim["indices"]]
        assert "bufferView" not in acc and acc["count"] == 3 * faces and acc["type"] == "SCALAR"
    assert coded[(0, 0)][1] >= len(src["pos"])                      # (crossing seams may add points, never lose one)
    # every primitive that was skipped reads back byte for byte; the LINES primitive shares the compressed one's positions, which stay
    for s in skipped:
        was, now = asset.doc["meshes"][s.mesh]["primitives"][s.primitive], doc["meshes"][s.mesh]["primitives"][s.primitive]
        assert set(was) == set(now) and gltf.EXTENSION not in now.get("extensions", {})
        for sem in was["attributes"]:
            assert gltf.read_accessor(new, now["attributes"][sem]).tobytes() == gltf.read_accessor(asset, was["attributes"][sem]).tobytes()
        if "indices" in was:
            assert gltf.read_accessor(new, now["indices"]).tobytes() == gltf.read_accessor(asset, was["indices"]).tobytes()
    # nothing to compress: the document comes back without the extension
    plain = gltf.read_asset(gltf.rewrite_asset(asset, {}))
    assert "extensionsUsed" not in plain.doc and gltf.draco_primitives(plain) == []
    assert gltf.read_accessor(plain, plain.doc["meshes"][0]["primitives"][0]["attributes"]["TEXCOORD_0"]).tobytes() == src["uvs"].tobytes()


@pytest.mark.gpu
def test_assets_compressed_in_one_call_load_back():
    glb, src, grid = mixed_asset()
    b = Builder()
    meshes = []
    for k, (kind, charts) in enumerate(((synth.GRID, (None, "checker")), (synth.TORUS, ("checker", "island")))):
        p, f, n, u = seamed(kind, 12, 9, 5 + k, charts)
        b.primitive({"POSITION": b.accessor(p), "NORMAL": b.accessor(n), "TEXCOORD_0": b.accessor(u)}, b.accessor(f.reshape(-1)))
        meshes.append((p, f, n, u))
    sp, sn, su, sf = synth.make_mesh(synth.GRID, 4, 3, 6)              # a two-sided sheet with two normals: the strict coder refuses it
    both = np.concatenate([sf, sf[:, ::-1] + len(sp)])
    b.primitive({"POSITION": b.accessor(np.concatenate([sp, sp])), "NORMAL": b.accessor(np.concatenate([sn, -sn]))}, b.accessor(both.reshape(-1)))
    second = b.glb()
    ctx = dsa.Context(0)
    try:
        results = gltf.GltfDracoWriter(ctx).compress([glb, second])
        assert [[(m, p) for m, p, _, _ in r.compressed] for r in results] == [[(0, 0), (1, 3)], [(0, 0), (1, 0)]]
        assert sorted((s.mesh, s.primitive) for s in results[0].skipped) == [(0, 1), (1, 0), (1, 1), (1, 2)]
        (refused,) = results[1].skipped
        assert (refused.mesh, refused.primitive) == (2, 0) and "non-manifold" in refused.reason
        was, now = gltf.read_asset(second), gltf.read_asset(results[1].glb)
        for sem, a in was.doc["meshes"][2]["primitives"][0]["attributes"].items():
            assert gltf.read_accessor(now, now.doc["meshes"][2]["primitives"][0]["attributes"][sem]).tobytes() == gltf.read_accessor(was, a).tobytes()
        assert gltf.read_accessor(now, now.doc["meshes"][2]["primitives"][0]["indices"]).tobytes() == both.astype(np.uint32).tobytes()
        loaded = gltf.GltfDracoLoader(ctx).load([r.glb for r in results], quantized=True)
        assert [len(x) for x in loaded] == [2, 2]
        sources = [[(src["pos"], src["faces"], src["normals"], src["uvs"]), None], meshes]
        for a, prims in enumerate(loaded):
            for k, d in enumerate(prims):
                if sources[a][k] is None:
                    assert len(d.indices) == 3 * len(grid["faces"])
                    continue
                p, f, n, u = sources[a][k]
                keys = np.concatenate([np.asarray(d.attributes[s], np.int64).reshape(len(d.attributes["POSITION"]), -1) for s in ("POSITION", "NORMAL", "TEXCOORD_0")], axis=1)
                want, _ = meshutil.source_corner_faces(p, n, u, f)
                have = meshutil.face_multiset_fast(d.indices.reshape(-1, 3), keys)
                assert have.shape == want.shape and (have == want).all(), (a, k)
                acc = d.source.asset.doc["accessors"][d.source.accessors["POSITION"]]
                assert acc["count"] == len(keys) >= len(p)
    finally:
        ctx.close()
