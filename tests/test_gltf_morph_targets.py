"""Morph targets through the glTF writer: plan_compression no longer skips a primitive for having `targets` -- it carries their
deltas beside the stream by the rows the encoder tracks (Config(track_rows), Batch.source_rows) -- and skips only what cannot be
carried: a target semantic without a base attribute of that name in the stream, deltas that differ between points the weld joins.
The plan needs no device; GltfDracoWriter.compress is held, on a seamed primitive with two targets, to a pin made from the decoded
stream alone: the deltas are functions of the quantised base value, so the delta written at point p must be that function of what
the stream decodes to at p."""
import numpy as np
import pytest

import meshutil
import oracle
import draco_sharp_amd as dsa
import draco_sharp_amd.synth as synth
from draco_sharp_amd import gltf
from test_gltf_writer import Builder, seamed


def deltas_of(p, n, u):
    """Deltas that are functions of the quantised base values (what a stream of the default bits decodes to): exact pins."""
    qp = meshutil.source_quantization(p, 11)[2].astype(np.float32)
    qn = meshutil.oct_quantize(n, 8).astype(np.float32)
    qu = meshutil.source_quantization(u, 10)[2].astype(np.float32)
    dp = np.ascontiguousarray(qp * np.float32(0.001) + np.float32(0.5))
    dn = np.ascontiguousarray(np.concatenate([qn * np.float32(0.01), np.ones((len(n), 1), np.float32)], axis=1))
    du = np.ascontiguousarray(qu * np.float32(0.25))
    return dp, dn, du


def asset_with_targets(edit=None):
    b = Builder()
    p, f, n, u = seamed(synth.SPHERE, 12, 9, 3)
    dp, dn, du = deltas_of(p, n, u)
    targets = [{"POSITION": dp, "NORMAL": dn}, {"POSITION": dp * np.float32(2), "TEXCOORD_0": du}]
    if edit:
        edit(targets, p)
    base = {"POSITION": b.accessor(p), "NORMAL": b.accessor(n), "TEXCOORD_0": b.accessor(u)}
    b.primitive(base, b.accessor(f.astype(np.uint16).reshape(-1)), 4, targets=[{s: b.accessor(d) for s, d in t.items()} for t in targets])
    g = synth.make_mesh(synth.GRID, 5, 4, 2)
    b.primitive({"POSITION": b.accessor(g[0])}, b.accessor(g[3].reshape(-1)))
    return b.glb(), dict(pos=p, faces=f, normals=n, uvs=u), targets


def test_the_plan_takes_primitives_with_targets():
    glb, src, targets = asset_with_targets()
    planned, skipped = gltf.plan_compression([gltf.read_asset(glb)])
    assert [(p.mesh, p.primitive) for p in planned] == [(0, 0), (1, 0)] and not skipped
    assert [sorted(t) for t in planned[0].targets] == [["NORMAL", "POSITION"], ["POSITION", "TEXCOORD_0"]] and planned[1].targets == []
    for got, want in zip(planned[0].targets, targets):
        for s in want:
            assert got[s].tobytes() == want[s].tobytes()


def test_deltas_that_differ_between_points_the_weld_joins_are_skipped():
    def split(targets, p):
        # two points of one position (the seams duplicate positions): give one of them another delta
        key = np.ascontiguousarray(p).view(np.uint32).reshape(len(p), -1)
        _, first, inverse, counts = np.unique(key, axis=0, return_index=True, return_inverse=True, return_counts=True)
        twice = np.flatnonzero(counts[inverse.reshape(-1)] > 1)
        assert len(twice)
        targets[1]["POSITION"] = targets[1]["POSITION"].copy()
        targets[1]["POSITION"][twice[-1]] += np.float32(1)
    glb, _, _ = asset_with_targets(split)
    planned, skipped = gltf.plan_compression([gltf.read_asset(glb)])
    assert [(p.mesh, p.primitive) for p in planned] == [(1, 0)]
    assert [(s.mesh, s.primitive, s.reason) for s in skipped] == [(0, 0, "morph target 1 of POSITION differs between points the weld joins")]


def test_a_target_without_its_base_attribute_is_skipped():
    def colour(targets, p):
        targets[0]["COLOR_0"] = np.zeros((len(p), 4), np.float32)
    glb, _, _ = asset_with_targets(colour)
    planned, skipped = gltf.plan_compression([gltf.read_asset(glb)])
    assert [(p.mesh, p.primitive) for p in planned] == [(1, 0)]
    assert [(s.mesh, s.primitive) for s in skipped] == [(0, 0)] and skipped[0].reason == "morph target 0 of COLOR_0: no base attribute of that name in the stream"


def check_rewritten(glb, stream, num_points, src):
    """The target accessors of primitive (0, 0) of a rewritten asset against the pin made from the decoded stream."""
    ref = oracle.decode(stream)
    assert ref.num_points == num_points > len(np.unique(src["pos"], axis=0))            # seams: more points than positions
    at = lambda a: np.asarray(a.portable, np.float32)[np.asarray(a.point_map, np.int64)]      # noqa: E731
    qp, qn, qu = (at(a) for a in ref.attributes)
    want = [{"POSITION": qp * np.float32(0.001) + np.float32(0.5), "NORMAL": np.concatenate([qn * np.float32(0.01), np.ones((num_points, 1), np.float32)], axis=1)},
            {"POSITION": (qp * np.float32(0.001) + np.float32(0.5)) * np.float32(2), "TEXCOORD_0": qu * np.float32(0.25)}]
    back = gltf.read_asset(glb)
    prim = back.doc["meshes"][0]["primitives"][0]
    assert gltf.EXTENSION in prim["extensions"] and len(prim["targets"]) == 2
    for k, t in enumerate(want):
        assert sorted(prim["targets"][k]) == sorted(t)
        for s, rows in t.items():
            acc = back.doc["accessors"][prim["targets"][k][s]]
            got = gltf.read_accessor(back, prim["targets"][k][s])
            assert acc["count"] == num_points and got.dtype == np.float32 and got.tobytes() == np.ascontiguousarray(rows).tobytes(), (k, s)
            if s == "POSITION":
                assert acc["min"] == rows.min(axis=0).tolist() and acc["max"] == rows.max(axis=0).tolist()
    assert "targets" not in back.doc["meshes"][1]["primitives"][0]


def test_the_rewritten_targets_from_the_cpu_coder():
    """rewrite_asset with what the writer's encode and decode batches give, made by the CPU coder, its entry rows and the oracle."""
    glb, src, _ = asset_with_targets()
    asset = gltf.read_asset(glb)
    planned, _ = gltf.plan_compression([asset])
    coded = {}
    for p in planned:
        d = p.data
        stream = synth.encode_mesh_points(d.positions, d.faces, d.normals, d.texcoords)
        entry = synth.entry_rows(d.positions, d.faces, d.normals, d.texcoords, form=2)
        ref = oracle.decode(stream)
        rows = [e[np.asarray(a.point_map, np.int64)].astype(np.int64) for e, a in zip(entry, ref.attributes)]
        moved = [{s: t[s][rows[p.attribute_ids[s]]] for s in t} for t in p.targets]
        coded[(p.mesh, p.primitive)] = (stream, ref.num_points, len(ref.faces), p.attribute_ids, moved)
    check_rewritten(gltf.rewrite_asset(asset, coded), coded[(0, 0)][0], coded[(0, 0)][1], src)


@pytest.mark.gpu
def test_compress_carries_the_deltas_to_the_points_of_the_stream():
    glb, src, targets = asset_with_targets()
    ctx = dsa.Context(0)
    try:
        out = gltf.GltfDracoWriter(ctx).compress([glb])[0]
        assert not out.skipped and [(m, p) for m, p, _, _ in out.compressed] == [(0, 0), (1, 0)]
        check_rewritten(out.glb, out.compressed[0][2], out.compressed[0][3], src)
        # the result through the device loader: its points are the rows of the target accessors, and the deltas are the functions
        # of what it decodes at every point (quantized: the integers the stream carries)
        loaded = gltf.GltfDracoLoader(ctx).load([out.glb], quantized=True)[0]
        assert len(loaded) == 2
        prim = gltf.read_asset(out.glb)
        targets = prim.doc["meshes"][0]["primitives"][0]["targets"]
        q = {s: np.asarray(v, np.float32) for s, v in loaded[0].attributes.items()}
        assert len(q["POSITION"]) == out.compressed[0][3] and all(prim.doc["accessors"][a]["count"] == len(q["POSITION"]) for t in targets for a in t.values())
        dp = q["POSITION"] * np.float32(0.001) + np.float32(0.5)
        assert gltf.read_accessor(prim, targets[0]["POSITION"]).tobytes() == dp.tobytes()
        assert gltf.read_accessor(prim, targets[1]["POSITION"]).tobytes() == (dp * np.float32(2)).tobytes()
        assert gltf.read_accessor(prim, targets[0]["NORMAL"])[:, :2].tobytes() == np.ascontiguousarray(q["NORMAL"][:, :2] * np.float32(0.01)).tobytes()
        assert gltf.read_accessor(prim, targets[1]["TEXCOORD_0"]).tobytes() == (q["TEXCOORD_0"] * np.float32(0.25)).tobytes()
    finally:
        ctx.close()
