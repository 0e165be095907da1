"""The HIP decode and encode kernels on irregular connectivity (tests/irregular.py: flipped, subdivided, thickened and shuffled
meshes, fans, a strip, many components).  Every other GPU test takes its meshes from synth.make_mesh -- regular grids, on which
the run detection of k_chain / k_connectivity and the speculation of the traversal wave are nearly always right; here the
wrong-guess side of those checks, the scalar steps behind failed pairs, the split-corner tables, all six valence context lists
with both clamps and vertex fans of 1 .. 60 000 corners are what runs.

Decode: reference = the oracle (test_gpu_parity.assert_same: faces, point maps, portable integers, floats bit for bit, and the debug
arrays opposite / corner_to_vertex / data_to_corner) and, independently, the numpy pin of the INPUT; tests/test_irregular_cpu.py shows
that the two agree on this input.  Which kernels a batch takes depends on its size and make-up, so each test says from the kernel
timers which side it reached:
  small batches, seamed batches   k_connectivity + k_traverse (+ k_seam_tables, k_traverse_att, k_texcoords with seams)
  4096 small unseamed streams     k_chain
  4096 streams of 60 - 70 k faces k_chain + k_predict_oct_streams (the bench step's kernels)
Encode: reference = the CPU coder (byte equality) and the pin (round trip through the device decoder).
No case is skipped, filtered or allowed to be refused."""
import numpy as np
import pytest

import irregular
import oracle
import draco_sharp_amd as dsa
import draco_sharp_amd.synth as synth
from meshutil import face_multiset_fast, source_corner_faces, source_corner_faces_seamed
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

SEAM_DIALECTS = [("standard", dict()), ("stock-default", irregular.DIALECTS["stock-default"]), ("texcoords-portable", dict(uv_prediction=5)),
                 ("multi-parallelogram", dict(pos_prediction=4))]
UNFUSED = ("k_connectivity", "k_traverse")


@pytest.fixture(scope="module")
def ctx():
    c = dsa.Context(0)
    yield c
    c.close()


_refs = {}


def ref_of(stream):
    if stream not in _refs:
        _refs[stream] = oracle.decode(stream)
    return _refs[stream]


def pin_equal(mesh, expected):
    keys = np.concatenate([np.asarray(a.PortableValues, np.int64)[np.asarray(a.PointMap, np.int64)] for a in mesh.Attributes], axis=1)
    got = face_multiset_fast(mesh.Faces, keys)
    assert got.shape == expected.shape and np.array_equal(got, expected)


def path_ok(info, opt, ref):
    """The path follows from the dialect, not from the topology: what the grid tests assert per dialect (test_gpu_parity,
    test_seams) holds here -- the wave-per-mesh kernels for everything but prediction-degree order, and a valence stream of under
    1000 faces may carry tagged context lists, which take the second chance (decode_path 2)."""
    if opt.get("traversal_method"):
        return info.decode_path != 0
    return info.decode_path == 0 or (info.decode_path == 2 and ref.traversal_type == 2 and ref.num_faces < 1000)


def per_vertex_streams(cases):
    """[(name, dialect name, options, stream, pin)]"""
    out = []
    for c in cases:
        pos, nrm, uv, faces = irregular.mesh(c)
        pin = source_corner_faces(pos, nrm, uv, faces)[0]
        for dname, opt in irregular.DIALECTS.items():
            out.append((c.name, dname, opt, synth.encode_mesh(pos, faces, nrm, uv, opt=synth.options(**opt)), pin))
    return out


def decode_profiled(ctx, streams, times=1):
    ctx.set_profiling(True)
    try:
        b = dsa.Batch(ctx, streams)
        for _ in range(times):
            b.decode()
        kernels = b.kernel_times()
    finally:
        ctx.set_profiling(False)
    print("kernels:", {k: round(v, 3) for k, v in kernels.items() if v > 0})
    return b, kernels


def check(b, i, item, debug=True):
    name, dname, opt, stream, pin = item
    info = b.mesh_info(i)
    assert info.status == 0, (i, name, dname, info.status, info.detail)
    ref = ref_of(stream)
    got = b.result(i)
    assert_same(got, ref, b if debug else None, i)
    pin_equal(got.ConnectedData, pin)
    assert path_ok(info, opt, ref), (i, name, dname, info.decode_path)
    return info.decode_path


# ------------------------------------------------------------------------------------------------------------ decode
def test_small_cases_in_every_dialect_on_the_unfused_kernels(ctx):
    items = per_vertex_streams(irregular.SMALL)
    assert len(items) == len(irregular.SMALL) * 6
    order = np.random.default_rng(1).permutation(len(items))
    for batch in (items, [items[k] for k in order]):          # the same streams beside other neighbours, in other slots
        b, kernels = decode_profiled(ctx, [it[3] for it in batch])
        assert all(kernels.get(k, 0) > 0 for k in UNFUSED) and kernels.get("k_chain", 0) == 0, kernels
        paths = [check(b, i, it) for i, it in enumerate(batch)]
        b.close()
        fast = sum(p == 0 for p in paths)
        print("decode paths:", {p: paths.count(p) for p in sorted(set(paths))})
        assert fast >= len(irregular.SMALL) * 3          # standard, multi-parallelogram and single connectivity: always path 0


def test_small_cases_with_seams(ctx):
    items = []
    for c in irregular.SMALL:
        for k, charts in enumerate(irregular.CHARTS):
            args = irregular.with_seams(*irregular.mesh(c), *charts, seed=40 + k)
            pin = source_corner_faces_seamed(*args)[0]
            for dname, opt in SEAM_DIALECTS:
                items.append((c.name + " " + str(charts), dname, opt, synth.encode_mesh_corners(*args, opt=synth.options(**opt)), pin))
    assert len(items) == len(irregular.SMALL) * len(irregular.CHARTS) * 4
    b, kernels = decode_profiled(ctx, [it[3] for it in items])
    assert all(kernels.get(k, 0) > 0 for k in UNFUSED + ("k_seam_tables", "k_traverse_att", "k_texcoords")) and kernels.get("k_chain", 0) == 0, kernels
    paths = [check(b, i, it) for i, it in enumerate(items)]
    b.close()
    print("decode paths:", {p: paths.count(p) for p in sorted(set(paths))})
    assert sum(p == 0 for p in paths) >= len(items) // 2          # the standard and the multi-parallelogram half at the least


def test_crowded_batch_of_small_irregular_meshes(ctx):
    """4096 unseamed streams, the 84 small ones repeated: k_chain with small meshes of unequal size, four to a wave.  Decoded twice
    (the context's two stream sets); every distinct stream compared at its first and at its last position, after each decode."""
    items = per_vertex_streams(irregular.SMALL)
    n = 4096
    crowd = [items[i % len(items)] for i in range(n)]
    picks = sorted(set(range(len(items))) | set(range(n - len(items), n)))
    assert {crowd[i][3] for i in picks[:len(items)]} == {crowd[i][3] for i in picks[len(items):]} == {it[3] for it in items}
    ctx.set_profiling(True)
    try:
        b = dsa.Batch(ctx, [it[3] for it in crowd])
        for _ in range(2):
            b.decode()
            kernels = b.kernel_times()
            print("kernels:", {k: round(v, 3) for k, v in kernels.items() if v > 0})
            assert kernels.get("k_chain", 0) > 0 and kernels.get("k_traverse", 0) == 0, kernels
            assert all(b.status(i) == 0 for i in range(n))
            for i in picks:
                check(b, i, crowd[i])
    finally:
        ctx.set_profiling(False)
    b.close()


def test_the_bench_batch_made_irregular(ctx):
    """The shape of test_the_bench_batch_at_full_size (4096 streams of 60 - 70 k faces in ONE batch, the crowded-batch kernels
    asserted from the timers), with the three bench-size irregular cases x {standard, valence, stock default} in place of the grid:
    5 000 - 6 700 split events per mesh, a fifth of the vertices at valence 6."""
    items = [it for it in per_vertex_streams(irregular.BENCH_SIZE) if it[1] in ("standard", "valence", "stock-default")]
    assert len(items) == 9 and all(60000 <= ref_of(it[3]).num_faces <= 70000 for it in items)
    n = 4096
    crowd = [items[i % 9] for i in range(n)]
    b, kernels = decode_profiled(ctx, [it[3] for it in crowd])
    try:
        assert kernels.get("k_chain", 0) > 0 and kernels.get("k_predict_oct_streams", 0) > 0 and kernels.get("k_traverse", 0) == 0, kernels
        bad = [(i, b.mesh_info(i).detail) for i in range(n) if b.status(i) != 0]
        assert not bad, bad[:10]
        assert all(b.mesh_info(i).decode_path == 0 for i in range(0, n, 37))
        picks = sorted(set(range(9)) | set(range(n - 9, n)) | {int(x) for x in np.linspace(0, n - 1, 128)})
        assert len(picks) >= 130
        for i in picks:
            assert check(b, i, crowd[i], debug=i < 9) == 0
    finally:
        b.close()
        ctx.trim()          # the arena goes back before the next test


def test_the_odd_extremes(ctx):
    """One vertex of valence 60 000, a band of 2 x 100 000 boundary vertices, 20 000 components: parity with the oracle and the
    pin.  (No bound on their time: nobody has measured them on these kernels.)"""
    items = []
    for name, m in (("fan", irregular.fan(60000)), ("strip", irregular.strip(100000)), ("components", irregular.components(20000))):
        pos, nrm, uv, faces = m
        assert irregular.is_oriented_manifold(len(pos), faces)
        pin = source_corner_faces(pos, nrm, uv, faces)[0]
        for dname in ("standard", "stock-default"):
            opt = irregular.DIALECTS[dname]
            items.append((name, dname, opt, synth.encode_mesh(pos, faces, nrm, uv, opt=synth.options(**opt)), pin))
    b, kernels = decode_profiled(ctx, [it[3] for it in items])
    print("stages:", {k: round(v, 2) for k, v in b.stage_times().items()})
    for i, it in enumerate(items):
        assert check(b, i, it) == 0
    b.close()


# ------------------------------------------------------------------------------------------------------------ encode
def encoder_configs():
    from test_gpu_encode_stock import CONFIGS
    return [dsa.Config()] + CONFIGS


@pytest.mark.parametrize("host", ["0", "1"])
def test_device_encoder_matches_the_cpu_coder(ctx, monkeypatch, host):
    """The small cases with ids, face order and face corners shuffled, per vertex and with seams, under every configuration of
    tests/test_gpu_encode_stock.py and the default, on both connectivity paths: every stream byte-equal to the CPU coder's."""
    import test_gpu_encode_stock as S
    S.force_path(monkeypatch, host)
    meshes = [(name, dsa.MeshData(pos, faces, nrm, uv)) for name, (pos, nrm, uv, faces) in irregular.shuffled_small()]
    meshes += [(name + " " + str(charts), S.corner_data(args)) for name, charts, args in irregular.seamed_small(shuffled=True)]
    assert len(meshes) == 3 * len(irregular.SMALL)
    for ci, cfg in enumerate(encoder_configs()):
        got = S.encode(ctx, [m for _, m in meshes], cfg)
        for (name, m), (st, g) in zip(meshes, got):
            assert st == 0, (name, ci, st)
            assert g == S.cpu(m, cfg), (name, ci)


@pytest.mark.parametrize("host", ["0", "1"])
def test_device_encoded_streams_decode_to_the_input(ctx, monkeypatch, host):
    import test_gpu_encode_stock as S
    S.force_path(monkeypatch, host)
    inputs = [(dsa.MeshData(pos, faces, nrm, uv), source_corner_faces(pos, nrm, uv, faces)[0]) for _, (pos, nrm, uv, faces) in irregular.shuffled_small()]
    inputs += [(S.corner_data(args), source_corner_faces_seamed(*args)[0]) for _, _, args in irregular.seamed_small(shuffled=True)]
    for cfg in (dsa.Config(), dsa.Config(**S.STOCK)):
        got = S.encode(ctx, [m for m, _ in inputs], cfg)
        assert all(st == 0 for st, _ in got)
        b, paths = S.decode_paths(ctx, [g for _, g in got])
        b2, cpu_paths = S.decode_paths(ctx, [S.cpu(m, cfg) for m, _ in inputs])
        b2.close()
        assert paths == cpu_paths
        for i, (m, pin) in enumerate(inputs):
            pin_equal(b.result(i).ConnectedData, pin)
        b.close()


def test_device_encoder_on_bench_size_and_small_meshes_in_one_call(ctx, monkeypatch):
    """256 meshes on the default device path, bench-size and small ones mixed: the chunk pipeline with unequal meshes."""
    import test_gpu_encode_stock as S
    monkeypatch.delenv("DSA_ENC_HOST_CONN", raising=False)
    monkeypatch.delenv("DSA_ENC_HOST_PLAN", raising=False)
    pos, nrm, uv, faces = irregular.mesh("holes-128x128-flipped-thickened")
    big = dsa.MeshData(pos, faces, nrm, uv)
    small = [dsa.MeshData(pos, faces, nrm, uv) for _, (pos, nrm, uv, faces) in irregular.shuffled_small()]
    small += [S.corner_data(args) for _, _, args in irregular.seamed_small(shuffled=True)[:6]]
    meshes = [big if i % 16 == 5 else small[i % len(small)] for i in range(256)]
    cfg = dsa.Config(**S.STOCK)
    got = S.encode(ctx, meshes, cfg)
    want = {id(m): S.cpu(m, cfg) for m in [big] + small}
    for i, (m, (st, g)) in enumerate(zip(meshes, got)):
        assert st == 0 and g == want[id(m)], i
