"""Integer attributes beyond uint8 through every decode kernel: int8 / uint8 / int16 / uint16 / int32 / uint32 of 1 - 4 components
(tests/typedcases.py) on the wave-per-mesh kernels, on the general path, with tags of up to 28 bits on a wave of their own,
with dense alphabets of 16-bit noise that exhaust the pooled tables, in a crowded batch (k_chain), beside seams, in sequential
streams, and out through result(), device_views() and the compact download.

Every stream must decode (status 0), every array must equal the oracle's AND the pin, which is the input array itself: integer
attributes are lossless.  test_typed_attributes_cpu.py holds the cases to their conditions (negative wrap bounds, values that
differ from their low byte, tags >= 27, alphabets past SYM_MAX_LDS) and shows what the pin catches."""
import numpy as np
import pytest

import irregular
import oracle
import typedcases as T
import draco_sharp_amd as dsa
import draco_sharp_amd.synth as synth
import test_gpu_parity
from test_gpu_parity import assert_same, assert_same_attributes

pytestmark = pytest.mark.gpu

# option sets that stay on the wave-per-mesh kernels (decode_path 0); (name, options, which cases)
FAST = [
    ("default", dict(), lambda c: True),
    ("tagged", dict(force_scheme=0), lambda c: True),
    ("raw", dict(force_scheme=1), T.raw_scheme_legal),
    ("positions-difference", dict(pos_prediction=0), lambda c: True),
    ("constrained-multi-parallelogram", dict(pos_prediction=4), lambda c: True),
    ("uncompressed-3", dict(raw_integers=3), lambda c: T.raw_width_fits(c, 3)),
    ("uncompressed-4", dict(raw_integers=4), lambda c: True),
    ("no-prediction", dict(no_prediction=8), lambda c: True),
]
# schemes the general path takes by itself
GENERAL = [("multi-parallelogram", dict(pos_prediction=2)), ("prediction-degree", dict(traversal_method=1)),
           ("predictive-connectivity", dict(predictive_connectivity=1))]
# one mid-size mesh per topology, the sizes of test_gpu_parity.test_tag_streams_on_a_wave_of_their_own
MID = [(synth.GRID, 128, 256), (synth.TORUS, 96, 128), (synth.HOLES, 70, 90), (synth.SPHERE, 40, 60)]


@pytest.fixture(scope="module")
def ctx():
    c = dsa.Context(0)
    yield c
    c.close()


_streams, _refs, _mid = {}, {}, {}


def stream_of(case, **opt):
    key = (case.name, tuple(sorted(opt.items())))
    if key not in _streams:
        _streams[key] = T.encode(case, opt)
    return _streams[key]


def ref_of(stream):
    if stream not in _refs:
        _refs[stream] = oracle.decode(stream)
    return _refs[stream]


def mid_mesh(k):
    if k not in _mid:
        kind, nx, ny = MID[k]
        _mid[k] = synth.make_mesh(kind, nx, ny, 80 + k)
    return _mid[k]


def check(b, i, stream, dtype, expected, debug=True):
    """Stream i of batch b: decoded, equal to the oracle (with the connectivity's debug arrays), typed as the input, equal to the pin."""
    info = b.mesh_info(i)
    assert info.status == 0, (i, info.status, info.detail)
    got = b.result(i)
    assert_same(got, ref_of(stream), b if debug else None, i)
    g = got.ConnectedData.Attributes[-1]
    assert g.Values.dtype == dtype and g.DataType == T.DATA_TYPE[np.dtype(dtype)]
    assert T.same_multiset(T.device_multiset(got.ConnectedData), expected), i
    return info


def items_of(option_sets, cases=None):
    """[(case, option name, stream)] of every case under every option set that applies to it."""
    out = []
    for name, opt, legal in option_sets:
        out += [(c, name, stream_of(c, **opt)) for c in (cases or T.CASES) if legal(c)]
    return out


def test_the_meshes_are_those_of_the_parity_tests():
    assert [tuple(k) for k in T.KINDS] == [tuple(k) for k in test_gpu_parity.KINDS]


# ------------------------------------------------------------------------------------------------------ 1 fast kernels
@pytest.mark.parametrize("name", [o[0] for o in FAST])
def test_every_case_on_the_fast_kernels(ctx, name):
    items = items_of([o for o in FAST if o[0] == name])
    assert len(items) >= 64
    b = dsa.Batch(ctx, [it[2] for it in items])
    b.decode()
    for i, (c, _, s) in enumerate(items):
        info = check(b, i, s, c.dtype, T.pin_of(c))
        assert info.decode_path == 0, (c.name, name, info.decode_path)
    b.close()


# ------------------------------------------------------------------------------------------------------ 2 general path
@pytest.mark.parametrize("name", [o[0] for o in FAST])
def test_every_case_on_the_general_path_when_forced(ctx, monkeypatch, name):
    monkeypatch.setenv("DSA_FORCE_GENERAL", "1")
    items = items_of([o for o in FAST if o[0] == name])
    b = dsa.Batch(ctx, [it[2] for it in items])
    b.decode()
    for i, (c, _, s) in enumerate(items):
        check(b, i, s, c.dtype, T.pin_of(c))
        assert b.debug_array(i, 4, np.uint32, 12)[6] == 0, c.name        # no k_traverse clock: the fast kernels skipped the mesh
    b.close()


@pytest.mark.parametrize("name", [o[0] for o in GENERAL])
def test_every_case_with_the_schemes_that_go_to_the_general_path(ctx, name):
    opt = dict(GENERAL)[name]
    items = [(c, name, stream_of(c, **opt)) for c in T.CASES]
    b = dsa.Batch(ctx, [it[2] for it in items])
    b.decode()
    for i, (c, _, s) in enumerate(items):
        info = check(b, i, s, c.dtype, T.pin_of(c))
        assert info.decode_path != 0, (c.name, name)
    b.close()


# ----------------------------------------------------------------------------------------- 3 wide tags on their own wave
def test_wide_tags_on_a_wave_of_their_own(ctx):
    """Tags of 27 - 28 bits (int32 / uint32 noise) and of 16 - 17 (int16 noise) in meshes large enough for k_tags + k_locate_resume,
    a uint8 attribute of the same mesh beside them: out_cap, where the tag bytes are parked and by which the symbol kernel is chosen,
    is 16 times as large for uint32 x 4 as for uint8 x 1."""
    items = []
    for k in range(len(MID)):
        pos, nrm, uv, faces = mid_mesh(k)
        for j, (dtype, nc) in enumerate(((np.int32, 1), (np.uint32, 4), (np.int16, 3), (np.uint8, 1))):
            gen = T.values(dtype, "random", len(pos), nc, seed=900 + 4 * k + j)
            s = synth.encode_mesh(pos, faces, nrm, uv, generic=gen, opt=synth.options(force_scheme=0, generic_components=nc))
            items.append((s, np.dtype(dtype), T.pin(pos, faces, gen), len(pos) * (nc - 1) * 4 >= 4096 * 10))
    ctx.set_profiling(True)
    try:
        b = dsa.Batch(ctx, [it[0] for it in items])
        b.decode()
        kernels = b.kernel_times()
    finally:
        ctx.set_profiling(False)
    print("kernels:", {k: round(v, 3) for k, v in kernels.items() if v > 0})
    assert kernels.get("k_tags", 0) > 0, kernels
    top, on_their_own_wave = 0, []
    for i, (s, dtype, expected, _) in enumerate(items):
        info = check(b, i, s, dtype, expected)
        assert info.decode_path == 0, (i, info.decode_path)
        source, _, by_k_tags, _ = b.debug_array(i, 5, np.uint32, 64).reshape(16, 4)[3]
        assert source == 0, i                                                           # source 0: the generic attribute's symbols are tagged
        on_their_own_wave.append(int(by_k_tags))
        top = max(top, int(ref_of(s).attributes[-1].symbols.max()).bit_length())
    assert top >= 27, top
    print("generic tag streams decoded by k_tags:", on_their_own_wave)
    # k_tags takes a tag stream where the attribute's work region (4 bytes per value) holds its tables (REG_SCRATCH_BYTES, 40 KB)
    # beside the tags (4 bytes per entry): rows of 3 and 4 on all but the smallest mesh; a one-component attribute never has the
    # room, whatever its type, and the stream walk decodes its tags (dsa_kernels.h: reg_decode_stream<REG_TAGS>)
    assert on_their_own_wave == [int(room) for _, _, _, room in items], on_their_own_wave
    assert sum(on_their_own_wave) == 6
    b.close()


# -------------------------------------------------------------------------------------------- 4 large dense alphabets
def test_dense_16_bit_alphabets_exhaust_the_pooled_tables(ctx):
    """int16 / uint16 noise under the raw scheme on the mid-size meshes: 16 - 17 bit symbols, nearly every one distinct, rANS
    precision up to 20 bits; 512 copies in one batch, so that the pool of cumulative tables runs out and meshes are decoded again by
    the general path.  The verdict of a stream does not depend on its neighbours: every copy decodes, and equally."""
    base = []
    for k in range(len(MID)):
        pos, nrm, uv, faces = mid_mesh(k)
        for j, (dtype, nc) in enumerate(((np.int16, 1), (np.uint16, 4))):
            gen = T.values(dtype, "random", len(pos), nc, seed=950 + 2 * k + j)
            s = synth.encode_mesh(pos, faces, nrm, uv, generic=gen, opt=synth.options(force_scheme=1, generic_components=nc))
            base.append((s, np.dtype(dtype), T.pin(pos, faces, gen)))
    dense = 0
    for s, _, _ in base:
        sym = ref_of(s).attributes[-1].symbols
        distinct = len(np.unique(sym))
        assert int(sym.max()) + 1 > 4032 and (distinct > 4032 or distinct >= 0.9 * sym.size)      # an alphabet past SYM_MAX_LDS, densely used
        dense += distinct > 4032
    assert dense >= 6                                                                    # (the sphere's 2 362 entries x 1 cannot hold that many)
    n = 512
    b = dsa.Batch(ctx, [base[i % len(base)][0] for i in range(n)])
    b.decode()
    bad = [(i, b.status(i), b.mesh_info(i).detail) for i in range(n) if b.status(i) != 0]
    assert not bad, bad[:8]
    paths = [b.mesh_info(i).decode_path for i in range(n)]
    print("decode paths:", {p: paths.count(p) for p in sorted(set(paths))})
    for i in sorted(set(list(range(0, n, 37)) + list(range(len(base))) + [n - 1])):
        check(b, i, *base[i % len(base)], debug=False)
    b.close()
    ctx.trim()


# ------------------------------------------------------------------------------------------------------ 5 crowded batch
def test_crowded_batch_of_typed_attributes(ctx):
    """The default streams of every case repeated to 4096: k_chain, four small meshes of unequal size to a wave."""
    items = items_of(FAST[:1])
    n = 4096
    ctx.set_profiling(True)
    try:
        b = dsa.Batch(ctx, [items[i % len(items)][2] for i in range(n)])
        b.decode()
        kernels = b.kernel_times()
    finally:
        ctx.set_profiling(False)
    print("kernels:", {k: round(v, 3) for k, v in kernels.items() if v > 0})
    assert kernels.get("k_chain", 0) > 0, kernels
    bad = [(i, b.status(i), b.mesh_info(i).detail) for i in range(n) if b.status(i) != 0]
    assert not bad, bad[:8]
    for i in sorted(set(list(range(0, n, 37)) + [0, n - 1])):
        c, _, s = items[i % len(items)]
        info = check(b, i, s, c.dtype, T.pin_of(c))
        assert info.decode_path == 0
    b.close()


# ----------------------------------------------------------------------------- 6 seams, sequential meshes, point clouds
def test_typed_attributes_beside_seams(ctx):
    items = []
    for k, c in enumerate(T.CASES[::3]):
        pos, nrm, uv, faces = T.mesh(c.mesh)
        args = irregular.with_seams(pos, nrm, uv, faces, *irregular.CHARTS[k % len(irregular.CHARTS)], seed=70 + k)
        # (ConstrainedMultiParallelogram on an attribute located behind the seam tables is the general path's: not here)
        opt = (dict(), dict(uv_prediction=5, normal_prediction=6), dict(uv_prediction=5), dict(force_scheme=0))[k % 4]
        items.append((c, synth.encode_mesh_corners(*args, generic=T.generic_of(c), opt=synth.options(generic_components=c.nc, **opt))))
    b = dsa.Batch(ctx, [s for _, s in items])
    b.decode()
    for i, (c, s) in enumerate(items):
        info = check(b, i, s, c.dtype, T.pin_of(c))
        assert info.decode_path == 0, (c.name, info.decode_path)
    b.close()


@pytest.mark.parametrize("geometry", ["mesh-compressed", "mesh-raw", "cloud"])
def test_typed_attributes_in_sequential_streams(ctx, geometry):
    """Difference prediction in the caller's order: the decoded array is the input array."""
    items = []
    for k, c in enumerate(T.CASES):
        pos, nrm, uv, faces = T.mesh(c.mesh)
        opt = synth.options(force_scheme=(-1, 0, 1)[k % 3] if T.raw_scheme_legal(c) else (-1, 0)[k % 2])
        if geometry == "cloud":
            items.append((c, synth.encode_point_cloud_attributes(pos, nrm if k % 2 else None, None, T.generic_of(c), opt=opt)))
        else:
            items.append((c, synth.encode_sequential(pos, faces, None, uv if k % 2 else None, T.generic_of(c), compressed=geometry == "mesh-compressed", opt=opt)))
    b = dsa.Batch(ctx, [s for _, s in items])
    b.decode()
    for i, (c, s) in enumerate(items):
        assert b.status(i) == 0, (c.name, b.status(i), b.mesh_info(i).detail)
        ref = ref_of(s)
        m = b.result(i).ConnectedData
        assert_same_attributes(m, ref)
        g = m.Attributes[-1]
        assert np.array_equal(g.PointMap, np.arange(len(T.generic_of(c)), dtype=np.uint32))
        assert g.Values.dtype == c.dtype and np.array_equal(g.Values, T.generic_of(c)), (geometry, c.name)
        if geometry != "cloud":
            assert np.array_equal(m.Faces, ref.faces) and np.array_equal(m.Faces, T.mesh(c.mesh)[3].astype(np.int32))
    b.close()


# ------------------------------------------------------------------------------------------------------------ 7 outputs
def test_result_device_views_and_the_compact_download_keep_the_type(ctx):
    import torch
    # one case per type with values beyond the low byte and (signed) below zero; a uint8 x 1 attribute of an odd entry count in front
    # of an int16 one: in the compact block the 2-byte values follow an odd number of bytes
    names = ["uint8-sentinel-x1", "int16-random-x2", "int8-extremes-x3", "uint16-sentinel-x4", "int32-random-x1", "uint32-sentinel-x2", "uint32-random-x3",
             "uint16-joints-x4", "int16-constant-x3"]
    cases = [next(c for c in T.CASES if c.name == n) for n in names]
    assert {c.dtype for c in cases} == set(T.DTYPES)
    streams = [T.encode(c, normals=False, uvs=False) if k < 2 else stream_of(c) for k, c in enumerate(cases)]
    assert ref_of(streams[0]).attributes[-1].num_entries % 2 == 1
    b = dsa.Batch(ctx, streams)
    b.decode()
    for i, (c, s) in enumerate(zip(cases, streams)):
        check(b, i, s, c.dtype, T.pin_of(c))
        g = b.result(i).ConnectedData.Attributes[-1]
        ref = ref_of(s).attributes[-1]
        dv = b.device_views(i)["attributes"][-1]
        signed = np.dtype(c.dtype.kind.replace("u", "i") + str(c.dtype.itemsize)) if c.dtype.itemsize > 1 else c.dtype
        on_host = dv["values"].cpu().numpy()
        assert dv["values"].is_cuda and on_host.dtype == signed and on_host.shape == g.Values.shape
        assert on_host.tobytes() == ref.values.tobytes() and np.array_equal(on_host.view(c.dtype), g.Values)        # bit for bit through the signed view
        assert np.array_equal(dv["point_map"].cpu().numpy().view(np.uint32), g.PointMap)
    for compact in (True, False, True):
        b.decode(wait=False)
        b.download(compact=compact)
        for i, (c, s) in enumerate(zip(cases, streams)):
            ref = ref_of(s)
            v = b.host_views(i)
            a, r = v["attributes"][-1], ref.attributes[-1]
            assert a["values"].dtype == c.dtype and a["values"].tobytes() == r.values.tobytes(), (compact, c.name)
            assert np.array_equal(np.asarray(v["faces"], np.int64), ref.faces)
            pm = np.arange(ref.num_points, dtype=np.uint32) if a["point_map"] is None else a["point_map"]
            got = T.decoded_multiset(v["faces"], b.result(i).ConnectedData.Attributes[0].PortableValues, v["attributes"][0]["point_map"], a["values"], pm)
            assert T.same_multiset(got, T.pin_of(c)), (compact, c.name)
            assert b.result(i).ConnectedData.Attributes[-1].Values.tobytes() == r.values.tobytes()                     # the accessors, served from the host copy
    b.close()


# ---------------------------------------------------------------------------------------------------------- 8 refusals
def test_data_types_an_integer_attribute_cannot_have_fail_alone(ctx, monkeypatch):
    """int64, uint64, float64, bool in the descriptor of an integer attribute: the reference's StoreValues knows int8 ... uint32 and
    throws for the rest; the device refuses the stream and decodes its neighbours."""
    good, bad = [], []
    for c in (T.CASES[0], next(c for c in T.CASES if c.name == "uint32-sentinel-x2")):
        for s, at in T.descriptor_streams(c):
            good.append(s)
            for dt in (7, 8, 10, 11):
                d = bytearray(s)
                d[at] = dt
                bad.append(bytes(d))
    streams = []
    for k, s in enumerate(bad):
        streams += [good[k % len(good)], s]
    for general in (False, True):
        if general:
            monkeypatch.setenv("DSA_FORCE_GENERAL", "1")
        b = dsa.Batch(ctx, streams)
        b.decode()
        for i, s in enumerate(streams):
            if i % 2:
                with pytest.raises(oracle.OracleError):
                    oracle.decode(s)
                assert b.status(i) != 0, (i, general)
            else:
                assert b.status(i) == 0, (i, general, b.mesh_info(i).detail)
                assert_same_attributes(b.result(i).ConnectedData, ref_of(s))
        b.close()


@pytest.mark.parametrize("general", [False, True])
def test_three_byte_integers_on_both_paths(ctx, monkeypatch, general):
    """Uncompressed integers at 3 bytes (the decoder takes 1 ... 4): every attribute of the stream, typed one included."""
    if general:
        monkeypatch.setenv("DSA_FORCE_GENERAL", "1")
    items = [(c, stream_of(c, raw_integers=3, pos_prediction=k % 2)) for k, c in enumerate(T.CASES) if T.raw_width_fits(c, 3)][::2]
    assert len(items) >= 32
    b = dsa.Batch(ctx, [s for _, s in items])
    b.decode()
    for i, (c, s) in enumerate(items):
        info = check(b, i, s, c.dtype, T.pin_of(c))
        assert general or info.decode_path == 0, (c.name, info.decode_path)
        assert (b.debug_array(i, 4, np.uint32, 12)[6] == 0) == general
    b.close()
