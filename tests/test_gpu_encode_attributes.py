"""The attribute list of the device encoder (dsa_encode_attributes_batch / dsa_encode_attributes_sequential_batch): typed
integer and float attributes behind the built-in ones must come out, byte for byte, as the CPU coder writes them
(draco-sharp_amd/csrc/dsa_encode_host.h through draco_sharp_amd.synth), and decode to the INPUT arrays."""
import ctypes as C
import struct

import numpy as np
import pytest

import encodecall
import attrcases as A
import irregular
import oracle
import typedcases as T
import draco_sharp_amd as dsa
import draco_sharp_amd.synth as synth
from draco_sharp_amd import native

pytestmark = pytest.mark.gpu

LEVELS = (3, 5, 7, 10)
SCHEMES = (-1, 0, 1)


@pytest.fixture(scope="module")
def ctx():
    c = dsa.Context(0)
    yield c
    c.close()


def set_paths(monkeypatch, host_conn, host_plan):
    for name, v in (("DSA_ENC_HOST_CONN", host_conn), ("DSA_ENC_HOST_PLAN", host_plan)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)


def synth_options(cfg, m):
    return synth.options(pos_bits=cfg.position_bits, uv_bits=cfg.texcoord_bits, normal_bits=cfg.normal_bits,
                         single_connectivity=1 if cfg.single_connectivity else 0, force_scheme=cfg.symbol_scheme,
                         compression_level=10 - cfg.speed, pos_prediction=cfg.position_prediction, uv_prediction=cfg.texcoord_prediction,
                         normal_prediction=cfg.normal_prediction, predictive_connectivity=2 if cfg.edgebreaker_method == 2 else 0,
                         generic_components=m.generic.shape[1] if m.generic is not None else 1)


def extras_of(m):
    return [synth.Extra(a.values, a.attribute_type, a.normalized, a.unique_id, a.quantization_bits) for a in m.attributes]


def cpu(m, cfg):
    """The CPU coder's stream of MeshData / PointCloudData m (its attribute list included) under cfg."""
    opt = synth_options(cfg, m)
    if isinstance(m, dsa.PointCloudData):
        return synth.encode_point_cloud_attributes(m.positions, m.normals, m.texcoords, m.generic, opt=opt, extra=extras_of(m))
    if cfg.sequential:
        return synth.encode_sequential(m.positions, m.faces, m.normals, m.texcoords, m.generic, compressed=cfg.compress_connectivity, opt=opt, extra=extras_of(m))
    return synth.encode_mesh_corners(m.positions, m.faces, m.normals, m.normal_corners, m.texcoords, m.texcoord_corners, opt=opt, generic=m.generic,
                                     extra=extras_of(m))


def raw(ctx, meshes, cfg, geometry=1, edit=None, opt=None):
    """The entry point cfg asks for, straight: (call status, [(status, bytes or the mesh's message)]).  edit(arr, keep): changes
    to the native array before the call."""
    sequential = geometry == 0 or cfg.sequential
    if opt is None:
        opt = cfg._native_sequential(geometry) if sequential else cfg._native_ex()
    return encodecall.call(ctx, "dsa_encode_attributes_sequential_batch" if sequential else "dsa_encode_attributes_batch", meshes, opt, edit=edit)


def check_equal(ctx, meshes, cfg, names=None, geometry=1):
    got = dsa.DracoEncoder(ctx).EncodeBatch(meshes, cfg)
    assert len(got) == len(meshes)
    for i, m in enumerate(meshes):
        exp = cpu(m, cfg)
        assert got[i] == exp, (names[i] if names else i, len(got[i]), len(exp))
    return got


# ------------------------------------------------------------------------------------------ the 99 typed cases
def case_mesh(c, sequential, k):
    pos, nrm, uv, faces = T.mesh(c.mesh)
    att = dsa.Attribute(T.generic_of(c), attribute_type=4)
    if sequential:
        return dsa.MeshData(pos, faces, nrm if k % 2 else None, uv if k % 3 else None, attributes=[att])
    return dsa.MeshData(pos, faces, nrm, uv, attributes=[att])


def typed_round(ctx, sequential, turn):
    """Every typed case as one extra under every symbol scheme legal for it; the compression levels go round the cases (case k
    under scheme s takes level (k + s + turn) % 4, `turn` the path combination), so every level meets every scheme and, over the
    path combinations, every case.  One call per (scheme, level): dozens of meshes each."""
    ran = 0
    for si, scheme in enumerate(SCHEMES):
        for li, level in enumerate(LEVELS):
            group = [(k, c) for k, c in enumerate(T.CASES) if (k + si + turn) % len(LEVELS) == li and (scheme != 1 or T.raw_scheme_legal(c))]
            cfg = dsa.Config(symbol_scheme=scheme, speed=10 - level, encoding_method=0 if sequential else 1, compress_connectivity=bool(li & 1))
            assert len(group) >= 12
            check_equal(ctx, [case_mesh(c, sequential, k) for k, c in group], cfg, [c.name for _, c in group])
            ran += len(group)
    assert ran == 2 * len(T.CASES) + sum(T.raw_scheme_legal(c) for c in T.CASES)


@pytest.mark.parametrize("host_conn", ["0", "1"])
@pytest.mark.parametrize("host_plan", ["0", "1"])
def test_typed_cases_edgebreaker(ctx, monkeypatch, host_conn, host_plan):
    set_paths(monkeypatch, host_conn, host_plan)
    typed_round(ctx, False, 2 * int(host_conn) + int(host_plan))


@pytest.mark.parametrize("host_conn", ["0", "1"])
@pytest.mark.parametrize("host_plan", ["0", "1"])
def test_typed_cases_sequential(ctx, monkeypatch, host_conn, host_plan):
    set_paths(monkeypatch, host_conn, host_plan)
    typed_round(ctx, True, 2 * int(host_conn) + int(host_plan))


def test_typed_case_equals_the_generic_path_of_the_cpu_coder(ctx):
    """(what ties the above to tests/typedcases.py: the expectation is typedcases.encode's stream)"""
    cases = T.CASES[::9]
    got = dsa.DracoEncoder(ctx).EncodeBatch([case_mesh(c, False, 0) for c in cases])
    for c, g in zip(cases, got):
        assert g == T.encode(c), c.name


# ----------------------------------------------------------------------------------------------- equivalence
def plain_meshes():
    out = []
    for k, name in enumerate(["kind0", "kind1", "kind2", "kind3", "kind4", "shuffled-fan-open"]):
        pos, nrm, uv, faces = T.mesh(name)
        gen = ((np.arange(len(pos))[:, None] * (3 + np.arange(1 + k % 4))) % 251).astype(np.uint8)
        out.append((pos, faces, nrm if k != 2 else None, uv if k != 4 else None, gen))
    return out


@pytest.mark.parametrize("kind", ["edgebreaker", "valence-stock", "sequential-compressed", "sequential-raw", "cloud"])
def test_no_extras_and_uint8_extra_equal_the_calls_before(ctx, kind):
    cfg = {"edgebreaker": dsa.Config(), "valence-stock": dsa.Config(edgebreaker_method=2, texcoord_prediction=5, normal_prediction=6),
           "sequential-compressed": dsa.Config(encoding_method=0, compress_connectivity=True), "sequential-raw": dsa.Config(encoding_method=0),
           "cloud": dsa.Config()}[kind]
    geometry = 0 if kind == "cloud" else 1
    make = (lambda p, f, n, u, **kw: dsa.PointCloudData(p, n, u, **kw)) if kind == "cloud" else dsa.MeshData
    with_generic = [make(p, f, n, u, generic=g) for p, f, n, u, g in plain_meshes()]
    before = list(dsa.DracoEncoder(ctx).EncodeBatch(with_generic, cfg))
    # no extras through the new entry points: the bytes of dsa_encode_batch_ex / dsa_encode_sequential_batch
    st, got = raw(ctx, with_generic, cfg, geometry)
    assert st == 0 and [g for g in got] == [(0, b) for b in before]
    # one uint8 type-4 extra in place of mesh.generic: the same bytes
    as_extra = [make(p, f, n, u, attributes=[dsa.Attribute(g, attribute_type=4)]) for p, f, n, u, g in plain_meshes()]
    assert list(dsa.DracoEncoder(ctx).EncodeBatch(as_extra, cfg)) == before


def test_generic_together_with_two_extras(ctx):
    meshes = []
    for k, (p, f, n, u, g) in enumerate(plain_meshes()):
        extras = [dsa.Attribute((np.arange(len(p) * 2).reshape(len(p), 2) * 37 - 20000).astype(np.int16), attribute_type=4, unique_id=90 + k),
                  dsa.Attribute(np.ascontiguousarray(p[:, :2] * np.float32(3)), attribute_type=3)]
        meshes.append(dsa.MeshData(p, f, n, u, generic=g, attributes=extras))
    for cfg in (dsa.Config(), dsa.Config(single_connectivity=True, symbol_scheme=0), dsa.Config(encoding_method=0, compress_connectivity=True, texcoord_bits=13)):
        got = check_equal(ctx, meshes, cfg)
        ref = oracle.decode(got[0])
        assert [a.att_type for a in ref.attributes] == [0, 1, 3, 4, 4, 3] and ref.attributes[4].unique_id == 90


# --------------------------------------------------------------------------------------------- the three extras
class Desc:
    """A decoded dsa attribute under the names attrcases uses for the oracle's."""

    def __init__(self, a):
        self.att_type, self.data_type, self.num_components, self.normalized = a.AttributeType, a.DataType, a.NumComponents, int(a.Normalized)
        self.unique_id, self.seq_type, self.q_bits, self.q_min, self.q_range = a.UniqueId, a.DecoderType, a.QuantizationBits, a.MinValues, a.Range


def skinned_mesh(name, cloud=False):
    pos, nrm, uv, faces = T.mesh(name)
    atts = [dsa.Attribute(a, **kw) for a, kw in A.skinned(name)]
    return dsa.PointCloudData(pos, nrm, uv, attributes=atts) if cloud else dsa.MeshData(pos, faces, nrm, uv, attributes=atts)


SKINNED_CONFIGS = {"edgebreaker": dict(), "valence": dict(edgebreaker_method=2), "sequential-raw": dict(encoding_method=0),
                   "sequential-compressed": dict(encoding_method=0, compress_connectivity=True), "cloud": dict()}


@pytest.mark.parametrize("kind", A.KINDS)
def test_three_extras_equal_the_cpu_coder_and_decode_to_the_input(ctx, kind):
    cfg = dsa.Config(**SKINNED_CONFIGS[kind])
    meshes = [skinned_mesh(name, kind == "cloud") for name in A.MESHES]
    got = check_equal(ctx, meshes, cfg, A.MESHES)
    for name, g in zip(A.MESHES, got):
        assert g == A.cpu_stream(kind, name, A.skinned(name)), name                # the stream of the CPU test
    b = dsa.Batch(ctx, list(got))
    b.decode()
    for i, name in enumerate(A.MESHES):
        assert b.status(i) == 0
        pos, nrm, uv, faces = T.mesh(name)
        items = A.skinned(name)
        d = b.result(i).ConnectedData
        for k, (array, kw) in enumerate(items):          # type, data type, normalised flag and unique id as passed (dsa_batch_attribute_info)
            A.check_descriptor(Desc(d.Attributes[3 + k]), array, kw, 3 + k)
        atts = [(Desc(a), a.Values, a.PortableValues, a.PointMap) for a in d.Attributes]
        if kind in ("edgebreaker", "valence"):
            A.check_connected(d.Faces, atts, pos, faces, items, 3)
        else:
            for k, (array, kw) in enumerate(items):      # the caller's order: point i is row i
                desc, values, portable, pmap = atts[3 + k]
                keys, exact = A.expected_rows(array, kw)
                rows = np.asarray(values)[np.asarray(pmap, np.int64)] if pmap is not None and len(pmap) else np.asarray(values)
                assert rows.dtype == exact.dtype and rows.tobytes() == np.ascontiguousarray(exact).tobytes(), (name, k)
    b.close()


def test_three_extras_beside_normals_and_uvs_given_per_corner(ctx, monkeypatch):
    meshes, names = [], []
    for k, name in enumerate(A.MESHES):
        pos, nrm, uv, faces = T.mesh(name)
        p, f, n, nci, u, uci = irregular.with_seams(pos, nrm, uv, faces, *irregular.CHARTS[(5 + k) % len(irregular.CHARTS)], seed=40 + k)
        meshes.append(dsa.MeshData(p, f, n, u, normal_corners=nci, texcoord_corners=uci, attributes=[dsa.Attribute(a, **kw) for a, kw in A.skinned(name)]))
        names.append(name)
    for host_conn in ("1", "0"):
        set_paths(monkeypatch, host_conn, host_conn)
        got = check_equal(ctx, meshes, dsa.Config(), names)
    ref = oracle.decode(got[0])
    A.check_connected(ref.faces, A.oracle_atts(ref), *T.mesh(A.MESHES[0])[::3], A.skinned(A.MESHES[0]), 3)


# ------------------------------------------------------------------------------------------- the alphabet edges
def symbols_of(stream):
    return oracle.decode(stream).attributes[-1].symbols


def both_entries(ctx, monkeypatch, array, name="kind5", schemes=(-1, 0), att=None, expect_symbols=None):
    """One extra on mesh `name` through both entry points, device and host plans: the CPU coder's bytes.  expect_symbols(symbols
    of the sequential stream as the CPU coder codes them): the test's claim about the alphabet."""
    pos, nrm, uv, faces = T.mesh(name)
    att = att or dsa.Attribute(array, attribute_type=4)
    mesh, cloud = dsa.MeshData(pos, faces, None, None, attributes=[att]), dsa.PointCloudData(pos, attributes=[att])
    if expect_symbols:
        expect_symbols(symbols_of(cpu(cloud, dsa.Config())))
    for host in ("0", "1"):
        set_paths(monkeypatch, host, host)
        for scheme in schemes:
            check_equal(ctx, [mesh, mesh], dsa.Config(symbol_scheme=scheme))
            check_equal(ctx, [mesh], dsa.Config(symbol_scheme=scheme, encoding_method=0, compress_connectivity=True))
            check_equal(ctx, [cloud], dsa.Config(symbol_scheme=scheme))
    return mesh, cloud


@pytest.mark.parametrize("distinct", [4096, 4097, 4098])
def test_uint16_alphabet_at_the_lds_histogram_switch(ctx, monkeypatch, distinct):
    """Exactly `distinct` symbol values 0 .. distinct - 1 (value range distinct - 1, histogram of distinct + 2 entries): 4096 is
    the last alphabet k_enc_corr counts in LDS (4098 entries), 4097 and 4098 the first it counts in global memory."""
    nv = len(T.mesh("kind5")[0])
    array = A.residue_walk(distinct - 1, nv, 3, np.uint16)
    assert int(array.max()) - int(array.min()) == distinct - 1

    def claim(sym):
        assert len(np.unique(sym)) == distinct and int(sym.max()) == distinct - 1
    both_entries(ctx, monkeypatch, array, schemes=(-1, 0, 1), expect_symbols=claim)


def test_int32_largest_symbol_just_below_the_raw_limit(ctx, monkeypatch):
    span = (1 << 18) - 1
    array = A.largest_symbol_values(span, len(T.mesh("kind0")[0]), 1 << 17)

    def claim(sym):
        assert int(sym.max()) == (1 << 18) - 1
    both_entries(ctx, monkeypatch, array, "kind0", schemes=(-1, 0, 1), expect_symbols=claim)


def test_int32_largest_symbol_at_the_raw_limit(ctx, monkeypatch):
    """A symbol of 2^18: the CPU coder builds no histogram of values and writes the tagged scheme; so must the device.  The raw
    scheme forced: that mesh fails alone with DSA_ERR_INVALID_DATA while its neighbours encode."""
    span = 1 << 18
    array = A.largest_symbol_values(span, len(T.mesh("kind0")[0]), 1 << 17)

    def claim(sym):
        assert int(sym.max()) == 1 << 18
    mesh, cloud = both_entries(ctx, monkeypatch, array, "kind0", expect_symbols=claim)
    pos, nrm, uv, faces = T.mesh("kind0")
    small = dsa.Attribute((np.arange(len(pos)) % 300).astype(np.int32))
    # (through the parallelogram the corrections of `array` stay below the limit; spread values do not)
    spread = T.values(np.int32, "random", len(pos), 1, seed=3)
    assert int(symbols_of(cpu(dsa.MeshData(pos, faces, None, None, attributes=[dsa.Attribute(spread)]), dsa.Config())).max()) >= 1 << 18
    for host in ("0", "1"):
        set_paths(monkeypatch, host, host)
        for seq in (False, True):
            cfg = dsa.Config(symbol_scheme=1, encoding_method=0 if seq else 1)
            good = dsa.MeshData(pos, faces, nrm, uv, attributes=[small])
            bad = dsa.MeshData(pos, faces, None, None, attributes=[dsa.Attribute(array if seq else spread)])
            st, got = raw(ctx, [good, bad, good], cfg)
            assert st == 0
            assert got[0] == (0, cpu(good, cfg)) and got[2] == got[0]
            assert got[1][0] == native.DSA_ERR_INVALID_DATA and "2^18" in got[1][1], got[1]


def test_int8_and_int16_with_negative_wrap_bounds(ctx, monkeypatch):
    nv = len(T.mesh("kind3")[0])
    rng = np.random.default_rng(5)
    for array, lo, hi in ((rng.integers(-120, -2, (nv, 3)).astype(np.int8), -120, -3), (rng.integers(-30000, -99, (nv, 2)).astype(np.int16), -30000, -100)):
        array[0], array[1] = lo, hi
        pos, nrm, uv, faces = T.mesh("kind3")
        s = cpu(dsa.MeshData(pos, faces, None, None, attributes=[dsa.Attribute(array)]), dsa.Config())
        assert struct.unpack("<ii", s[-8:]) == (lo, hi)
        both_entries(ctx, monkeypatch, array, "kind3", schemes=(-1,))


def test_the_all_ones_sentinel_in_uint32(ctx, monkeypatch):
    nv = len(T.mesh("kind1")[0])
    array = (np.arange(nv * 2, dtype=np.uint32).reshape(nv, 2) % 500).astype(np.uint32)
    array[::7] = 0xFFFFFFFF
    mesh, cloud = both_entries(ctx, monkeypatch, array, "kind1", schemes=(-1, 0, 1))
    got = oracle.decode(dsa.DracoEncoder(ctx).Encode(cloud)).attributes[-1].values
    assert got.dtype == np.uint32 and np.array_equal(got, array)


def test_a_constant_attribute(ctx, monkeypatch):
    nv = len(T.mesh("kind2")[0])
    for array in (np.full((nv, 4), 51234, np.uint16), np.full((nv, 1), -77, np.int32), np.full((nv, 2), np.float32(0.25))):
        both_entries(ctx, monkeypatch, array, "kind2", schemes=(-1, 0, 1))
    s = cpu(dsa.MeshData(*T.mesh("kind2")[::3], attributes=[dsa.Attribute(np.full((nv, 4), 51234, np.uint16))]), dsa.Config())
    assert struct.unpack("<ii", s[-8:]) == (51234, 51234)                           # max_dif = 1


# --------------------------------------------------------------------------------------------- a crowded batch
def test_a_crowded_batch_of_mixed_types(ctx, monkeypatch):
    """300 small meshes, above the 256-mesh switch: the device does connectivity and symbol plans by its own rule."""
    set_paths(monkeypatch, None, None)
    monkeypatch.delenv("DSA_ENC_CHUNK", raising=False)
    kinds = [(synth.GRID, 7, 5), (synth.TORUS, 6, 5), (synth.SPHERE, 6, 6), (synth.HOLES, 12, 9), (synth.TWO_PARTS, 6, 4)]
    dtypes = T.DTYPES + [np.dtype(np.float32)]
    meshes = []
    for i in range(300):
        kind, nx, ny = kinds[i % len(kinds)]
        pos, nrm, uv, faces = synth.make_mesh(kind, nx + i % 3, ny + (i // 3) % 2, 500 + i)
        atts = []
        for j in range(1 + i % 3):
            dt, nc = dtypes[(i + 3 * j) % len(dtypes)], 1 + (i + j) % 4
            if dt == np.float32:
                v = np.random.default_rng([i, j]).random((len(pos), nc)).astype(np.float32)
                atts.append(dsa.Attribute(v, attribute_type=(3, 4, 2)[j], quantization_bits=(0, 12, 5)[j]))
            else:
                v = T.values(dt, T.PATTERNS[(i + j) % len(T.PATTERNS)], len(pos), nc, seed=i)
                atts.append(dsa.Attribute(v, attribute_type=(4, 2, 4)[j], normalized=bool(j & 1), unique_id=None if i % 2 else 20 + j))
        meshes.append(dsa.MeshData(pos, faces, nrm if i % 4 else None, uv if i % 5 else None, attributes=atts))
    check_equal(ctx, meshes, dsa.Config())
    check_equal(ctx, meshes, dsa.Config(encoding_method=0, compress_connectivity=True))


# -------------------------------------------------------------------------------------------------- refusals
def bad_lists(nv):
    """[(what, edit of the second mesh's native attribute list, words the message must hold)]"""
    def setter(field, value, k=1):
        def edit(arr, keep):
            setattr(arr[1].attributes[k], field, value)
        return edit

    def reserved_word(arr, keep):
        arr[1].attributes[0].reserved[1] = 5

    def mesh_reserved(arr, keep):
        arr[1].reserved = 1

    def too_many(arr, keep):
        big = (native.AttributeInput * 14)()
        for k in range(14):
            C.memmove(C.byref(big[k]), C.byref(arr[1].attributes[0]), C.sizeof(native.AttributeInput))
        keep.append(big)
        arr[1].attributes, arr[1].num_attributes = big, 14

    return [("attribute_type", setter("attribute_type", 1), ("attribute 1", "attribute_type 1")),
            ("data_type", setter("data_type", 7), ("attribute 1", "data_type 7")),
            ("no components", setter("num_components", 0), ("attribute 1", "num_components 0")),
            ("five components", setter("num_components", 5, 0), ("attribute 0", "num_components 5")),
            ("normalized", setter("normalized", 2), ("attribute 1", "normalized 2")),
            ("quantization_bits", setter("quantization_bits", 21), ("attribute 1", "quantization_bits 21")),      # (the float32 one)
            ("values", setter("values", None), ("attribute 1", "values")),
            ("reserved word", reserved_word, ("attribute 0", "reserved[1]")),
            ("mesh reserved", mesh_reserved, ("dsa_mesh_attr_input.reserved",)),
            ("unique id of a built-in attribute", setter("unique_id", 2), ("attribute 1", "unique_id 2")),
            ("unique id twice", setter("unique_id", A.JOINTS_ID, 2), ("attribute 2", "unique_id %d" % A.JOINTS_ID)),
            ("seventeen attributes", too_many, ("exceed",))]


@pytest.mark.parametrize("sequential", [False, True])
def test_a_bad_attribute_list_fails_its_mesh_alone(ctx, sequential):
    name = "kind0"
    cfg = dsa.Config(encoding_method=0 if sequential else 1)
    meshes = [skinned_mesh(name), skinned_mesh(name), skinned_mesh("kind3")]
    expected = [cpu(m, cfg) for m in meshes]
    for what, edit, words in bad_lists(len(meshes[0].positions)):
        st, got = raw(ctx, meshes, cfg, edit=edit)
        assert st == 0, what
        assert got[0] == (0, expected[0]) and got[2] == (0, expected[2]), what
        assert got[1][0] == native.DSA_ERR_INVALID_ARGUMENT, (what, got[1])
        assert all(w in got[1][1] for w in words), (what, got[1][1])


def test_the_sequential_call_refuses_corner_ids(ctx):
    pos, nrm, uv, faces = T.mesh("kind0")
    p, f, n, nci, u, uci = irregular.with_seams(pos, nrm, uv, faces, None, "stripes", seed=3)
    seamed = dsa.MeshData(p, f, n, u, texcoord_corners=uci, attributes=[np.zeros(len(p), np.uint8)])
    good = skinned_mesh("kind0")
    cfg = dsa.Config(encoding_method=0)
    st, got = raw(ctx, [good, seamed, good], cfg)
    assert st == 0 and got[0] == (0, cpu(good, cfg)) and got[2] == got[0]
    assert got[1][0] == native.DSA_ERR_INVALID_ARGUMENT and "corner ids" in got[1][1]
    with pytest.raises(ValueError, match="per corner"):
        dsa.DracoEncoder(ctx).EncodeBatch([good, seamed], cfg)


def test_reserved_options_fail_the_call(ctx):
    good = [skinned_mesh("kind0")]
    o = dsa.Config()._native_ex()
    o.reserved[3] = 1
    assert raw(ctx, good, dsa.Config(), opt=o)[0] == native.DSA_ERR_INVALID_ARGUMENT and "reserved" in ctx.error()
    o = dsa.Config(encoding_method=0)._native_sequential(1)
    o.reserved[0] = 1
    assert raw(ctx, good, dsa.Config(encoding_method=0), opt=o)[0] == native.DSA_ERR_INVALID_ARGUMENT and "reserved" in ctx.error()
    o = dsa.Config()._native_ex()
    o.normal_prediction = 3
    assert raw(ctx, good, dsa.Config(), opt=o)[0] == native.DSA_ERR_INVALID_ARGUMENT and "normal_prediction" in ctx.error()
