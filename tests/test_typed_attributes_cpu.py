"""Integer attributes of every element type (int8 ... uint32) through the CPU coder, the oracle and the serial general path's
source on the host.  The expectation is the pin of tests/typedcases.py: the input array itself.  This file also holds the list
of cases to the conditions the GPU test (test_gpu_typed_attributes.py) relies on, so that it cannot pass on attributes that
are 8-bit in disguise, and shows that the pin catches the mistakes a width or sign error would make."""
import struct

import numpy as np
import pytest

import irregular
import oracle
import typedcases as T
import draco_sharp_amd.synth as synth
from test_hostcheck import exe, host_decode, assert_equals_oracle          # noqa: F401  (exe: the fixture that builds general_host)
from test_hostcheck_lanes import exe as lanes_exe, lanes_decode            # noqa: F401  (the fixture that builds lanes_host)

SYM_MAX_LDS = 4032          # draco-sharp_amd/csrc/dsa_locate.h

# option sets every case goes through; "legal" says which cases a set applies to
OPTION_SETS = [
    ("default", dict(), lambda c: True),
    ("tagged", dict(force_scheme=0), lambda c: True),
    ("raw", dict(force_scheme=1), T.raw_scheme_legal),
    ("positions-difference", dict(pos_prediction=0), lambda c: True),
    ("positions-multi-parallelogram", dict(pos_prediction=2), lambda c: True),
    ("constrained-multi-parallelogram", dict(pos_prediction=4), lambda c: True),
    ("prediction-degree", dict(traversal_method=1), lambda c: True),
    ("valence", dict(predictive_connectivity=2), lambda c: True),
    ("uncompressed-2", dict(raw_integers=2), lambda c: T.raw_width_fits(c, 2)),
    ("uncompressed-3", dict(raw_integers=3), lambda c: T.raw_width_fits(c, 3)),
    ("uncompressed-4", dict(raw_integers=4), lambda c: True),
    ("no-prediction", dict(no_prediction=8), lambda c: True),
    ("no-prediction-uncompressed-4", dict(no_prediction=15, raw_integers=4), lambda c: True),
]

_decoded = {}


def decoded(case, **opt):
    """(stream, oracle mesh) of a case under an option set, once per process."""
    key = (case.name, tuple(sorted(opt.items())))
    if key not in _decoded:
        s = T.encode(case, opt)
        _decoded[key] = (s, oracle.decode(s))
    return _decoded[key]


def wrap_bounds(stream):
    """(min, max) of the wrap transform of the last attribute of a stream with a connectivity per attribute: the generic
    attribute's prediction data closes the stream and integer attributes have no transform parameters behind it."""
    return struct.unpack("<ii", stream[-8:])


def as_int32(v):
    v = np.asarray(v)
    return (v.view(np.int32) if v.dtype == np.uint32 else v).astype(np.int64)


# ------------------------------------------------------------------------------------------------- the list of cases
def test_the_list_holds_every_type_pattern_and_width():
    assert len({c.name for c in T.CASES}) == len(T.CASES)
    have = {(c.dtype, c.pattern, c.nc) for c in T.CASES}
    assert all((d, p, n) in have for d in T.DTYPES for p in T.PATTERNS for n in (1, 2, 3, 4))
    assert {c.pattern for c in T.CASES} >= {"constant", "constant-zero", "joints"}
    assert {c.mesh for c in T.CASES} == set(T.mesh_names())                  # every small mesh and every shuffled case is in use
    assert len(T.mesh_names()) == 7 + len(irregular.SMALL)
    for c in T.CASES:
        v = T.generic_of(c)
        assert v.dtype == c.dtype and v.shape == (len(T.mesh(c.mesh)[0]), c.nc) and not v.flags.writeable
        assert np.abs(as_int32(v)).max() <= T.LIMIT32
        assert np.array_equal(v, T.values(c.dtype, c.pattern, len(v), c.nc, seed=T.CASES.index(c)))      # deterministic


def test_the_cases_are_what_the_gpu_test_takes_them_for():
    wide_low_byte = set()
    negative_min = set()
    top_tag = 0
    raw_alphabets = []
    for c in T.CASES:
        s, ref = decoded(c)
        g = ref.attributes[-1]
        assert (g.att_type, g.seq_type, g.data_type, g.num_components, g.pred_method, g.pred_transform) == (4, 1, T.DATA_TYPE[c.dtype], c.nc, 1, 1)
        assert g.values.dtype == c.dtype
        if np.any((g.values.astype(np.int64) & 0xFF) != g.values.astype(np.int64)):
            wide_low_byte.add(c.dtype)
        mn, mx = wrap_bounds(s)
        src = as_int32(T.generic_of(c))
        assert (mn, mx) == (int(src.min()), int(src.max())), c.name            # the transform's bounds are those of the input, signed
        if mn < 0 and c.dtype.kind == "i":
            negative_min.add(c.dtype)
        # per entry the tag is the bit length of its largest symbol
        s0, ref0 = decoded(c, force_scheme=0)
        top_tag = max(top_tag, int(ref0.attributes[-1].symbols.max()).bit_length())
        if T.raw_scheme_legal(c):
            sym = decoded(c, force_scheme=1)[1].attributes[-1].symbols
            raw_alphabets.append((int(sym.max()) + 1, len(np.unique(sym)), sym.size, c.name))
    assert wide_low_byte >= {d for d in T.DTYPES if d.itemsize > 1}
    assert negative_min == {d for d in T.DTYPES if d.kind == "i"}
    assert top_tag >= 27, top_tag
    # raw streams: an alphabet past the LDS search whose symbols are nearly all distinct, one of the middle tier, a small one
    assert any(n > SYM_MAX_LDS and distinct > SYM_MAX_LDS and distinct >= 0.9 * count for n, distinct, count, _ in raw_alphabets)
    assert any(65 <= n <= 2048 for n, _, _, _ in raw_alphabets) and any(n <= 64 for n, _, _, _ in raw_alphabets)
    assert sum(T.raw_width_fits(c, 3) for c in T.CASES) >= 64                               # streams at the 3-byte width: all but wide 32-bit ones
    print("largest tag %d; raw alphabet %d with %d distinct symbols of %d" % ((top_tag,) + max(raw_alphabets, key=lambda r: r[1])[:3]))


# ------------------------------------------------------------------------------------------------- oracle == the pin
@pytest.mark.parametrize("name", [o[0] for o in OPTION_SETS])
def test_oracle_returns_the_input(name):
    _, opt, legal = next(o for o in OPTION_SETS if o[0] == name)
    ran = 0
    for c in T.CASES:
        if not legal(c):
            continue
        s, ref = decoded(c, **opt)
        g = ref.attributes[-1]
        assert g.data_type == T.DATA_TYPE[c.dtype] and g.values.dtype == c.dtype
        if "no_prediction" in opt:
            assert g.pred_method == -2
        assert T.same_multiset(T.oracle_multiset(ref), T.pin_of(c)), (name, c.name)
        assert np.array_equal(as_int32(g.values), g.portable)                      # the typed values are the narrowed integers
        ran += 1
    assert ran >= (len(T.CASES) if name not in ("raw", "uncompressed-2", "uncompressed-3") else 40), ran


def test_uncompressed_widths_refuse_what_does_not_fit():
    wide = next(c for c in T.CASES if c.name == "int32-random-x1")
    for width in (1, 2, 3):
        with pytest.raises(RuntimeError, match="does not fit"):
            T.encode(wide, dict(raw_integers=width))
    with pytest.raises(RuntimeError, match="raw_integers"):
        T.encode(wide, dict(raw_integers=5))
    # one byte holds everything else of this stream (6-bit positions and texture coordinates, 5-bit normals) but not 16-bit noise
    noise = next(c for c in T.CASES if c.name == "int16-random-x1")
    narrow = dict(pos_bits=6, uv_bits=6, normal_bits=5)
    T.encode(next(c for c in T.CASES if c.name == "uint8-ramp-x1"), dict(raw_integers=1, **narrow))
    with pytest.raises(RuntimeError, match="does not fit"):
        T.encode(noise, dict(raw_integers=1, **narrow))
    for width in (2, 3, 4):
        ref = oracle.decode(T.encode(noise, dict(raw_integers=width, **narrow)))
        assert 255 < int(ref.attributes[-1].symbols.max()) <= 65535
        assert T.same_multiset(T.oracle_multiset(ref), T.pin_of(noise, pos_bits=6))


def test_with_seams_beside_the_typed_attribute():
    """Normals and texture coordinates given per corner (corner attributes, seam tables); the typed attribute stays per vertex."""
    ran = 0
    for k, c in enumerate(T.CASES[::3]):
        pos, nrm, uv, faces = T.mesh(c.mesh)
        charts = irregular.CHARTS[k % len(irregular.CHARTS)]
        args = irregular.with_seams(pos, nrm, uv, faces, *charts, seed=70 + k)
        s = synth.encode_mesh_corners(*args, generic=T.generic_of(c), opt=synth.options(generic_components=c.nc, pos_prediction=(1, 4)[k & 1]))
        ref = oracle.decode(s)
        assert ref.attributes[-1].data_type == T.DATA_TYPE[c.dtype]
        assert T.same_multiset(T.oracle_multiset(ref), T.pin_of(c)), c.name
        ran += 1
    assert ran == 33


@pytest.mark.parametrize("geometry", ["mesh-compressed", "mesh-raw", "cloud"])
def test_sequential_streams_keep_the_callers_order(geometry):
    for k, c in enumerate(T.CASES):
        pos, nrm, uv, faces = T.mesh(c.mesh)
        gen = T.generic_of(c)
        opt = synth.options(force_scheme=(-1, 0, 1)[k % 3] if T.raw_scheme_legal(c) else (-1, 0)[k % 2])
        if geometry == "cloud":
            s = synth.encode_point_cloud_attributes(pos, nrm if k % 2 else None, None, gen, opt=opt)
        else:
            s = synth.encode_sequential(pos, faces, None, uv if k % 2 else None, gen, compressed=geometry == "mesh-compressed", opt=opt)
        ref = oracle.decode(s)
        g = ref.attributes[-1]
        assert g.data_type == T.DATA_TYPE[c.dtype] and g.pred_method == 0 and len(g.point_map) == 0
        assert g.values.dtype == gen.dtype and np.array_equal(g.values, gen), (geometry, c.name)
        if geometry != "cloud":
            assert np.array_equal(ref.faces, faces.astype(np.int32))


# ------------------------------------------------------------------------------- the general path's source on the host
SMALL = [c for c in T.CASES if c.mesh in ("kind0", "kind1", "kind2", "kind4")]
HOST_OPTIONS = [dict(), dict(force_scheme=0), dict(pos_prediction=2), dict(pos_prediction=4), dict(traversal_method=1), dict(raw_integers=4),
                dict(raw_integers=3), dict(no_prediction=8)]


@pytest.mark.parametrize("k", range(len(SMALL)))
def test_general_path_source_on_typed_attributes(exe, tmp_path, k):
    c = SMALL[k]
    opt = HOST_OPTIONS[k % len(HOST_OPTIONS)]
    if opt.get("raw_integers") == 3 and not T.raw_width_fits(c, 3):
        opt = dict(raw_integers=4)
    s, ref = decoded(c, **opt)
    status, detail, got = host_decode(exe, s, tmp_path, force=True)
    assert status == 0, (c.name, detail)
    assert_equals_oracle(got, ref)
    faces, npnt, atts = got
    typed = T._cast(atts[-1][2], c.dtype)                                         # the narrowing store of the output kernel
    assert T.same_multiset(T.decoded_multiset(faces, atts[0][2], atts[0][1], typed, atts[-1][1]), T.pin_of(c)), c.name


def test_stream_walk_and_lane_kernels_on_typed_attributes(lanes_exe, tmp_path):
    """The stream walk of k_locate accepts every typed stream, and the lane-per-stream symbol and prediction bodies (where the
    alphabet is within their tiers) return the oracle's integers -- the product's source on the host under ASan + UBSan."""
    options = [dict(), dict(force_scheme=0), dict(force_scheme=1), dict(pos_prediction=0), dict(raw_integers=3), dict(raw_integers=4), dict(no_prediction=8)]
    decoded_by_lanes = 0
    for k, c in enumerate(T.CASES[::2]):
        opt = options[k % len(options)]
        if (opt.get("force_scheme") == 1 and not T.raw_scheme_legal(c)) or (opt.get("raw_integers") == 3 and not T.raw_width_fits(c, 3)):
            opt = dict()
        s, ref = decoded(c, **opt)
        status, detail, atts = lanes_decode(lanes_exe, s, tmp_path, ref)
        assert status == 0, (c.name, opt, detail)
        if atts[-1] is not None:
            assert np.array_equal(atts[-1], ref.attributes[-1].portable), (c.name, opt)
            decoded_by_lanes += 1
    assert decoded_by_lanes >= 5


def test_the_small_cases_cover_the_types():
    assert {c.dtype for c in SMALL} == set(T.DTYPES) and len(SMALL) >= 12


# ---------------------------------------------------------------------------------------------------------- refusals
def test_data_types_an_integer_attribute_cannot_have_are_refused():
    """int64, uint64, float64 and bool in the descriptor of an integer attribute (DataType ids 7, 8, 10, 11)."""
    for c in (T.CASES[0], next(c for c in T.CASES if c.name == "uint32-sentinel-x2")):
        for s, at in T.descriptor_streams(c):
            assert s[at] == T.DATA_TYPE[c.dtype]
            oracle.decode(s)
            for bad in (7, 8, 10, 11):
                d = bytearray(s)
                d[at] = bad
                with pytest.raises(oracle.OracleError):
                    oracle.decode(bytes(d))


# --------------------------------------------------------------------------------------------------------- mutations
def test_the_pin_catches_width_and_sign_mistakes():
    """What a wrong narrowing store, a lost sign, a wrong element width or a misplaced row would deliver must not pass."""
    caught = 0
    for name in ("int16-random-x2", "uint16-ramp-x4", "int32-sentinel-x1", "uint32-random-x3", "int8-extremes-x3", "int16-constant-x3"):
        c = next(c for c in T.CASES if c.name == name)
        s, ref = decoded(c)
        p, g = ref.attributes[0], ref.attributes[-1]
        expected = T.pin_of(c)

        def multiset(values):
            return T.decoded_multiset(ref.faces, p.portable, p.point_map, values, g.point_map)
        assert T.same_multiset(multiset(g.values), expected)
        if c.dtype.itemsize > 1:
            assert not T.same_multiset(multiset(g.values & 0xFF), expected), name
            caught += 1
        if c.dtype.kind == "i":
            assert not T.same_multiset(multiset(np.abs(g.values.astype(np.int64))), expected), name
            caught += 1
        if c.dtype.itemsize == 2 and c.nc % 2 == 0:
            assert not T.same_multiset(T.oracle_multiset(ref, generic_dtype=np.dtype(c.dtype.kind + "4")), expected), name
            caught += 1
        # uint32 read as int32: all-ones and everything above 2^31 change sign
        if c.dtype == np.dtype(np.uint32) and c.pattern == "sentinel":
            assert not T.same_multiset(multiset(g.values.view(np.int32)), expected), name
            caught += 1
        if c.pattern != "constant":
            rows = g.values.copy()
            i, j = next((i, j) for i in range(len(rows)) for j in range(i + 1, len(rows)) if not np.array_equal(rows[i], rows[j]))
            rows[[i, j]] = rows[[j, i]]
            assert not T.same_multiset(multiset(rows), expected), name
            caught += 1
    assert caught >= 14
    # and in the caller's order (sequential streams): the same four against array_equal
    c = next(c for c in T.CASES if c.name == "int16-random-x2")
    gen = T.generic_of(c)
    got = oracle.decode(synth.encode_point_cloud_attributes(T.mesh(c.mesh)[0], generic=gen)).attributes[-1].values
    swapped = got.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    assert np.array_equal(got, gen)
    for wrong in (got & 0xFF, np.abs(got), np.frombuffer(got.tobytes(), np.int32).reshape(len(got), -1), swapped):
        assert not np.array_equal(wrong, gen)
