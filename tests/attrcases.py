"""Attribute lists (extras behind the built-in attributes) for the CPU and the GPU tests of the encoder's attribute list: the
skinned-vertex set (uint16 x 4 joints, float32 x 4 weights, uint8 x 3 normalised colour), the numpy pin of a quantised float
attribute, and the comparison of a decoded stream with the INPUT arrays."""
import numpy as np

import irregular
import meshutil
import typedcases as T
import draco_sharp_amd.synth as synth

GRIDS = ["kind0", "kind3"]
SHUFFLED = ["shuffled-grid-flipped", "shuffled-holes-thickened"]
MESHES = GRIDS + SHUFFLED
assert all(n in T.mesh_names() for n in MESHES) and len(irregular.SMALL) >= 6

WEIGHT_BITS = 8
JOINTS_ID, WEIGHTS_ID, COLOUR_ID = 40, 7, 1000          # unique ids a caller chose (no order, none the attribute's index)

_sets = {}


def skinned(name):
    """[(array, Extra keywords)] for mesh `name`: joints, weights, colour; built once and never written to."""
    if name not in _sets:
        nv = len(T.mesh(name)[0])
        rng = np.random.default_rng([17, len(name), nv])
        joints = np.sort(rng.integers(0, 900, (nv, 4)), axis=1).astype(np.uint16)
        w = rng.random((nv, 4)).astype(np.float32)
        weights = (w / w.sum(axis=1, keepdims=True)).astype(np.float32)
        colour = rng.integers(0, 256, (nv, 3)).astype(np.uint8)
        for a in (joints, weights, colour):
            a.setflags(write=False)
        _sets[name] = [(joints, dict(attribute_type=4, unique_id=JOINTS_ID)),
                       (weights, dict(attribute_type=4, unique_id=WEIGHTS_ID, quantization_bits=WEIGHT_BITS)),
                       (colour, dict(attribute_type=2, normalized=True, unique_id=COLOUR_ID))]
    return _sets[name]


def synth_extras(items):
    return [synth.Extra(a, **kw) for a, kw in items]


def float_pin(values, bits):
    """(min[c], range, quantised ints, dequantised float32) of a float32 attribute by the rules of the independent pin
    (meshutil.source_quantization): min / range / floor(x * (max_q / range) + 0.5) in float32, and the decoder's
    q * (range / max_q) + min, every step rounded to float32."""
    v = np.asarray(values, np.float32).reshape(len(values), -1)
    mn, rng, q = meshutil.source_quantization(v, bits)
    delta = np.float32(rng / np.float32((1 << bits) - 1))
    deq = ((q.astype(np.float32) * delta).astype(np.float32) + mn).astype(np.float32)
    return mn, rng, q, deq


def expected_bits(att_type, bits, uv_bits=10):
    return bits if bits else (uv_bits if att_type == 3 else 8)


def check_descriptor(att, array, kw, index, uv_bits=10):
    """att: an oracle attribute or a decoded dsa attribute info turned into the same names."""
    array = np.asarray(array)
    is_float = array.dtype == np.float32
    assert att.att_type == kw.get("attribute_type", 4)
    assert att.data_type == (9 if is_float else T.DATA_TYPE[array.dtype])
    assert att.num_components == array.reshape(len(array), -1).shape[1]
    assert att.normalized == (0 if is_float else int(kw.get("normalized", False)))
    uid = kw.get("unique_id")
    assert att.unique_id == (index if uid is None else uid)
    assert att.seq_type == (2 if is_float else 1)
    if is_float:
        assert att.q_bits == expected_bits(att.att_type, kw.get("quantization_bits", 0), uv_bits)


def expected_rows(array, kw, uv_bits=10):
    """Per vertex what the stream must return for an extra: (integer key rows for the multiset, exact value rows)."""
    array = np.asarray(array).reshape(len(array), -1)
    if array.dtype == np.float32:
        _, _, q, deq = float_pin(array, expected_bits(kw.get("attribute_type", 4), kw.get("quantization_bits", 0), uv_bits))
        return q.astype(np.int64), deq
    return array.astype(np.int64), array


def check_linear(ref, pos, items, first, uv_bits=10):
    """A sequential stream (point i is row i): extras `items` are the oracle's attributes first .. in the caller's order."""
    assert len(ref.attributes) == first + len(items)
    for k, (array, kw) in enumerate(items):
        att = ref.attributes[first + k]
        check_descriptor(att, array, kw, first + k, uv_bits)
        keys, exact = expected_rows(array, kw, uv_bits)
        assert len(att.point_map) == 0
        assert np.array_equal(att.portable.astype(np.int64), keys if exact.dtype == np.float32 else as_int32(exact)), k
        assert att.values.dtype == exact.dtype and att.values.tobytes() == np.ascontiguousarray(exact).tobytes(), k
        if exact.dtype == np.float32:
            mn, rng, _, _ = float_pin(array, att.q_bits)
            assert np.array_equal(np.asarray(att.q_min[:len(mn)], np.float32), mn) and np.float32(att.q_range) == rng


def as_int32(v):
    v = np.asarray(v)
    return (v.view(np.int32) if v.dtype == np.uint32 else v).astype(np.int64)


def check_connected(faces_out, atts, pos, faces, items, first, uv_bits=10, pos_bits=11):
    """An Edgebreaker stream: the multiset of face corners keyed by (quantised position, every extra's row) equals the one of the
    input; per entry the typed values are the exact rows.  atts: [(descriptor, typed values, portable, point map)]."""
    assert len(atts) == first + len(items)
    npnt = int(np.asarray(faces_out).max()) + 1
    ident = np.arange(npnt, dtype=np.int64)

    def per_point(vals, pmap):
        return np.asarray(vals)[np.asarray(pmap, np.int64) if pmap is not None and len(pmap) else ident]
    qp = meshutil.source_quantization(pos, pos_bits)[2]
    want, got = [qp], [per_point(atts[0][2], atts[0][3]).astype(np.int64)]
    for k, (array, kw) in enumerate(items):
        desc, values, portable, pmap = atts[first + k]
        check_descriptor(desc, array, kw, first + k, uv_bits)
        keys, exact = expected_rows(array, kw, uv_bits)
        want.append(keys)
        if exact.dtype == np.float32:
            got.append(per_point(portable, pmap).astype(np.int64))
            # every decoded float is the numpy dequantisation of its integer
            mn, rng, _, _ = float_pin(array, desc.q_bits)
            delta = np.float32(rng / np.float32((1 << desc.q_bits) - 1))
            deq = ((np.asarray(portable).astype(np.float32) * delta).astype(np.float32) + mn).astype(np.float32)
            assert np.asarray(values).dtype == np.float32 and np.asarray(values).tobytes() == deq.tobytes(), k
            assert np.array_equal(np.asarray(desc.q_min[:len(mn)], np.float32), mn) and np.float32(desc.q_range) == rng
        else:
            assert np.asarray(values).dtype == exact.dtype, k
            got.append(per_point(values, pmap).astype(np.int64))
    expected = meshutil.face_multiset_fast(faces, np.concatenate(want, axis=1))
    found = meshutil.face_multiset_fast(faces_out, np.concatenate(got, axis=1))
    assert found.shape == expected.shape and np.array_equal(found, expected)


def oracle_atts(ref):
    return [(a, a.values, a.portable, a.point_map) for a in ref.attributes]


# the five stream kinds the attribute list goes through: name -> (CPU coder call, device Config keywords, point cloud)
def cpu_stream(kind, name, items, generic=None, normals=True, uvs=True, opt=None):
    pos, nrm, uv, faces = T.mesh(name)
    nrm, uv = (nrm if normals else None), (uv if uvs else None)
    extra = synth_extras(items)
    o = dict(opt or {})
    if kind == "edgebreaker":
        return synth.encode_mesh(pos, faces, nrm, uv, generic=generic, opt=synth.options(**o), extra=extra)
    if kind == "valence":
        return synth.encode_mesh(pos, faces, nrm, uv, generic=generic, opt=synth.options(predictive_connectivity=2, **o), extra=extra)
    if kind == "sequential-raw":
        return synth.encode_sequential(pos, faces, nrm, uv, generic, compressed=False, opt=synth.options(**o), extra=extra)
    if kind == "sequential-compressed":
        return synth.encode_sequential(pos, faces, nrm, uv, generic, compressed=True, opt=synth.options(**o), extra=extra)
    if kind == "cloud":
        return synth.encode_point_cloud_attributes(pos, nrm, uv, generic, opt=synth.options(**o), extra=extra)
    raise ValueError(kind)


KINDS = ["edgebreaker", "valence", "sequential-raw", "sequential-compressed", "cloud"]


# ------------------------------------------------------------------------------------------------ alphabet edges
def residue_walk(span, nv, nc, dtype, base=100):
    """(nv, nc) array of `dtype` with values base .. base + span (base >= 0) whose wrapped differences along every component, in
    row order, take every residue modulo span + 1: on a sequential stream (Difference prediction, entry i = row i) the attribute
    has exactly span + 1 distinct symbols, 0 .. span.  The residues 1 .. span are dealt over the components in turn; each
    component starts at base (correction 0 against the clamped zero prediction) and steps by its residues modulo span + 1."""
    m = span + 1
    per = 1 + (span + nc - 1) // nc
    assert per + 2 <= nv and base >= 0
    x = np.zeros((nv, nc), np.int64)
    for c in range(nc):
        steps = np.arange(1 + c, span + 1, nc, dtype=np.int64)
        chain = np.concatenate([[0], np.cumsum(steps) % m])
        x[:len(chain), c] = chain
        x[len(chain):, c] = chain[-1]
    x[nv - 2, 0], x[nv - 1, 0] = span, 0          # both ends of the range are present (their residues are in the set already)
    return np.ascontiguousarray((x + base).astype(dtype))


def largest_symbol_values(span, nv, first):
    """(nv, 1) int32 values 0 .. span whose first entry is `first` (its correction against the zero prediction is `first`
    wrapped) and whose range is exactly span."""
    rng = np.random.default_rng([span, nv])
    x = rng.integers(0, span + 1, (nv, 1), dtype=np.int64)
    x[0, 0], x[1, 0], x[2, 0] = first, 0, span
    return np.ascontiguousarray(x.astype(np.int32))
