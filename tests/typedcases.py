"""Integer attributes of every element type the bitstream allows below 64 bits (int8, uint8, int16, uint16, int32, uint32: joint
indices, 16-bit colours, feature and batch ids with an all-ones "none" value, scan labels): value generators, the fixed list of
cases the CPU and the GPU tests share, and the pin (generators and pin: tools/typedvalues.py, which the randomised tools use too).  Integer attributes are lossless, so the expectation is the INPUT array
itself, bit for bit -- not the oracle, which the writer's author wrote as well.

32-bit values stay within +-2^27 as int32 (the all-ones value is -1): the sum of four parallelogram predictions then fits
int32.  Beyond that the wrap transform of the reference leans on overflow the language defines, which is not the subject."""
import collections

import numpy as np

import os
import sys

import irregular
import draco_sharp_amd.synth as synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

from typedvalues import (DTYPES, DATA_TYPE, PATTERNS, LIMIT32, bounds, all_ones, _cast, values, pin, decoded_multiset,      # noqa: F401
                         same_multiset, device_multiset)


# ------------------------------------------------------------------------------------------------------------ meshes
KINDS = [(0, 9, 7), (1, 8, 6), (2, 8, 7), (3, 20, 16), (4, 9, 6), (0, 40, 33), (1, 24, 40)]       # test_gpu_parity.KINDS
_meshes = {}


def mesh_names():
    return ["kind%d" % k for k in range(len(KINDS))] + ["shuffled-" + c.name for c in irregular.SMALL]


def mesh(name):
    """(pos, nrm, uv, faces) of a small synthetic mesh of test_gpu_parity.KINDS or of a small shuffled case of irregular.py,
    built once per process."""
    if name not in _meshes:
        if name.startswith("kind"):
            kind, nx, ny = KINDS[int(name[4:])]
            _meshes[name] = synth.make_mesh(kind, nx, ny, 61)
        else:
            _meshes.update(("shuffled-" + n, m) for n, m in irregular.shuffled_small())
    return _meshes[name]


Case = collections.namedtuple("Case", "name mesh dtype pattern nc")


def _cases():
    out = []
    names = mesh_names()
    for dtype in DTYPES:
        for pattern in PATTERNS:
            for nc in (1, 2, 3, 4):
                # (the largest mesh for the 16-bit random rows of 3 and 4: more than SYM_MAX_LDS values, nearly all distinct)
                big = dtype.itemsize == 2 and pattern == "random" and nc >= 3
                out.append(Case("%s-%s-x%d" % (dtype.name, pattern, nc), "kind5" if big else names[(5 * len(out) + 3) % len(names)], dtype, pattern, nc))
    out.append(Case("int16-constant-x3", "kind3", np.dtype(np.int16), "constant", 3))
    out.append(Case("uint32-constant-zero-x1", "shuffled-fan-open", np.dtype(np.uint32), "constant-zero", 1))
    out.append(Case("uint16-joints-x4", "kind5", np.dtype(np.uint16), "joints", 4))
    return out


CASES = _cases()
_values = {}


def generic_of(case):
    """The input array of a case, built once and never written to."""
    if case.name not in _values:
        v = values(case.dtype, case.pattern, len(mesh(case.mesh)[0]), case.nc, seed=[c.name for c in CASES].index(case.name))
        v.setflags(write=False)
        _values[case.name] = v
    return _values[case.name]


def raw_scheme_legal(case):
    """The raw symbol scheme takes symbols below 2^18: every 8- and 16-bit attribute, and the 32-bit ones whose corrections stay
    small (the wrap transform measures them from the smallest value present)."""
    return case.dtype.itemsize < 4 or case.pattern in ("ramp", "sentinel", "constant", "constant-zero")


def raw_width_fits(case, width):
    """Uncompressed integers at `width` bytes hold zig-zagged wrapped corrections: those reach max - min of the values (as int32),
    no further (corrections lie within +-(max - min + 1) / 2, the positive end one short where that is even)."""
    if width >= 4:
        return True
    v = generic_of(case).astype(np.int64) if case.dtype != np.dtype(np.uint32) else generic_of(case).view(np.int32).astype(np.int64)
    return int(v.max()) - int(v.min()) < (1 << (8 * width))


def encode(case, opt=None, normals=True, uvs=True):
    """The Edgebreaker stream of a case: positions, (normals, texture coordinates,) the typed generic attribute."""
    pos, nrm, uv, faces = mesh(case.mesh)
    o = dict(generic_components=case.nc)
    o.update(opt or {})
    return synth.encode_mesh(pos, faces, nrm if normals else None, uv if uvs else None, generic=generic_of(case), opt=synth.options(**o))


# --------------------------------------------------------------------------------------------------------------- pin
def pin_of(case, pos_bits=11):
    pos, nrm, uv, faces = mesh(case.mesh)
    return pin(pos, faces, generic_of(case), pos_bits)


def oracle_multiset(ref, generic_dtype=None):
    """decoded_multiset of an oracle.OracleMesh (first attribute: positions, last: the generic one).  generic_dtype: read the
    stored value bytes as that type instead of the descriptor's (the mutation tests)."""
    p, g = ref.attributes[0], ref.attributes[-1]
    gv = g.values if generic_dtype is None else np.frombuffer(g.values.tobytes(), generic_dtype).reshape(g.num_entries, -1)
    return decoded_multiset(ref.faces, p.portable, p.point_map, gv, g.point_map)


# ---------------------------------------------------------------------------------------------------------- refusals
def descriptor_streams(case):
    """[(stream, offset of the data type byte in the generic attribute's descriptor)]: an Edgebreaker stream of positions and the
    typed attribute (descriptor {type 4, data type, components, normalized 0, unique id 1} and decoder type 1 behind it, found by
    search and required to be the only match), and a point cloud, whose head has a fixed layout (11 bytes of header, int32
    points, one decoder, attribute count, the 5-byte descriptor of the positions)."""
    pos, nrm, uv, faces = mesh(case.mesh)
    gen = generic_of(case)
    eb = synth.encode_mesh(pos, faces, None, None, generic=gen, opt=synth.options(generic_components=case.nc))
    needle = bytes([4, DATA_TYPE[case.dtype], case.nc, 0, 1, 1])
    assert eb.count(needle) == 1
    cloud = synth.encode_point_cloud_attributes(pos, generic=gen)
    at = 11 + 4 + 1 + 1 + 5 + 1
    assert cloud[at - 1:at + 4] == needle[:5]
    return [(eb, eb.index(needle) + 1), (cloud, at)]
