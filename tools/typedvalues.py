"""Integer attributes of every element type the bitstream allows below 64 bits (int8, uint8, int16, uint16, int32, uint32): the
value generators and the pin that tests/typedcases.py and the randomised tools (soak.py, dialect_matrix.py) share.  They live beside
the tools, which the suite of any revision runs, and are numpy only; tests/typedcases.py has the list of cases and says more.

32-bit values stay within +-2^27 as int32 (the all-ones value is -1): the sum of four parallelogram predictions then fits int32."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import meshutil          # noqa: E402

DTYPES = [np.dtype(t) for t in (np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32)]
DATA_TYPE = {np.dtype(np.int8): 1, np.dtype(np.uint8): 2, np.dtype(np.int16): 3, np.dtype(np.uint16): 4, np.dtype(np.int32): 5,
             np.dtype(np.uint32): 6}                        # Draco's ids
PATTERNS = ("random", "ramp", "extremes", "sentinel")
LIMIT32 = 1 << 27


def bounds(dtype):
    """(lo, hi) the generators use: the type's range, 32-bit types within +-2^27 as int32."""
    dtype = np.dtype(dtype)
    info = np.iinfo(dtype)
    if dtype.itemsize < 4:
        return int(info.min), int(info.max)
    return (-LIMIT32, LIMIT32 - 1) if dtype.kind == "i" else (0, LIMIT32 - 1)


def all_ones(dtype):
    return -1 if np.dtype(dtype).kind == "i" else int(np.iinfo(dtype).max)


def _cast(v, dtype):
    """int64 -> dtype keeping the low bits (C conversion), whatever numpy's casting rules of the day."""
    dtype = np.dtype(dtype)
    return (np.asarray(v, np.int64) & ((1 << (8 * dtype.itemsize)) - 1)).astype(np.uint64).astype("<u%d" % dtype.itemsize).view(dtype)


def values(dtype, pattern, nv, nc, seed=0):
    """(nv, nc) array of `dtype`, deterministic.
    random: uniform over bounds(dtype) -- dense alphabets as large as they get; beyond 18 bits for the 32-bit types (tagged scheme)
    ramp: 3 * vertex + 1000 * component + lo / 2 -- small corrections (raw scheme), negative for signed types
    extremes: only lo, hi, 0, 1 and (signed) -1 -- the corrections wrap
    sentinel: ids vertex % 500, one entry in eight all-ones
    constant / constant-zero: one value everywhere (a negative one where the type has them)
    joints: values 0 .. 63, each row sorted (joint indices)"""
    dtype = np.dtype(dtype)
    lo, hi = bounds(dtype)
    rng = np.random.default_rng([seed, DATA_TYPE[dtype], nc, len(pattern)])
    vid = np.arange(nv, dtype=np.int64)[:, None]
    comp = np.arange(nc, dtype=np.int64)[None, :]
    if pattern == "random":
        v = rng.integers(lo, hi + 1, (nv, nc), dtype=np.int64)
    elif pattern == "ramp":
        v = 3 * vid + 1000 * comp + lo // 2
    elif pattern == "extremes":
        pool = np.array([lo, hi, 0, 1] + ([-1] if dtype.kind == "i" else []), np.int64)
        v = pool[rng.integers(0, len(pool), (nv, nc))]
    elif pattern == "sentinel":
        v = np.broadcast_to(vid % 500, (nv, nc)).copy()
        v[rng.integers(0, 8, (nv, nc)) == 0] = all_ones(dtype)
    elif pattern == "constant":
        v = np.full((nv, nc), -12345 if dtype.kind == "i" else 12345, np.int64)
    elif pattern == "constant-zero":
        v = np.zeros((nv, nc), np.int64)
    elif pattern == "joints":
        v = np.sort(rng.integers(0, 64, (nv, nc), dtype=np.int64), axis=1)
    else:
        raise ValueError(pattern)
    return np.ascontiguousarray(_cast(v, dtype))


# --------------------------------------------------------------------------------------------------------------- pin
def pin(pos, faces, generic, pos_bits=11):
    """What an Edgebreaker stream of this input must decode to, from the input alone: the multiset of face corners keyed by
    (quantised position, generic row), rotation-canonical and sorted (meshutil.face_multiset_fast).  The generic values enter as
    the numbers they are (uint32 4294967295 is not int32 -1)."""
    qp = meshutil.source_quantization(pos, pos_bits)[2]
    g = np.asarray(generic)
    keys = np.concatenate([qp, g.reshape(len(g), -1).astype(np.int64)], axis=1)
    return meshutil.face_multiset_fast(faces, keys)


def decoded_multiset(faces, positions, position_map, generic, generic_map):
    """The same multiset from decoded arrays: faces [F,3] of point ids, the integer positions per entry, the typed generic values
    per entry, and the point -> entry maps of both (None or empty: identity)."""
    def per_point(vals, pmap):
        vals = np.asarray(vals)
        return vals if pmap is None or len(pmap) == 0 else vals[np.asarray(pmap, np.int64)]
    keys = np.concatenate([per_point(positions, position_map).astype(np.int64), per_point(generic, generic_map).astype(np.int64)], axis=1)
    return meshutil.face_multiset_fast(faces, keys)


def same_multiset(got, expected):
    return got.shape == expected.shape and np.array_equal(got, expected)


def device_multiset(mesh_data):
    """decoded_multiset of a decoded dsa mesh (ConnectedData)."""
    p, g = mesh_data.Attributes[0], mesh_data.Attributes[-1]
    return decoded_multiset(mesh_data.Faces, p.PortableValues, p.PointMap, g.Values, g.PointMap)
