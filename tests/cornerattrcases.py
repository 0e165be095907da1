"""Meshes whose LISTED attributes (a second UV set, a colour, feature ids) are given per corner, for the encoder's corner ids
beyond normals and the first UV set (synth.Extra(corners=), dsa_encode_corner_attributes_batch), and the pin of what such a
stream must decode to, written from the contract and not from the coder:

  * a mesh is the multiset of its faces, a face the cyclically normalised triple of its corners' keys;
  * the key of a corner is the quantised position of its vertex, the octahedral normal / quantised texture coordinate of its
    normal / UV row, and of every listed attribute the row ids[corner] -- integers as they are, bit for bit, floats quantised by the
    numpy restatement of tests/meshutil.py with the bounds over ALL rows passed.

The charts of the listed attributes are chosen to differ from those of the first UV set, so that the seams do not coincide.
numpy only; deterministic."""
import collections

import numpy as np

import draco_sharp_amd.synth as synth
import irregular
import meshutil

# kinds of listed attribute: name -> (attribute type, dtype, components, normalized)
KINDS = collections.OrderedDict([
    ("uv1", (3, np.float32, 2, False)),          # a lightmap set
    ("colour", (2, np.uint8, 4, True)),
    ("fid16", (4, np.uint16, 1, False)),         # feature ids
    ("fid32", (4, np.int32, 1, False)),
])
# how an attribute is cut: a pattern of meshutil.chart_of_faces ("none": ids, no interior seam), "corner" (one row per corner: every
# edge a seam), "one-row" (every id names the same row), or None (per vertex, no ids)
Case = collections.namedtuple("Case", "name mesh charts attrs")
Case.__doc__ = "name; mesh() -> (pos, nrm, uv, faces); charts: (normal charts, uv charts) of irregular.with_seams; attrs: [(kind, cut)]"

Built = collections.namedtuple("Built", "name pos faces nrm nid uv uid extras")
Built.__doc__ = "the arguments of synth.encode_mesh_corners behind the name, and the synth.Extra list"


def _base_values(kind, pos, seed):
    """A value row per vertex, smooth enough to predict and with every byte of the element in use."""
    pos = np.asarray(pos, np.float64)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    u = (pos - lo) / np.where(hi > lo, hi - lo, 1.0)
    if kind == "uv1":
        return np.stack([0.1 + 0.3 * u[:, 1] + 0.05 * u[:, 2], 0.2 + 0.25 * u[:, 0]], axis=1).astype(np.float32)
    if kind == "colour":
        return np.stack([40 + 150 * u[:, 0], 20 + 200 * u[:, 1], 250 - 240 * u[:, 2], np.full(len(u), 255.0)], axis=1).astype(np.uint8)
    if kind == "fid16":
        return (300 + 40000 * u[:, :1] + seed).astype(np.uint16)
    if kind == "fid32":
        return (-70000 + 200000 * u[:, 1:2] - seed).astype(np.int32)
    raise ValueError(kind)


def _cut(kind, cut, pos, faces, seed):
    """(rows, ids or None) of one listed attribute."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    base = _base_values(kind, pos, seed)
    if cut is None:
        return base, None
    if cut == "corner":
        rng = np.random.default_rng(600 + seed)
        rows = base[faces.ravel()]
        if rows.dtype == np.float32:
            rows = (rows + rng.uniform(0, 0.01, rows.shape)).astype(np.float32)
        else:
            rows = (rows.astype(np.int64) + rng.integers(0, 7, rows.shape)).astype(rows.dtype)      # (wraps like the type)
        return np.ascontiguousarray(rows), np.arange(3 * len(faces), dtype=np.uint32).reshape(-1, 3)
    if cut == "one-row":
        return np.ascontiguousarray(base[:1]), np.zeros(faces.shape, np.uint32)
    chart = np.asarray(meshutil.chart_of_faces(pos, faces, cut, seed), np.int64)
    n = int(chart.max()) + 1
    key = faces * n + chart[:, None]
    uniq, inv = np.unique(key.ravel(), return_inverse=True)
    rows = base[uniq // n]
    jump = (uniq % n)[:, None]
    if rows.dtype == np.float32:
        rows = (rows + jump.astype(np.float32) * np.array([0.5, 0.25], np.float32)[None, :]).astype(np.float32)
    else:
        rows = (rows.astype(np.int64) + jump * (37 if rows.dtype.itemsize == 1 else 1000)).astype(rows.dtype)
    return np.ascontiguousarray(rows), inv.reshape(faces.shape).astype(np.uint32)


def extra_of(kind, rows, ids):
    at, _, _, normalized = KINDS[kind]
    return synth.Extra(rows, attribute_type=at, normalized=normalized, corners=ids)


_built = {}


def build(case):
    if case.name not in _built:
        pos, nrm, uv, faces = case.mesh()
        pos, faces, nrm, nid, uv, uid = irregular.with_seams(pos, nrm, uv, faces, *case.charts, seed=11)
        extras = [extra_of(kind, *_cut(kind, cut, pos, faces, 5 + k)) for k, (kind, cut) in enumerate(case.attrs)]
        _built[case.name] = Built(case.name, np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(faces, np.uint32).reshape(-1, 3), nrm, nid, uv, uid, extras)
    return _built[case.name]


def _grid(nx, ny, seed=1):
    return lambda: synth.make_mesh(synth.GRID, nx - 1, ny - 1, seed)          # nx x ny points


def _small(name):
    return lambda: irregular.mesh(name)


# grids from 3 x 3 to 33 x 17 points (561 points: more than one 256-thread block and several waves), every kind of attribute under
# every pattern, the degenerate cuts, several listed attributes with seams of their own beside seamed normals / UV0
GRIDS = [
    Case("grid3x3/uv1-single", _grid(3, 3), (None, None), [("uv1", "single")]),
    Case("grid4x3/colour-corner", _grid(4, 3), (None, "stripes"), [("colour", "corner")]),
    Case("grid5x4/fid16-one-row", _grid(5, 4), (None, None), [("fid16", "one-row")]),
    Case("grid6x5/fid32-none", _grid(6, 5), (None, "island"), [("fid32", "none")]),
    Case("grid7x7/uv1-checker+colour-random", _grid(7, 7), (None, "stripes"), [("uv1", "checker"), ("colour", "random")]),
    Case("grid9x8/colour-island+fid16-random", _grid(9, 8), ("checker", "stripes"), [("colour", "island"), ("fid16", "random")]),
    Case("grid16x9/fid32-stripes+vertex+uv1-island", _grid(16, 9), (None, "checker"), [("fid32", "stripes"), ("colour", None), ("uv1", "island")]),
    Case("grid17x16/uv1-random", _grid(17, 16), (None, "island"), [("uv1", "random")]),
    Case("grid33x17/uv1-stripes+colour-checker+fid16-island+fid32-single", _grid(33, 17), ("random", "stripes"),
         [("uv1", "checker"), ("colour", "island"), ("fid16", "random"), ("fid32", "single")]),
    Case("grid33x17/uv1-corner", _grid(33, 17), (None, None), [("uv1", "corner")]),
    Case("grid33x17/no-ids", _grid(33, 17), (None, "stripes"), [("uv1", None), ("fid16", None)]),
]
_PATTERNS = ["checker", "island", "random", "single", "stripes", "none", "corner"]
_KIND_NAMES = list(KINDS)
IRREGULAR = [Case("%s/%s-%s" % (c.name, _KIND_NAMES[k % 4], _PATTERNS[k % len(_PATTERNS)]), _small(c.name), irregular.CHARTS[k % len(irregular.CHARTS)],
                  [(_KIND_NAMES[k % 4], _PATTERNS[k % len(_PATTERNS)])] + ([(_KIND_NAMES[(k + 1) % 4], _PATTERNS[(k + 2) % len(_PATTERNS)])] if k % 2 else []))
             for k, c in enumerate(irregular.SMALL)]
CASES = GRIDS + IRREGULAR


def encode(b, opt=None, **kw):
    """The CPU coder on a Built (kw: synth.options fields)."""
    return synth.encode_mesh_corners(b.pos, b.faces, b.nrm, b.nid, b.uv, b.uid, opt=opt or synth.options(**kw), extra=b.extras)


# ------------------------------------------------------------------------------------------------------------- the pin
def _as_int(v):
    v = np.asarray(v)
    return (v.view(np.int32) if v.dtype == np.uint32 else v).astype(np.int64)


def extra_bits(e, uv_bits=10):
    return e.quantization_bits or (uv_bits if e.attribute_type == 3 else 8)


def pin(b, pos_bits=11, normal_bits=8, uv_bits=10, keep=None):
    """The face multiset [F, 3 K] int64 sorted that a stream of `b` must decode to (keep: a mask of the faces that are coded)."""
    faces = np.asarray(b.faces, np.int64).reshape(-1, 3)
    sel = np.ones(len(faces), bool) if keep is None else np.asarray(keep, bool)
    f = faces[sel]
    ids = lambda a: f if a is None else np.asarray(a, np.int64).reshape(-1, 3)[sel]      # noqa: E731
    cols = [meshutil.source_quantization(b.pos, pos_bits)[2][f.ravel()]]
    if b.nrm is not None:
        cols.append(meshutil.oct_quantize(b.nrm, normal_bits)[ids(b.nid).ravel()])
    if b.uv is not None:
        cols.append(meshutil.source_quantization(b.uv, uv_bits)[2][ids(b.uid).ravel()])
    for e in b.extras:
        rows = e.values
        q = meshutil.source_quantization(rows, extra_bits(e, uv_bits))[2] if rows.dtype == np.float32 else _as_int(rows)
        cols.append(q[ids(e.corners).ravel()])
    keys = np.concatenate(cols, axis=1)
    return meshutil.face_multiset_fast(np.arange(len(keys)).reshape(-1, 3), keys)


def decoded_multiset(faces, attributes):
    """attributes: [(values [N, K] integers, point map or an empty array)] of a decoded mesh -> its face multiset."""
    cols = []
    for values, point_map in attributes:
        values = _as_int(values)
        cols.append(values[np.asarray(point_map, np.int64)] if len(point_map) else values)
    return meshutil.face_multiset_fast(np.asarray(faces, np.int64), np.concatenate(cols, axis=1))


def oracle_multiset(ref):
    """Of an oracle.OracleMesh: integer attributes by their typed values, quantised ones by their portable integers."""
    return decoded_multiset(ref.faces, [(a.values if a.seq_type == 1 else a.portable, a.point_map) for a in ref.attributes])


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------- per-point (weld) input
def unweld(b, rng):
    """One shuffled row per distinct (vertex, normal row, UV row, row of every listed attribute) of a Built:
    -> (pos [P,3], faces over points, normals or None, uvs or None, [extra arrays with one row per point])."""
    faces = np.asarray(b.faces, np.int64).reshape(-1, 3)
    ids = lambda a: faces.ravel() if a is None else np.asarray(a, np.int64).ravel()      # noqa: E731
    cols = [faces.ravel(), ids(b.nid if b.nrm is not None else None), ids(b.uid if b.uv is not None else None)] + [ids(e.corners) for e in b.extras]
    uniq, inv = np.unique(np.stack(cols, axis=1), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    place = rng.permutation(len(uniq))

    def rows(values, col):
        if values is None:
            return None
        values = np.asarray(values)
        out = np.empty((len(uniq),) + values.shape[1:], values.dtype)
        out[place] = values[uniq[:, col]]
        return np.ascontiguousarray(out)
    extra = [rows(e.values, 3 + k) for k, e in enumerate(b.extras)]
    return rows(b.pos, 0), place[inv].reshape(-1, 3).astype(np.uint32), rows(b.nrm, 1), rows(b.uv, 2), extra


def point_extras(b, arrays):
    """The Extras of a Built over per-point arrays (no ids)."""
    return [synth.Extra(a, attribute_type=e.attribute_type, normalized=bool(e.normalized)) for e, a in zip(b.extras, arrays)]


def with_listed(m, attrs, seed=40):
    """A mesh in the form of seamdefects.Seamed (name, pos, faces, nrm, nid, uv, uid) with listed attributes [(kind, cut)] -> Built."""
    extras = [extra_of(kind, *_cut(kind, cut, m.pos, m.faces, seed + k)) for k, (kind, cut) in enumerate(attrs)]
    return Built(m.name, np.ascontiguousarray(m.pos, np.float32), np.ascontiguousarray(m.faces, np.uint32).reshape(-1, 3), m.nrm, m.nid, m.uv, m.uid, extras)
