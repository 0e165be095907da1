"""Meshes that are not clean AND carry normals / texture coordinates per corner -- UV charts and hard edges over a doubled face,
a fin, a sliver with a repeated index, a bow-tie, a two-sided sheet -- for the encoder's topology repair with corner attributes
(synth.options(repair_topology=2), dsa_encode_seam_repair_batch with corner_repair = 1), and the pin of what such a mesh must
decode to, written from the contract and not from the coder:

  * degenerate faces (two equal indices) are dropped, with their ids;
  * every row passed is quantised with the numpy restatements of tests/meshutil.py, the bounds over ALL rows of an array;
  * a mesh is the multiset of its faces, a face the cyclically normalised triple of (quantised position of the corner's vertex
    row, octahedral normal of its normal row, quantised texture coordinate of its UV row).  A vertex the repair made carries its
    parent's row and a corner keeps its ids, so the multiset of the repaired mesh is that of the input's faces.

The defects of tests/defects.py are injected with the ids carried along: a new face takes the ids of the face it was made from, a
flip reverses the ids with the indices, a pinch leaves the ids alone.  numpy only; the generators are deterministic (seeded)."""
import collections

import numpy as np

import defects
from meshutil import chart_of_faces, source_corner_faces_seamed, split_by_chart

Seamed = collections.namedtuple("Seamed", "name pos faces nrm nid uv uid")      # the arguments of synth.encode_mesh_corners behind the name (ids None: per vertex)

ID_KINDS = ("vertex", "corner", "stripes")
# the stream dialects every mesh is coded in: the default level; valence Edgebreaker with TexCoordsPortable and GeometricNormal;
# ConstrainedMultiParallelogram with every decoder in prediction-degree order; all of it at once
OPTIONS = (dict(),
           dict(predictive_connectivity=2, uv_prediction=5, normal_prediction=6),
           dict(pos_prediction=4, uv_prediction=4, traversal_method=2),
           dict(predictive_connectivity=2, pos_prediction=4, uv_prediction=5, normal_prediction=6, traversal_method=1))
CHARTS = ((None, "stripes"), (None, "checker"), (None, "random"), ("checker", "island"), ("random", "stripes"))


def _unit(n):
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)


def with_ids(c, kind, seed=0):
    """A defects.Defect (nv, faces) with values and ids of one kind: 'vertex' ids equal to the indices (ids per corner, no seam),
    'corner' one row per (face, corner) (every edge a seam), 'stripes' chart_of_faces stripes over the positions."""
    faces = np.asarray(c.faces, np.uint32).reshape(-1, 3)
    pos, nrm, uv, _, _ = defects.attributes(c.nv, seed)
    if kind == "vertex":
        nid, uid = faces.copy(), faces.copy()
    elif kind == "corner":
        rng = np.random.default_rng(4000 + seed + 3 * len(faces))
        nid = np.arange(3 * len(faces), dtype=np.uint32).reshape(-1, 3)
        uid = nid.copy()
        nrm, uv = _unit(rng.normal(size=(3 * len(faces), 3))), rng.random((3 * len(faces), 2)).astype(np.float32)
    elif kind == "stripes":
        chart = chart_of_faces(pos, faces, "stripes")
        nid, nrm = split_by_chart(faces, nrm, chart, [0.0, 0.0, 0.0])
        nrm = _unit(nrm + (np.arange(len(nrm)) % 3)[:, None].astype(np.float32) * np.float32(0.4))
        uid, uv = split_by_chart(faces, uv, chart, [1.5, 0.25])
    else:
        raise ValueError(kind)
    return Seamed("%s/%s" % (c.name, kind), pos, faces, nrm, nid, uv, uid)


def inject(m, kind, count, rng):
    """defects.inject with the ids carried along: -> Seamed.  double / fin: the new face has the ids of the face it copies / stands
    on; flip: ids reversed with the indices; degenerate: the new face has the ids of the face at whose place it is put; isolated: a
    position row more, no id names anything new; pinch: the indices change, the ids stay."""
    faces = np.array(m.faces, np.int64).reshape(-1, 3)
    ids = [None if a is None else np.array(a, np.int64).reshape(-1, 3) for a in (m.nid, m.uid)]
    pos = np.asarray(m.pos, np.float32)
    nv = len(pos)
    for _ in range(count):
        k = int(rng.integers(0, len(faces)))
        if kind == "double":
            faces = np.concatenate([faces, faces[k:k + 1]])
            ids = [None if a is None else np.concatenate([a, a[k:k + 1]]) for a in ids]
        elif kind == "fin":
            faces = np.concatenate([faces, [[faces[k, 0], faces[k, 1], int(rng.integers(0, nv))]]])
            ids = [None if a is None else np.concatenate([a, a[k:k + 1]]) for a in ids]
        elif kind == "flip":
            faces[k] = faces[k][::-1]
            for a in ids:
                if a is not None:
                    a[k] = a[k][::-1]
        elif kind == "degenerate":
            v = int(rng.integers(0, nv))
            faces = np.insert(faces, k, [v, int(rng.integers(0, nv)), v], axis=0)
            ids = [None if a is None else np.insert(a, k, a[min(k, len(a) - 1)], axis=0) for a in ids]
        elif kind == "isolated":
            nv += 1
            pos = np.concatenate([pos, rng.random((1, 3)).astype(np.float32)])
        elif kind == "pinch":
            a, b = int(rng.integers(0, nv)), int(rng.integers(0, nv))
            faces[faces == b] = a
        else:
            raise ValueError(kind)
    # an attribute without ids is per vertex: it needs a row for every vertex there is now
    nrm, uv = m.nrm, m.uv
    if ids[0] is None and nrm is not None and len(nrm) < nv:
        nrm = np.concatenate([nrm, np.tile(np.array([[0, 0, 1]], np.float32), (nv - len(nrm), 1))])
    if ids[1] is None and uv is not None and len(uv) < nv:
        uv = np.concatenate([uv, np.zeros((nv - len(uv), 2), np.float32)])
    u32 = lambda a: None if a is None else np.ascontiguousarray(a, np.uint32)      # noqa: E731
    return Seamed("%s+%d-%s" % (m.name, count, kind), pos, u32(faces), nrm, u32(ids[0]), uv, u32(ids[1]))


def seamed_source(synth, kind_name, kind, nx, ny, charts, seed):
    from meshutil import seamed_mesh
    pos, faces, nrm, nid, uv, uid = seamed_mesh(synth, kind, nx, ny, seed, *charts)
    faces = np.asarray(faces, np.uint32).reshape(-1, 3)
    r = lambda a: None if a is None else np.asarray(a, np.uint32).reshape(-1, 3)      # noqa: E731
    return Seamed("%s/%s-%s" % (kind_name, charts[0], charts[1]), pos, faces, nrm, r(nid), uv, r(uid))


def soup_with_ids(c, k):
    """A defects.soups mesh with seeded random ids into 2 - 6 rows (every third mesh: the normals per vertex, without ids): almost
    every edge two faces share is a seam."""
    rng = np.random.default_rng(9000 + k)
    faces = np.asarray(c.faces, np.uint32).reshape(-1, 3)
    pos = defects.attributes(c.nv, k)[0]
    rows_n, rows_u = int(rng.integers(2, 7)), int(rng.integers(2, 7))
    nid = rng.integers(0, rows_n, faces.shape).astype(np.uint32)
    uid = rng.integers(0, rows_u, faces.shape).astype(np.uint32)
    if k % 3 == 0:
        nid, rows_n = None, c.nv
    return Seamed(c.name, pos, faces, _unit(rng.normal(size=(rows_n, 3))), nid, rng.random((rows_u, 2)).astype(np.float32), uid)


def pin(m, pos_bits=11, normal_bits=8, uv_bits=10):
    """(the face multiset the stream must decode to [F', 3 K] int64 sorted, (position min, range, uv min, range))"""
    keep = ~defects.is_degenerate(m.faces)
    f = np.asarray(m.faces, np.int64).reshape(-1, 3)[keep]
    nid = None if m.nid is None else np.asarray(m.nid, np.int64).reshape(-1, 3)[keep]
    uid = None if m.uid is None else np.asarray(m.uid, np.int64).reshape(-1, 3)[keep]
    return source_corner_faces_seamed(m.pos, f, m.nrm, nid, m.uv, uid, pos_bits, normal_bits, uv_bits)


def encode(synth, m, **opt):
    return synth.encode_mesh_corners(m.pos, m.faces, m.nrm, m.nid, m.uv, m.uid, opt=synth.options(**opt))


def header_counts(stream):
    """(vertices, faces) as an Edgebreaker stream's header says them: the two varints behind the 11 bytes of the file header (no
    metadata) and the traversal byte."""
    assert stream[:5] == b"DRACO" and stream[7:9] == b"\x01\x01" and not stream[10] & 0x80
    out, at = [], 12
    for _ in range(2):
        v = shift = 0
        while True:
            b = stream[at]
            at += 1
            v |= (b & 0x7F) << shift
            shift += 7
            if not b & 0x80:
                break
        out.append(v)
    return tuple(out)


def check(oracle, stream, m, points=None):
    """The stream decodes in the oracle to the pin; its header counts (points: V' - isolated, where the caller knows it; F -
    degenerate) and quantisation parameters.  -> the decoded mesh"""
    want, (pmin, prange, umin, urange) = pin(m)
    d = oracle.decode(stream)
    assert d.end_pos == len(stream), m.name
    assert d.num_faces == len(want) == int((~defects.is_degenerate(m.faces)).sum()) == header_counts(stream)[1], m.name
    if points is not None:
        assert header_counts(stream)[0] == points, m.name
    got = defects.decoded(d.faces, [(a.portable, a.point_map) for a in d.attributes])
    assert got.shape == want.shape and np.array_equal(got, want), m.name
    assert np.array_equal(np.asarray(d.attributes[0].q_min[:3], np.float32), pmin) and np.float32(d.attributes[0].q_range) == prange, m.name
    if umin is not None:
        au = d.attributes[-1]
        assert np.array_equal(np.asarray(au.q_min[:2], np.float32), umin) and np.float32(au.q_range) == urange, m.name
    return d
