"""Meshes given as one row per point, for the weld in front of the Edgebreaker encoder (synth.weld_points, the kernels of
dsa_encode_weld.h, dsa_weld_batch / dsa_encode_points_batch): the generator that unwelds a seamed mesh, the numpy pin of the weld,
and the cases every test of the weld runs.

The pin is written from the rule alone: a point is used when a face names it; used points whose rows are equal byte for byte
in every array that stays per vertex are one vertex; the representative of a class is its point of smallest index, classes are
numbered by ascending representative; normals and texture coordinates likewise, each alone; an attribute no vertex has two rows
of is handed on per vertex."""
import collections

import numpy as np

import draco_sharp_amd.synth as synth
import irregular

INVALID = 0xFFFFFFFF


def unweld(pos, faces, nrm, nid, uv, uid, rng):
    """One shuffled row per distinct (vertex, normal row, uv row) of a mesh in the form of synth.encode_mesh_corners (ids None: the
    vertex's).  Returns (pos[P,3], faces[F,3] over points, normals[P,3] or None, uvs[P,2] or None)."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    nid = faces if nid is None else np.asarray(nid, np.int64).reshape(-1, 3)
    uid = faces if uid is None else np.asarray(uid, np.int64).reshape(-1, 3)
    triples = np.stack([faces.ravel(), nid.ravel() if nrm is not None else faces.ravel(), uid.ravel() if uv is not None else faces.ravel()], axis=1)
    uniq, inv = np.unique(triples, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    place = rng.permutation(len(uniq))                    # point of triple j
    def rows(values, col):
        if values is None:
            return None
        out = np.empty((len(uniq), np.asarray(values).shape[1]), np.float32)
        out[place] = np.asarray(values, np.float32)[uniq[:, col]]
        return out
    return rows(pos, 0), place[inv].reshape(-1, 3).astype(np.uint32), rows(nrm, 1), rows(uv, 2)


def _classes(arrays, used):
    """(class of every point or INVALID, representative of every class): byte-equal rows, first-occurrence numbering."""
    P = len(used)
    idx = np.flatnonzero(used)
    of = np.full(P, INVALID, np.uint32)
    if len(idx) == 0:
        return of, np.zeros(0, np.uint32)
    key = np.concatenate([np.ascontiguousarray(a).reshape(P, -1).view(np.uint8).reshape(P, -1) for a in arrays], axis=1)[idx]
    if key.shape[1] % 4 == 0:
        key = np.ascontiguousarray(key).view(np.uint32)
    _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(first), np.int64)
    rank[order] = np.arange(len(first))
    of[idx] = rank[inv]
    return of, idx[first[order]].astype(np.uint32)


def pin(pos, faces, normals=None, uvs=None, generic=None, extra=()):
    """The weld in numpy; the fields of synth.Welded as a namespace."""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    P = len(pos)
    if len(faces) and faces.max() >= P:
        raise ValueError("face index out of range")
    used = np.zeros(P, bool)
    used[faces.ravel()] = True
    per_vertex = [pos] + ([np.asarray(generic).reshape(P, -1)] if generic is not None else []) + [np.asarray(e).reshape(P, -1) for e in extra]
    w = collections.namedtuple("Pin", "vertex_of_point vertex_point normal_of_point normal_point texcoord_of_point texcoord_point faces "
                               "normal_corners uv_corners normals uvs pos generic extra normals_per_vertex texcoords_per_vertex")
    vof, vpoint = _classes(per_vertex, used)
    out = dict(vertex_of_point=vof, vertex_point=vpoint, faces=vof[faces].astype(np.uint32).reshape(-1, 3), pos=pos[vpoint],
               generic=None if generic is None else np.asarray(generic).reshape(P, -1)[vpoint], extra=[np.asarray(e).reshape(P, -1)[vpoint] for e in extra])
    for name, values, short in (("normal", normals, "normals"), ("texcoord", uvs, "uvs")):
        corners = "normal_corners" if name == "normal" else "uv_corners"
        if values is None:
            out.update({name + "_of_point": None, name + "_point": None, corners: None, short: None, short.replace("uvs", "texcoords") + "_per_vertex": True})
            continue
        values = np.ascontiguousarray(values, np.float32).reshape(P, -1)
        of, point = _classes([values], used)
        u = np.flatnonzero(used)
        same = bool((of[u] == of[vpoint[vof[u]]]).all())
        out.update({name + "_of_point": of, name + "_point": point, short.replace("uvs", "texcoords") + "_per_vertex": same,
                    corners: None if same else of[faces].astype(np.uint32).reshape(-1, 3), short: values[vpoint] if same else values[point]})
    return w(**out)


def same_welded(got, want):
    """Array for array; the name of the first that differs, or None."""
    for f in want._fields:
        a, b = getattr(got, f), getattr(want, f)
        if f == "extra":
            if len(a) != len(b) or any(x.shape != y.shape or x.tobytes() != y.tobytes() for x, y in zip(a, b)):
                return f
        elif isinstance(b, bool):
            if bool(a) != b:
                return f
        elif (a is None) != (b is None) or (b is not None and (np.asarray(a).shape != np.asarray(b).shape or np.asarray(a).tobytes() != np.asarray(b).tobytes())):
            return f
    return None


Case = collections.namedtuple("Case", "name pos faces normals uvs generic extra refused weld_only")
Case.__new__.__defaults__ = (None, None, None, (), None, False)
# refused: the text the strict coder refuses the welded mesh with (None: it is coded); weld_only: not given to the coder (NaN
# positions have no quantised value)
KINDS = [("grid", synth.GRID), ("holes", synth.HOLES), ("sphere", synth.SPHERE), ("torus", synth.TORUS), ("two-parts", synth.TWO_PARTS)]


def _pair(a, b):
    """Two triangles over the edge (1,0,0) - (0,1,0), their third points a and b, every triangle with points of its own."""
    pos = np.array([a, [1, 0, 0], [0, 1, 0], b, [0, 1, 0], [1, 0, 0]], np.float32)
    return pos, np.array([[0, 1, 2], [3, 4, 5]], np.uint32)


def _flat(pos):
    pos = np.asarray(pos, np.float32)
    n = np.tile(np.array([[0, 0, 1]], np.float32), (len(pos), 1))
    return n, np.ascontiguousarray(pos[:, :2] * 0.5 + 0.25)


_cases = None


def cases():
    global _cases
    if _cases is not None:
        return _cases
    out = []
    for kname, kind in KINDS:
        m = synth.make_mesh(kind, 12, 9, 5)
        for j, charts in enumerate(irregular.CHARTS):
            p, f, n, u = unweld(*irregular.with_seams(*m, *charts, seed=7 + j), np.random.default_rng(100 + j))
            out.append(Case("%s/%s-%s" % (kname, charts[0], charts[1]), p, f, n, u))
    for k, (name, charts, args) in enumerate(irregular.seamed_small(shuffled=True)):
        p, f, n, u = unweld(*args, np.random.default_rng(500 + k))
        out.append(Case("small/%s/%s-%s" % (name, charts[0], charts[1]), p, f, n, u))
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    out.append(Case("triangle", tri, np.array([[0, 1, 2]], np.uint32), *_flat(tri)))
    one = np.tile(np.array([[0.5, 0.25, 1.0]], np.float32), (3, 1))
    out.append(Case("all-equal", one, np.array([[0, 1, 2]], np.uint32), *_flat(one), refused="mesh needs positions and faces"))      # (one vertex)
    deg = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 0, 0], [0, 1, 0], [0, 1, 0]], np.float32)
    out.append(Case("degenerate-after-weld", deg, np.array([[0, 1, 2], [4, 3, 5]], np.uint32), *_flat(deg), refused="degenerate face in input mesh"))
    # unused points at the front, in the middle and at the end (copies of used rows among them)
    p, n, u, f = synth.make_mesh(synth.GRID, 5, 4, 9)
    new = np.where(np.arange(len(p)) < 10, np.arange(len(p)) + 2, np.arange(len(p)) + 5)
    spread = lambda a: np.concatenate([a[:2], a[:10], a[3:6], a[10:], a[-2:]])      # noqa: E731  (the unused rows: copies of used ones)
    out.append(Case("unused-points", spread(p), new[f].astype(np.uint32), spread(n), spread(u)))
    # rows that differ in one place only
    z = _pair([0.25, 0.25, 0.0], [0.25, 0.25, 1.0])
    out.append(Case("differ-in-z", *z, *_flat(z[0])))
    m = _pair([0.25, 0.25, 0.0], [np.nextafter(np.float32(0.25), np.float32(1)), 0.25, 0.0])
    out.append(Case("differ-in-last-bit", *m, *_flat(m[0])))
    s = _pair([0.25, 0.25, 0.0], [0.25, 0.25, -0.0])
    assert s[0][0].tobytes() != s[0][3].tobytes()
    out.append(Case("differ-in-sign-of-zero", *s, *_flat(s[0])))
    q = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, 0], [1, 1, 0], [1, 0, 0]], np.float32)
    bits = q.view(np.uint32)
    bits[0, 2] = bits[3, 2] = 0x7FC00001                  # the same NaN twice: one vertex
    bits[6, 2] = 0x7FC00002                               # another payload: another vertex
    out.append(Case("nan-rows", q, np.arange(9, dtype=np.uint32).reshape(3, 3), *_flat(np.nan_to_num(q)), weld_only=True))
    # 40 000 points over 2 positions; 40 000 distinct points
    two = np.where((np.arange(40000) % 2)[:, None] == 0, np.array([[0, 0, 0]], np.float32), np.array([[1, 2, 3]], np.float32)).astype(np.float32)
    ftwo = np.concatenate([np.arange(39999, dtype=np.uint32).reshape(-1, 3), np.array([[39999, 0, 1]], np.uint32)])
    out.append(Case("40000-points-2-positions", two, ftwo, refused="mesh needs positions and faces"))      # (two vertices)
    p, n, u, f = irregular.shuffle(*synth.make_mesh(synth.GRID, 199, 199, 3), np.random.default_rng(8))
    assert len(p) == 40000
    out.append(Case("40000-distinct", p, f, n, u))
    # P around 2^16: a seamed grid of 64 256 vertices, filled up with points no face names
    m = synth.make_mesh(synth.GRID, 250, 255, 4)
    p, f, n, u = unweld(*irregular.with_seams(*m, None, "island", seed=3), np.random.default_rng(9))
    assert len(p) < 65535
    for P in (65535, 65536, 65537):
        fill = P - len(p)
        grow = lambda a: np.concatenate([a, np.tile(a[:1], (fill, 1))])      # noqa: E731  (copies of a used row: the value ranges stay)
        out.append(Case("P=%d" % P, grow(p), f, grow(n), grow(u)))
    # uint8 colours that split vertices which share a position
    m = synth.make_mesh(synth.GRID, 6, 5, 2)
    p, f, n, u = unweld(*irregular.with_seams(*m, None, "stripes", seed=1), np.random.default_rng(10))
    colour = np.stack([np.floor(u[:, 0]).astype(np.uint8) * 40 + 10, np.full(len(u), 7, np.uint8), np.full(len(u), 200, np.uint8)], axis=1)
    out.append(Case("colours-split", p, f, n, u, None, (np.ascontiguousarray(colour),)))
    gen = np.ascontiguousarray((np.floor(u[:, 0]).astype(np.uint8) + 1)[:, None])
    out.append(Case("generic-splits", p, f, n, u, gen))
    # a two-sided sheet: every face twice, turned over, the back with points of its own
    p, n, u, f = synth.make_mesh(synth.GRID, 4, 3, 6)
    both = np.concatenate([f, f[:, ::-1] + len(p)])
    out.append(Case("two-sided-sheet", np.concatenate([p, p]), both, np.concatenate([n, n]), np.concatenate([u, u]),
                    refused="non-manifold edge (duplicate half-edge)"))
    out.append(Case("two-sided-sheet-two-normals", np.concatenate([p, p]), both, np.concatenate([n, -n]), np.concatenate([u, u]),
                    refused="non-manifold edge (duplicate half-edge)"))
    out.append(Case("no-faces", tri, np.zeros((0, 3), np.uint32), *_flat(tri), refused="mesh needs positions and faces"))
    out.append(Case("index-out-of-range", tri, np.array([[0, 1, 3]], np.uint32), *_flat(tri), refused="face index out of range"))
    _cases = out
    return out


def small_cases():
    """The cases below 1 000 points: what a crowded batch is made of."""
    return [c for c in cases() if len(c.pos) < 1000]


def extras_of(c):
    return [synth.Extra(e, attribute_type=2, normalized=True) for e in c.extra]
