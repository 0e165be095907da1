"""Meshes that are not clean -- the same face twice, fins, fans that meet at a vertex, faces turned over, faces with a repeated
index, vertices no face uses -- for the encoder's topology repair (synth.options(repair_topology=1), dsa_encode_repair_batch with
topology = 1), and a pin of what such a mesh must decode to that is written from the contract, not from the coder:

  * degenerate faces (two equal indices) are dropped;
  * every input row is quantised with the numpy restatements of tests/meshutil.py (the pin of tests/test_independent_pin.py),
    the bounds taken over ALL rows the caller passed, isolated ones included;
  * a mesh is the multiset of its faces, a face the cyclically normalised triple of the value tuples at its corners (position,
    normal, texture coordinate, generic, extras).  A vertex the repair made carries its parent's row, so the multiset of the
    repaired mesh is that of the input's faces.

numpy only; the generators are deterministic (seeded)."""
import collections

import numpy as np

import irregular
from meshutil import face_multiset_fast, oct_quantize, source_quantization

Defect = collections.namedtuple("Defect", "name nv faces points num_faces")      # points / num_faces: the header counts of the repaired mesh


def _grid(n):
    """n x n vertices, 2 (n - 1)^2 faces, oriented"""
    f = []
    for j in range(n - 1):
        for i in range(n - 1):
            a = j * n + i
            f += [[a, a + 1, a + n + 1], [a, a + n + 1, a + n]]
    return n * n, f


def _moebius(n=8):
    """a band of n quads over two rows of n vertices, closed with a half twist: 2 n faces"""
    f = []
    for i in range(n):
        b0, t0 = i, n + i
        b1, t1 = ((i + 1), n + i + 1) if i + 1 < n else (n, 0)      # the twist: the last quad meets the first row for row swapped
        f += [[b0, b1, t1], [b0, t1, t0]]
    return 2 * n, f


def named():
    """The small cases with the header counts (points, faces) of the repaired mesh.  Each count by hand, from the three passes
    (corner c of face f faces the directed edge next(c) -> prev(c); it takes the earliest pending reverse edge whose face has
    another tip vertex; every fan of a vertex behind the first met in face order is a new point):

    two tetrahedra sharing vertex 0 (7 vertices): both are closed and oriented, every edge matches inside its tetrahedron; vertex 0
        has two closed fans, the second tetrahedron's becomes a new point: 7 + 1 = 8 points, 8 faces.
    fin [[0,1,2],[1,0,3],[0,1,4]]: face 1's corner at 3 faces 1 -> 0 and takes face 0's pending 0 -> 1; face 2's corner at 4 faces
        0 -> 1 again and finds no pending 1 -> 0 (taken): face 2 stays alone, its corners at 0 and 1 are second fans: 5 + 2 = 7, 3.
    a face twice [[0,1,2],[0,1,2]]: the copy's corners face the same directed edges, never a reverse one: two separate triangles,
        the second's three corners are second fans: 3 + 3 = 6, 2.
    a mirrored pair [[0,1,2],[1,0,2]]: every reverse edge exists, but always in a face with the same tip vertex (the same three
        vertices): no pair is made: 3 + 3 = 6, 2.
    a neighbour turned over [[0,1,2],[0,1,3]]: both faces have 0 -> 1, neither 1 -> 0: no pair; the second face's corners at 0 and
        1 are second fans: 4 + 2 = 6, 2.
    two triangles sharing an apex [[0,1,2],[0,3,4]]: no shared edge; vertex 0 has two fans: 5 + 1 = 6, 2.
    a 16-face Moebius band (16 vertices): every interior edge pairs except along the seam where the band closes with a half twist:
        there the two faces run the shared edge in the same direction, so the band is cut open into a strip whose two ends both
        carry vertices 0 and 8 -- second fans at the far end: 16 + 2 = 18, 16.
    the smallest edge break [[1,0,2],[2,4,1],[1,3,2],[2,3,4]] over 5 vertices: 1 -> 2 is faced by faces 0 and 2, 2 -> 1 by face 1:
        face 1 pairs with face 0 (earlier).  Around vertex 2 the fan then reaches vertex 1 over two different edges (face 2's open
        2-1 edge and the paired one): BreakNonManifoldEdges cuts both, one break; the faces fall into fans that share vertices
        1, 2 (and 4): 5 + 3 = 8, 4.
    the renumbering trap [[2,0,4],[3,1,0],[1,4,0],[4,3,0],[3,4,1]] over 5 vertices: two breaks; a cut edge keeps both end points on
        both sides, so matching the renumbered faces again would join what was cut: 5 + 2 = 7, 5.
    [[0,1,2],[2,2,3],[0,2,4]] over 7 vertices: face 1 is degenerate and dropped; faces 0 and 2 pair over 2 -> 0 / 0 -> 2; vertices
        3, 5, 6 have no fan: 7 - 3 = 4, 3 - 1 = 2.
    a 4 x 4 grid (16 vertices, 18 faces) with face 5 doubled: the copy stays alone, three second fans: 16 + 3 = 19, 19.
    a 4 x 4 grid with a fin on an interior edge to a new vertex 16: the fin's two corners on the edge are second fans:
        17 + 2 = 19, 19."""
    nv_g, grid = _grid(4)
    nv_m, moebius = _moebius(8)
    tets = [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2], [0, 4, 5], [0, 6, 4], [0, 5, 6], [4, 6, 5]]
    a, b, _ = grid[5]
    cases = [
        Defect("two-tetrahedra-one-vertex", 7, tets, 8, 8),
        Defect("fin", 5, [[0, 1, 2], [1, 0, 3], [0, 1, 4]], 7, 3),
        Defect("face-twice", 3, [[0, 1, 2], [0, 1, 2]], 6, 2),
        Defect("mirrored-pair", 3, [[0, 1, 2], [1, 0, 2]], 6, 2),
        Defect("neighbour-turned-over", 4, [[0, 1, 2], [0, 1, 3]], 6, 2),
        Defect("two-triangles-one-apex", 5, [[0, 1, 2], [0, 3, 4]], 6, 2),
        Defect("moebius-16", nv_m, moebius, 18, 16),
        Defect("smallest-edge-break", 5, [[1, 0, 2], [2, 4, 1], [1, 3, 2], [2, 3, 4]], 8, 4),
        Defect("renumbering-trap", 5, [[2, 0, 4], [3, 1, 0], [1, 4, 0], [4, 3, 0], [3, 4, 1]], 7, 5),
        Defect("isolated-and-degenerate", 7, [[0, 1, 2], [2, 2, 3], [0, 2, 4]], 4, 2),
        Defect("grid-face-doubled", nv_g, grid + [grid[5]], 19, 19),
        Defect("grid-fin", nv_g + 1, grid + [[a, b, 16]], 19, 19),
    ]
    return [c._replace(faces=np.array(c.faces, np.uint32)) for c in cases]


BREAKS = {"smallest-edge-break": 1, "renumbering-trap": 2}      # edges BreakNonManifoldEdges cuts (every other named case: none)


def placed():
    """Isolated vertices first, in the middle and last in the vertex array; degenerate faces first and last in the face list; a fan
    of valence 300 with one face doubled.  Header counts where they are plain."""
    nv, grid = _grid(4)
    g = np.array(grid, np.uint32)
    out = [
        Defect("isolated-first", nv + 2, g + 2, 16, 18),
        Defect("isolated-middle", nv + 1, np.where(g >= 7, g + 1, g).astype(np.uint32), 16, 18),
        Defect("isolated-last", nv + 3, g, 16, 18),
        Defect("degenerate-first", nv, np.concatenate([[[3, 3, 4], [5, 6, 5]], g]).astype(np.uint32), 16, 18),
        Defect("degenerate-last", nv, np.concatenate([g, [[0, 1, 1]]]).astype(np.uint32), 16, 18),
    ]
    _, _, _, fan = irregular.fan(300, True)
    fan = np.asarray(fan, np.uint32)
    out.append(Defect("fan-300-face-doubled", 301, np.concatenate([fan, fan[77:78]]), 304, 301))
    return out


ALL_DEGENERATE = Defect("all-degenerate", 4, np.array([[0, 0, 1], [2, 3, 2], [1, 1, 1]], np.uint32), 0, 0)

KINDS = ("double", "fin", "flip", "degenerate", "isolated", "pinch")


def inject(nv, faces, kind, count, rng):
    """`count` defects of one kind into a mesh: -> (nv', faces').  double: a face again; fin: a face on an existing edge to a vertex
    of the mesh; flip: a face turned over; degenerate: a face with a repeated index, somewhere in the list; isolated: a vertex no
    face uses; pinch: every use of one vertex replaced by another (the one left is isolated, the other a meeting of fans)."""
    faces = np.array(faces, np.int64).reshape(-1, 3)
    for _ in range(count):
        k = int(rng.integers(0, len(faces)))
        if kind == "double":
            faces = np.concatenate([faces, faces[k:k + 1]])
        elif kind == "fin":
            faces = np.concatenate([faces, [[faces[k, 0], faces[k, 1], int(rng.integers(0, nv))]]])
        elif kind == "flip":
            faces[k] = faces[k][::-1]
        elif kind == "degenerate":
            v = int(rng.integers(0, nv))
            faces = np.insert(faces, k, [v, int(rng.integers(0, nv)), v], axis=0)
        elif kind == "isolated":
            nv += 1
        elif kind == "pinch":
            a, b = int(rng.integers(0, nv)), int(rng.integers(0, nv))
            faces[faces == b] = a
        else:
            raise ValueError(kind)
    return nv, faces.astype(np.uint32)


def injected_small(seed=5):
    """Every mesh of irregular.SMALL with 1 - 8 injected defects of one kind, the kinds in turn."""
    rng = np.random.default_rng(seed)
    out = []
    for k, case in enumerate(irregular.SMALL):
        pos, _, _, faces = irregular.mesh(case)
        kind = KINDS[k % len(KINDS)]
        nv, f = inject(len(pos), faces, kind, int(rng.integers(1, 9)), rng)
        out.append(Defect("%s+%s" % (case.name, kind), nv, f, None, None))
    return out


def soups(count, seed=77):
    """Random face soups: 3 - 7 vertices, 2 - 10 faces, repeated indices allowed."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        nv = int(rng.integers(3, 8))
        out.append(Defect("soup-%d" % k, nv, rng.integers(0, nv, (int(rng.integers(2, 11)), 3)).astype(np.uint32), None, None))
    return out


def is_degenerate(faces):
    f = np.asarray(faces).reshape(-1, 3)
    return (f[:, 0] == f[:, 1]) | (f[:, 0] == f[:, 2]) | (f[:, 1] == f[:, 2])


def attributes(nv, seed=0):
    """Values for nv rows: positions, normals, texture coordinates, a generic uint8 attribute of 2 components, an int16 extra."""
    rng = np.random.default_rng(1000 + seed + nv)
    pos = rng.random((nv, 3)).astype(np.float32)
    nrm = rng.normal(size=(nv, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True).astype(np.float32)
    uv = rng.random((nv, 2)).astype(np.float32)
    generic = rng.integers(0, 256, (nv, 2)).astype(np.uint8)
    extra = rng.integers(-3000, 3000, (nv, 1)).astype(np.int16)
    return pos, nrm, uv, generic, extra


def pin(faces, pos, nrm=None, uv=None, integers=(), pos_bits=11, normal_bits=8, uv_bits=10):
    """The face multiset the stream of a repaired mesh must decode to ([F', 3 K] int64, sorted) and the quantisation parameters it
    must carry (position min, range, uv min, range -- uv None without texture coordinates).  integers: arrays of one row per
    vertex that are coded as they are (the generic attribute, integer extras), in stream order."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    faces = faces[~is_degenerate(faces)]
    pmin, prange, qp = source_quantization(pos, pos_bits)
    cols, umin, urange = [qp], None, None
    if nrm is not None:
        cols.append(oct_quantize(nrm, normal_bits))
    if uv is not None:
        umin, urange, qu = source_quantization(uv, uv_bits)
        cols.append(qu)
    for g in integers:
        cols.append(np.asarray(g, np.int64).reshape(len(pos), -1))
    return face_multiset_fast(faces, np.concatenate(cols, axis=1)), (pmin, prange, umin, urange)


def decoded(faces, attributes_):
    """The same multiset of a decoded mesh; attributes_: [(portable values [entries, nc], point map [points] or empty)] in stream order."""
    cols = []
    for portable, point_map in attributes_:
        p = np.asarray(portable, np.int64)
        cols.append(p[np.asarray(point_map, np.int64)] if len(point_map) else p)
    return face_multiset_fast(np.asarray(faces, np.int64), np.concatenate(cols, axis=1))
