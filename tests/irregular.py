"""Irregular meshes for the tests (numpy only, deterministic from a seed).  synth.make_mesh makes regular grids: interior
vertices of valence 6, vertex ids rising along the rows, faces in row order -- the input the traversal kernels' run
detection and speculation are built around.  The generators here break each of those regularities while keeping the mesh
an oriented manifold, so that no coder may refuse it: diagonal flips and 1->3 splits spread the valences, thicken() turns
holes into handles (topology splits), fan / strip / components are the degenerate extremes, shuffle() takes away the
order of vertex ids and faces.  Each mesh is (pos, nrm, uv, faces) like synth.make_mesh returns it.

CASES is the fixed list that tests/test_irregular_cpu.py, tests/test_gpu_irregular.py and the host checks share; the
conditions it has to meet are asserted in tests/test_irregular_cpu.py."""
import collections

import numpy as np

import meshutil


# ------------------------------------------------------------------------------------------------------ connectivity
def flip_edges(faces, count, rng):
    """`count` random diagonal flips of interior edges.  The two triangles (a, b, c), (b, a, d) on an edge a-b become
    (a, d, c), (b, c, d): the four outer edges keep their direction, so the mesh stays oriented, and a flip whose new edge
    c-d exists already is skipped, so it stays a manifold.  Gives up after 20 * count draws."""
    f = [[int(x) for x in t] for t in np.asarray(faces, np.int64)]
    n = int(np.max(faces)) + 1
    half = {}                                           # directed edge a * n + b -> (face, corner of a)
    for i, t in enumerate(f):
        for k in range(3):
            half[t[k] * n + t[(k + 1) % 3]] = (i, k)
    done = 0
    draws = rng.integers(0, 3 * len(f), 20 * count)
    for x in draws:
        if done == count:
            break
        i, k = int(x) // 3, int(x) % 3
        a, b, c = f[i][k], f[i][(k + 1) % 3], f[i][(k + 2) % 3]
        other = half.get(b * n + a)
        if other is None:                               # a boundary edge
            continue
        j, kj = other
        d = f[j][(kj + 2) % 3]
        if c == d or c * n + d in half or d * n + c in half:
            continue
        del half[a * n + b], half[b * n + a]
        f[i], f[j] = [a, d, c], [b, c, d]
        for face, t in ((i, f[i]), (j, f[j])):
            for q in range(3):
                half[t[q] * n + t[(q + 1) % 3]] = (face, q)
        done += 1
    return np.array(f, np.uint32)


def subdivide_random(faces, count, rng):
    """`count` 1->3 splits of random faces, one after the other (a child face may be split again): every new vertex has
    valence 3 and raises the valence of its three neighbours.  Returns (faces, parents[count, 3]): new vertex k has the id
    (number of vertices before) + k and lies inside the face parents[k] had; see with_centroids."""
    f = [[int(x) for x in t] for t in np.asarray(faces, np.int64)]
    nv = int(np.max(faces)) + 1
    parents = []
    for _ in range(count):
        i = int(rng.integers(0, len(f)))
        a, b, c = f[i]
        v = nv + len(parents)
        parents.append((a, b, c))
        f[i] = [a, b, v]
        f.append([b, c, v])
        f.append([c, a, v])
    return np.array(f, np.uint32), np.array(parents, np.int64).reshape(-1, 3)


def with_centroids(pos, nrm, uv, parents):
    """The attribute rows of subdivide_random's new vertices: the mean of the three corners of the face each one split."""
    out = []
    for a in (pos, nrm, uv):
        rows = [r for r in np.asarray(a, np.float32)]
        for p in parents:
            rows.append(((rows[p[0]].astype(np.float64) + rows[p[1]] + rows[p[2]]) / 3.0).astype(np.float32))
        out.append(np.array(rows, np.float32))
    return tuple(out)


def boundary_edges(faces):
    """The directed edges (a, b) of `faces` whose opposite (b, a) belongs to no face, as an int64 array [n, 2]."""
    f = np.asarray(faces, np.int64)
    n = int(f.max()) + 1
    e = np.stack([f, np.roll(f, -1, axis=1)], axis=2).reshape(-1, 2)
    return e[~np.isin(e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0])]


def count_components(faces):
    """Connected components of the vertices `faces` use."""
    f = np.asarray(faces, np.int64)
    label = np.arange(int(f.max()) + 1)
    while True:
        low = label[f].min(axis=1)
        new = label.copy()
        for k in range(3):
            np.minimum.at(new, f[:, k], low)
        new = new[new]
        if np.array_equal(new, label):
            return len(np.unique(label[np.unique(f)]))
        label = new


def count_boundary_loops(faces):
    b = boundary_edges(faces)
    nxt = dict(zip(b[:, 0].tolist(), b[:, 1].tolist()))
    assert len(nxt) == len(b), "a vertex on two boundary loops"
    loops = 0
    while nxt:
        start = next(iter(nxt))
        v = nxt.pop(start)
        while v != start:
            v = nxt.pop(v)
        loops += 1
    return loops


def euler_characteristic(faces):
    f = np.asarray(faces, np.int64)
    n = int(f.max()) + 1
    e = np.stack([f, np.roll(f, -1, axis=1)], axis=2).reshape(-1, 2)
    return len(np.unique(f)) - len(np.unique(e.min(axis=1) * n + e.max(axis=1))) + len(f)


def genus(faces):
    """Of a closed connected surface: V - E + F = 2 - 2g."""
    assert len(boundary_edges(faces)) == 0 and count_components(faces) == 1
    chi = euler_characteristic(faces)
    assert chi % 2 == 0
    return (2 - chi) // 2


def thicken(pos, nrm, uv, faces):
    """Two copies of an open mesh, the second with reversed winding and moved against the normals, every boundary loop
    stitched with a band of quads: a closed surface.  A component with b boundary loops becomes a closed surface of genus
    b - 1, which the Euler characteristic of the result is checked against."""
    f = np.asarray(faces, np.int64)
    nv = len(pos)
    b = boundary_edges(f)
    assert len(b), "thicken needs an open mesh"
    back = f[:, ::-1] + nv
    band = np.concatenate([np.stack([b[:, 1], b[:, 0], b[:, 0] + nv], axis=1), np.stack([b[:, 1], b[:, 0] + nv, b[:, 1] + nv], axis=1)])
    out = np.concatenate([f, back, band])
    parts, loops = count_components(f), count_boundary_loops(f)
    assert len(boundary_edges(out)) == 0
    assert euler_characteristic(out) == 4 * parts - 2 * loops, "thicken: V - E + F does not match the boundary loops"
    nrm = np.asarray(nrm, np.float32)
    pos2 = (np.asarray(pos, np.float32) - np.float32(0.05) * nrm).astype(np.float32)
    uv2 = (np.asarray(uv, np.float32) + np.array([1.0, 0.0], np.float32)).astype(np.float32)
    return (np.concatenate([np.asarray(pos, np.float32), pos2]), np.concatenate([nrm, -nrm]), np.concatenate([np.asarray(uv, np.float32), uv2]),
            out.astype(np.uint32))


def shuffle(pos, nrm, uv, faces, rng):
    """A permutation of the vertex ids, another of the face order, and a rotation of each face's corners: the same mesh for
    a decoder, other tables, other start faces and another traversal for an encoder."""
    f = np.asarray(faces, np.int64)
    new_id = rng.permutation(len(pos))                  # old id -> new id
    old_id = np.argsort(new_id)
    f = new_id[f][rng.permutation(len(f))]
    rot = rng.integers(0, 3, len(f))
    f = np.stack([f[np.arange(len(f)), (rot + k) % 3] for k in range(3)], axis=1)
    return np.asarray(pos)[old_id], np.asarray(nrm)[old_id], np.asarray(uv)[old_id], f.astype(np.uint32)


# --------------------------------------------------------------------------------------------------- the odd extremes
def _flat_attributes(pos):
    pos = np.asarray(pos, np.float32)
    nrm = np.stack([0.3 * np.sin(5 * pos[:, 0]), 0.3 * np.cos(3 * pos[:, 1]), np.ones(len(pos))], axis=1)
    nrm = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(np.float32)
    lo, hi = pos[:, :2].min(axis=0), pos[:, :2].max(axis=0)
    uv = ((pos[:, :2] - lo) / np.where(hi > lo, hi - lo, 1)).astype(np.float32)
    return pos, nrm, uv


def fan(k, closed=True):
    """One vertex with k triangles around it: a closed disc (valence k), or an open fan of k triangles."""
    rim = k if closed else k + 1
    ang = np.linspace(0, 2 * np.pi, rim, endpoint=False)
    pos = np.concatenate([[[0, 0, 0]], np.stack([np.cos(ang), np.sin(ang), 0.1 * np.sin(7 * ang)], 1)]).astype(np.float32)
    i = np.arange(k)
    faces = np.stack([np.zeros(k, np.int64), 1 + i, 1 + (i + 1) % rim], 1).astype(np.uint32)
    return _flat_attributes(pos) + (faces,)


def strip(m):
    """A band of 2 x m vertices, 2 (m - 1) triangles: every vertex on the boundary."""
    x = np.arange(m, dtype=np.float32) / m
    pos = np.concatenate([np.stack([x, np.zeros(m, np.float32), np.sin(40 * x)], 1), np.stack([x, np.full(m, 0.01, np.float32), np.sin(40 * x)], 1)]).astype(np.float32)
    i = np.arange(m - 1)
    faces = np.concatenate([np.stack([i, i + 1, m + i], 1), np.stack([i + 1, m + i + 1, m + i], 1)]).astype(np.uint32)
    return _flat_attributes(pos) + (faces,)


def components(n, seed=3):
    """n disjoint quads of two triangles each."""
    base = np.random.default_rng(seed).uniform(-1, 1, (n, 1, 3)).astype(np.float32)
    quad = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32) * 0.01
    pos = (base + quad[None]).reshape(-1, 3)
    faces = (np.arange(n)[:, None, None] * 4 + np.array([[0, 1, 2], [0, 2, 3]])[None]).reshape(-1, 3).astype(np.uint32)
    return _flat_attributes(pos) + (faces,)


def roughen(pos, nrm, uv, faces, rng):
    """The irregular draw of the randomised tools (tools/soak.py, soak_encode.py, dialect_matrix.py): flips on a tenth to six
    tenths of the faces, half of the time 1->3 splits, a quarter of the time thicken() where the mesh is open, two times in
    three a shuffle.  All draws come from `rng`, which the tools keep apart from the generator of their options."""
    nf = len(faces)
    faces = flip_edges(faces, max(1, int(rng.uniform(0.1, 0.6) * nf)), rng)
    if rng.integers(0, 2):
        faces, parents = subdivide_random(faces, max(1, nf // int(rng.integers(4, 20))), rng)
        pos, nrm, uv = with_centroids(pos, nrm, uv, parents)
    if rng.integers(0, 4) == 0 and len(boundary_edges(faces)):
        pos, nrm, uv, faces = thicken(pos, nrm, uv, faces)
    if rng.integers(0, 3):
        pos, nrm, uv, faces = shuffle(pos, nrm, uv, faces, rng)
    return (np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(nrm, np.float32), np.ascontiguousarray(uv, np.float32),
            np.ascontiguousarray(faces, np.uint32))


# -------------------------------------------------------------------------------------------------------------- seams
def with_seams(pos, nrm, uv, faces, normal_charts=None, uv_charts="stripes", seed=0):
    """Normals and / or texture coordinates of a given mesh per corner (meshutil.chart_of_faces patterns; None: that
    attribute stays per vertex).  Returns the arguments of synth.encode_mesh_corners:
    (pos, faces, normal rows, normal ids or None, uv rows, uv ids or None)."""
    nid = uid = None
    if normal_charts:
        nid, nrm = meshutil.split_by_chart(faces, nrm, meshutil.chart_of_faces(pos, faces, normal_charts, seed + 1), [0.3, -0.2, 0.1])
    if uv_charts:
        uid, uv = meshutil.split_by_chart(faces, uv, meshutil.chart_of_faces(pos, faces, uv_charts, seed + 2), [1.25, 0.5])
    return pos, faces, nrm, nid, uv, uid


# ----------------------------------------------------------------------------------------------------- self-description
def valence_histogram(faces):
    """{valence: number of vertices}, valence = number of faces at the vertex."""
    return dict(sorted(collections.Counter(np.bincount(np.asarray(faces, np.int64).ravel()).tolist()).items()))


def is_oriented_manifold(nv, faces):
    """Every vertex 0 .. nv - 1 in use, no degenerate face, no directed edge twice, and the faces at every vertex one fan
    (a closed one, or an open one between two boundary edges)."""
    f = np.asarray(faces, np.int64)
    if len(f) == 0 or f.min() < 0 or f.max() >= nv or len(np.unique(f)) != nv:
        return False
    if ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])).any():
        return False
    e = np.stack([f, np.roll(f, -1, axis=1)], axis=2).reshape(-1, 2)
    key = e[:, 0] * nv + e[:, 1]
    if len(np.unique(key)) != len(key):
        return False
    # at vertex v the face (v, a, b) leads from spoke a to spoke b: the spokes of v must form one path or one cycle
    nxt = {}
    for t in f.tolist():
        for k in range(3):
            nxt[(t[k], t[(k + 1) % 3])] = t[(k + 2) % 3]
    degree = np.bincount(f.ravel(), minlength=nv)
    firsts = {}
    incoming = set((v, b) for (v, a), b in nxt.items())
    for (v, a) in nxt:
        if (v, a) not in incoming:
            if v in firsts:
                return False                            # two open fans at one vertex
            firsts[v] = a
    for t in f.tolist():
        for v, a in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            firsts.setdefault(v, a)
    for v, a in firsts.items():
        steps, s = 0, a
        while (v, s) in nxt and steps < degree[v]:
            s = nxt[(v, s)]
            steps += 1
            if s == a:
                break
        if steps != degree[v]:
            return False
    return True


# -------------------------------------------------------------------------------------------------------------- CASES
Case = collections.namedtuple("Case", "name build spread genus splits")
Case.__doc__ = """name; build() -> (pos, nrm, uv, faces); spread: flipped or subdivided (the valence conditions apply); genus: of a
thickened case, else None; splits: the traversal of this case has to split (handles, holes, several components larger than a quad)."""


def _make(kind, nx, ny, seed):
    import draco_sharp_amd.synth as synth
    return synth.make_mesh(kind, nx, ny, seed)


def _flipped(kind, nx, ny, seed, share=0.55):
    pos, nrm, uv, faces = _make(kind, nx, ny, seed)
    return pos, nrm, uv, flip_edges(faces, int(share * len(faces)), np.random.default_rng(seed))


def _flipped_thickened(nx, ny, seed):
    pos, nrm, uv, faces = _flipped(3, nx, ny, seed)
    pos, nrm, uv, faces = thicken(pos, nrm, uv, faces)
    # flips across the bands as well, so that the two sheets do not mirror each other
    return pos, nrm, uv, flip_edges(faces, len(faces) // 8, np.random.default_rng(seed + 1))


def _subdivided(kind, nx, ny, seed, count, flips=0):
    pos, nrm, uv, faces = _make(kind, nx, ny, seed)
    rng = np.random.default_rng(seed)
    if flips:
        faces = flip_edges(faces, flips, rng)
    faces, parents = subdivide_random(faces, count, rng)
    return with_centroids(pos, nrm, uv, parents) + (faces,)


def _shuffled(mesh, seed):
    return shuffle(*mesh, np.random.default_rng(seed))


def holes_of(nx, ny):
    """The number of cells synth.make_mesh(HOLES, nx, ny) leaves out."""
    return len(range(2, ny - 2, 5)) * len(range(2, nx - 2, 7))


GRID, TORUS, SPHERE, HOLES, TWO_PARTS = 0, 1, 2, 3, 4          # synth.make_mesh kinds

SMALL = [
    Case("grid-flipped", lambda: _flipped(GRID, 24, 20, 101), True, None, False),
    Case("torus-flipped", lambda: _flipped(TORUS, 24, 40, 102), True, None, True),
    Case("sphere-flipped", lambda: _flipped(SPHERE, 20, 17, 103), True, None, False),
    Case("holes-flipped", lambda: _flipped(HOLES, 30, 23, 104), True, None, True),
    Case("two-parts-flipped", lambda: _flipped(TWO_PARTS, 20, 14, 105), True, None, True),
    Case("holes-thickened", lambda: thicken(*_make(HOLES, 16, 13, 106)), False, holes_of(16, 13), True),
    Case("holes-flipped-thickened", lambda: _flipped_thickened(23, 18, 107), True, holes_of(23, 18), True),
    Case("grid-subdivided", lambda: _subdivided(GRID, 16, 12, 108, 300), True, None, False),
    Case("torus-flipped-subdivided-shuffled", lambda: _shuffled(_subdivided(TORUS, 16, 20, 109, 250, flips=400), 9), True, None, True),
    Case("sphere-flipped-shuffled", lambda: _shuffled(_flipped(SPHERE, 14, 15, 110), 10), True, None, False),
    Case("fan-closed", lambda: fan(300, True), False, None, False),
    Case("fan-open", lambda: fan(257, False), False, None, False),
    Case("strip", lambda: strip(400), False, None, False),
    Case("components", lambda: components(150), False, None, False),
]
BENCH_SIZE = [
    Case("grid-128x256-flipped", lambda: _flipped(GRID, 128, 256, 201), True, None, False),
    Case("holes-128x128-flipped-thickened", lambda: _flipped_thickened(128, 128, 202), True, holes_of(128, 128), True),
    Case("torus-128x256-flipped", lambda: _flipped(TORUS, 128, 256, 203), True, None, True),
]
CASES = SMALL + BENCH_SIZE

_built = {}


def mesh(case):
    """(pos, nrm, uv, faces) of a Case or of its name, built once per process."""
    if isinstance(case, str):
        case = next(c for c in CASES if c.name == case)
    if case.name not in _built:
        pos, nrm, uv, faces = case.build()
        _built[case.name] = (np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(nrm, np.float32), np.ascontiguousarray(uv, np.float32),
                             np.ascontiguousarray(faces, np.uint32))
    return _built[case.name]


# the stream dialects the irregular tests put every case through (synth.options keywords)
DIALECTS = collections.OrderedDict([
    ("standard", dict()),
    ("valence", dict(predictive_connectivity=2)),
    ("stock-default", dict(predictive_connectivity=2, uv_prediction=5, normal_prediction=6)),
    ("multi-parallelogram", dict(pos_prediction=4)),
    ("prediction-degree", dict(traversal_method=1)),
    ("single-connectivity", dict(single_connectivity=1)),
])

# the charts the seamed tests cut the cases by: (normal charts, uv charts) -- each pattern on the texture coordinates, and
# seams on both attributes
CHARTS = [(None, "stripes"), (None, "checker"), (None, "island"), (None, "random"), (None, "single"), ("checker", "island"), ("random", "stripes")]


def shuffled_small():
    """[(name, (pos, nrm, uv, faces))]: the small cases with their vertex ids, face order and face corners permuted -- what the
    encoder's table kernels and start faces see."""
    return [(c.name, shuffle(*mesh(c), np.random.default_rng(300 + k))) for k, c in enumerate(SMALL)]


def seamed_small(shuffled=False):
    """[(name, charts, encode_mesh_corners arguments)]: every small case cut by two of CHARTS (all of them in turn)."""
    out = []
    for k, (name, m) in enumerate(shuffled_small() if shuffled else [(c.name, mesh(c)) for c in SMALL]):
        for j in (k, k + 3):
            charts = CHARTS[j % len(CHARTS)]
            out.append((name, charts, with_seams(*m, *charts, seed=20 + j)))
    return out
