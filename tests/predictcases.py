"""Designed geometry for the prediction arithmetic, and a reference of that arithmetic in Python integers.

synth.make_mesh gives smooth, finely divided surfaces: every triangle small and well shaped, every kernel on one path.  The
DESIGNS here are small meshes (a few to 169 vertices) whose GEOMETRY carries the design: triangles that span the whole box at 17 -
20 bits (squared edges beyond 2^32, products beyond 2^64, dividends beyond 2^52 and 4e15), collinear, flat, coincident and
collapsed vertices, axis-aligned normals of mixed sign, vertices that alternate between opposite walls of the box, and strips
whose entry counts sit around the groups of 12 the texture-coordinate chain works in.

reference() restates the ENCODER's side of the prediction schemes from the bitstream rules (SURVEY.md App. D and the rules the
kernels cite: TexCoordsPortable with both candidates and the closer one taken, GeometricNormal with its flipped twin and the
smaller correction kept, parallelogram and difference under the wrap transform, the canonicalised octahedral transform) in
Python integers: math.isqrt, reduction modulo 2^64 written out, division truncated toward zero.  It takes from an oracle.decode
result only the decoded integers, data_to_corner and the corner table, returns the symbols every entry must have been coded
with, and counts the branches each entry took.  Nothing in it is shared with the C++ of the coders, the oracle or the kernels."""
import collections
import math

import numpy as np

import irregular

M64 = (1 << 64) - 1
INVALID = 0xFFFFFFFF


def u64(x):
    return x & M64


def s64(x):
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def s32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x


def tdiv(x, y):
    """x / y truncated toward zero (y != 0)."""
    q = abs(x) // abs(y)
    return q if (x < 0) == (y < 0) else -q


def zigzag(v):
    return 2 * v if v >= 0 else -2 * v - 1


# ------------------------------------------------------------------------------------------------------------- designs
def grid_faces(nx, ny):
    """Two triangles per cell of an nx x ny vertex grid, vertex id = j * nx + i."""
    f = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a, b, c, d = j * nx + i, j * nx + i + 1, (j + 1) * nx + i, (j + 1) * nx + i + 1
            f += [(a, b, c), (b, d, c)]
    return np.array(f, np.uint32)


def strip_faces(n):
    """A triangle strip of n vertices, n - 2 triangles of one orientation."""
    return np.array([(i, i + 1, i + 2) if i % 2 == 0 else (i + 1, i, i + 2) for i in range(n - 2)], np.uint32)


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=1)[:, None]).astype(np.float32)


def _grid_xy(n):
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return np.stack([i.ravel(), j.ravel()], axis=1).astype(np.float64) / (n - 1)


def rough(n, seed, faces=None):
    """n x n grid, every vertex moved by up to 0.45 of a cell and the plane warped (x, y -> x^1.7, y^1.7), z anywhere between 0 and
    a height that grows from nothing at the origin's corner to the whole box at the far one: triangles of every shape, from a
    twentieth of the box to all of it, so that from 17 to 19 bits a chain meets squared edges on both sides of 2^32.  Texture
    coordinates: the jittered plane turned, so that both candidates and both orientations occur."""
    rng = np.random.default_rng(seed)
    g = np.abs(_grid_xy(n) + rng.uniform(-0.45, 0.45, (n * n, 2)) / (n - 1))
    xy = g ** 1.7
    height = np.minimum(1.0, (g.sum(axis=1) / 2) ** 2 * 3.0)
    pos = np.concatenate([xy, (rng.uniform(0, 1, n * n) * height)[:, None]], axis=1).astype(np.float32)
    uv = np.stack([0.8 * g[:, 0] - 0.6 * g[:, 1], 0.6 * g[:, 0] + 0.8 * g[:, 1]], axis=1) + rng.uniform(-0.3, 0.3, (n * n, 2)) / (n - 1)
    nrm = _unit(rng.normal(size=(n * n, 3)))
    return pos, nrm, uv.astype(np.float32), grid_faces(n, n) if faces is None else faces


def collinear(n=7, seed=5):
    pos, nrm, uv, faces = rough(n, seed)
    pos[:, 1] = 0.25
    pos[:, 2] = 0.5
    return pos, nrm, uv, faces


def flat(n=7):
    xy = _grid_xy(n)
    pos = np.concatenate([xy, np.zeros((n * n, 1))], axis=1).astype(np.float32)
    nrm = np.tile(np.array([[0, 0, 1]], np.float32), (n * n, 1))
    return pos, nrm, xy.astype(np.float32), grid_faces(n, n)


def lattice(n=7, seed=7):
    rng = np.random.default_rng(seed)
    pos = (rng.integers(0, 4, (n * n, 3)) / 3.0).astype(np.float32)
    uv = (rng.integers(0, 3, (n * n, 2)) / 2.0).astype(np.float32)
    nrm = _unit(rng.integers(-1, 2, (n * n, 3)) + np.array([[0.0, 0.0, 0.001]]))
    return pos, nrm, uv, grid_faces(n, n)


def collapsed(n=5):
    pos = np.full((n * n, 3), 0.375, np.float32)
    rng = np.random.default_rng(9)
    return pos, _unit(rng.normal(size=(n * n, 3))), rng.uniform(0, 1, (n * n, 2)).astype(np.float32), grid_faces(n, n)


def box_fold(n=9, axes=(0, 1, 2), seed=11):
    """A grid whose rows follow a square wave in the plane of axes[0], axes[1] and whose columns run along axes[2]: every face lies
    in an axis plane, the normals of consecutive panels are +a, -b, -a, -b, ... and the summed normals at the folds lie in the
    coordinate planes, on both sides of every axis.  Vertex normals: the axis-aligned normal of the panel that starts at the vertex."""
    step = [(0, 1), (1, 0), (0, -1), (1, 0)]
    p, prof, nr = [0, 0], [], []
    for i in range(n):
        prof.append(tuple(p))
        dx, dy = step[i % 4]
        nr.append((dy, -dx))                         # tangent x extrusion axis
        p[0] += dx
        p[1] += dy
    pos = np.zeros((n * n, 3))
    nrm = np.zeros((n * n, 3))
    for j in range(n):
        for i in range(n):
            pos[j * n + i, axes[0]], pos[j * n + i, axes[1]], pos[j * n + i, axes[2]] = prof[i][0], prof[i][1], j * 0.5
            nrm[j * n + i, axes[0]], nrm[j * n + i, axes[1]] = nr[i]
    rng = np.random.default_rng(seed)
    sign = np.where(rng.integers(0, 4, n * n) == 0, -1.0, 1.0)        # a quarter of the normals point inward: the flipped twin
    return pos.astype(np.float32), (nrm * sign[:, None]).astype(np.float32), _grid_xy(n).astype(np.float32), grid_faces(n, n)


def fold_exact(normal_bits):
    """The fold s = 0 of the octahedron needs a summed normal (-x, -y, 0) whose x and y scale to the absolute sum `center` without a
    remainder (the z of the scaled vector is the rest, and the fold wants it 0).  Five columns on the profile (0,0) (0,a) (ra,a) (ra,0)
    (E,0), extruded along z in eight equal steps: the interior vertices of the fourth column sum panels of the normals -y and -x in the
    ratio r : 1, and r + 1 divides center = 2^(bits-1) - 1 (7, 127 prime, 511 = 7 * 73, 8191 prime).  Integer coordinates, the largest
    extent E = 2^b - 1 of the position bits b, so the quantiser keeps them; all sums below 2^29.  Normals: the summed face normals.
    Returns (mesh, position bits)."""
    r, a, h, b = {4: (6, 100, 50, 12), 8: (126, 10, 50, 12), 10: (6, 100, 50, 12), 14: (8190, 1, 1000, 13)}[normal_bits]
    prof = [(0, 0), (0, a), (r * a, a), (r * a, 0), ((1 << b) - 1, 0)]
    rows = 8
    pos = np.array([(x, y, j * h) for j in range(rows) for (x, y) in prof], np.float64)
    faces = grid_faces(len(prof), rows)
    nrm = np.zeros_like(pos)
    for f in faces.astype(np.int64):
        n = np.cross(pos[f[1]] - pos[f[0]], pos[f[2]] - pos[f[0]])
        for v in f:
            nrm[v] += n
    uv = np.stack([pos[:, 0] / pos[:, 0].max(), pos[:, 2] / pos[:, 2].max()], axis=1)
    return (pos.astype(np.float32), _unit(nrm), uv.astype(np.float32), faces), b


def wall_hugger(n=7, seed=13):
    """Vertices alternate between the walls x = 0 and x = 1 (u = 0 and u = 1), chequerwise: a parallelogram a + b - c over two
    vertices on one wall and one on the other lands a box width outside, on either side."""
    rng = np.random.default_rng(seed)
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    wall = ((i + j) % 2).ravel().astype(np.float64)
    pos = np.stack([wall, rng.uniform(0, 1, n * n), rng.uniform(0, 1, n * n)], axis=1).astype(np.float32)
    uv = np.stack([wall, rng.uniform(0, 1, n * n)], axis=1).astype(np.float32)
    return pos, _unit(rng.normal(size=(n * n, 3))), uv, grid_faces(n, n)


def strip(n, seed=17):
    """A strip of n vertices (n entries per attribute) that zigzags between y = 0 and y = 1 with z anywhere: long triangles."""
    rng = np.random.default_rng(seed + n)
    k = np.arange(n)
    pos = np.stack([k / max(n - 1, 1) + rng.uniform(-0.3, 0.3, n) / n, (k % 2) + rng.uniform(-0.2, 0.2, n), rng.uniform(0, 1, n)], axis=1).astype(np.float32)
    uv = np.stack([pos[:, 0] * 0.7 + pos[:, 1] * 0.3, pos[:, 1] * 0.9 - pos[:, 0] * 0.2], axis=1) + rng.uniform(-0.05, 0.05, (n, 2))
    return pos, _unit(rng.normal(size=(n, 3))), uv.astype(np.float32), strip_faces(n)


def needle(n, seed=29):
    """A strip whose vertices come in pairs one quantum of the position grid apart (at 20 bits) with texture coordinates a box apart,
    the pairs alternating between the ends of the box: every other entry projects a far tip on an edge of squared length 1 .. 3, and
    the quotient (cn . pn) (uv P - uv N) / |pn|^2 needs 40 bits -- the prediction is what its low 32 bits say."""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    q = 1.0 / ((1 << 20) - 1)
    far = ((k // 2) % 2).astype(np.float64)
    x = np.where(far > 0, 1.0 - (k % 2) * q, (k % 2) * q)
    pos = np.stack([x, far * 0.9 + (k % 2) * q * rng.integers(0, 2, n), rng.uniform(0, 1, n) * far], axis=1)
    uv = np.stack([(k % 2) * 1.0, ((k + k // 2) % 2) * 0.75 + rng.uniform(0, 0.25, n)], axis=1)
    return pos.astype(np.float32), _unit(rng.normal(size=(n, 3))), uv.astype(np.float32), strip_faces(n)


def holed(n=8, seed=19):
    """rough() with two cells cut out: boundary fans at the rims of the holes beside closed fans."""
    cells = [(k // 2 // (n - 1), k // 2 % (n - 1)) for k in range(2 * (n - 1) * (n - 1))]
    keep = [k for k, (j, i) in enumerate(cells) if (j, i) not in ((3, 3), (5, 1))]
    return rough(n, seed, grid_faces(n, n)[keep])


def two_parts(n=5, seed=23):
    a, b = rough(n, seed), rough(n, seed + 1)
    pb = b[0] * np.array([[0.5, 1.0, 1.0]], np.float32) + np.array([[1.5, 0.0, 0.0]], np.float32)
    return (np.concatenate([a[0], pb]), np.concatenate([a[1], b[1]]), np.concatenate([a[2], b[2] + np.array([[0.0, 1.5]], np.float32)]),
            np.concatenate([a[3], b[3] + n * n]).astype(np.uint32))


Design = collections.namedtuple("Design", "name pos normals uv faces bits seams")
Design.__doc__ = """name; pos, normals, uv, faces; bits = (position, uv, normal); seams: None, or (normal charts, uv charts) of irregular.with_seams."""

ROUGH_BITS = (8, 14, 17, 18, 19, 20)
MIXED_BITS = (17, 18, 19)                       # a rough design at these has entries on both sides of pn_norm2 = 2^32
STRIP_ENTRIES = (3, 4, 5, 12, 13, 24, 25, 80)   # 80: 78 geometric entries, orientation bits in three words


def _designs():
    out = []

    def add(name, mesh, bits, seams=None):
        pos, nrm, uv, faces = mesh
        out.append(Design(name, np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(nrm, np.float32), np.ascontiguousarray(uv, np.float32),
                          np.ascontiguousarray(faces, np.uint32), bits, seams))
    for n in (7, 13):
        for b in ROUGH_BITS:
            add("rough-n%d-%db" % (n, b), rough(n, 100 + n), (b, b, min(b, 14)))
    add("collinear-18b", collinear(), (18, 18, 10))
    add("flat-16b", flat(), (16, 16, 8))
    add("flat-20b", flat(), (20, 20, 8))
    add("lattice-8b", lattice(), (8, 8, 6))
    add("lattice-20b", lattice(), (20, 20, 10))
    add("collapsed-14b", collapsed(), (14, 14, 8))
    for k, nb in enumerate((4, 8, 10, 14)):
        add("box-fold-xy-n%db" % nb, box_fold(9, (0, 1, 2), 11 + k), (12 + 2 * k, 10, nb))
        add("box-fold-zx-n%db" % nb, box_fold(9, (2, 0, 1), 31 + k), (12 + 2 * k, 10, nb))
        mesh, b = fold_exact(nb)
        add("fold-exact-n%db" % nb, mesh, (b, 10, nb))
    add("wall-hugger-8b", wall_hugger(), (8, 8, 8))
    add("wall-hugger-14b", wall_hugger(), (14, 14, 8))
    add("wall-hugger-20b", wall_hugger(), (20, 20, 8))
    # flipped diagonals on a larger grid: three and four parallelograms around an entry (ConstrainedMultiParallelogram)
    pos, nrm, uv, faces = wall_hugger(13, 14)
    for b in (8, 14, 20):
        add("wall-hugger-flipped-%db" % b, (pos, nrm, uv, irregular.flip_edges(faces, len(faces) // 2, np.random.default_rng(14))), (b, b, 8))
    for n in STRIP_ENTRIES:
        add("strip-%d-18b" % n, strip(n), (18, 18, 10))
    add("needle-20b", needle(40), (20, 20, 10))
    add("needle-12b", needle(40), (12, 12, 10))
    add("hole-18b", holed(), (18, 18, 10))
    add("two-parts-19b", two_parts(), (19, 19, 12))
    add("rough-n7-seamed-18b", rough(7, 107), (18, 18, 10), ("checker", "stripes"))
    add("rough-n7-seamed-20b", rough(7, 107), (20, 20, 12), ("random", "island"))
    add("box-fold-xy-seamed-n8b", box_fold(9, (0, 1, 2), 11), (14, 12, 8), ("checker", "checker"))
    add("box-fold-zx-seamed-n14b", box_fold(9, (2, 0, 1), 31), (18, 18, 14), ("stripes", "random"))
    return out


DESIGNS = _designs()
PLAIN = [d for d in DESIGNS if d.seams is None]
SEAMED = [d for d in DESIGNS if d.seams is not None]

# the stream dialects every design goes through (synth.options keywords beside the bit depths)
OPTION_SETS = collections.OrderedDict([
    ("stock", dict(uv_prediction=5, normal_prediction=6)),
    ("stock-valence", dict(uv_prediction=5, normal_prediction=6, predictive_connectivity=2)),
    ("default", dict()),
    ("difference", dict(pos_prediction=0, uv_prediction=0)),
])
MULTI = dict(pos_prediction=4, uv_prediction=4)
MULTI_DESIGNS = [d for d in PLAIN if d.name.split("-")[0] in ("rough", "wall", "lattice") and d.bits[0] in (8, 14, 20)]


_decoded = {}


def decoded(d, opt_name):
    """oracle.decode of stream(d, opt_name), once per process; nobody writes to it."""
    import oracle
    key = (d.name, opt_name)
    if key not in _decoded:
        _decoded[key] = oracle.decode(stream(d, opt_name))
    return _decoded[key]


def design(name):
    return next(d for d in DESIGNS if d.name == name)


def options_of(d, opt):
    import draco_sharp_amd.synth as synth
    return synth.options(pos_bits=d.bits[0], uv_bits=d.bits[1], normal_bits=d.bits[2], **opt)


def corner_arguments(d):
    """The arguments of synth.encode_mesh_corners for a seamed design."""
    return irregular.with_seams(d.pos, d.normals, d.uv, d.faces, d.seams[0], d.seams[1], seed=sum(map(ord, d.name)))


_streams = {}


def stream(d, opt_name):
    """The CPU coder's stream of a design under OPTION_SETS[opt_name] (or "multi"), made once per process."""
    import draco_sharp_amd.synth as synth
    key = (d.name, opt_name)
    if key not in _streams:
        opt = options_of(d, MULTI if opt_name == "multi" else OPTION_SETS[opt_name])
        if d.seams is None:
            _streams[key] = synth.encode_mesh(d.pos, d.faces, d.normals, d.uv, opt=opt)
        else:
            _streams[key] = synth.encode_mesh_corners(*corner_arguments(d), opt=opt)
    return _streams[key]


def pin(d):
    """The face-corner multiset of the quantised INPUT (meshutil.source_corner_faces): what any decoder has to give back."""
    import meshutil
    if d.seams is None:
        return meshutil.source_corner_faces(d.pos, d.normals, d.uv, d.faces, d.bits[0], d.bits[2], d.bits[1])[0]
    return meshutil.source_corner_faces_seamed(*corner_arguments(d), pos_bits=d.bits[0], normal_bits=d.bits[2], uv_bits=d.bits[1])[0]


# ----------------------------------------------------------------------------------------------------------- reference
def _nx(c):
    return c - 2 if c % 3 == 2 else c + 1


def _pv(c):
    return c + 2 if c % 3 == 0 else c - 1


class Tables:
    """What the prediction of one attribute sees of a decoded mesh: per corner the attribute's entry and the position, the opposite
    corners (cut at the attribute's seams where it is a corner attribute) and the corner every entry was reached through."""

    def __init__(self, ref, a):
        dec = ref.decoders[ref.decoders_of_attributes()[a]]
        att = ref.attributes[a]
        points = np.asarray(ref.faces, np.int64).ravel()
        ident = np.arange(ref.num_points, dtype=np.int64)

        def entries(x):
            return (np.asarray(x.point_map, np.int64) if len(x.point_map) else ident)[points]
        self.entry = entries(att).tolist()
        opp = [-1 if o == INVALID else int(o) for o in ref.opposite.tolist()]
        if dec["element_type"] == 1:                  # an edge across which either end changes its entry is a seam of the attribute
            e = self.entry
            for c, o in enumerate(opp):
                if o >= 0 and (e[_nx(c)] != e[_pv(o)] or e[_pv(c)] != e[_nx(o)]):
                    opp[c] = -1
        self.opp = opp
        self.d2c = [int(c) for c in dec["data_to_corner"].tolist()]
        assert len(self.d2c) == att.num_entries and all(self.entry[c] == p for p, c in enumerate(self.d2c)), "entries are not in sequence order"
        pos_att = next(x for x in ref.attributes if x.att_type == 0)
        pp = np.asarray(pos_att.portable, np.int64)[entries(pos_att)]
        self.pos = [tuple(int(v) for v in r) for r in pp]

    def swing_left(self, c):
        o = self.opp[_nx(c)]
        return -1 if o < 0 else _nx(o)

    def swing_right(self, c):
        o = self.opp[_pv(c)]
        return -1 if o < 0 else _pv(o)

    def fan(self, c0):
        """The corners around the vertex of c0: to the left until the fan closes or ends, then to the right from c0.  (corners, closed)"""
        out, c = [c0], self.swing_left(c0)
        while c >= 0 and c != c0:
            out.append(c)
            c = self.swing_left(c)
        if c == c0:
            return out, True
        c = self.swing_right(c0)
        while c >= 0:
            out.append(c)
            c = self.swing_right(c)
        return out, False


class Wrap:
    """The wrap transform, encoder's side (App. D "Wrap bounds"): bounds over all values, prediction clamped, correction wrapped."""

    def __init__(self, values, count):
        self.mn, self.mx = int(values.min()), int(values.max())
        self.max_dif = 1 + self.mx - self.mn
        self.max_corr = self.max_dif // 2
        self.min_corr = -self.max_corr
        if self.max_dif % 2 == 0:
            self.max_corr -= 1
        self.count = count

    def symbol(self, orig, pred):
        if pred > self.mx:
            pred = self.mx
            self.count["wrap:clamp-above"] += 1
        elif pred < self.mn:
            pred = self.mn
            self.count["wrap:clamp-below"] += 1
        corr = orig - pred
        if corr < self.min_corr:
            corr += self.max_dif
            self.count["wrap:correction-wraps-up"] += 1
        elif corr > self.max_corr:
            corr -= self.max_dif
            self.count["wrap:correction-wraps-down"] += 1
        return zigzag(corr)


def _parallelogram(t, p, val):
    """The parallelogram across the corner of entry p, or None: the three entries of the opposite face, all coded before p."""
    o = t.opp[t.d2c[p]] if p > 0 else -1
    if o < 0:
        return None
    eo, en, ep = t.entry[o], t.entry[_nx(o)], t.entry[_pv(o)]
    if not (eo < p and en < p and ep < p):
        return None
    return [val[en][k] + val[ep][k] - val[eo][k] for k in range(len(val[p]))]


def ref_wrap(t, val, method, count):
    """Difference (0) or parallelogram (1) under the wrap transform: symbols [entries][nc]."""
    w = Wrap(np.asarray(val), count)
    out = []
    for p in range(len(val)):
        pred = _parallelogram(t, p, val) if method == 1 else None
        if pred is not None:
            count["para:parallelogram"] += 1
        else:
            count["para:difference"] += 1
            pred = val[p - 1] if p else [0] * len(val[p])
        out.append([w.symbol(val[p][k], s32(pred[k])) for k in range(len(val[p]))])
    return out


def _operand_class(dist):
    return "tc:operand-1-back" if dist == 1 else ("tc:operand-2..7-back" if dist < 8 else ("tc:operand-8..11-back" if dist < 12 else "tc:operand-12-or-more-back"))


def ref_texcoords(t, uv, count, roots):
    """TexCoordsPortable, encoder's side.  With N, P the entries at the next and previous corner of the entry's corner, both coded
    earlier and of different texture coordinates, and pn = pos P - pos N of squared length d != 0: the foot X of the tip on the edge
    (an integer division per component), x_uv = uv N * d + (cn . pn) (uv P - uv N), the offset (pn_v, -pn_u) * isqrt(|tip - X|^2 * d),
    the candidates (x_uv + offset) / d and (x_uv - offset) / d, the one closer to the value taken.  Sums and products modulo 2^64,
    the product under the root as an unsigned number, quotients truncated toward zero.  Otherwise the entry at N, else the entry
    before, else zero; and the shared value where N and P agree."""
    w = Wrap(np.asarray(uv), count)
    out = []
    for p in range(len(uv)):
        c = t.d2c[p]
        n_id, p_id = t.entry[_nx(c)], t.entry[_pv(c)]
        pred = None
        if n_id < p and p_id < p:
            for e in (n_id, p_id):
                count[_operand_class(p - e)] += 1
            n_uv, p_uv = uv[n_id], uv[p_id]
            if n_uv == p_uv:
                count["tc:equal-uv"] += 1
                pred = list(p_uv)
            else:
                tip, npos, ppos = t.pos[c], t.pos[t.d2c[n_id]], t.pos[t.d2c[p_id]]
                pn = [ppos[k] - npos[k] for k in range(3)]
                cn = [tip[k] - npos[k] for k in range(3)]
                d = s64(sum(x * x for x in pn))
                if d == 0:
                    count["tc:pn_norm2==0"] += 1
                else:
                    count["tc:geometric"] += 1
                    count["tc:pn_norm2>=2^32" if d >= 1 << 32 else "tc:pn_norm2<2^32"] += 1
                    dot = s64(sum(pn[k] * cn[k] for k in range(3)))
                    pn_uv = [p_uv[k] - n_uv[k] for k in range(2)]
                    exact = [n_uv[k] * d + dot * pn_uv[k] for k in range(2)]
                    x_uv = [s64(v) for v in exact]
                    cx2 = 0
                    for k in range(3):
                        num = s64(dot * pn[k])
                        count["tc:foot-dividend>=2^52" if abs(num) >> 52 else "tc:foot-dividend<2^52"] += 1
                        if num < 0 and num % d:
                            count["tc:foot-negative-with-remainder"] += 1
                        cx = tip[k] - s64(npos[k] + tdiv(num, d))
                        cx2 += cx * cx
                    cx2 = u64(cx2)
                    if cx2 * d > M64:
                        count["tc:root-argument-wraps"] += 1
                    roots.append(u64(cx2 * d))
                    norm = math.isqrt(u64(cx2 * d))
                    cx_uv = [s64(pn_uv[1] * norm), s64(-pn_uv[0] * norm)]
                    cand, sums = [], []
                    for sign in (1, -1):
                        sx = [s64(x_uv[k] + sign * cx_uv[k]) for k in range(2)]
                        sums.append(sx)
                        cand.append([tdiv(sx[k], d) for k in range(2)])
                    err = [u64(sum((uv[p][k] - q[k]) ** 2 for k in range(2))) for q in cand]
                    first = err[0] < err[1]
                    count["tc:orientation-1" if first else "tc:orientation-0"] += 1
                    pred, sx = (cand[0], sums[0]) if first else (cand[1], sums[1])
                    if any(v != s64(v) for v in exact) or any(x_uv[k] + s * cx_uv[k] != s64(x_uv[k] + s * cx_uv[k]) for k in range(2) for s in (1, -1)):
                        count["tc:sum-wraps-2^63"] += 1
                    if any(abs(v) >= 4e15 for v in sx):
                        count["tc:|sx|>=4e15"] += 1
                    if any(abs(q) >= 1 << 31 for q in pred):
                        count["tc:quotient-beyond-31-bits"] += 1
                    if any(v < 0 and v % d for v in sx):
                        count["tc:negative-dividend-with-remainder"] += 1
                    if any(v % d == 0 for v in sx):
                        count["tc:exact-division"] += 1
        if pred is None:
            if n_id < p:
                count["tc:fallback-next"] += 1
                pred = list(uv[n_id])
            elif p > 0:
                count["tc:fallback-entry-before"] += 1
                pred = list(uv[p - 1])
            else:
                count["tc:fallback-zero"] += 1
                pred = [0, 0]
        out.append([w.symbol(uv[p][k], s32(pred[k])) for k in range(2)])
    return out


class Octahedron:
    """The octahedral box of q bits and the canonicalised transform's correction (encoder's side)."""

    def __init__(self, bits):
        self.max_q = (1 << bits) - 1
        self.max_value = self.max_q - 1
        self.center = self.max_value // 2

    def from_vector(self, v):
        """An integer vector whose components have the absolute sum `center` -> canonical (s, t), and the branches taken."""
        c, m = self.center, self.max_value
        tags = []
        if v[0] >= 0:
            s, t = v[1] + c, v[2] + c
        else:
            tags.append("gn:left-half")
            s = abs(v[2]) if v[1] < 0 else m - abs(v[2])
            t = abs(v[1]) if v[2] < 0 else m - abs(v[1])
        if (s, t) in ((0, 0), (0, m), (m, 0)):
            return (m, m), tags + ["gn:corner"]
        if s == 0 and t > c:
            return (s, c - (t - c)), tags + ["gn:fold-s-0"]
        if s == m and t < c:
            return (s, c + (c - t)), tags + ["gn:fold-s-max"]
        if t == m and s < c:
            return (c + (c - s), t), tags + ["gn:fold-t-max"]
        if t == 0 and s > c:
            return (c - (s - c), t), tags + ["gn:fold-t-0"]
        return (s, t), tags

    def invert_diamond(self, s, t):
        c = self.center
        if s >= 0 and t >= 0:
            ss, st = 1, 1
        elif s <= 0 and t <= 0:
            ss, st = -1, -1
        else:
            ss, st = (1 if s > 0 else -1), (1 if t > 0 else -1)
        us, ut = 2 * s - ss * c, 2 * t - st * c
        if ss * st >= 0:
            us, ut = -ut, -us
        else:
            us, ut = ut, us
        return tdiv(us + ss * c, 2), tdiv(ut + st * c, 2)

    def correction(self, orig, pred):
        """The correction that turns `pred` into `orig` (both canonical (s, t)), and the branches taken."""
        c = self.center
        tags = []
        o, q = [orig[0] - c, orig[1] - c], [pred[0] - c, pred[1] - c]
        if abs(q[0]) + abs(q[1]) > c:
            tags.append("oct:prediction-outside-diamond")
            o, q = list(self.invert_diamond(*o)), list(self.invert_diamond(*q))
        if not (q == [0, 0] or (q[0] < 0 and q[1] <= 0)):
            if q[0] == 0:
                r = 0 if q[1] == 0 else (3 if q[1] > 0 else 1)
            elif q[0] > 0:
                r = 2 if q[1] >= 0 else 1
            else:
                r = 0 if q[1] <= 0 else 3
            tags.append("oct:rotation-%d" % r)
            rot = {0: lambda v: v, 1: lambda v: [v[1], -v[0]], 2: lambda v: [-v[0], -v[1]], 3: lambda v: [-v[1], v[0]]}[r]
            o, q = rot(o), rot(q)
        return [x + self.max_q if x < 0 else x for x in (o[0] - q[0], o[1] - q[1])], tags

    def mod_max(self, x):
        return x - self.max_q if x > self.center else (x + self.max_q if x < -self.center else x)


def ref_normals_difference(val, bits, count):
    o = Octahedron(bits)
    out = []
    for p in range(len(val)):
        corr, tags = o.correction(val[p], val[p - 1] if p else [0, 0])
        count.update(tags)
        out.append(corr)
    return out


def ref_geometric_normal(t, val, bits, count):
    """GeometricNormal, encoder's side: the cross products (next - tip) x (previous - tip) of the corners around the entry's vertex
    summed modulo 2^64; divided by abs_sum >> 29 where the absolute sum exceeds 2^29; cut to 32 bits; scaled to the absolute sum
    `center` (x and y by truncating divisions, z by the rest); that vector and its negation to canonical (s, t); both corrections
    under the canonicalised transform, the one of the smaller absolute sum (after folding into +-center) kept, the flipped one on a tie."""
    o = Octahedron(bits)
    out = []
    for p in range(len(val)):
        corners, closed = t.fan(t.d2c[p])
        count["gn:closed-fan" if closed else "gn:open-fan"] += 1
        tip = t.pos[t.d2c[p]]
        n = [0, 0, 0]
        for c in corners:
            a = [t.pos[_nx(c)][k] - tip[k] for k in range(3)]
            b = [t.pos[_pv(c)][k] - tip[k] for k in range(3)]
            n = [n[0] + a[1] * b[2] - a[2] * b[1], n[1] + a[2] * b[0] - a[0] * b[2], n[2] + a[0] * b[1] - a[1] * b[0]]
        if any(x != s64(x) for x in n):
            count["gn:sum-wraps-2^63"] += 1
        n = [s64(x) for x in n]
        abs_sum = min(sum(abs(x) for x in n), (1 << 63) - 1)
        if abs_sum > 1 << 29:
            count["gn:scaled"] += 1
            q = abs_sum >> 29
            if any(abs(x) >> 52 for x in n):
                count["gn:scale-dividend>=2^52"] += 1
            if any(x < 0 and x % q for x in n):
                count["gn:negative-dividend-with-remainder"] += 1
            n = [tdiv(x, q) for x in n]
        else:
            count["gn:small"] += 1
        v = [s32(x) for x in n]
        s3 = sum(abs(x) for x in v)
        if s3 == 0:
            count["gn:s3==0"] += 1
            v[0] = o.center
        else:
            if any(x < 0 and (x * o.center) % s3 for x in v[:2]):
                count["gn:negative-dividend-with-remainder"] += 1
            v[0], v[1] = tdiv(v[0] * o.center, s3), tdiv(v[1] * o.center, s3)
            rest = o.center - abs(v[0]) - abs(v[1])
            v[2] = rest if v[2] >= 0 else -rest
        twins = []
        for w in (v, [-x for x in v]):
            st, tags = o.from_vector(w)
            corr, more = o.correction(val[p], st)
            twins.append((corr, tags + more))
        flip = not (sum(abs(o.mod_max(x)) for x in twins[0][0]) < sum(abs(o.mod_max(x)) for x in twins[1][0]))
        count["gn:flipped" if flip else "gn:not-flipped"] += 1
        count.update(twins[flip][1])                    # the branches a decoder takes: those of the twin that was kept
        out.append(twins[flip][0])
    return out


Reference = collections.namedtuple("Reference", "symbols branches roots")
Reference.__doc__ = """symbols: {attribute index: int64 [entries, nc]} of the attributes the reference covers; branches: Counter; roots: the
arguments (below 2^64) the integer square root of TexCoordsPortable was taken of."""


def reference(ref):
    """The symbols of every attribute of an oracle.decode result that is coded by difference, parallelogram, TexCoordsPortable (under
    the wrap transform) or, for normals, difference or GeometricNormal under the canonicalised octahedral transform."""
    count, roots, symbols = collections.Counter(), [], {}
    for a, att in enumerate(ref.attributes):
        if att.portable is None:
            continue
        val = [[int(x) for x in r] for r in att.portable.tolist()]
        t = Tables(ref, a)
        if att.seq_type == 3 and att.pred_transform == 3 and att.pred_method in (0, 6):
            s = ref_geometric_normal(t, val, att.oct_bits, count) if att.pred_method == 6 else ref_normals_difference(val, att.oct_bits, count)
        elif att.seq_type != 3 and att.pred_transform == 1 and att.pred_method in (0, 1):
            s = ref_wrap(t, val, att.pred_method, count)
        elif att.seq_type != 3 and att.pred_transform == 1 and att.pred_method == 5:
            s = ref_texcoords(t, val, count, roots)
        else:
            continue
        symbols[a] = np.array(s, np.int64).reshape(len(val), -1)
    return Reference(symbols, count, roots)


def multi_parallelogram_branches(ref):
    """Of the attributes coded by ConstrainedMultiParallelogram, from the decoded values alone (which parallelograms an entry uses is
    the coder's choice, so its symbols have no reference here): the parallelograms around every entry, left swing first, then to the
    right of the start, four at the most; counted is every entry at which the sum of the first k of them, k = 2, 3, 4, is negative
    and leaves a remainder when divided by k -- the truncation toward zero of the average."""
    count = collections.Counter()
    for a, att in enumerate(ref.attributes):
        if att.portable is None or att.pred_method != 4:
            continue
        val = [[int(x) for x in r] for r in att.portable.tolist()]
        t = Tables(ref, a)
        for p in range(1, len(val)):
            found = []
            for c in t.fan(t.d2c[p])[0]:
                o = t.opp[c]
                if o < 0:
                    continue
                eo, en, ep = t.entry[o], t.entry[_nx(o)], t.entry[_pv(o)]
                if eo < p and en < p and ep < p and len(found) < 4:
                    found.append([val[en][k] + val[ep][k] - val[eo][k] for k in range(len(val[p]))])
            count["mp:parallelograms-%d" % len(found)] += 1
            for k in range(2, len(found) + 1):
                if any(sum(f[j] for f in found[:k]) < 0 and sum(f[j] for f in found[:k]) % k for j in range(len(val[p]))):
                    count["mp:negative-sum-with-remainder-by-%d" % k] += 1
    return count
